// route_select.hip -- dual / triple granularity router select ("scatter/gather") for gfx950.
//
// Replaces the routing tails of the reference encoders in eval mode:
//   modules/dynamic_modules/EncoderDual.py:134-149   (argmax, x2 repeat_interleave, where, mask)
//   modules/dynamic_modules/EncoderTriple.py:148-176 (argmax, x4/x2 repeat_interleave, 3 wheres, mask)
//   modules/dynamic_modules/RouterDual.py:53-57      (entropy threshold gate)
// One pass: every output float4 reads exactly one source (the branch that won its cell), so HBM
// traffic is the algorithmic 1 read + 1 write per element; the reference materialises two
// upsampled copies and reads all branches.  Pure data movement -> HBM-bound: each thread moves
// 16 B, consecutive lanes consecutive addresses; LDS only holds the image's grain map (1 B / cell).
#include "launchers.h"

// MODE 0: f32 gate logits, 1: int64 gate, 2: f32 entropy map + threshold (the fixed-entropy router fused in:
// gate = [(ent <= thr), (ent > thr)], whose argmax is (ent > thr); NaN compares false twice -> 0)
template <int G, int MODE>
__device__ __forceinline__ int gate_argmax(const void *gate, size_t cell, float thr)
{
    // torch.argmax semantics: first maximal value wins, NaN counts as the maximum
    if (MODE == 2) {
        return (((const float *)gate)[cell] > thr) ? 1 : 0;
    } else if (MODE == 1) {
        const long long *g = (const long long *)gate + cell * G;
        long long best = g[0];
        int bi = 0;
#pragma unroll
        for (int i = 1; i < G; ++i) {
            long long v = g[i];
            if (v > best) { best = v; bi = i; }
        }
        return bi;
    } else {
        const float *g = (const float *)gate + cell * G;
        float best = g[0];
        int bi = 0;
#pragma unroll
        for (int i = 1; i < G; ++i) {
            float v = g[i];
            if ((v > best) || (v != v && best == best)) { best = v; bi = i; }
        }
        return bi;
    }
}

// G = 2: dual (fine grid = 2x coarse); G = 3: triple (fine grid = 4x coarse, median 2x).
// One workgroup = one image b and a run of PLANES_PER_BLOCK planes p in [0, C]: planes 0..C-1 are
// the feature channels, plane C is the codebook_mask plane (which also emits `indices`).  The
// image's grain map (argmax per coarse cell) is evaluated once per workgroup into LDS; after that
// every thread streams float4s: one 16-B load from the branch that won the cell, one 16-B store.
constexpr int PLANES_PER_BLOCK = 8;
constexpr int MAX_CELLS = 4096;                 // grain map bytes kept in LDS (64 x 64 coarse cells)

// V = floats per thread and access: 4 (rows are whole float4s), or 2 for the dual select on an odd coarse width (rows of 2 wc floats
// are then only 8-byte pieces; both floats of a piece lie in one coarse cell)
template <int V> struct VecOf;
template <> struct VecOf<4> { typedef f32x4 type; };
template <> struct VecOf<2> { typedef f32x2 type; };
template <int G, int MODE, int V = 4>
__global__ __launch_bounds__(256) void route_select_kernel(
    const void *__restrict__ gate, const float *__restrict__ h_coarse,
    const float *__restrict__ h_median, const float *__restrict__ h_fine,
    int B, int C, int hc, int wc,
    float *__restrict__ h_out, long long *__restrict__ indices, float *__restrict__ cmask,
    float thr, long long *__restrict__ gate_out)
{
    constexpr int SC = (G == 2) ? 2 : 4;          // fine pixels per coarse cell edge
    __shared__ unsigned char grain[MAX_CELLS];
    typedef typename VecOf<V>::type vec_t;
    const int H = SC * hc, W = SC * wc, W4 = W / V;
    const int per_plane = H * W4;
    const int ncell = hc * wc;
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const int p0 = blockIdx.x * PLANES_PER_BLOCK;
    const int p1 = (p0 + PLANES_PER_BLOCK < C + 1) ? p0 + PLANES_PER_BLOCK : C + 1;
    const bool in_lds = ncell <= MAX_CELLS;
    if (in_lds) {
        for (int cell = threadIdx.x; cell < ncell; cell += 256)
            grain[cell] = (unsigned char)gate_argmax<G, MODE>(gate, (size_t)b * ncell + cell, thr);
        __syncthreads();
    }
    auto grain_of = [&](int cell) -> int {
        return in_lds ? (int)grain[cell] : gate_argmax<G, MODE>(gate, (size_t)b * ncell + cell, thr);
    };
    for (int p = p0; p < p1; ++p) {
        const size_t plane = (size_t)b * C + p;
        for (int i = threadIdx.x; i < per_plane; i += 256) {
            const int y = i / W4, x = (i - y * W4) * V;
            const int cy = y / SC;
            const int cx0 = x / SC, cx1 = (x + V - 1) / SC;   // the (up to two) coarse cells of this piece
            const int cell0 = cy * wc + cx0;
            const int g0 = grain_of(cell0);
            const int g1 = (cx1 != cx0) ? grain_of(cell0 + 1) : g0;
            if (p == C) {
                vec_t m;
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    int g = ((x + j) / SC == cx0) ? g0 : g1;
                    m[j] = (G == 2) ? (g == 0 ? 0.25f : 1.0f)
                                    : (g == 0 ? 0.0625f : (g == 1 ? 0.25f : 1.0f));
                }
                *(vec_t *)(cmask + ((size_t)b * H + y) * W + x) = m;
                if (y % SC == 0) {
                    if (x % SC == 0) indices[(size_t)b * ncell + cell0] = g0;
                    if (cx1 != cx0) indices[(size_t)b * ncell + cell0 + 1] = g1;
                    if (MODE == 2 && gate_out != nullptr) {        // the router's int64 gate, a by-product
                        const float *ent = (const float *)gate + (size_t)b * ncell;
                        if (x % SC == 0) {
                            const float e = ent[cell0];
                            longlong2 gg; gg.x = (e <= thr) ? 1 : 0; gg.y = (e > thr) ? 1 : 0;
                            *(longlong2 *)(gate_out + 2 * ((size_t)b * ncell + cell0)) = gg;
                        }
                        if (cx1 != cx0) {
                            const float e = ent[cell0 + 1];
                            longlong2 gg; gg.x = (e <= thr) ? 1 : 0; gg.y = (e > thr) ? 1 : 0;
                            *(longlong2 *)(gate_out + 2 * ((size_t)b * ncell + cell0 + 1)) = gg;
                        }
                    }
                }
                continue;
            }
            const size_t o = (plane * H + y) * W + x;
            vec_t v;
            if (g0 == G - 1 && g1 == G - 1) {
                v = *(const vec_t *)(h_fine + o);
            } else {
                vec_t f = {};
                if (g0 == G - 1 || g1 == G - 1) f = *(const vec_t *)(h_fine + o);
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    const int xx = x + j;
                    const int g = (xx / SC == cx0) ? g0 : g1;
                    float sv;
                    if (g == 0)
                        sv = h_coarse[(plane * hc + cy) * wc + xx / SC];
                    else if (G == 3 && g == 1)
                        sv = h_median[(plane * (2 * hc) + y / 2) * (2 * wc) + xx / 2];
                    else
                        sv = f[j];
                    v[j] = sv;
                }
            }
            *(vec_t *)(h_out + o) = v;
        }
    }
    if (in_lds) __syncthreads();                  // the next image overwrites the grain map
    }
}

// ---- the same select on 2-byte elements (fp16 / bf16 branch features; DVQ_FEATURES in dvq.h).  Nothing is converted, so ONE
// kernel serves both types: elements are unsigned shorts.  V = elements per thread and access, a power of two chosen by the
// launcher: 8 (16 bytes) where the rows, the planes and the pointers allow, else 4, 2 or 1.  A piece starts at a column that
// is a multiple of V, and V and SC are powers of two, so a piece of V >= SC elements covers exactly V / SC WHOLE coarse cells
// (dual at V = 8: four; triple: two) and a shorter one lies inside one cell: the float kernel's cx0 / cx1 pair becomes the
// compile-time array g[NC], and element j of a piece belongs to cell j / SC of it.  MODE 0 / 1 as above (no entropy form: the
// fixed-entropy router runs as entropy_gate_kernel + the int64 gate).  indices and cmask are written as by the float kernel.
template <int V> struct U16Of { typedef unsigned short type __attribute__((ext_vector_type(V))); };
template <> struct U16Of<1> { struct type { unsigned short s; __device__ unsigned short &operator[](int) { return s; } }; };
template <int V> __device__ __forceinline__ void store_mask(float *p, const float (&m)[V])
{
    if constexpr (V == 1) {
        p[0] = m[0];
    } else if constexpr (V == 2) {
        *(f32x2 *)p = (f32x2){m[0], m[1]};
    } else {
#pragma unroll
        for (int q = 0; q < V; q += 4) *(f32x4 *)(p + q) = (f32x4){m[q], m[q + 1], m[q + 2], m[q + 3]};
    }
}
template <int G, int MODE, int V>
__global__ __launch_bounds__(256) void route_select_x16_kernel(
    const void *__restrict__ gate, const unsigned short *__restrict__ h_coarse,
    const unsigned short *__restrict__ h_median, const unsigned short *__restrict__ h_fine,
    int B, int C, int hc, int wc,
    unsigned short *__restrict__ h_out, long long *__restrict__ indices, float *__restrict__ cmask)
{
    static_assert(MODE == 0 || MODE == 1, "float32 logits or the int64 gate");
    constexpr int SC = (G == 2) ? 2 : 4;          // fine pixels per coarse cell edge
    constexpr int NC = V >= SC ? V / SC : 1;      // coarse cells a piece covers
    __shared__ unsigned char grain[MAX_CELLS];
    typedef typename U16Of<V>::type vec_t;
    const int H = SC * hc, W = SC * wc, WV = W / V;
    const int per_plane = H * WV;
    const int ncell = hc * wc;
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const int p0 = blockIdx.x * PLANES_PER_BLOCK;
    const int p1 = (p0 + PLANES_PER_BLOCK < C + 1) ? p0 + PLANES_PER_BLOCK : C + 1;
    const bool in_lds = ncell <= MAX_CELLS;
    if (in_lds) {
        for (int cell = threadIdx.x; cell < ncell; cell += 256)
            grain[cell] = (unsigned char)gate_argmax<G, MODE>(gate, (size_t)b * ncell + cell, 0.0f);
        __syncthreads();
    }
    auto grain_of = [&](int cell) -> int {
        return in_lds ? (int)grain[cell] : gate_argmax<G, MODE>(gate, (size_t)b * ncell + cell, 0.0f);
    };
    // one loop over the pieces of all of the workgroup's planes: a 32 x 32 plane is only 128 16-byte pieces, half a workgroup
    {
        for (int idx = threadIdx.x; idx < (p1 - p0) * per_plane; idx += 256) {
            const int p = p0 + idx / per_plane, i = idx - (p - p0) * per_plane;
            const size_t plane = (size_t)b * C + p;
            const int y = i / WV, x = (i - y * WV) * V;
            const int cy = y / SC, cx0 = x / SC;
            const int cell0 = cy * wc + cx0;      // the piece's first (V < SC: only) coarse cell
            int g[NC];
            bool all_fine = true, any_fine = false;
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                g[c] = grain_of(cell0 + c);
                all_fine = all_fine && g[c] == G - 1;
                any_fine = any_fine || g[c] == G - 1;
            }
            if (p == C) {
                float m[V];
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    const int gg = g[V >= SC ? j / SC : 0];
                    m[j] = (G == 2) ? (gg == 0 ? 0.25f : 1.0f)
                                    : (gg == 0 ? 0.0625f : (gg == 1 ? 0.25f : 1.0f));
                }
                store_mask<V>(cmask + ((size_t)b * H + y) * W + x, m);
                if (y % SC == 0 && (V >= SC || x % SC == 0)) {
#pragma unroll
                    for (int c = 0; c < NC; ++c) indices[(size_t)b * ncell + cell0 + c] = g[c];
                }
                continue;
            }
            const size_t o = (plane * H + y) * W + x;
            vec_t v;
            if (all_fine) {
                v = *(const vec_t *)(h_fine + o);
            } else {
                vec_t f = {};
                if (any_fine) f = *(const vec_t *)(h_fine + o);
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    const int xx = x + j;
                    const int gg = g[V >= SC ? j / SC : 0];
                    unsigned short sv;
                    if (gg == 0)
                        sv = h_coarse[(plane * hc + cy) * wc + xx / SC];
                    else if (G == 3 && gg == 1)
                        sv = h_median[(plane * (2 * hc) + y / 2) * (2 * wc) + xx / 2];
                    else
                        sv = f[j];
                    v[j] = sv;
                }
            }
            *(vec_t *)(h_out + o) = v;
        }
    }
    if (in_lds) __syncthreads();                  // the next image overwrites the grain map
    }
}

// ---- the same select on channels_last branches (DVQ_NHWC in dvq.h): every branch and h_out are [B, rows, cols, C] row-major, a
// pixel is ONE run of C elements.  Nothing is converted and nothing depends on the element type, so one kernel serves float32,
// fp16 and bf16: a pixel's run is moved as raw bytes in pieces of V bytes, V the widest of 16, 8, 4, 2 that divides the run
// (row_bytes = C x element size) and fits the actual alignment of the four tensors (the launcher's choice: a view that starts one
// element into its storage moves narrower pieces).  Workgroup = one row y of one image's output: its W x ppr pieces (ppr =
// row_bytes / V) are dealt to the threads in memory order, so a wave's accesses to h_out and to a fine source are one contiguous
// run.  The grain of a piece's cell is evaluated where it is needed, by the rule of the kernels above (gate_argmax): the logits
// of a cell are a few bytes that the SC x SC x ppr pieces of the cell share (a broadcast within a wave, an L1 / L2 hit across
// waves) -- no grain map in LDS, hence no second regime at many cells.  A fine pixel that is not selected is never read; coarse
// and median runs are read with plain loads (each is wanted 4 or 16 times), fine runs and h_out non-temporally when nt is set
// (the launcher: the output exceeds DVQ_CACHED_MAX_BYTES).  The thread that moves a pixel's first piece writes its codebook_mask
// value, and at a cell's first pixel the cell's index: the values of the NCHW kernels.  MODE 0 / 1 as above.
template <int V> struct PieceOf;
template <> struct PieceOf<16> { typedef unsigned type __attribute__((ext_vector_type(4))); };
template <> struct PieceOf<8> { typedef unsigned type __attribute__((ext_vector_type(2))); };
template <> struct PieceOf<4> { typedef unsigned type; };
template <> struct PieceOf<2> { typedef unsigned short type; };
template <int G, int MODE, int V>
__global__ __launch_bounds__(256) void route_select_rows_kernel(
    const void *__restrict__ gate, const char *__restrict__ h_coarse, const char *__restrict__ h_median,
    const char *__restrict__ h_fine, int B, unsigned row_bytes, int hc, int wc, char *__restrict__ h_out,
    long long *__restrict__ indices, float *__restrict__ cmask, unsigned ppr, int ppr_shift, int nt)
{
    static_assert(MODE == 0 || MODE == 1, "float32 logits or the int64 gate");
    constexpr unsigned SC = (G == 2) ? 2 : 4;     // fine pixels per coarse cell edge
    typedef typename PieceOf<V>::type piece_t;
    const unsigned H = SC * (unsigned)hc, W = SC * (unsigned)wc;
    const unsigned per_row = W * ppr;             // pieces of one row of pixels (< 2^31: dvq_abi.hip)
    for (unsigned b = blockIdx.y; b < (unsigned)B; b += gridDim.y)
    for (unsigned y = blockIdx.x; y < H; y += gridDim.x) {
        const unsigned cy = y / SC;
        const size_t orow = ((size_t)b * H + y) * W;                     // the row's first pixel in h_out / h_fine / cmask
        const size_t crow = ((size_t)b * hc + cy) * wc;                  // its row of cells
        const size_t mrow = ((size_t)b * (2 * hc) + y / 2) * (2 * wc);   // (triple) its row of median pixels
        for (unsigned j = threadIdx.x; j < per_row; j += 256) {
            unsigned x, q;
            if (ppr_shift >= 0) { x = j >> ppr_shift; q = j & (ppr - 1); }
            else { x = j / ppr; q = j - x * ppr; }
            const size_t cell = crow + x / SC;
            const int g = gate_argmax<G, MODE>(gate, cell, 0.0f);
            const size_t off = (size_t)q * V;
            piece_t v;
            if (g == G - 1) {
                const piece_t *s = (const piece_t *)(h_fine + (orow + x) * row_bytes + off);
                v = nt ? __builtin_nontemporal_load(s) : *s;
            } else if (G == 3 && g == 1) {
                v = *(const piece_t *)(h_median + (mrow + x / 2) * row_bytes + off);
            } else {
                v = *(const piece_t *)(h_coarse + cell * row_bytes + off);
            }
            piece_t *d = (piece_t *)(h_out + (orow + x) * row_bytes + off);
            if (nt) __builtin_nontemporal_store(v, d);
            else *d = v;
            if (q == 0) {
                cmask[orow + x] = (G == 2) ? (g == 0 ? 0.25f : 1.0f) : (g == 0 ? 0.0625f : (g == 1 ? 0.25f : 1.0f));
                if (y % SC == 0 && x % SC == 0) indices[cell] = g;
            }
        }
    }
}

__global__ __launch_bounds__(256) void entropy_gate_kernel(const float *__restrict__ ent, long n,
                                                           float thr, long long *__restrict__ gate)
{
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (long)gridDim.x * blockDim.x) {
        float e = ent[i];
        longlong2 g;
        g.x = (e <= thr) ? 1 : 0;
        g.y = (e > thr) ? 1 : 0;
        *(longlong2 *)(gate + 2 * i) = g;
    }
}

// out[n, :] = E[idx[n], :], D % 4 == 0; invalid index -> NaN row
__global__ __launch_bounds__(256) void embed_gather_kernel(const float *__restrict__ E, int K, int D,
                                                           const long long *__restrict__ idx, long n,
                                                           float *__restrict__ out)
{
    const int D4 = D / 4;
    const size_t total = (size_t)n * D4;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (size_t)gridDim.x * blockDim.x) {
        size_t row = i / D4;
        int q = (int)(i - row * D4);
        long long j = idx[row];
        f32x4 v;
        if (j >= 0 && j < K) {
            v = *(const f32x4 *)(E + (size_t)j * D + 4 * q);
        } else {
            float nanv = __builtin_nanf("");
            v = (f32x4){nanv, nanv, nanv, nanv};
        }
        *(f32x4 *)(out + row * D + 4 * q) = v;
    }
}

static int grid_for(size_t items)
{
    size_t blocks = (items + 255) / 256;
    if (blocks > 256 * 16) blocks = 256 * 16;     // 256 CUs x 16 resident 256-thread blocks
    if (blocks < 1) blocks = 1;
    return (int)blocks;
}

int dvq_launch_route_select(int G, int gate_mode, const void *gate, const float *h_coarse,
                            const float *h_median, const float *h_fine, int B, int C, int hc, int wc,
                            float *h_out, long long *indices, float *cmask, float thr, long long *gate_out,
                            hipStream_t st)
{
    dim3 grid((C + 1 + PLANES_PER_BLOCK - 1) / PLANES_PER_BLOCK, B < 65535 ? B : 65535), block(256);
#define DVQ_SEL(GG, MM) hipLaunchKernelGGL((route_select_kernel<GG, MM>), grid, block, 0, st, gate, h_coarse, h_median, h_fine, B, C, hc, wc, h_out, indices, cmask, thr, gate_out)
#define DVQ_SEL2(MM) hipLaunchKernelGGL((route_select_kernel<2, MM, 2>), grid, block, 0, st, gate, h_coarse, h_median, h_fine, B, C, hc, wc, h_out, indices, cmask, thr, gate_out)
    if (G == 2 && (wc & 1)) {                                // odd coarse width: 8-byte pieces
        if (gate_mode == 2) DVQ_SEL2(2);
        else if (gate_mode == 1) DVQ_SEL2(1);
        else DVQ_SEL2(0);
    } else
    if (G == 2 && gate_mode == 2) DVQ_SEL(2, 2);
    else if (G == 2 && gate_mode == 1) DVQ_SEL(2, 1);
    else if (G == 2) DVQ_SEL(2, 0);
    else if (gate_mode == 1) DVQ_SEL(3, 1);
    else DVQ_SEL(3, 0);
#undef DVQ_SEL
#undef DVQ_SEL2
    return (int)hipGetLastError();
}

// 2-byte features.  The piece width: the widest power of two up to 8 elements that divides the row length (and with it the
// plane, H rows of it: plane bases are only 2 H W bytes aligned -- a C = 7, 2 x 2 fine map has 8-byte planes) AND fits the actual
// alignment of h_fine, h_out (2 V bytes) and cmask (V floats, at most 16 bytes per store): a view that starts one element into
// its storage moves 2-byte pieces.  h_coarse / h_median are read one element at a time (2-byte aligned: dvq_abi.hip).
int dvq_launch_route_select_x16(int G, int gate_mode, const void *gate, const void *h_coarse, const void *h_median,
                                const void *h_fine, int B, int C, int hc, int wc, void *h_out, long long *indices,
                                float *cmask, hipStream_t st)
{
    const long W = (long)(G == 2 ? 2 : 4) * wc, H = (long)(G == 2 ? 2 : 4) * hc;
    const uintptr_t a16 = (uintptr_t)h_fine | (uintptr_t)h_out, am = (uintptr_t)cmask;
    int V = 8;
    while (V > 1 && (W % V != 0 || (H * W) % V != 0 || a16 % (2 * V) != 0 || am % (4 * V < 16 ? 4 * V : 16) != 0)) V >>= 1;
    dim3 grid((C + 1 + PLANES_PER_BLOCK - 1) / PLANES_PER_BLOCK, B < 65535 ? B : 65535), block(256);
    typedef const unsigned short *cu16;
#define DVQ_SEL16(GG, MM, VV) hipLaunchKernelGGL((route_select_x16_kernel<GG, MM, VV>), grid, block, 0, st, gate, (cu16)h_coarse, (cu16)h_median, (cu16)h_fine, B, C, hc, wc, (unsigned short *)h_out, indices, cmask)
#define DVQ_SEL16V(GG, MM) do { if (V == 8) DVQ_SEL16(GG, MM, 8); else if (V == 4) DVQ_SEL16(GG, MM, 4); else if (V == 2) DVQ_SEL16(GG, MM, 2); else DVQ_SEL16(GG, MM, 1); } while (0)
    if (G == 2 && gate_mode == 1) DVQ_SEL16V(2, 1);
    else if (G == 2) DVQ_SEL16V(2, 0);
    else if (gate_mode == 1) DVQ_SEL16V(3, 1);
    else DVQ_SEL16V(3, 0);
#undef DVQ_SEL16V
#undef DVQ_SEL16
    return (int)hipGetLastError();
}

// channels_last features of es-byte elements (see route_select_rows_kernel): the piece width from the run length and the actual
// alignment of the four tensors; cached / non-temporal by the size of the output (DVQ_CACHED_MAX_BYTES, as the gate's pooling pass)
int dvq_launch_route_select_rows(int G, int gate_mode, const void *gate, const void *h_coarse, const void *h_median,
                                 const void *h_fine, int es, int B, int C, int hc, int wc, void *h_out, long long *indices,
                                 float *cmask, hipStream_t st)
{
    const unsigned SC = G == 2 ? 2 : 4;
    const unsigned row_bytes = (unsigned)C * (unsigned)es;
    const uintptr_t al = (uintptr_t)h_coarse | (uintptr_t)h_median | (uintptr_t)h_fine | (uintptr_t)h_out;
    unsigned V = 16;
    while (V > 2 && (row_bytes % V != 0 || al % V != 0)) V >>= 1;
    const unsigned ppr = row_bytes / V;
    int ppr_shift = -1;
    if ((ppr & (ppr - 1)) == 0) { ppr_shift = 0; while ((1u << ppr_shift) < ppr) ++ppr_shift; }
    const int nt = (size_t)B * SC * hc * SC * wc * row_bytes > DVQ_CACHED_MAX_BYTES;
    dim3 grid(SC * (unsigned)hc, B < 65535 ? B : 65535), block(256);
    typedef const char *cch;
#define DVQ_SELR(GG, MM, VV) hipLaunchKernelGGL((route_select_rows_kernel<GG, MM, VV>), grid, block, 0, st, gate, (cch)h_coarse, (cch)h_median, (cch)h_fine, B, row_bytes, hc, wc, (char *)h_out, indices, cmask, ppr, ppr_shift, nt)
#define DVQ_SELRV(GG, MM) do { if (V == 16) DVQ_SELR(GG, MM, 16); else if (V == 8) DVQ_SELR(GG, MM, 8); else if (V == 4) DVQ_SELR(GG, MM, 4); else DVQ_SELR(GG, MM, 2); } while (0)
    if (G == 2 && gate_mode == 1) DVQ_SELRV(2, 1);
    else if (G == 2) DVQ_SELRV(2, 0);
    else if (gate_mode == 1) DVQ_SELRV(3, 1);
    else DVQ_SELRV(3, 0);
#undef DVQ_SELRV
#undef DVQ_SELR
    return (int)hipGetLastError();
}

int dvq_launch_entropy_gate(const float *ent, long n, float thr, long long *gate, hipStream_t st)
{
    hipLaunchKernelGGL(entropy_gate_kernel, dim3(grid_for((size_t)n)), dim3(256), 0, st, ent, n, thr, gate);
    return (int)hipGetLastError();
}

int dvq_launch_embed_gather(const float *E, int K, int D, const long long *idx, long n, float *out,
                            hipStream_t st)
{
    hipLaunchKernelGGL(embed_gather_kernel, dim3(grid_for((size_t)n * (D / 4))), dim3(256), 0, st, E, K, D, idx, n, out);
    return (int)hipGetLastError();
}
