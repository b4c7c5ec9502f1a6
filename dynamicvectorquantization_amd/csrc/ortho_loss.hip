// ortho_loss.hip -- the orthogonal codebook regulariser (eq. 2 of arXiv 2112.00384) and its gradient, fused (gfx950).
//
// Replaces (reference modules/vector_quantization/quantize_lucidrains.py:18-24, orthogonal_loss_fn): F.normalize, torch.eye, the
// [h, n, n] einsum, the subtraction, the square and the sum -- about five n x n tensors forward and as many again for autograd (1 GiB
// each at n = 16384) for one scalar and an [n, d] gradient.  Here nothing of size n x n reaches memory.
//
//   rinv_i = 1 / max(|w_i|, 1e-12)       F.normalize's rule; computed once (ortho_rinv_kernel), kept by the caller for backward
//   C_ij   = fl(fl(dot(w_i, w_j) rinv_i) rinv_j)      the cosine of rows i and j
//   loss   = sum_ij (C_ij - delta_ij)^2 / (h n^2)
//   G_i    = (4 g / (h n^2)) sum_j (C_ij - delta_ij) rinv_j w_j            dloss / d c^_i, c^ = the normalised rows
//   grad_i = (G_i - c^_i (c^_i . G_i)) rinv_i                              F.normalize's backward
//
// The dots are the assign's D/2 chained v_mfma_f32_32x32x2_f32 per 32 x 32 tile (vq_assign_exact.hip), operands raw rows: the two
// inverse norms scale the tile's 16 results per lane, not the 32 D operands.  A lane (c, h) of a wave holds row 32 t + c of "its"
// tile in registers, channels k(s, h) = 8 (s / 4) + 4 h + s % 4 for MFMA step s (any pairing of the channels gives the same sum as
// long as both operands use it; this one makes a lane's operands 16-byte pieces of a row); the other tile is staged in LDS by the
// workgroup, rows padded to D + 8 floats.
//
// Forward (ortho_gram_kernel): the Gram matrix is symmetric, so only tiles (ti <= tj) are scored; an off-diagonal tile counts
// twice, a diagonal tile subtracts the identity.  A workgroup = 4 waves = 4 column tiles tj against OL_ROWCHUNK row tiles; a
// tile's 1024 squares are summed in fp32 per lane, tiles in double; one double partial per workgroup, finalised by one workgroup in
// one fixed order: the loss is the same bits on every run.  No atomics.
// Backward (ortho_backward_kernel, ortho_backward_combine_kernel): a wave owns 32 rows i and sweeps the column tiles of its slice
// (the sweep is split over up to 8 slices, each writing its partial G to the workspace; the combine kernel adds them in slice order
// and applies F.normalize's backward): the score tile, P_ji = (C_ij - delta_ij)
// rinv_j in the 16 accumulators of the first MFMA, which ARE the second MFMA's B operand (k = the tile's row j in the accumulator's
// own order 8 g + 4 h + q; the A operand, channel d of row j, is read from the staged tile in that order), D / 32 accumulators of
// 32 channels x 32 rows, each tile's contribution summed on its own and added once.  One plain 16-byte store per four channels of
// a gradient row; no atomics, bit-reproducible.
#include "launchers.h"

#define OL_ROWCHUNK 8          // row tiles a forward workgroup scores against its four column tiles

// one wave per row: rinv = 1 / max(sqrt(sum w^2), 1e-12)
__global__ __launch_bounds__(256) void ortho_rinv_kernel(const float *__restrict__ t, long rows, int D, float *__restrict__ rinv)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long i = (long)blockIdx.x * 4 + wave;
    if (i >= rows) return;
    const float *p = t + (size_t)i * D;
    float s = 0.0f;
    for (int k = 4 * lane; k < D; k += 256) {
        const f32x4 v = *(const f32x4 *)(p + k);
        s += (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if (lane == 0) rinv[i] = 1.0f / fmaxf(__fsqrt_rn(s), 1e-12f);
}

// the workgroup stages row tile `tile` (rows 32 tile .. + 31 of th [n, D], zero rows past n) and the rows' inverse norms (0 past n)
template <int D>
__device__ __forceinline__ void ortho_stage(const float *__restrict__ th, const float *__restrict__ rh, int n, int tile, float *lds,
                                            float *rl)
{
    constexpr int STR = D + 8, Q = D / 4;
    for (int p = threadIdx.x; p < 32 * Q; p += blockDim.x) {
        const int row = p / Q, c4 = p - row * Q;
        const int j = tile * 32 + row;
        f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
        if (j < n) v = *(const f32x4 *)(th + (size_t)j * D + 4 * c4);
        *(f32x4 *)(lds + row * STR + 4 * c4) = v;
    }
    if (threadIdx.x < 32) {
        const int j = tile * 32 + (int)threadIdx.x;
        rl[threadIdx.x] = (j < n) ? rh[j] : 0.0f;
    }
}

// acc[r] of lane (c, h) = dot(staged row 8 (r / 4) + 4 h + r % 4, the lane's own row c)
template <int D>
__device__ __forceinline__ f32x16 ortho_dots(const float *lds, const float (&zr)[D / 2], int c, int h)
{
    constexpr int STR = D + 8;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    const float *ap = lds + c * STR + 4 * h;
#pragma unroll
    for (int q = 0; q < D / 8; ++q) {
        const f32x4 a = *(const f32x4 *)(ap + 8 * q);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[0], zr[4 * q + 0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[1], zr[4 * q + 1], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[2], zr[4 * q + 2], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[3], zr[4 * q + 3], acc, 0, 0, 0);
    }
    return acc;
}

template <int D>
__global__ __launch_bounds__(256) void ortho_gram_kernel(const float *__restrict__ t, const float *__restrict__ rinv, int n,
                                                         double *__restrict__ partials)
{
    constexpr int STR = D + 8;
    extern __shared__ __attribute__((aligned(16))) float lds[];        // 32 * STR tile floats, 32 inverse norms
    __shared__ double red[4];
    float *rl = lds + 32 * STR;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 31, h = lane >> 5;
    const int head = blockIdx.z;
    const float *th = t + (size_t)head * n * D;
    const float *rh = rinv + (size_t)head * n;
    const int T = (n + 31) / 32;
    const int tj = blockIdx.x * 4 + wave;                               // this wave's column tile
    const int tjmax = (int)blockIdx.x * 4 + 3 < T - 1 ? (int)blockIdx.x * 4 + 3 : T - 1;
    const int ti0 = blockIdx.y * OL_ROWCHUNK;
    int ti1 = ti0 + OL_ROWCHUNK < T ? ti0 + OL_ROWCHUNK : T;
    ti1 = ti1 < tjmax + 1 ? ti1 : tjmax + 1;                            // the upper triangle: ti <= tj (workgroup-uniform bound)
    double dsum = 0.0;
    if (ti0 < ti1) {
        const int i = tj * 32 + c;
        const bool iv = i < n;
        float zr[D / 2];
        const float *zp = th + (size_t)(iv ? i : 0) * D + 4 * h;
#pragma unroll
        for (int q = 0; q < D / 8; ++q) {
            f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
            if (iv) v = *(const f32x4 *)(zp + 8 * q);
            zr[4 * q + 0] = v[0]; zr[4 * q + 1] = v[1]; zr[4 * q + 2] = v[2]; zr[4 * q + 3] = v[3];
        }
        const float ri = iv ? rh[i] : 0.0f;
        for (int ti = ti0; ti < ti1; ++ti) {
            __syncthreads();                                            // everyone is done with the previous tile
            ortho_stage<D>(th, rh, n, ti, lds, rl);
            __syncthreads();
            if (ti <= tj && tj < T) {                                   // (wave-uniform)
                const f32x16 acc = ortho_dots<D>(lds, zr, c, h);
                float ts = 0.0f;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const f32x4 rj = *(const f32x4 *)(rl + 8 * g + 4 * h);
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int j = ti * 32 + 8 * g + 4 * h + q;
                        float cv = __fmul_rn(__fmul_rn(acc[4 * g + q], ri), rj[q]);
                        if (j == i && iv) cv = __fsub_rn(cv, 1.0f);
                        ts = __fadd_rn(ts, __fmul_rn(cv, cv));
                    }
                }
                dsum += (double)(ti < tj ? __fmul_rn(2.0f, ts) : ts);
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) dsum += __shfl_xor(dsum, off);
    __syncthreads();
    if (lane == 0) red[wave] = dsum;
    __syncthreads();
    if (tid == 0)
        partials[((size_t)head * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// one workgroup: the partials in one fixed order, loss = sum * inv (inv = 1 / (h n^2))
__global__ __launch_bounds__(256) void ortho_finalize_kernel(const double *__restrict__ partials, long nparts, double inv,
                                                             float *__restrict__ loss)
{
    __shared__ double red[256];
    double s = 0.0;
    for (long p = threadIdx.x; p < nparts; p += 256) s += partials[p];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = (float)(red[0] * inv);
}

template <int D>
__global__ __launch_bounds__(256) void ortho_backward_kernel(const float *__restrict__ t, const float *__restrict__ rinv,
                                                             int n, int tper, float *__restrict__ gpart)
{
    constexpr int STR = D + 8, NC = D / 32;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *rl = lds + 32 * STR;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 31, h = lane >> 5;
    const int head = blockIdx.y;
    const float *th = t + (size_t)head * n * D;
    const float *rh = rinv + (size_t)head * n;
    float *gh = gpart + ((size_t)blockIdx.z * gridDim.y + head) * n * D;   // this column slice's partial G of this head
    const int T = (n + 31) / 32;
    const int tj0 = blockIdx.z * tper, tj1 = tj0 + tper < T ? tj0 + tper : T;
    const int i = (blockIdx.x * 4 + wave) * 32 + c;                     // this lane's own row (both lane halves hold it)
    const bool iv = i < n;
    float zr[D / 2];
    const float *zp = th + (size_t)(iv ? i : 0) * D + 4 * h;
#pragma unroll
    for (int q = 0; q < D / 8; ++q) {
        f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
        if (iv) v = *(const f32x4 *)(zp + 8 * q);
        zr[4 * q + 0] = v[0]; zr[4 * q + 1] = v[1]; zr[4 * q + 2] = v[2]; zr[4 * q + 3] = v[3];
    }
    const float ri = iv ? rh[i] : 0.0f;
    f32x16 gacc[NC];
#pragma unroll
    for (int ch = 0; ch < NC; ++ch)
#pragma unroll
        for (int r = 0; r < 16; ++r) gacc[ch][r] = 0.0f;

    for (int tj = tj0; tj < tj1; ++tj) {
        __syncthreads();
        ortho_stage<D>(th, rh, n, tj, lds, rl);
        __syncthreads();
        const f32x16 acc = ortho_dots<D>(lds, zr, c, h);
        float pj[16];                                                   // P[j][i], j = 8 g + 4 h + q of this tile: (C_ij - delta_ij) rinv_j
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4 rj = *(const f32x4 *)(rl + 8 * g + 4 * h);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int j = tj * 32 + 8 * g + 4 * h + q;
                float cv = __fmul_rn(__fmul_rn(acc[4 * g + q], ri), rj[q]);
                if (j == i && iv) cv = __fsub_rn(cv, 1.0f);
                pj[4 * g + q] = __fmul_rn(cv, rj[q]);
            }
        }
        // G[i][d] += sum_j P[j][i] w_j[d]: MFMA rows = 32 channels of chunk ch, columns = the 32 own rows, k = j in pj's order
#pragma unroll
        for (int ch = 0; ch < NC; ++ch) {
            const float *bp = lds + (4 * h) * STR + 32 * ch + c;
            // this tile's 32 terms on their own, then ONE add into the running sum: the sum's error grows with the number of tiles,
            // not of rows (as one chain, n = 1024 gave 3e-6 of max |g|, four times the torch CPU gradient's error)
            f32x16 part;
#pragma unroll
            for (int r = 0; r < 16; ++r) part[r] = 0.0f;
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                const float a = bp[(8 * (s >> 2) + (s & 3)) * STR];
                part = __builtin_amdgcn_mfma_f32_32x32x2f32(a, pj[s], part, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) gacc[ch][r] = __fadd_rn(gacc[ch][r], part[r]);
        }
    }

    // gacc[ch][r] of lane (c, h) = G[i = c][d = 32 ch + 8 (r / 4) + 4 h + r % 4]: the slice's partial sums, one 16-byte store per four channels
    if (iv) {
#pragma unroll
        for (int ch = 0; ch < NC; ++ch)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 o = {gacc[ch][4 * g + 0], gacc[ch][4 * g + 1], gacc[ch][4 * g + 2], gacc[ch][4 * g + 3]};
                *(f32x4 *)(gh + (size_t)i * D + 32 * ch + 8 * g + 4 * h) = o;
            }
    }
}

// one wave per row: G = the S slices' partial sums in slice order, then F.normalize's backward and the scale
//   grad_i = (G_i - c^_i (c^_i . G_i)) rinv_i coef g,   c^_i = w_i rinv_i
__global__ __launch_bounds__(256) void ortho_backward_combine_kernel(const float *__restrict__ t, const float *__restrict__ rinv,
                                                                     const float *__restrict__ gout, const float *__restrict__ gpart,
                                                                     int S, long rows, int D, float coef, float *__restrict__ grad)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long i = (long)blockIdx.x * 4 + wave;
    if (i >= rows) return;
    const bool on = 4 * lane < D;                                       // D <= 256: a lane owns four channels
    f32x4 G = {0.0f, 0.0f, 0.0f, 0.0f}, w = {0.0f, 0.0f, 0.0f, 0.0f};
    if (on) {
        w = *(const f32x4 *)(t + (size_t)i * D + 4 * lane);
        for (int sl = 0; sl < S; ++sl) {
            const f32x4 p = *(const f32x4 *)(gpart + ((size_t)sl * rows + i) * D + 4 * lane);
            G[0] = __fadd_rn(G[0], p[0]); G[1] = __fadd_rn(G[1], p[1]); G[2] = __fadd_rn(G[2], p[2]); G[3] = __fadd_rn(G[3], p[3]);
        }
    }
    const float ri = rinv[i];
    f32x4 chat;
    float dotp = 0.0f;
#pragma unroll
    for (int q = 0; q < 4; ++q) { chat[q] = __fmul_rn(w[q], ri); dotp = __fadd_rn(dotp, __fmul_rn(chat[q], G[q])); }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) dotp = __fadd_rn(dotp, __shfl_xor(dotp, off));
    const float sc = __fmul_rn(__fmul_rn(coef, gout[0]), ri);
    if (on) {
        f32x4 o;
#pragma unroll
        for (int q = 0; q < 4; ++q) o[q] = __fmul_rn(__fsub_rn(G[q], __fmul_rn(chat[q], dotp)), sc);
        *(f32x4 *)(grad + (size_t)i * D + 4 * lane) = o;
    }
}

static inline size_t ortho_lds_bytes(int D) { return (size_t)(32 * (D + 8) + 32) * sizeof(float); }

void dvq_ortho_grid(int h, int n, unsigned *gx, unsigned *gy)
{
    const int T = (n + 31) / 32;
    *gx = (unsigned)((T + 3) / 4);
    *gy = (unsigned)((T + OL_ROWCHUNK - 1) / OL_ROWCHUNK);
    (void)h;
}

template <int D>
static int launch_ortho_forward(const float *t, int h, int n, float *rinv, float *loss, double *partials, hipStream_t st)
{
    unsigned gx, gy;
    dvq_ortho_grid(h, n, &gx, &gy);
    hipLaunchKernelGGL(ortho_gram_kernel<D>, dim3(gx, gy, (unsigned)h), dim3(256), ortho_lds_bytes(D), st, t, rinv, n, partials);
    int rc = (int)hipGetLastError();
    if (rc) return rc;
    hipLaunchKernelGGL(ortho_finalize_kernel, dim3(1), dim3(256), 0, st, partials, (long)gx * gy * h,
                       1.0 / ((double)h * (double)n * (double)n), loss);
    return (int)hipGetLastError();
}

int dvq_launch_ortho_forward(const float *t, int h, int n, int D, float *rinv, float *loss, double *partials, hipStream_t st)
{
    const long rows = (long)h * n;
    hipLaunchKernelGGL(ortho_rinv_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, t, rows, D, rinv);
    int rc = (int)hipGetLastError();
    if (rc) return rc;
    switch (D) {
    case 64:  return launch_ortho_forward<64>(t, h, n, rinv, loss, partials, st);
    case 128: return launch_ortho_forward<128>(t, h, n, rinv, loss, partials, st);
    case 256: return launch_ortho_forward<256>(t, h, n, rinv, loss, partials, st);
    default:  return -1000;
    }
}

// The backward sweep of a block of rows is split over S column slices (grid z) so that small codebooks do not run as a few long
// chains and large ones fill every SIMD: about 1024 waves, at most 8 slices.  tper = column tiles per slice.
void dvq_ortho_backward_slices(int h, int n, int *S, int *tper)
{
    const int T = (n + 31) / 32;
    long waves = (long)T * h;
    int s = (int)(1024 / (waves < 1 ? 1 : waves));
    s = s < 1 ? 1 : (s > 8 ? 8 : s);
    s = s > T ? T : s;
    *tper = (T + s - 1) / s;
    *S = (T + *tper - 1) / *tper;
}

template <int D>
static int launch_ortho_backward(const float *t, const float *rinv, const float *gout, int h, int n, float *grad, float *gpart,
                                 hipStream_t st)
{
    const int T = (n + 31) / 32;
    int S, tper;
    dvq_ortho_backward_slices(h, n, &S, &tper);
    const float coef = (float)(4.0 / ((double)h * (double)n * (double)n));
    hipLaunchKernelGGL(ortho_backward_kernel<D>, dim3((unsigned)((T + 3) / 4), (unsigned)h, (unsigned)S), dim3(256), ortho_lds_bytes(D),
                       st, t, rinv, n, tper, gpart);
    int rc = (int)hipGetLastError();
    if (rc) return rc;
    const long rows = (long)h * n;
    hipLaunchKernelGGL(ortho_backward_combine_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, t, rinv, gout, gpart, S, rows,
                       D, coef, grad);
    return (int)hipGetLastError();
}

int dvq_launch_ortho_backward(const float *t, const float *rinv, const float *gout, int h, int n, int D, float *grad, float *gpart,
                              hipStream_t st)
{
    switch (D) {
    case 64:  return launch_ortho_backward<64>(t, rinv, gout, h, n, grad, gpart, st);
    case 128: return launch_ortho_backward<128>(t, rinv, gout, h, n, grad, gpart, st);
    case 256: return launch_ortho_backward<256>(t, rinv, gout, h, n, grad, gpart, st);
    default:  return -1000;
    }
}
