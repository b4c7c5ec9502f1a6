// code_sums_det.hip -- the per-code sums of the training step in ONE FIXED summation order (include/dvq.h: dvq_code_sums_det,
// dvq_vq_backward_codebook_det_f32), for gfx950.  The atomic kernels of ema_update.hip / train_rows.hip add in arrival order; here
// no float atomic and no returning atomic is on the path, so the bits are a pure function of (values, codes, N, D, K):
//   tiles of DET_T = 2048 consecutive tokens; inside a tile a code's members in ascending token index, cut into runs of DET_R = 32;
//   a run summed sequentially from its first member; the run sums added sequentially in run order; a code's tile partials added
//   sequentially in ascending tile index, from the first tile that has a member.
// Three launches on a caller-provided workspace:
//   sort     one workgroup per tile: keys (code << 11 | token) bitonic-sorted in LDS (keys are distinct, so the sorted order IS the
//            token order inside a code), segment heads numbered by a prefix sum -> order[], the tile's list of codes, the segment
//            starts, the list of long segments, and the row slot[tile][code] = entry (0xFFFF: no member) the reduce looks up.
//   partial  one workgroup per (tile, 16-channel slice): [16][2048] values in LDS, a group of 16 lanes per entry walks its segment
//            run by run; a segment longer than DET_LONG tokens has its runs summed by all 64 lane groups and added up in run
//            order by one.  Every partial row is written ONCE with plain stores: ws.partial[tile][entry][D].
//   reduce   a thread per (code, four channels) adds the code's rows in tile order and writes the result (x c for the gradient).
// The layout (NCHW / row-major), the storage type and the load width change only how a value reaches LDS, never the order.
#include "launchers.h"

#define DET_T 2048
#define DET_R 32
#define DET_BC 16
#define DET_STR (DET_T + 4)
#define DET_LONG 128                      // a segment longer than this is summed by all lane groups (at most 15 per tile)
#define DET_MAXLONG 16
#define DET_SEGSTR (DET_T + 8)            // seg[nd] = the tile's valid tokens
#define DET_NONE 0xFFFFu
static_assert(DET_T / DET_R == 64 && DET_T / DET_LONG <= DET_MAXLONG, "64 lane groups take the 64 runs of a full tile");

struct DetWs {
    unsigned short *order;                // [nt][DET_T] the tile's tokens by (code, token)
    unsigned short *seg;                  // [nt][DET_SEGSTR] start of entry e in order[]
    unsigned short *tcode;                // [nt][DET_T] code of entry e
    unsigned short *slot;                 // [nt][K] entry of a code in the tile, DET_NONE
    int *meta;                            // [nt][DET_MAXLONG + 2]: nd, nlong, long entries
    float *partial;                       // [nt][cap][D]
    size_t total;
};

static inline size_t det_up(size_t b) { return (b + 255) / 256 * 256; }

static DetWs det_layout(void *ws, long N, int D, int K)
{
    const size_t nt = (size_t)((N + DET_T - 1) / DET_T), cap = K < DET_T ? K : DET_T;
    char *p = (char *)ws;
    size_t off = 0;
    DetWs w;
    w.order = (unsigned short *)(p + off); off += det_up(nt * DET_T * 2);
    w.seg = (unsigned short *)(p + off); off += det_up(nt * DET_SEGSTR * 2);
    w.tcode = (unsigned short *)(p + off); off += det_up(nt * DET_T * 2);
    w.slot = (unsigned short *)(p + off); off += det_up(nt * (size_t)K * 2);
    w.meta = (int *)(p + off); off += det_up(nt * (DET_MAXLONG + 2) * 4);
    w.partial = (float *)(p + off); off += det_up(nt * cap * (size_t)D * 4);
    w.total = off;
    return w;
}

size_t dvq_code_sums_det_ws_bytes(long N, int D, int K) { return det_layout(nullptr, N, D, K).total; }

// exclusive prefix sum of one int per thread over a 1024-thread workgroup (wtot: [17] ints of LDS); *total = the sum
__device__ __forceinline__ int det_block_scan(int v, int *wtot, int *total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const int o = __shfl_up(inc, off); if (lane >= off) inc += o; }
    __syncthreads();                                                     // (wtot of a previous scan has been read)
    if (lane == 63) wtot[wave] = inc;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) { const int x = wtot[w]; tot += x; if (w < wave) base += x; }
    *total = tot;
    return base + inc - v;
}

__global__ __launch_bounds__(1024) void det_sort_kernel(const long long *__restrict__ codes, long N, int K,
                                                        unsigned short *__restrict__ order_g, unsigned short *__restrict__ seg_g,
                                                        unsigned short *__restrict__ tcode_g, unsigned short *__restrict__ slot_g,
                                                        int *__restrict__ meta_g)
{
    __shared__ unsigned keys[DET_T];
    __shared__ unsigned short slot_s[16384];
    __shared__ unsigned short seg_s[DET_SEGSTR];
    __shared__ int wtot[17];
    const int tid = threadIdx.x;
    const long tile = blockIdx.x, tok0 = tile * DET_T;
    for (int k = tid; k < K; k += 1024) slot_s[k] = (unsigned short)DET_NONE;
    for (int t = tid; t < DET_T; t += 1024) {
        const long n = tok0 + t;
        const long long cj = n < N ? codes[n] : -1;
        keys[t] = (cj >= 0 && cj < K) ? ((unsigned)cj << 11 | (unsigned)t) : 0xFFFFFFFFu;
    }
    __syncthreads();
    for (int k = 2; k <= DET_T; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            const int l = ((tid & ~(j - 1)) << 1) | (tid & (j - 1)), r = l + j;
            const unsigned a = keys[l], b = keys[r];
            if ((a > b) == ((l & k) == 0)) { keys[l] = b; keys[r] = a; }
            __syncthreads();
        }
    // entries: thread owns positions 2 tid, 2 tid + 1 of the sorted tile
    const int i0 = 2 * tid;
    const unsigned k0 = keys[i0], k1 = keys[i0 + 1], kp = i0 > 0 ? keys[i0 - 1] : 0xFFFFFFFFu;
    const bool v0 = k0 != 0xFFFFFFFFu, v1 = k1 != 0xFFFFFFFFu;
    const bool h0 = v0 && (i0 == 0 || (kp >> 11) != (k0 >> 11)), h1 = v1 && (k0 >> 11) != (k1 >> 11);
    int nd, nvalid;
    int e = det_block_scan((int)h0 + (int)h1, wtot, &nd);
    (void)det_block_scan((int)v0 + (int)v1, wtot, &nvalid);
    unsigned short *order = order_g + (size_t)tile * DET_T, *tcode = tcode_g + (size_t)tile * DET_T;
    order[i0] = (unsigned short)(k0 & 2047u);
    order[i0 + 1] = (unsigned short)(k1 & 2047u);
    if (h0) { tcode[e] = (unsigned short)(k0 >> 11); seg_s[e] = (unsigned short)i0; slot_s[k0 >> 11] = (unsigned short)e; ++e; }
    if (h1) { tcode[e] = (unsigned short)(k1 >> 11); seg_s[e] = (unsigned short)(i0 + 1); slot_s[k1 >> 11] = (unsigned short)e; }
    if (tid == 0) seg_s[nd] = (unsigned short)nvalid;
    __syncthreads();
    unsigned short *seg = seg_g + (size_t)tile * DET_SEGSTR;
    for (int i = tid; i <= nd; i += 1024) seg[i] = seg_s[i];
    unsigned short *slot = slot_g + (size_t)tile * K;
    for (int k = tid; k < K; k += 1024) slot[k] = slot_s[k];
    // the long segments, in entry order
    const int e0 = 2 * tid;
    const bool l0 = e0 < nd && (int)seg_s[e0 + 1] - (int)seg_s[e0] > DET_LONG;
    const bool l1 = e0 + 1 < nd && (int)seg_s[e0 + 2] - (int)seg_s[e0 + 1] > DET_LONG;
    int nlong;
    int li = det_block_scan((int)l0 + (int)l1, wtot, &nlong);
    int *meta = meta_g + (size_t)tile * (DET_MAXLONG + 2);
    if (l0) meta[2 + li++] = e0;
    if (l1) meta[2 + li] = e0 + 1;
    if (tid == 0) { meta[0] = nd; meta[1] = nlong; }
}

// four consecutive latents at p (aligned to the four), widened
template <int XT>
__device__ __forceinline__ f32x4 det_load4(const typename DvqLat<XT>::T *p)
{
    if constexpr (XT == 0) {
        return *(const f32x4 *)p;
    } else {
        const uint2 u = *(const uint2 *)p;
        f32x4 v;
        v[0] = dvq_widen_bits<XT>((unsigned short)(u.x & 0xFFFFu));
        v[1] = dvq_widen_bits<XT>((unsigned short)(u.x >> 16));
        v[2] = dvq_widen_bits<XT>((unsigned short)(u.y & 0xFFFFu));
        v[3] = dvq_widen_bits<XT>((unsigned short)(u.y >> 16));
        return v;
    }
}

// XT: storage type of z.  ROWS: z is [N, D], else [B, D, HW].  VEC: four elements along the contiguous axis per load (NCHW: HW % 4 == 0;
// z aligned to the four).  GRAD: the value of a token is (z - E[code]) * mask (XT == 0).
template <int XT, bool ROWS, bool VEC, bool GRAD>
__global__ __launch_bounds__(1024) void det_partial_kernel(const typename DvqLat<XT>::T *__restrict__ z, const float *__restrict__ E,
                                                           const float *__restrict__ mask, int D, int HW, long N, int K, int cap,
                                                           const unsigned short *__restrict__ order_g,
                                                           const unsigned short *__restrict__ seg_g,
                                                           const unsigned short *__restrict__ tcode_g, const int *__restrict__ meta_g,
                                                           float *__restrict__ partial)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *tile = (float *)smem;                                                   // [DET_BC][DET_STR]
    float *red = tile + DET_BC * DET_STR;                                          // [64][DET_BC]
    unsigned short *order = (unsigned short *)(red + 64 * DET_BC);                 // [DET_T]
    unsigned short *seg = order + DET_T;                                           // [DET_SEGSTR]
    unsigned short *tcode = seg + DET_SEGSTR;                                      // [DET_T]
    float *m_s = (float *)(tcode + DET_T);                                         // GRAD: [DET_T]
    const int tid = threadIdx.x;
    const int nslice = (D + DET_BC - 1) / DET_BC;
    const long tb = blockIdx.x / nslice;
    const int c0 = (int)(blockIdx.x % nslice) * DET_BC;
    const long tok0 = tb * DET_T;
    const int *meta = meta_g + (size_t)tb * (DET_MAXLONG + 2);
    const int nd = meta[0], nlong = meta[1];
    for (int i = tid; i < DET_T; i += 1024) order[i] = order_g[(size_t)tb * DET_T + i];
    for (int i = tid; i <= nd; i += 1024) seg[i] = seg_g[(size_t)tb * DET_SEGSTR + i];
    for (int i = tid; i < nd; i += 1024) tcode[i] = tcode_g[(size_t)tb * DET_T + i];
    if constexpr (GRAD)
        for (int t = tid; t < DET_T; t += 1024) { const long n = tok0 + t; m_s[t] = (mask != nullptr && n < N) ? mask[n] : 1.0f; }
    if constexpr (ROWS && VEC) {                                                   // piece: token idx / 4, channels 4 (idx % 4) ..
#pragma unroll 4
        for (int idx = tid; idx < DET_T * 4; idx += 1024) {
            const int t = idx >> 2, q = 4 * (idx & 3);
            const long n = tok0 + t;
            f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
            if (n < N && c0 + q < D) v = det_load4<XT>(z + (size_t)n * D + c0 + q);
#pragma unroll
            for (int j = 0; j < 4; ++j) tile[(q + j) * DET_STR + t] = v[j];
        }
    } else if constexpr (ROWS) {
#pragma unroll 4
        for (int idx = tid; idx < DET_T * DET_BC; idx += 1024) {
            const int t = idx >> 4, ch = idx & 15;
            const long n = tok0 + t;
            tile[ch * DET_STR + t] = (n < N && c0 + ch < D) ? dvq_widen<XT>(z[(size_t)n * D + c0 + ch]) : 0.0f;
        }
    } else if constexpr (VEC) {                                                    // piece: channel idx / 512, tokens 4 (idx % 512) ..
#pragma unroll 4
        for (int idx = tid; idx < DET_BC * (DET_T / 4); idx += 1024) {
            const int ch = idx >> 9, t = 4 * (idx & 511);
            const long n = tok0 + t;                                               // (HW % 4 == 0: the four share an image, N % 4 == 0)
            f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
            if (n < N && c0 + ch < D) {
                const unsigned b = (unsigned)n / (unsigned)HW, hw = (unsigned)n - b * (unsigned)HW;
                v = det_load4<XT>(z + ((size_t)b * D + c0 + ch) * HW + hw);
            }
            *(f32x4 *)(tile + ch * DET_STR + t) = v;
        }
    } else {
#pragma unroll 4
        for (int idx = tid; idx < DET_BC * DET_T; idx += 1024) {
            const int ch = idx >> 11, t = idx & 2047;
            const long n = tok0 + t;
            float v = 0.0f;
            if (n < N && c0 + ch < D) {
                const unsigned b = (unsigned)n / (unsigned)HW, hw = (unsigned)n - b * (unsigned)HW;
                v = dvq_widen<XT>(z[((size_t)b * D + c0 + ch) * HW + hw]);
            }
            tile[ch * DET_STR + t] = v;
        }
    }
    __syncthreads();
    const int ch = tid & 15, g = tid >> 4;
    const bool ch_ok = c0 + ch < D;
    const float *row = tile + ch * DET_STR;
    float *prow = partial + (size_t)tb * cap * D + c0 + ch;
    auto value = [&](int t, float ev) -> float {
        if constexpr (GRAD) return __fmul_rn(__fsub_rn(row[t], ev), m_s[t]);
        return row[t];
    };
    // one run, [r0, r1) of order[], summed sequentially from its first member
    auto run_sum = [&](int r0, int r1, float ev) -> float {
        float acc = value(order[r0], ev);
        int i = r0 + 1;
        for (; i + 4 <= r1; i += 4) {
            const int t0 = order[i], t1 = order[i + 1], t2 = order[i + 2], t3 = order[i + 3];
            const float a0 = value(t0, ev), a1 = value(t1, ev), a2 = value(t2, ev), a3 = value(t3, ev);
            acc = __fadd_rn(__fadd_rn(__fadd_rn(__fadd_rn(acc, a0), a1), a2), a3);
        }
        for (; i < r1; ++i) acc = __fadd_rn(acc, value(order[i], ev));
        return acc;
    };
    for (int e = g; e < nd; e += 64) {
        const int s = seg[e], en = seg[e + 1];
        if (en - s > DET_LONG) continue;                                           // everybody's work, below
        float ev = 0.0f;
        if constexpr (GRAD) ev = ch_ok ? E[(size_t)tcode[e] * D + c0 + ch] : 0.0f;
        float total = 0.0f;
        for (int r0 = s; r0 < en; r0 += DET_R) {
            const float acc = run_sum(r0, r0 + DET_R < en ? r0 + DET_R : en, ev);
            total = r0 == s ? acc : __fadd_rn(total, acc);
        }
        if (ch_ok) prow[(size_t)e * D] = total;
    }
    for (int li = 0; li < nlong; ++li) {                                           // (nlong is the workgroup's: the barriers are uniform)
        const int e = meta[2 + li];
        const int s = seg[e], en = seg[e + 1];
        const int nruns = (en - s + DET_R - 1) / DET_R;                            // <= 64
        float ev = 0.0f;
        if constexpr (GRAD) ev = ch_ok ? E[(size_t)tcode[e] * D + c0 + ch] : 0.0f;
        if (g < nruns) {
            const int r0 = s + g * DET_R;
            red[g * DET_BC + ch] = run_sum(r0, r0 + DET_R < en ? r0 + DET_R : en, ev);
        }
        __syncthreads();
        if (g == 0) {
            float total = red[ch];
            for (int r = 1; r < nruns; ++r) total = __fadd_rn(total, red[r * DET_BC + ch]);
            if (ch_ok) prow[(size_t)e * D] = total;
        }
        __syncthreads();                                                           // red[] is free again
    }
}

// a thread per (code, four channels): the code's partial rows in ascending tile order, from the first tile that has one.
// scale == nullptr: out = the sum, count[k] = the members.  Else out = c * sum, c = -(scale[0] * coef_scale).
__global__ __launch_bounds__(256) void det_reduce_kernel(const unsigned short *__restrict__ slot, const unsigned short *__restrict__ seg_g,
                                                         const float *__restrict__ partial, int nt, int K, int D, int cap,
                                                         const float *__restrict__ scale, float coef_scale, float *__restrict__ count,
                                                         float *__restrict__ out)
{
    const int D4 = D >> 2;
    const long gid = (long)blockIdx.x * 256 + threadIdx.x;
    const int k = (int)(gid / D4), q = (int)(gid - (long)k * D4);
    if (k >= K) return;
    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    bool have = false;
    int cnt = 0;
    for (int t0 = 0; t0 < nt; t0 += 8) {
        unsigned e[8];
        f32x4 r[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) e[u] = t0 + u < nt ? (unsigned)slot[(size_t)(t0 + u) * K + k] : DET_NONE;
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (e[u] != DET_NONE) r[u] = *(const f32x4 *)(partial + ((size_t)(t0 + u) * cap + e[u]) * D + 4 * q);
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (e[u] != DET_NONE) {
                if (have) { for (int j = 0; j < 4; ++j) acc[j] = __fadd_rn(acc[j], r[u][j]); }
                else acc = r[u];
                have = true;
                if (count != nullptr && q == 0) {
                    const unsigned short *sg = seg_g + (size_t)(t0 + u) * DET_SEGSTR + e[u];
                    cnt += (int)sg[1] - (int)sg[0];
                }
            }
    }
    if (scale != nullptr) {
        const float c = -__fmul_rn(scale[0], coef_scale);
        for (int j = 0; j < 4; ++j) acc[j] = __fmul_rn(c, acc[j]);
    }
    *(f32x4 *)(out + (size_t)k * D + 4 * q) = acc;
    if (count != nullptr && q == 0) count[k] = (float)cnt;
}

template <int XT, bool GRAD>
static int det_launch_partial(const void *zv, const float *E, const float *mask, int D, int HW, long N, int K, int cap, const DetWs &w,
                              hipStream_t st)
{
    typedef typename DvqLat<XT>::T T;
    const T *z = (const T *)zv;
    const unsigned grid = (unsigned)(((N + DET_T - 1) / DET_T) * ((D + DET_BC - 1) / DET_BC));
    const size_t shm = (size_t)DET_BC * DET_STR * 4 + 64 * DET_BC * 4 + DET_T * 2 + DET_SEGSTR * 2 + DET_T * 2 + (GRAD ? DET_T * 4 : 0);
    const bool rows = HW == 1;
    const bool vec = ((uintptr_t)zv & (4 * sizeof(T) - 1)) == 0 && (rows || (HW & 3) == 0);
#define DET_GO(R, V) dvq_launch_lds<det_partial_kernel<XT, R, V, GRAD>>(dim3(grid), dim3(1024), shm, st, z, E, mask, D, HW, N, K, cap, \
                                                                        w.order, w.seg, w.tcode, w.meta, w.partial)
    if (rows) return vec ? DET_GO(true, true) : DET_GO(true, false);
    return vec ? DET_GO(false, true) : DET_GO(false, false);
#undef DET_GO
}

// xt: 0 = float32, DVQ_DTYPE_F16 / DVQ_DTYPE_BF16.  E == nullptr: the statistics (count and out [K, D] overwritten).  Else the
// codebook gradient (xt == 0): out[j] = c * sum of (z - E[j]) * mask, rows 0 .. K - 1 written.  D % 4 == 0, K <= 16384, N < 2^31.
int dvq_launch_code_sums_det(const void *z, int xt, const float *E, const long long *codes, const float *mask, const float *g_loss,
                             float coef_scale, int D, int HW, long N, int K, float *count, float *out, void *ws, hipStream_t st)
{
    if (xt < 0 || xt > 2 || K > 16384 || (D & 3) != 0 || (E != nullptr && xt != 0)) return -1000;
    const DetWs w = det_layout(ws, N, D, K);
    const int nt = (int)((N + DET_T - 1) / DET_T), cap = K < DET_T ? K : DET_T;
    hipLaunchKernelGGL(det_sort_kernel, dim3((unsigned)nt), dim3(1024), 0, st, codes, N, K, w.order, w.seg, w.tcode, w.slot, w.meta);
    if (int rc = (int)hipGetLastError()) return rc;
    int rc;
    if (E != nullptr) rc = det_launch_partial<0, true>(z, E, mask, D, HW, N, K, cap, w, st);
    else if (xt == 0) rc = det_launch_partial<0, false>(z, nullptr, nullptr, D, HW, N, K, cap, w, st);
    else if (xt == 1) rc = det_launch_partial<1, false>(z, nullptr, nullptr, D, HW, N, K, cap, w, st);
    else rc = det_launch_partial<2, false>(z, nullptr, nullptr, D, HW, N, K, cap, w, st);
    if (rc) return rc;
    const long nthreads = (long)K * (D >> 2);
    hipLaunchKernelGGL(det_reduce_kernel, dim3((unsigned)((nthreads + 255) / 256)), dim3(256), 0, st, w.slot, w.seg, w.partial, nt, K, D,
                       cap, E != nullptr ? g_loss : nullptr, coef_scale, E != nullptr ? nullptr : count, out);
    return (int)hipGetLastError();
}
