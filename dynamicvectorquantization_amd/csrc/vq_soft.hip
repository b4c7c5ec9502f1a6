// vq_soft.hip -- fused soft code assignment on the fp32 matrix cores (gfx950): distances, softmax(-d / temp), the hard code and
// the multinomial draw of get_soft_codes in one launch.
//
// Replaces VQEmbedding.compute_distances + F.softmax(-distances / temp) + argmin / torch.multinomial
// (reference modules/vector_quantization/quantize2_mask.py:29-48,193-205; quantize_rqvae.py:372-400, once per depth).
//
// Built on the exact-chain tile loop's pieces (dvq_exact_tile.h), every dot the same bits as the hard assign's.  What this kernel
// adds: it takes the chain in the TOKEN_ROWS order -- accumulator register r of lane (c, h) holds token (r&3) + 8(r>>2) + 4h,
// code 32 t + c -- because its outputs are row-major [N, K] rows.  The price is that a token's running argmin lives in 32 lanes;
// they are merged once, after the loop.
//
// Phase A (tile loop): d = fl(fl(xn + en) - 2 dot) -> dist (optional); s = (-d) / temp -> the soft row (or the workspace when only
// the draw is wanted); running first-index argmin per (lane, register).  The row maximum of s needs no second running value:
// temp > 0, so max s = (-min d) / temp, the same division on the argmin's distance (a NaN distance is the argmin AND makes the
// whole softmax row NaN, as in torch).
// Phase B (each wave on its own 32 rows, freshly written, read back with 16-byte accesses): sum of expf(s - max) in double, one
// fixed order (lane-strided, then a butterfly); p = expf(s - max) / float(sum) written in place; argmax of p / q for the draw.
// design (a) of DESIGN.md section 4.13: one MFMA sweep, one re-read of the rows; the alternative doubles the MFMA work that
// bounds the kernel.
#include "launchers.h"
#include "dvq_exact_tile.h"

template <int V>
__device__ __forceinline__ void soft_ld(const float *p, float (&v)[V])
{
    if constexpr (V == 4) {
        const f32x4 t = *(const f32x4 *)p;
        v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
    } else {
        v[0] = *p;
    }
}
template <int V>
__device__ __forceinline__ void soft_st(float *p, const float (&v)[V])
{
    if constexpr (V == 4) {
        const f32x4 t = {v[0], v[1], v[2], v[3]};
        *(f32x4 *)p = t;
    } else {
        *p = v[0];
    }
}

// one row of phase B by one wave; V = 4: K % 4 == 0 and 16-byte aligned rows
template <int V>
__device__ __forceinline__ void soft_row(const float *srow, float *prow, const float *qrow, int K, float m, int lane,
                                         long long *code_out)
{
    double dsum = 0.0;
    for (int j = lane * V; j < K; j += 64 * V) {
        float s[V];
        soft_ld<V>(srow + j, s);
#pragma unroll
        for (int i = 0; i < V; ++i) dsum += (double)expf(s[i] - m);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) dsum += __shfl_xor(dsum, off);
    const float sum = (float)dsum;
    float bv = -__builtin_inff();
    int bi = 0x7fffffff;
    for (int j = lane * V; j < K; j += 64 * V) {
        float s[V], p[V];
        soft_ld<V>(srow + j, s);
#pragma unroll
        for (int i = 0; i < V; ++i) p[i] = expf(s[i] - m) / sum;
        if (prow != nullptr) soft_st<V>(prow + j, p);
        if (qrow != nullptr) {
            float qv[V];
            soft_ld<V>(qrow + j, qv);
#pragma unroll
            for (int i = 0; i < V; ++i) argmax_pair(bv, bi, p[i] / qv[i], j + i);
        }
    }
    if (qrow != nullptr) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) argmax_pair(bv, bi, __shfl_xor(bv, off), __shfl_xor(bi, off));
        if (lane == 0) *code_out = (long long)(bi == 0x7fffffff ? 0 : bi);      // every ratio NaN -> index 0
    }
}

// x [N, D] row-major; tiles: the f32 tile images of dvq_codebook_prepare_f32.  sbuf [N, K] (WANT_S) receives s in phase A and is
// what phase B reads: the soft output itself, or the workspace when only the draw is wanted.  soft: nullptr or == sbuf.
template <int D, bool WANT_DIST, bool WANT_S>
__global__ __launch_bounds__(256, 2) void vq_soft_assign_kernel(
    const float *__restrict__ x, const float *__restrict__ tiles, int K, long N, float temp,
    const float *__restrict__ q, float *soft, float *__restrict__ dist, float *sbuf, long long *__restrict__ codes, int vec)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];   // dvq_exact_lds_bytes(D)

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 31, h = lane >> 5;
    const long n0 = ((long)blockIdx.x * 4 + wave) * 32;          // the wave's first token
    const long nn = (n0 + c < N) ? n0 + c : N - 1;
    const float *zp = x + (size_t)nn * D + h;                    // channel k = 2s + h of token c at zp[2s]

    float zr[D / 2];
#pragma unroll
    for (int s = 0; s < D / 2; ++s) zr[s] = zp[2 * s];

    const int T = dvq_num_tiles(K);
    exact_stage<D>(tiles, 0, lds, wave, lane);

    // ---- xn of token c, then of the 16 tokens of this lane's accumulator rows
    float xnr[16];
    {
        const float xn = exact_token_sumsq<D>(zr, h);
#pragma unroll
        for (int r = 0; r < 16; ++r) xnr[r] = __shfl(xn, (r & 3) + 8 * (r >> 2) + 4 * h);
    }

    float best[16];
    int bt[16];                                      // the tile the best distance was found in (code = 32 tile + c)
#pragma unroll
    for (int r = 0; r < 16; ++r) { best[r] = __builtin_inff(); bt[r] = -1; }
    const long rowh = n0 + 4 * h;                    // accumulator register r: token row rowh + (r&3) + 8(r>>2)

    for (int t = 0; t < T; ++t) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();                      // tile t landed; everyone is done with tile t-1
        float *buf = exact_buf<D>(lds, t);
        if (t + 1 < T) exact_stage<D>(tiles, t + 1, exact_buf<D>(lds, t + 1), wave, lane);

        f32x16 acc;
        exact_tile_dots<D, true>(buf, zr, c, h, acc);
        const float en = buf[32 * D + c];
        const int code = t * 32 + c;
        const bool cvalid = code < K;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int tk = (r & 3) + 8 * (r >> 2);
            const float bias = __fadd_rn(xnr[r], en);
            const float d = __builtin_fmaf(-2.0f, acc[r], bias);   // fl(bias - 2 dot), 2 dot exact
            const bool take = argmin_take(d, best[r]) && cvalid;
            best[r] = take ? d : best[r];
            bt[r] = take ? t : bt[r];
            if (WANT_DIST || WANT_S) {
                if (cvalid && rowh + tk < N) {
                    const size_t off = (size_t)(rowh + tk) * (size_t)K + (size_t)code;
                    if (WANT_DIST) dist[off] = d;
                    if (WANT_S) sbuf[off] = (-d) / temp;
                }
            }
        }
    }

    // ---- merge a token's 32 lanes (one per code column); then hand (distance, code) of the wave's 32 tokens over through LDS
    __syncthreads();                                 // all waves are done with the tile buffers
    float *rb = lds + wave * 32;
    int *ri = (int *)(lds + 128) + wave * 32;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        float b = best[r];
        int i = bt[r] < 0 ? 0x7fffffff : bt[r] * 32 + c;
#pragma unroll
        for (int off = 1; off < 32; off <<= 1) {
            const float ob = __shfl_xor(b, off);
            const int oi = __shfl_xor(i, off);
            argmin_merge(b, i, ob, oi);
        }
        if (c == 0) {
            const int tk = (r & 3) + 8 * (r >> 2) + 4 * h;
            rb[tk] = b;
            ri[tk] = (i == 0x7fffffff) ? 0 : i;      // every distance +inf -> index 0
        }
    }
    __syncthreads();
    const float mybest = rb[c];
    const int mycode = ri[c];
    if (q == nullptr && h == 0 && n0 + c < N) codes[n0 + c] = (long long)mycode;
    if (!WANT_S) return;

    // ---- phase B: the wave normalises its own rows
    __threadfence();                                 // this wave's phase-A stores have landed before any lane reads them back
    for (int tk = 0; tk < 32; ++tk) {
        const long row = n0 + tk;
        if (row >= N) break;
        const float m = (-__shfl(mybest, tk)) / temp;            // the row maximum of s
        const size_t off = (size_t)row * (size_t)K;
        const float *srow = sbuf + off;
        float *prow = soft != nullptr ? soft + off : nullptr;
        const float *qrow = q != nullptr ? q + off : nullptr;
        if (vec) soft_row<4>(srow, prow, qrow, K, m, lane, codes + row);
        else soft_row<1>(srow, prow, qrow, K, m, lane, codes + row);
    }
}

template <int D>
static int launch_soft(const float *x, const float *tiles, int K, long N, float temp, const float *q, float *soft, float *dist,
                       float *sbuf, long long *codes, int vec, hipStream_t st)
{
    const size_t shmem = dvq_exact_lds_bytes(D);
    const dim3 grid((unsigned)((N + 127) / 128)), block(256);
    if (dist != nullptr && sbuf != nullptr)
        return dvq_launch_lds<vq_soft_assign_kernel<D, true, true>>(grid, block, shmem, st, x, tiles, K, N, temp, q, soft, dist, sbuf, codes, vec);
    if (dist != nullptr)
        return dvq_launch_lds<vq_soft_assign_kernel<D, true, false>>(grid, block, shmem, st, x, tiles, K, N, temp, q, soft, dist, sbuf, codes, vec);
    if (sbuf != nullptr)
        return dvq_launch_lds<vq_soft_assign_kernel<D, false, true>>(grid, block, shmem, st, x, tiles, K, N, temp, q, soft, dist, sbuf, codes, vec);
    return dvq_launch_lds<vq_soft_assign_kernel<D, false, false>>(grid, block, shmem, st, x, tiles, K, N, temp, q, soft, dist, sbuf, codes, vec);
}

// sbuf: where phase A parks the scores (soft itself, or the workspace when soft == nullptr and q != nullptr; nullptr: no phase B)
int dvq_launch_soft_assign(const float *x, const float *prep, int D, int K, long N, float temp, const float *q, float *soft,
                           float *dist, float *sbuf, long long *codes, hipStream_t st)
{
    // 16-byte row accesses of phase B: every row start aligned
    const uintptr_t bits = (uintptr_t)sbuf | (uintptr_t)soft | (uintptr_t)q;
    const int vec = (K % 4 == 0) && (bits & 15) == 0;
    switch (D) {
    case 64:  return launch_soft<64>(x, prep, K, N, temp, q, soft, dist, sbuf, codes, vec, st);
    case 128: return launch_soft<128>(x, prep, K, N, temp, q, soft, dist, sbuf, codes, vec, st);
    case 256: return launch_soft<256>(x, prep, K, N, temp, q, soft, dist, sbuf, codes, vec, st);
    default:  return -1000;
    }
}
