// vq_sample.hip -- scored / temperature-sampled code assignment and quantisation from given codes (gfx950): the learnable-codebook
// quantizers MaskVectorQuantize / VectorQuantize.
//
// Replaces (reference modules/vector_quantization/quantize_codebook_mask.py:97-121, quantize.py:92-119, common_utils.py:19-35):
// the [N, K] score matrix `dist` (L2: -sum x^2 - sum e^2 + 2 x E^T; cosine similarity: x_n E_n^T), `dist / temp`, the uniform
// noise's two logs and two clamps, the add and the argmax -- about ten passes over N x K floats -- by ONE sweep that reads the
// caller-drawn uniforms once and writes N codes; then the embedding gather, the (masked) loss and the straight-through add by one
// streaming kernel.
//
// vq_score_assign_kernel: built on the exact-chain tile loop's pieces (dvq_exact_tile.h; codes in rows, so the running argmax is
// lane-local), every dot the same bits as the hard assign's.  The tokens are read in place from NCHW [B, D, HW], or from row-major
// [N, D] as the case HW == 1.  What this kernel adds: a score per metric, and the noise -- a lane's 16 codes of a tile are four
// runs of four consecutive codes, so it fetches its 16 uniforms as four 16-byte loads of row c of u, issued before the stage and
// the MFMA chain that hide them.
//   score   L2:  s = -d, d = fl(fl(xn + en) - 2 dot) (ATen-order norms): the reference's expression negated, bit for bit
//           DOT: s = dot (operands L2-normalised by the caller)
//           CDIST: s = -sqrtf(d < 0 ? 0 : d), d as L2 (quantize_lucidrains.py:123, `-torch.cdist`): the square root does not commute
//                  with the noise, so the sampled code of the lucidrains-style codebook needs a score of its own; a NaN d stays NaN
//   u == nullptr: code = argmax s;  u given: code = argmax fl(fl(s / temp) + g), g = -logf(max(-logf(max(u, 1e-20f)), 1e-20f))
//   argmax with torch's rules: the first index among equal maxima, a NaN is the maximum and the first NaN wins.
// Nothing of size N x K is written; no workspace; no atomics.
//
// vq_apply_codes_kernel: z_q = fl(z + fl(e - z)) and the loss partial sum((e - z)^2 m) of given codes, the arithmetic of the exact
// assign's tail (vq_assign_exact.hip) in the streaming form of vq_backward.hip; double partials, one per workgroup, finalised in a
// fixed order by vq_loss_finalize_kernel.
#include "../../include/dvq.h"
#include "launchers.h"
#include "dvq_exact_tile.h"

// the METRIC of the kernel template: dvq.h's DVQ_METRIC_L2 / DVQ_METRIC_DOT, and one more that is internal to this unit
#define SCORE_INTERNAL_CDIST 2   // s = -sqrt(max(d, 0)): torch.cdist's score (dvq_vq_cdist_sample_assign_f32 only; not a value of the ABI's `metric`)
static_assert(SCORE_INTERNAL_CDIST != DVQ_METRIC_L2 && SCORE_INTERNAL_CDIST != DVQ_METRIC_DOT, "the internal metric must not collide");

// the reference's gumbel_noise of one uniform (common_utils.py:19-29): -log(clamp(-log(clamp(u, 1e-20)), 1e-20))
__device__ __forceinline__ float gumbel_of(float u)
{
    const float a = -logf(fmaxf(u, 1e-20f));
    return -logf(fmaxf(a, 1e-20f));
}

// NOISE: u [N, K] given.  VEC: K % 4 == 0 and u 16-byte aligned -- a lane's four codes of a run sit in one aligned 16-byte piece.
template <int D, int METRIC, bool NOISE, bool VEC>
__global__ __launch_bounds__(256, 2) void vq_score_assign_kernel(
    const float *__restrict__ z, const float *__restrict__ tiles, int HW, int K, long N, float temp,
    const float *__restrict__ u, long long *__restrict__ codes)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];   // dvq_exact_lds_bytes(D)

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 31, h = lane >> 5;
    const long n = ((long)blockIdx.x * 4 + wave) * 32 + c;
    const bool valid = n < N;
    const long nn = valid ? n : N - 1;               // lanes past the end re-read the last token; they store nothing
    const long b = nn / HW;
    float zr[D / 2];
    exact_load_token_nchw<D>(z, HW, b, nn, h, zr);

    const int T = dvq_num_tiles(K);
    exact_stage<D>(tiles, 0, lds, wave, lane);

    float xn = 0.0f;                                 // the DOT metric has no norms
    if constexpr (METRIC != DVQ_METRIC_DOT) xn = exact_token_sumsq<D>(zr, h);

    float best = -__builtin_inff();
    int bidx = 0x7fffffff;
    const float *urow = NOISE ? u + (size_t)nn * (size_t)K : nullptr;

    for (int t = 0; t < T; ++t) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();                      // tile t landed; everyone is done with tile t-1
        float *buf = exact_buf<D>(lds, t);

        // this tile's uniforms of the lane's token: in flight under the MFMA chain
        float uu[16];
        if constexpr (NOISE) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int code0 = exact_code_of(t, g, 0, h);
                if constexpr (VEC) {
                    f32x4 v = {0.5f, 0.5f, 0.5f, 0.5f};
                    if (code0 < K) v = __builtin_nontemporal_load((const f32x4 *)(urow + code0));     // K % 4 == 0: all four < K
                    uu[4 * g + 0] = v[0]; uu[4 * g + 1] = v[1]; uu[4 * g + 2] = v[2]; uu[4 * g + 3] = v[3];
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        uu[4 * g + q] = (code0 + q < K) ? __builtin_nontemporal_load(urow + code0 + q) : 0.5f;
                }
            }
        }
        if (t + 1 < T) exact_stage<D>(tiles, t + 1, exact_buf<D>(lds, t + 1), wave, lane);

        f32x16 acc;
        exact_tile_dots<D>(buf, zr, c, h, acc);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            f32x4 en4 = {0.0f, 0.0f, 0.0f, 0.0f};
            if constexpr (METRIC != DVQ_METRIC_DOT) en4 = exact_tile_en4<D>(buf, h, g);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int r = g * 4 + q;
                const int code = exact_code_of(t, g, q, h);
                float s;
                if constexpr (METRIC == DVQ_METRIC_L2) {
                    const float bias = __fadd_rn(xn, en4[q]);
                    s = -__builtin_fmaf(-2.0f, acc[r], bias);    // -(fl(bias - 2 dot)), 2 dot exact
                } else if constexpr (METRIC == SCORE_INTERNAL_CDIST) {
                    const float d = __builtin_fmaf(-2.0f, acc[r], __fadd_rn(xn, en4[q]));
                    s = -__fsqrt_rn(d < 0.0f ? 0.0f : d);        // (the conditional keeps a NaN; fmaxf would not)
                } else {
                    s = acc[r];
                }
                if constexpr (NOISE) s = __fadd_rn(s / temp, gumbel_of(uu[r]));
                const bool take = argmax_take(s, best) && (code < K);
                best = take ? s : best;
                bidx = take ? code : bidx;
            }
        }
    }

    const int code = exact_merge_halves_argmax(best, bidx);
    if (valid && h == 0) codes[n] = (long long)code;
}

template <int D, int METRIC>
static int launch_score(const float *z, const float *tiles, int HW, int K, long N, float temp, const float *u, long long *codes,
                        int vec, hipStream_t st)
{
    const size_t shmem = dvq_exact_lds_bytes(D);
    const dim3 grid((unsigned)((N + 127) / 128)), block(256);
    if (u == nullptr)
        return dvq_launch_lds<vq_score_assign_kernel<D, METRIC, false, false>>(grid, block, shmem, st, z, tiles, HW, K, N, temp, u, codes);
    if (vec)
        return dvq_launch_lds<vq_score_assign_kernel<D, METRIC, true, true>>(grid, block, shmem, st, z, tiles, HW, K, N, temp, u, codes);
    return dvq_launch_lds<vq_score_assign_kernel<D, METRIC, true, false>>(grid, block, shmem, st, z, tiles, HW, K, N, temp, u, codes);
}

// z [B, D, HW] (HW == 1: row-major [N, D]); prep: the f32 tile images; u nullable [N, K]
int dvq_launch_score_assign(const float *z, const float *prep, int D, int HW, int K, long N, int metric, float temp, const float *u,
                            long long *codes, hipStream_t st)
{
    const int vec = (K % 4 == 0) && ((uintptr_t)u & 15) == 0;     // 16-byte pieces of a row of u: every row start aligned
    const bool dot = metric == DVQ_METRIC_DOT;
    switch (D) {
    case 64:  return dot ? launch_score<64, DVQ_METRIC_DOT>(z, prep, HW, K, N, temp, u, codes, vec, st)
                         : launch_score<64, DVQ_METRIC_L2>(z, prep, HW, K, N, temp, u, codes, vec, st);
    case 128: return dot ? launch_score<128, DVQ_METRIC_DOT>(z, prep, HW, K, N, temp, u, codes, vec, st)
                         : launch_score<128, DVQ_METRIC_L2>(z, prep, HW, K, N, temp, u, codes, vec, st);
    case 256: return dot ? launch_score<256, DVQ_METRIC_DOT>(z, prep, HW, K, N, temp, u, codes, vec, st)
                         : launch_score<256, DVQ_METRIC_L2>(z, prep, HW, K, N, temp, u, codes, vec, st);
    default:  return -1000;
    }
}

// the sampled assign against -cdist (u required): the CDIST score of the same template
int dvq_launch_cdist_sample_assign(const float *z, const float *prep, int D, int HW, int K, long N, float temp, const float *u,
                                   long long *codes, hipStream_t st)
{
    const int vec = (K % 4 == 0) && ((uintptr_t)u & 15) == 0;
    switch (D) {
    case 64:  return launch_score<64, SCORE_INTERNAL_CDIST>(z, prep, HW, K, N, temp, u, codes, vec, st);
    case 128: return launch_score<128, SCORE_INTERNAL_CDIST>(z, prep, HW, K, N, temp, u, codes, vec, st);
    case 256: return launch_score<256, SCORE_INTERNAL_CDIST>(z, prep, HW, K, N, temp, u, codes, vec, st);
    default:  return -1000;
    }
}

// ---------------------------------------------------------------------------------------------
// quantise from given codes: z_q = z + (e - z), loss partials
// ---------------------------------------------------------------------------------------------
// Mapping as vq_backward.hip: a wave owns 32 consecutive tokens, lane = (token, half); per step of 16 channels a lane handles 8
// (two 16-byte gathers of its code's row, 8 loads / stores whose wave instructions cover 128-byte runs of NCHW).  A code outside
// [0, K) leaves its token unquantised (z_q = z) and adds nothing to the loss.
__global__ __launch_bounds__(256) void vq_apply_codes_kernel(
    const float *__restrict__ z, const float *__restrict__ E, const long long *__restrict__ codes,
    const float *__restrict__ mask, int D, int HW, int K, long N, float *__restrict__ zq, double *__restrict__ partials)
{
    __shared__ double red[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = lane & 31, h = lane >> 5;
    const long n = ((long)blockIdx.x * 4 + wave) * 32 + c;
    float lsum = 0.0f;
    if (n < N) {
        const long b = n / HW;
        const int hw = (int)(n - b * HW);
        const size_t base = ((size_t)b * D + 8 * h) * HW + hw;
        const long long cj = codes[n];
        const bool ok = cj >= 0 && cj < K;
        const float *ep = E + (size_t)(ok ? cj : 0) * D + 8 * h;
        const float m = (mask != nullptr) ? mask[n] : 1.0f;
        const float *zp = z + base;
        float *op = (zq != nullptr) ? zq + base : nullptr;
        const int S16 = D / 16;
#pragma unroll 2
        for (int s = 0; s < S16; ++s) {
            const f32x4 e0 = *(const f32x4 *)(ep + 16 * s), e1 = *(const f32x4 *)(ep + 16 * s + 4);
            float zz[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) zz[j] = __builtin_nontemporal_load(zp + (size_t)(16 * s + j) * HW);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float e = (j < 4) ? e0[j & 3] : e1[j & 3];
                const float diff = ok ? __fsub_rn(e, zz[j]) : 0.0f;
                if (op != nullptr) __builtin_nontemporal_store(__fadd_rn(zz[j], diff), op + (size_t)(16 * s + j) * HW);
                lsum = __fadd_rn(lsum, __fmul_rn(__fmul_rn(diff, diff), m));
            }
        }
    }
    if (partials != nullptr) {                   // (uniform: a kernel argument)
        double ds = (double)lsum;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) ds += __shfl_xor(ds, off);
        if (lane == 0) red[wave] = ds;
        __syncthreads();
        if (threadIdx.x == 0) partials[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
    }
}

int dvq_apply_codes_blocks(long N) { return (int)((N + 127) / 128); }

int dvq_launch_apply_codes(const float *z, const float *E, const long long *codes, const float *mask, int D, int HW, int K, long N,
                           float *zq, double *partials, hipStream_t st)
{
    hipLaunchKernelGGL(vq_apply_codes_kernel, dim3((unsigned)dvq_apply_codes_blocks(N)), dim3(256), 0, st, z, E, codes, mask, D, HW,
                       K, N, zq, partials);
    return (int)hipGetLastError();
}
