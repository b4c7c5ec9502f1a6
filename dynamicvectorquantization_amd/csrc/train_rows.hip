// train_rows.hip -- the training-side kernels for ROW-MAJOR latents [N, D] (gfx950): token rows as VectorQuantize2(channel_last=True),
// VectorQuantize2List, VQEmbedding.forward and every depth of RQBottleneck hand them over, and a channels_last (NHWC) image map,
// which is the same bytes.  vq_backward.hip and ema_update.hip hold the NCHW forms; run on rows with HW = 1 those give every lane
// a cache line of its own (lane = token, channel stride HW), and the EMA statistics had no row form at all.
//
//   vq_backward_rows_kernel   g_z = g_zq + (g_loss coef) ((z - e) m): lane = one 16-byte piece of a token's row (4 floats / 8 halves),
//                             so a wave instruction covers 1 KiB of consecutive memory -- one D = 256 f32 row, four D = 64 rows; the
//                             code's row is gathered in the same pieces.  z, g_zq and g_z move once, non-temporal: 12 (6) bytes per
//                             element, HBM-bound.  The fp32 expression and its operation order are vq_backward_z_kernel's.
//   rows_scatter_kernel       the per-code sums: EMA statistics (cluster_size, vectors_sum) or the codebook gradient.  A workgroup takes
//                             64 consecutive tokens, lane = channel: a wave reads 64 consecutive channels of one token (256 contiguous
//                             bytes) -- already the row shape the float atomics want, so there is no LDS transpose, no LDS at all and
//                             no barrier.  Equal codes of the tile are summed first and reach memory as ONE row of atomics (ema_update.hip
//                             records what skewed code usage costs without that): every wave holds the tile's 64 codes, lane = token;
//                             the members of token t's class are ballot(code == code_t) and t leads its class iff it is the lowest
//                             member, so there is no [K] table either and K has no limit.
#include "launchers.h"

template <int XT>
__global__ __launch_bounds__(256) void vq_backward_rows_kernel(
    const void *__restrict__ zv, const float *__restrict__ E, const long long *__restrict__ codes, const float *__restrict__ mask,
    const void *__restrict__ gv, const float *__restrict__ g_loss, float coef_scale, int D, int K, long N, void *__restrict__ ov)
{
    constexpr int PE = XT ? 8 : 4;                           // elements of a 16-byte piece
    constexpr int U = 4;                                     // pieces per lane, 256 lanes apart
    const int ppr = D / PE;                                  // pieces per row
    const long total = N * ppr;
    const long p0 = (long)blockIdx.x * (U * 256) + threadIdx.x;
    if (p0 >= total) return;
    const long n0 = p0 / ppr;
    const int r0 = (int)(p0 - n0 * ppr);
    const u32x4 *z4 = (const u32x4 *)zv, *g4 = (const u32x4 *)gv;
    u32x4 *o4 = (u32x4 *)ov;
    const float gl = (g_loss != nullptr) ? g_loss[0] : 0.0f;
    u32x4 zz[U], gg[U];
    f32x4 e[U][PE / 4];
    float m[U], c0[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {                            // every load first (a piece past the end repeats the last one)
        const long p = (p0 + u * 256 < total) ? p0 + u * 256 : total - 1;
        const int r = r0 + (int)(p - p0);
        const long n = n0 + r / ppr;
        const int col = (r % ppr) * PE;
        zz[u] = __builtin_nontemporal_load(z4 + p);
        gg[u] = (g4 != nullptr) ? __builtin_nontemporal_load(g4 + p) : u32x4{0u, 0u, 0u, 0u};
        const long long cj = codes[n];
        const bool ok = cj >= 0 && cj < K;                   // (the forward writes valid codes; anything else: no loss term)
        const float *ep = E + (size_t)(ok ? cj : 0) * D + col;
#pragma unroll
        for (int q = 0; q < PE / 4; ++q) e[u][q] = *(const f32x4 *)(ep + 4 * q);
        m[u] = (mask != nullptr) ? mask[n] : 1.0f;
        c0[u] = (g_loss != nullptr && ok) ? __fmul_rn(gl, coef_scale) : 0.0f;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        if (p0 + u * 256 >= total) break;
        u32x4 out;
        if constexpr (XT == 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned zw = zz[u][j], gw = gg[u][j];  // (scalars first: a bit cast of a vector element reads element 0)
                const float zf = __builtin_bit_cast(float, zw);
                const float gf = (g4 != nullptr) ? __builtin_bit_cast(float, gw) : 0.0f;
                const float diff = __fmul_rn(__fsub_rn(zf, e[u][0][j]), m[u]);
                out[j] = __builtin_bit_cast(unsigned, __fadd_rn(gf, __fmul_rn(c0[u], diff)));
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {                    // word j = elements 2j (low half) and 2j + 1
                const unsigned zw = zz[u][j], gw = gg[u][j];
                unsigned w = 0u;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int i = 2 * j + h;
                    const float zf = dvq_widen_bits<XT>((unsigned short)(zw >> (16 * h)));
                    const float gf = (g4 != nullptr) ? dvq_widen_bits<XT>((unsigned short)(gw >> (16 * h))) : 0.0f;
                    const float diff = __fmul_rn(__fsub_rn(zf, e[u][i >> 2][i & 3]), m[u]);
                    w |= (unsigned)dvq_narrow_bits<XT>(__fadd_rn(gf, __fmul_rn(c0[u], diff))) << (16 * h);
                }
                out[j] = w;
            }
        }
        __builtin_nontemporal_store(out, o4 + p0 + u * 256);
    }
}

// D % 16 == 0 and z, g_zq, gz, E 16-byte aligned (the ABI checks); xt as dvq_launch_vq_backward_z
int dvq_launch_vq_backward_rows(const void *z, int xt, const float *E, const long long *codes, const float *mask, const void *g_zq,
                                const float *g_loss, float coef_scale, int D, int K, long N, void *gz, hipStream_t st)
{
    if (xt < 0 || xt > 2 || D % 16 != 0) return -1000;
    const long total = N * (D / (xt ? 8 : 4));
    const dim3 grid((unsigned)((total + 1023) / 1024));
    if (xt == 0)
        hipLaunchKernelGGL(vq_backward_rows_kernel<0>, grid, dim3(256), 0, st, z, E, codes, mask, g_zq, g_loss, coef_scale, D, K, N, gz);
    else if (xt == 1)
        hipLaunchKernelGGL(vq_backward_rows_kernel<1>, grid, dim3(256), 0, st, z, E, codes, mask, g_zq, g_loss, coef_scale, D, K, N, gz);
    else
        hipLaunchKernelGGL(vq_backward_rows_kernel<2>, grid, dim3(256), 0, st, z, E, codes, mask, g_zq, g_loss, coef_scale, D, K, N, gz);
    return (int)hipGetLastError();
}

// GRAD = false: cluster_size[j] += #tokens of code j, sums[j, :] += their vectors (EMA statistics; E, mask, g_loss unused).
// GRAD = true:  sums[j, :] += c * sum over those tokens of (z - E[j]) m, c = -(g_loss coef_scale) (the codebook gradient; no counts).
// Per-element loads: any D, any alignment of the element type.
template <int XT, bool GRAD>
__global__ __launch_bounds__(256) void rows_scatter_kernel(const typename DvqLat<XT>::T *__restrict__ z, const long long *__restrict__ codes,
                                                           const float *__restrict__ E, const float *__restrict__ mask,
                                                           const float *__restrict__ g_loss, float coef_scale, int D, long N, int K,
                                                           float *__restrict__ cluster_size, float *__restrict__ sums)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long tok0 = (long)blockIdx.x * 64;
    const long n = tok0 + lane;                               // lane = token while the classes are formed
    int code = -1;
    float mval = 1.0f;
    if (n < N) {
        const long long cj = codes[n];
        if (cj >= 0 && cj < K) {
            code = (int)cj;
            if (GRAD && mask != nullptr) mval = mask[n];
        }
    }
    const float c = GRAD ? -__fmul_rn(g_loss[0], coef_scale) : 0.0f;
    for (int i = 0; i < 16; ++i) {                            // wave w leads tokens 16 w + i: lane = channel from here on
        const int tk = 16 * wave + i;
        const int cj = __builtin_amdgcn_readfirstlane(__shfl(code, tk));
        if (cj < 0) continue;
        const unsigned long long members = __ballot(code == cj);
        if (__builtin_ctzll(members) != tk) continue;         // an earlier token of the tile leads this code
        if (!GRAD && lane == 0) atomicAdd(&cluster_size[cj], (float)__popcll(members));
        for (int cb = 0; cb < D; cb += 256) {                 // four 64-channel runs at a time: independent loads per member
            float e[4], sum[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int ch = cb + 64 * u + lane;
                e[u] = (GRAD && ch < D) ? E[(size_t)cj * D + ch] : 0.0f;
                sum[u] = 0.0f;
            }
            unsigned long long mm = members;
            while (mm) {
                const int t = __builtin_ctzll(mm);
                mm &= mm - 1;
                const typename DvqLat<XT>::T *row = z + (size_t)(tok0 + t) * D;
                const float mt = GRAD ? __shfl(mval, t) : 1.0f;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int ch = cb + 64 * u + lane;
                    if (ch < D) {
                        const float v = dvq_widen<XT>(row[ch]);
                        sum[u] += GRAD ? (v - e[u]) * mt : v;
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int ch = cb + 64 * u + lane;
                if (ch < D) atomicAdd(&sums[(size_t)cj * D + ch], GRAD ? c * sum[u] : sum[u]);
            }
        }
    }
}

// overwrites cluster_size [K] and vectors_sum [K, D]
int dvq_launch_ema_accumulate_rows(const void *z, int xt, const long long *codes, int D, long N, int K, float *cluster_size,
                                   float *vectors_sum, hipStream_t st)
{
    if (xt < 0 || xt > 2) return -1000;
    if (int rc = dvq_launch_ema_zero(cluster_size, (size_t)K, vectors_sum, (size_t)K * D, st)) return rc;
    if (xt == 0) {                                           // many tokens, few codes: the big sorted tile of ema_update.hip
        const int rc = dvq_launch_ema_accumulate_sorted_rows((const float *)z, codes, D, N, K, cluster_size, vectors_sum, st);
        if (rc != -1) return rc;
    }
    const dim3 grid((unsigned)((N + 63) / 64));
    if (xt == 0)
        hipLaunchKernelGGL((rows_scatter_kernel<0, false>), grid, dim3(256), 0, st, (const float *)z, codes, nullptr, nullptr, nullptr, 0.0f,
                           D, N, K, cluster_size, vectors_sum);
    else if (xt == 1)
        hipLaunchKernelGGL((rows_scatter_kernel<1, false>), grid, dim3(256), 0, st, (const _Float16 *)z, codes, nullptr, nullptr, nullptr,
                           0.0f, D, N, K, cluster_size, vectors_sum);
    else
        hipLaunchKernelGGL((rows_scatter_kernel<2, false>), grid, dim3(256), 0, st, (const __bf16 *)z, codes, nullptr, nullptr, nullptr,
                           0.0f, D, N, K, cluster_size, vectors_sum);
    return (int)hipGetLastError();
}

// accumulates into gw [>= K rows, D]
int dvq_launch_codebook_grad_rows(const float *z, const float *E, const long long *codes, const float *mask, const float *g_loss,
                                  float coef_scale, int D, long N, int K, float *gw, hipStream_t st)
{
    hipLaunchKernelGGL((rows_scatter_kernel<0, true>), dim3((unsigned)((N + 63) / 64)), dim3(256), 0, st, z, codes, E, mask, g_loss,
                       coef_scale, D, N, K, nullptr, gw);
    return (int)hipGetLastError();
}
