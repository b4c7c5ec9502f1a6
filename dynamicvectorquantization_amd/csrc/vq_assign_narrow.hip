// vq_assign_narrow.hip -- bit-exact nearest-codebook assignment at NARROW widths (codebook_dim D = 4, 8, 16) on the vector
// ALUs (gfx950).
//
// Replaces, for taming-style VQModel / VectorQuantizer2 checkpoints (embed_dim 3 or 4, K = 8192 / 16384) and factorised
// low-dimensional codebooks, the same reference ops as vq_assign_exact.hip: VQEmbedding.compute_distances +
// find_nearest_embedding + embed and the forward glue around them (reference modules/vector_quantization/
// quantize2_mask.py:29-55,157-191; quantize_vqgan.py:271-312).
//
// A different regime from the wide kernels: 2 K D flop per token is tiny here (D = 4, K = 16384, N = 262144: 3.4e10 lane
// operations), a 32 x 32 MFMA tile would be mostly zero padding, and the fp16 filter has nothing to win.  So: one plain fp32
// FMA chain per (token, code) on the VALU, every rounding written out (__fmaf_rn / __fadd_rn / __fmul_rn: no contraction or
// reassociation is possible whatever the compiler flags).
//
// Arithmetic contract (oracle/dvq_oracle.c, pinned at these widths by tests/golden/narrow_D*.npz):
//   dot   = acc = 0; acc = fma(z[k], e[k], acc), k ascending
//   xn,en = dvq_oracle_sumsq at D < 32: D <= 8 the sequential sum of the rounded squares; D = 16 t[l] = sq[l] + sq[l + 8],
//           then t[0] + t[1] + ... + t[7] left to right
//   d     = fl(fl(xn + en) - 2 dot);  argmin first index, NaN = minimum
//   z_q   = fl(z + fl(e - z))
//
// Mapping: a workgroup of 128 lanes owns 256 consecutive tokens, two per lane (tokens tid and tid + 128 of the block: every
// code row fetched from LDS serves two chains), the token's D latents in VGPRs.  Up to DVQ_NARROW_SMALL_N tokens that grid
// would leave most of the chip idle (every workgroup walks the whole codebook): one wave of 64 tokens per workgroup then, one
// token per lane.  NCHW: channel plane k is read with lane-consecutive tokens -- coalesced dword loads, any HW, no alignment
// assumed.  Row-major [N, D]: a row is D / 4 16-byte loads (the launcher checks the base pointers).
// The codebook is walked in tiles of 4096 / D codes (16 KiB of rows + their norms: <= 20 KiB of LDS per workgroup, eight
// workgroups per CU by LDS) staged with plain loads, one code per thread, which also computes the code's norm in the order
// above.  All lanes of a wave read the same row: 16-byte LDS broadcast reads.  The last tile is guarded by the code index.
// Epilogue: e = E[code] from global memory, z_q in the input layout, the code as int64, one double loss partial per workgroup
// (summed in a fixed order by vq_loss_finalize_kernel: no float atomics, the same bits every run).
#include "../../include/dvq.h"
#include "launchers.h"

#define NARROW_TILE_FLOATS 4096                        // 16 KiB of codebook rows per tile

// dvq_oracle_sumsq for D in {4, 8, 16}
template <int D>
__device__ __forceinline__ float narrow_sumsq(const float (&v)[D])
{
    if constexpr (D <= 8) {
        float s = sq_rn(v[0]);
#pragma unroll
        for (int k = 1; k < D; ++k) s = __fadd_rn(s, sq_rn(v[k]));
        return s;
    } else {
        static_assert(D == 16, "narrow widths: 4, 8, 16");
        float s = __fadd_rn(sq_rn(v[0]), sq_rn(v[8]));
#pragma unroll
        for (int l = 1; l < 8; ++l) s = __fadd_rn(s, __fadd_rn(sq_rn(v[l]), sq_rn(v[l + 8])));
        return s;
    }
}

// THREADS lanes x TPL tokens per lane = the workgroup's tokens: 128 x 2, or 64 x 1 for small batches
template <int D, bool FLAT, int THREADS, int TPL>
__global__ __launch_bounds__(THREADS) void vq_assign_narrow_kernel(
    const float *__restrict__ z, const float *__restrict__ E, const float *__restrict__ mask, int HW, int K, long N,
    float *__restrict__ zq, long long *__restrict__ codes, double *__restrict__ partials)
{
    constexpr int TILE = NARROW_TILE_FLOATS / D, Q = D / 4, WAVES = THREADS / 64;
    __shared__ __attribute__((aligned(16))) float rows[NARROW_TILE_FLOATS];
    __shared__ __attribute__((aligned(16))) float ens[TILE];
    __shared__ double red[WAVES];
    const int tid = threadIdx.x;

    long n[TPL];
    bool valid[TPL];
    size_t base[TPL];                                  // element offset of channel 0 of the token, in z and in zq
    const size_t stride = FLAT ? 1 : (size_t)HW;
    float zr[TPL][D], xn[TPL], best[TPL];
    int bidx[TPL];
#pragma unroll
    for (int t = 0; t < TPL; ++t) {
        n[t] = (long)blockIdx.x * (THREADS * TPL) + t * THREADS + tid;
        valid[t] = n[t] < N;
        const long nn = valid[t] ? n[t] : N - 1;
        if constexpr (FLAT) {
            base[t] = (size_t)nn * D;
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                const f32x4 v = *(const f32x4 *)(z + base[t] + 4 * q);
                zr[t][4 * q + 0] = v[0]; zr[t][4 * q + 1] = v[1]; zr[t][4 * q + 2] = v[2]; zr[t][4 * q + 3] = v[3];
            }
        } else {
            const long b = nn / HW;
            base[t] = (size_t)b * D * HW + (size_t)(nn - b * HW);
#pragma unroll
            for (int k = 0; k < D; ++k) zr[t][k] = z[base[t] + (size_t)k * HW];
        }
        xn[t] = narrow_sumsq<D>(zr[t]);
        best[t] = __builtin_inff();
        bidx[t] = -1;
    }

    for (int t0 = 0; t0 < K; t0 += TILE) {
        const int cnt = (K - t0 < TILE) ? K - t0 : TILE;
        __syncthreads();                               // everyone is done with the previous tile
        for (int j = tid; j < cnt; j += THREADS) {
            const float *src = E + (size_t)(t0 + j) * D;
            float e[D];
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                const f32x4 v = *(const f32x4 *)(src + 4 * q);
                *(f32x4 *)(rows + j * D + 4 * q) = v;
                e[4 * q + 0] = v[0]; e[4 * q + 1] = v[1]; e[4 * q + 2] = v[2]; e[4 * q + 3] = v[3];
            }
            ens[j] = narrow_sumsq<D>(e);
        }
        __syncthreads();
        // four codes per step: one 16-byte read of their norms; rows [cnt, TILE) of the last tile hold stale bytes and are
        // refused by the index test (j0 + 3 < TILE always: TILE is a multiple of 4)
        for (int j0 = 0; j0 < cnt; j0 += 4) {
            const f32x4 en4 = *(const f32x4 *)(ens + j0);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = j0 + u;
                float e[D];
#pragma unroll
                for (int q = 0; q < Q; ++q) {
                    const f32x4 v = *(const f32x4 *)(rows + j * D + 4 * q);
                    e[4 * q + 0] = v[0]; e[4 * q + 1] = v[1]; e[4 * q + 2] = v[2]; e[4 * q + 3] = v[3];
                }
#pragma unroll
                for (int t = 0; t < TPL; ++t) {
                    float acc = 0.0f;
#pragma unroll
                    for (int k = 0; k < D; ++k) acc = __fmaf_rn(zr[t][k], e[k], acc);
                    const float bias = __fadd_rn(xn[t], en4[u]);
                    const float d = __fmaf_rn(-2.0f, acc, bias);          // fl(bias - 2 dot), 2 dot exact
                    const bool take = argmin_take(d, best[t]) && (j < cnt);
                    best[t] = take ? d : best[t];
                    bidx[t] = take ? t0 + j : bidx[t];
                }
            }
        }
    }

    // ---- codes, z_q = z + (e - z), loss partial sum((e - z)^2 * m)
    double block_sum = 0.0;
#pragma unroll
    for (int t = 0; t < TPL; ++t) {
        const int code = bidx[t] < 0 ? 0 : bidx[t];    // every distance +inf -> index 0
        if (!valid[t]) continue;
        codes[n[t]] = (long long)code;
        if (zq == nullptr && partials == nullptr) continue;
        const float *ep = E + (size_t)code * D;        // from global memory: the tile that held it is long gone
        const float m = (mask != nullptr) ? mask[n[t]] : 1.0f;
        float lsum = 0.0f;
        float out[D];
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const f32x4 v = *(const f32x4 *)(ep + 4 * q);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int k = 4 * q + i;
                const float diff = __fsub_rn(v[i], zr[t][k]);
                out[k] = __fadd_rn(zr[t][k], diff);
                lsum = __fadd_rn(lsum, __fmul_rn(__fmul_rn(diff, diff), m));
            }
        }
        if (zq != nullptr) {
            if constexpr (FLAT) {
#pragma unroll
                for (int q = 0; q < Q; ++q) {
                    const f32x4 v = {out[4 * q], out[4 * q + 1], out[4 * q + 2], out[4 * q + 3]};
                    *(f32x4 *)(zq + base[t] + 4 * q) = v;
                }
            } else {
#pragma unroll
                for (int k = 0; k < D; ++k) zq[base[t] + (size_t)k * stride] = out[k];
            }
        }
        block_sum += (double)lsum;
    }
    if (partials != nullptr) {                         // uniform: a kernel argument
        double ds = block_sum;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) ds += __shfl_xor(ds, off);
        if ((tid & 63) == 0) red[tid >> 6] = ds;
        __syncthreads();
        if (tid == 0) partials[blockIdx.x] = WAVES == 2 ? red[0] + red[1] : red[0];
    }
}

// ---------------------------------------------------------------------------------------------
// host launchers (called from dvq_abi.hip)
// ---------------------------------------------------------------------------------------------
int dvq_narrow_tile_codes(int D) { return (D == 4 || D == 8 || D == 16) ? NARROW_TILE_FLOATS / D : 0; }

static int narrow_block_tokens(long N) { return N <= DVQ_NARROW_SMALL_N ? 64 : 256; }

// workgroups = loss partials of a call with N tokens
int dvq_narrow_blocks(long N) { return (int)((N + narrow_block_tokens(N) - 1) / narrow_block_tokens(N)); }

template <int D, bool FLAT>
static int launch_narrow_form(const float *z, const float *E, const float *mask, int HW, int K, long N, float *zq, long long *codes,
                              double *partials, hipStream_t st)
{
    const dim3 grid((unsigned)dvq_narrow_blocks(N));
    if (narrow_block_tokens(N) == 64)
        hipLaunchKernelGGL((vq_assign_narrow_kernel<D, FLAT, 64, 1>), grid, dim3(64), 0, st, z, E, mask, HW, K, N, zq, codes, partials);
    else
        hipLaunchKernelGGL((vq_assign_narrow_kernel<D, FLAT, 128, 2>), grid, dim3(128), 0, st, z, E, mask, HW, K, N, zq, codes, partials);
    return (int)hipGetLastError();
}

template <int D>
static int launch_narrow(const float *z, const float *E, const float *mask, int HW, int K, long N, bool flat, float *zq,
                         long long *codes, double *partials, hipStream_t st)
{
    return flat ? launch_narrow_form<D, true>(z, E, mask, 1, K, N, zq, codes, partials, st)
                : launch_narrow_form<D, false>(z, E, mask, HW, K, N, zq, codes, partials, st);
}

// flat: z / zq are row-major [N, D] and 16-byte aligned (checked by the caller, as is E's alignment); else [B, D, HW]
int dvq_launch_narrow(const float *z, const float *E, const float *mask, int D, int HW, int K, long N, bool flat, float *zq,
                      long long *codes, double *partials, hipStream_t st)
{
    switch (D) {
    case 4:  return launch_narrow<4>(z, E, mask, HW, K, N, flat, zq, codes, partials, st);
    case 8:  return launch_narrow<8>(z, E, mask, HW, K, N, flat, zq, codes, partials, st);
    case 16: return launch_narrow<16>(z, E, mask, HW, K, N, flat, zq, codes, partials, st);
    default: return -1000;
    }
}
