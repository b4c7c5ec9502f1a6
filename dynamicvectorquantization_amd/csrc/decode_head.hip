// decode_head.hip -- codes -> the input of the decoder's conv_in, in one kernel (gfx950).
//
// Replaces, after permuter.forward_back (reference models/stage2_dynamic/dqtransformer_uncond_entropy.py:174-178,
// models/stage1_dynamic/dqvae_triple_feat.py:84-87):
//   quantize.get_codebook_entry(codes)            E[codes]  [B, H, W, D]            (quantize2_mask.py:207-210)
//   .permute(0, 3, 1, 2)                          a non-contiguous NCHW view
//   post_quant_conv (1x1, D -> C)                 (dqvae_dual_entropy.py:137)
//   position_bias_fourier, position_bias_learned  h + sin(conv1x1(coord)), then + (col_embed[x] + row_embed[y])
//                                                 (modules/dynamic_modules/DecoderPositional.py:109-118)
// The 1x1 conv acts per pixel, so conv(E[code]) is row `code` of the table T = E W^T + b (decode_table_kernel, built once
// per (codebook, conv) pair); the two position biases do not depend on the input, so they are two [C, HW] tables.  What is
// left is  h_in[b, c, p] = fl(fl(T[codes[b, p], c] + F[c, p]) + L[c, p]):  a row gather and a transpose.
//
// decode_head_kernel: a workgroup of 256 threads owns 64 consecutive tokens (of the flat [B * HW] order) x 64 channels.
//   gather   16 lanes read the 256-byte channel slab of one token's table row with one 16-byte load each (the table is
//            L2-resident: 1 MiB at K = 1024) and write it into an LDS tile [token][channel], leading dimension 65 words;
//   turn     a lane reads 4 consecutive tokens of one channel: banks (4g + i + c) mod 64 are distinct over the wave's
//            16 token groups x 4 channels (ld 65; at ld 64 the 16 groups of a channel would meet on 4 banks), as are the
//            banks (t + 4q + j) of the gather's writes;
//   stream   F and L are read and h_in is written with 16 bytes per lane along the token axis, 256 contiguous bytes per
//            16 lanes, when HW % 4 == 0 and the three bases are 16-byte aligned; else lane = token with 4-byte accesses.
// The grid is (ceil(B * HW / 64), ceil(C / 64)): sized from B * HW * C, so B = 16 still gives 1024 workgroups at C = 256.
#include "launchers.h"

typedef float dh_f32x4 __attribute__((ext_vector_type(4)));

constexpr int DH_TOK = 64;     // tokens per workgroup
constexpr int DH_CH = 64;      // channels per workgroup
constexpr int DH_LD = 65;      // leading dimension of the LDS tile, in words
constexpr int DT_ROWS = 8;     // table rows per workgroup of decode_table_kernel

// non-temporal output stores (h_in is consumed by another kernel and is far larger than L2): -DDVQ_DECODE_NT=0 for the A/B
#ifndef DVQ_DECODE_NT
#define DVQ_DECODE_NT 1
#endif

template <typename V>
__device__ __forceinline__ void dh_store(V *p, V v)
{
#if DVQ_DECODE_NT
    __builtin_nontemporal_store(v, p);
#else
    *p = v;
#endif
}

template <bool VEC>
__global__ __launch_bounds__(256) void decode_head_kernel(const long long *__restrict__ codes, int N, int HW,
                                                          const float *__restrict__ T, int rows, int C,
                                                          const float *__restrict__ F, const float *__restrict__ L,
                                                          float *__restrict__ out)
{
    __shared__ float tile[DH_TOK * DH_LD];
    const int tid = threadIdx.x;
    const int n0 = blockIdx.x * DH_TOK, c0 = blockIdx.y * DH_CH;
    const float nan = __builtin_nanf("");

    // the position tables do not depend on the codes: their loads are issued ahead of the gather and land under it
    dh_f32x4 pf[DH_CH / 16], pl[DH_CH / 16];
    if (VEC) {
        const int n = n0 + 4 * (tid & 15);
        if (n < N) {
            const int hw = n % HW;
#pragma unroll
            for (int p = 0; p < DH_CH / 16; ++p) {
                const int c = c0 + p * 16 + (tid >> 4);
                const size_t pos = (size_t)c * HW + hw;
                if (F && c < C) pf[p] = *reinterpret_cast<const dh_f32x4 *>(F + pos);
                if (L && c < C) pl[p] = *reinterpret_cast<const dh_f32x4 *>(L + pos);
            }
        }
    }

    // gather: 16 tokens per pass, 16 lanes x 16 bytes per token
    {
        const int q = tid & 15, tr = tid >> 4;
        const int c = c0 + 4 * q;
#pragma unroll
        for (int p = 0; p < DH_TOK / 16; ++p) {
            const int t = p * 16 + tr, n = n0 + t;
            if (n < N && c < C) {
                const long long code = codes[n];
                dh_f32x4 v = {nan, nan, nan, nan};
                if (code >= 0 && code < rows) v = *reinterpret_cast<const dh_f32x4 *>(T + (size_t)code * C + c);
                float *w = tile + t * DH_LD + 4 * q;
                w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
            }
        }
    }
    __syncthreads();

    if (VEC) {                                               // HW % 4 == 0: the 4 tokens of a group lie in one image
        const int g = tid & 15, cr = tid >> 4;
        const int n = n0 + 4 * g;
        if (n >= N) return;
        const int b = n / HW, hw = n - b * HW;
        const float *tl = tile + 4 * g * DH_LD;
#pragma unroll
        for (int p = 0; p < DH_CH / 16; ++p) {
            const int cl = p * 16 + cr, c = c0 + cl;
            if (c >= C) break;
            dh_f32x4 v = {tl[cl], tl[DH_LD + cl], tl[2 * DH_LD + cl], tl[3 * DH_LD + cl]};
            if (F) v = v + pf[p];
            if (L) v = v + pl[p];
            dh_store(reinterpret_cast<dh_f32x4 *>(out + ((size_t)b * C + c) * HW + hw), v);
        }
    } else {                                                 // lane = token, one channel per wave and pass
        const int t = tid & 63, cr = tid >> 6;
        const int n = n0 + t;
        if (n >= N) return;
        const int b = n / HW, hw = n - b * HW;
        for (int p = 0; p < DH_CH / 4; ++p) {
            const int cl = p * 4 + cr, c = c0 + cl;
            if (c >= C) break;
            float v = tile[t * DH_LD + cl];
            const size_t pos = (size_t)c * HW + hw;
            if (F) v = v + F[pos];
            if (L) v = v + L[pos];
            dh_store(out + ((size_t)b * C + c) * HW + hw, v);
        }
    }
}

// T[r, o] = fl(chain_k fma(W[o, k], E[r, k], .) + b[o]), k ascending from 0: one thread per output channel, DT_ROWS rows per
// workgroup so that a weight row is read once for 8 outputs; the codebook rows sit in LDS and are read as broadcasts.
// No atomics and one summation order: the same bits every run.
__global__ __launch_bounds__(256) void decode_table_kernel(const float *__restrict__ E, int rows, int D,
                                                           const float *__restrict__ W, const float *__restrict__ bias, int C,
                                                           float *__restrict__ T)
{
    extern __shared__ float erow[];                          // [DT_ROWS][D]
    const int r0 = blockIdx.x * DT_ROWS;
    const int nr = min(DT_ROWS, rows - r0);
    for (int i = threadIdx.x; i < DT_ROWS * D; i += 256) erow[i] = (i < nr * D) ? E[(size_t)r0 * D + i] : 0.0f;
    __syncthreads();
    for (int o = threadIdx.x; o < C; o += 256) {
        const float *w = W + (size_t)o * D;
        float acc[DT_ROWS];
#pragma unroll
        for (int j = 0; j < DT_ROWS; ++j) acc[j] = 0.0f;
        for (int k = 0; k < D; ++k) {
            const float wk = w[k];
#pragma unroll
            for (int j = 0; j < DT_ROWS; ++j) acc[j] = __builtin_fmaf(wk, erow[j * D + k], acc[j]);
        }
        const float bo = bias ? bias[o] : 0.0f;
#pragma unroll
        for (int j = 0; j < DT_ROWS; ++j)
            if (j < nr) T[(size_t)(r0 + j) * C + o] = bias ? acc[j] + bo : acc[j];
    }
}

int dvq_launch_decode_table(const float *E, int rows, int D, const float *W, const float *bias, int C, float *T, hipStream_t st)
{
    hipLaunchKernelGGL(decode_table_kernel, dim3((rows + DT_ROWS - 1) / DT_ROWS), dim3(256), (size_t)DT_ROWS * D * sizeof(float), st,
                       E, rows, D, W, bias, C, T);
    return (int)hipGetLastError();
}

int dvq_launch_decode_head(const long long *codes, int B, int HW, const float *T, int rows, int C, const float *F, const float *L,
                           float *out, hipStream_t st)
{
    const int N = B * HW;
    const dim3 grid((N + DH_TOK - 1) / DH_TOK, (C + DH_CH - 1) / DH_CH);
    const bool vec = HW % 4 == 0 && (((uintptr_t)out | (uintptr_t)F | (uintptr_t)L) & 15) == 0;
    if (vec)
        hipLaunchKernelGGL(decode_head_kernel<true>, grid, dim3(256), 0, st, codes, N, HW, T, rows, C, F, L, out);
    else
        hipLaunchKernelGGL(decode_head_kernel<false>, grid, dim3(256), 0, st, codes, N, HW, T, rows, C, F, L, out);
    return (int)hipGetLastError();
}
