// dvq_exact_tile.h -- the pieces of the exact-chain tile loop as helpers (gfx950 only).
//
// Four kernels score tokens against the prepared f32 tile images (dvq_common.h: the prep buffer) with the same arithmetic:
// vq_assign_exact_kernel, vq_soft_assign_kernel, vq_score_assign_kernel, vq_gumbel_assign_kernel.  A workgroup is 4 waves; a
// wave keeps its 32 tokens' D channels in registers -- lane (c, h), c = lane & 31, h = lane >> 5, holds channel k = 2s + h of
// token c in zr[s] -- and the codebook streams through LDS as 32-code tile images, two buffers, one barrier per tile: wait for
// the DMA (s_waitcnt vmcnt(0)), barrier, take exact_buf(t), stage tile t + 1 into the other buffer, score tile t.
// Each kernel writes that loop itself: where its own prefetch sits relative to the stage is the kernel's choice.  What the
// package's bit-exactness contract rests on -- the image layout, the dot's chain, the norm's order, which register is which
// code, the merge of the lane halves -- is here for vq_soft.hip, vq_sample.hip and vq_gumbel.hip; vq_assign_exact.hip, where
// these pieces come from, keeps its own text of them (its header comment says why) and marks each with the helper's name.
#pragma once
#include "dvq_common.h"
#include <utility>

template <int D> constexpr int EXACT_TILE_FLOATS = (int)dvq_tile_floats(D);     // one tile image: 32 x D values, en[32], 32 of padding
template <int D> constexpr int EXACT_CHUNKS_PER_WAVE = (32 * D * 4 / 1024) / 4; // 1-KiB DMA pieces per wave per tile

// dynamic LDS of a kernel built on these pieces: the two tile buffers (what a kernel parks there after its loop fits inside)
inline size_t dvq_exact_lds_bytes(int D) { return 2 * dvq_tile_floats(D) * sizeof(float); }

// buffer of tile t
template <int D>
__device__ __forceinline__ float *exact_buf(float *lds, int t) { return lds + (t & 1) * EXACT_TILE_FLOATS<D>; }

// global -> LDS copy of tile t's image, its 32 norms included (asynchronous: s_waitcnt vmcnt(0) and a barrier before the first read).
// The pieces are a pack expansion, not a loop: a loop would let the optimiser hoist `lane * 16` out of it and re-associate the
// addresses before it unrolls, and each kernel would get other address arithmetic than the one its ISA digest pins.
template <int D, int... I>
__device__ __forceinline__ void exact_stage_pieces(const char *src, char *dst, int wave, int lane, std::integer_sequence<int, I...>)
{
    (glds16(src + (wave * EXACT_CHUNKS_PER_WAVE<D> + I) * 1024 + lane * 16, dst + (wave * EXACT_CHUNKS_PER_WAVE<D> + I) * 1024), ...);
}
template <int D>
__device__ __forceinline__ void exact_stage(const float *__restrict__ tiles, int t, float *buf, int wave, int lane)
{
    const char *src = (const char *)(tiles + (size_t)t * EXACT_TILE_FLOATS<D>);
    exact_stage_pieces<D>(src, (char *)buf, wave, lane, std::make_integer_sequence<int, EXACT_CHUNKS_PER_WAVE<D>>{});
    if (wave == 0) glds4(src + 32 * D * 4 + lane * 4, (char *)buf + 32 * D * 4);
}

// Token nn = b HW + hw of an fp32 NCHW tensor [B, D, HW] (HW == 1: row-major [N, D]): zr[s] = its channel k = 2s + h, which sits
// 2s HW floats behind channel h
template <int D>
__device__ __forceinline__ void exact_load_token_nchw(const float *z, int HW, long b, long nn, int h, float (&zr)[D / 2])
{
    const float *zp = z + ((size_t)b * D + h) * HW + (size_t)(nn - b * HW);
#pragma unroll
    for (int s = 0; s < D / 2; ++s) zr[s] = zp[(size_t)2 * s * HW];
}

// ATen-order sum of squares of the lane's token (oracle/dvq_oracle.c: dvq_oracle_sumsq), the same value in both lane halves:
// 32 accumulators a[m] = sum over k0 of x[k0 + m]^2 in k0 order, then ((a[l] + a[l+8]) + a[l+16]) + a[l+24] summed over
// l = 0..7 in order.  Channel k = 2s + h sits in zr[s], so a[m] is the chain over zr[m/2 + 16 j] of the lane half h = m & 1:
// a lane forms the 16 accumulators of its own parity (p), fetches the other 16 from its partner lane ^ 32 (o), and both
// halves combine all 32 in the one order.
template <int D>
__device__ __forceinline__ float exact_token_sumsq(const float (&zr)[D / 2], int h)
{
    float p[16], o[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        float a = sq_rn(zr[q]);
#pragma unroll
        for (int j = 1; j < D / 32; ++j) a = __fadd_rn(a, sq_rn(zr[q + 16 * j]));
        p[q] = a;
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) o[q] = __shfl_xor(p[q], 32);
    float t[8];
#pragma unroll
    for (int l = 0; l < 8; ++l) {
        // a[m], m = l + 8g: even m lives in the h = 0 lane's p[m/2], odd m in the h = 1 lane's
        float a4[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            int m = l + 8 * g;
            float mine = p[m >> 1], other = o[m >> 1];
            a4[g] = ((m & 1) == h) ? mine : other;
        }
        t[l] = __fadd_rn(__fadd_rn(__fadd_rn(a4[0], a4[1]), a4[2]), a4[3]);
    }
    float xn = t[0];
#pragma unroll
    for (int l = 1; l < 8; ++l) xn = __fadd_rn(xn, t[l]);
    return xn;
}

// The 32 x 32 dots of the wave's tokens with the tile's codes: D/2 chained v_mfma_f32_32x32x2_f32 from a zero accumulator ARE the
// reference's sequential k = 0..D-1 fp32 FMA chain, two k per instruction (fma(a1, b1, fma(a0, b0, C)), one rounding per
// product).  A product a*b is the same number either way round, so the operand order only chooses where a dot lands:
//   TOKEN_ROWS = false  MFMA rows = codes, columns = tokens: register r of lane (c, h) is token c, code exact_code_of(t, r>>2, r&3, h) --
//                       a token's running arg-extremum is lane-local, two lane halves to merge (exact_merge_halves_argmax)
//   TOKEN_ROWS = true   MFMA rows = tokens, columns = codes: register r of lane (c, h) is token (r&3) + 8(r>>2) + 4h of the wave,
//                       code 32 t + c -- a register across the wave is two 128-byte runs of consecutive codes in two token
//                       rows, what a row-major [N, K] store wants; a token's arg-extremum then lives in 32 lanes
// (acc comes back through a reference: a by-value return is `noundef` to the optimiser, which then drops the freeze in front of the
// callers' select chains and schedules them differently from the code the kernels were measured with)
template <int D, bool TOKEN_ROWS = false>
__device__ __forceinline__ void exact_tile_dots(const float *buf, const float (&zr)[D / 2], int c, int h, f32x16 &acc)
{
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    const float *ap = buf + c * 8 + h * 4;
#pragma unroll
    for (int kg = 0; kg < D / 8; ++kg) {
        f32x4 a = *(const f32x4 *)(ap + kg * 256);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            acc = TOKEN_ROWS ? __builtin_amdgcn_mfma_f32_32x32x2f32(zr[kg * 4 + j], a[j], acc, 0, 0, 0)
                             : __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], zr[kg * 4 + j], acc, 0, 0, 0);
    }
}

// codes-in-rows order: accumulator register r = 4g + q of lane half h holds code 32 t + (r&3) + 8 (r>>2) + 4h -- four runs (g) of
// four consecutive codes (q) -- and the four values of run g in the tile's 32-float slot (the squared norms `en`; vq_gumbel.hip
// keeps proj.bias there)
__device__ __forceinline__ int exact_code_of(int t, int g, int q, int h) { return t * 32 + q + 8 * g + 4 * h; }
template <int D>
__device__ __forceinline__ f32x4 exact_tile_en4(const float *buf, int h, int g)
{
    return *(const f32x4 *)(buf + 32 * D + 4 * h + 8 * g);
}

// codes-in-rows order, after the loop: merge the (value, index) of a token's two lane halves in place; returns the token's code.
// bidx still 0x7fffffff: no candidate was ever taken (every score -inf) -> index 0, as torch
__device__ __forceinline__ int exact_merge_halves_argmax(float &best, int &bidx)
{
    const float ob = __shfl_xor(best, 32);
    const int oi = __shfl_xor(bidx, 32);
    argmax_merge(best, bidx, ob, oi);
    return (bidx == 0x7fffffff) ? 0 : bidx;
}
