// vq_assign_filter.hip -- nearest-codebook assignment at matrix-core speed with a proof obligation.
//
// Same contract as vq_assign_exact.hip (output identical bit for bit), reached in three steps:
//
//  pass 1   vq_assign_filter_kernel: approximate scores on the fp16 matrix cores
//             G_j = (zh . eh_j) - 2^(a+b-1) en_j   ~   -2^(a+b-1) (d_j - xn)
//           zh = fp16(2^a z), eh = fp16(2^b e), fp32 accumulate, en_j the exact reference norm
//           pre-loaded as the MFMA accumulator.  Per token a running top-2 and a RIGOROUS bound W
//           on |G_j - truth| that also covers the reference's own fp32 rounding.  The best code is
//           written for every token (codes, z_q, loss term -- z is read from HBM exactly once and
//           kept in registers in fp32 for z_q).  If best - second > 2W no other code can win in
//           the reference arithmetic either and the token is final.  Otherwise its operands are
//           dumped to a compact record and it is queued for the resolver.
//  resolve  vq_resolve_kernel (queued tokens only, a few %): re-runs the fp16 scores from the dumped
//           fragments, collects every code within 2W of the best, evaluates those few with the
//           bit-exact sequential fp32 FMA chain and the reference's d = fl(fl(xn+en) - 2 dot),
//           takes the first-index minimum, and rewrites codes / z_q / loss term if the winner
//           differs from pass 1's provisional choice.
//  exact    vq_assign_exact_kernel over a second list: NaN/Inf tokens, tokens fp16 cannot scale,
//           record or candidate overflow (normally empty; the kernel exits at once).
//
// Error budget (real-number analysis; zeta = 2^a z - zh and eta_j = 2^b e_j - eh_j are the ACTUAL
// rounding residuals, their 2-norms are computed, so fp16 subnormals need no special case):
//   |2^(a+b) z.e_j - zh.eh_j| <= ||zeta|| ||eh_j|| + ||zh|| ||eta_j|| + ||zeta|| ||eta_j||     (Cauchy-Schwarz)
//   MFMA fp32 accumulation        <= gamma' (||zh|| ||eh_j|| + |seed|),  gamma' = 2^-13  (>= 4x the
//                                    worst case of 272 roundings of 2^-23)
//   4 mantissa bits replaced by the accumulator-register index           <= 2^-19 |G|
//   reference side, d = fl(fl(xn+en) - 2 dotc), dotc the D-term fp32 chain:
//                                 <= 2^(a+b) [u(1+u)(xn+en) + (u + gamma_D)(1+gamma_D) ||z|| ||e_j||]
// W is the sum with ||e_j||, en_j, ||eta_j|| replaced by their maxima over the codebook.
#include "dvq_pass1.h"
#include "launchers.h"

#ifndef DVQ_WIDE_MIN_K
#define DVQ_WIDE_MIN_K 2048      // codebook size from which pass 1 takes the two-blocks-per-wave form (whole op at B = 256: -2 % at 1024, +8 % at 2048, +10 % at 4096 and 16384)
#endif
// ---------------------------------------------------------------------------------------------
// prep: meta (scale, norm maxima, finiteness), fp16 tile images, rounding-residual norm
//   image of tile t: [s < D/16][lane < 64][j < 8] halves = fp16(2^b E[32t + (lane&31)][16s + 8(lane>>5) + j])
//   -> the A fragment of k-step s is ONE ds_read_b128 at s*1024 + lane*16 (lane-linear, conflict-free)
// ---------------------------------------------------------------------------------------------
// Round 6: ONE kernel behind the f32 prep (vq_assign_exact.hip: codebook_prep_f32_kernel), which leaves per-workgroup partial
// maxima in the padding of its tiles -- until now six launches (partial scan, scan, two image kernels, residual norms: 42 us of
// every training step for 1 MiB of codebook).  A workgroup owns CPW codes of a tile, as the f32 prep does: every workgroup
// reduces the partials to the meta values itself (a few KiB from L2; maxima and an OR: any order gives the same bits) and workgroup 0
// writes them; a thread converts octets of channels and stores them into BOTH images (the 32x32x16 order and the 16x16x32 order
// hold the same fp16 values); the rounding residuals go through LDS so that a code's squared residual norm is summed in the order
// it always was (lane-strided, xor tree); etamax was zeroed by the f32 prep.
template <int CPW>
__global__ __launch_bounds__(256) void codebook_prep_f16_kernel(const float *__restrict__ E, int K, int D,
                                                                const float *__restrict__ tiles32,
                                                                const float *__restrict__ en_all,
                                                                DvqF16Meta *__restrict__ meta, char *__restrict__ img,
                                                                char *__restrict__ img16)
{
    extern __shared__ float r2[];                            // [CPW][D] squared rounding residuals
    __shared__ float s_a[4], s_e[4];
    __shared__ int s_b[4];
    constexpr int SUBS = 32 / CPW;
    const int t = blockIdx.x / SUBS, sub = blockIdx.x % SUBS, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int T = dvq_num_tiles(K);
    float amax = 0.0f, enmax = 0.0f;
    int bad = 0;
    {
        const size_t tf = dvq_tile_floats(D);
        for (int i = tid; i < T * SUBS; i += 256) {
            const f32x4 p = *(const f32x4 *)(tiles32 + (size_t)(i / SUBS) * tf + 32 * D + 32 + 4 * (i % SUBS));
            amax = fmaxf(amax, p[0]);
            enmax = fmaxf(enmax, p[1]);
            bad |= p[2] != 0.0f;
        }
        for (int off = 32; off > 0; off >>= 1) {
            amax = fmaxf(amax, __shfl_xor(amax, off));
            enmax = fmaxf(enmax, __shfl_xor(enmax, off));
            bad |= __shfl_xor(bad, off);
        }
        if (lane == 0) { s_a[wave] = amax; s_e[wave] = enmax; s_b[wave] = bad; }
        __syncthreads();
        amax = fmaxf(fmaxf(s_a[0], s_a[1]), fmaxf(s_a[2], s_a[3]));
        enmax = fmaxf(fmaxf(s_e[0], s_e[1]), fmaxf(s_e[2], s_e[3]));
        bad = s_b[0] | s_b[1] | s_b[2] | s_b[3];
    }
    int bexp = 0;
    if (amax > 0.0f) {
        int e;
        (void)frexpf(amax, &e);         // amax = m 2^e, m in [0.5, 1)
        bexp = 15 - e;                  // 2^b amax in [2^14, 2^15)
    }
    if (bexp > 100 || bexp < -100) bad = 1;
    const float sb = ldexpf(1.0f, bad ? 0 : bexp);
    if (blockIdx.x == 0 && tid == 0) {
        meta->ok = bad ? 0 : 1;
        meta->b_exp = bexp;
        meta->scale_b = sb;
        meta->emax = sqrtf(enmax) * 1.00001f;
        meta->enmax = enmax;
    }
    // image of tile t = [fp16 image: D/16 x 1 KiB][tail 256 B: seed[32] = -2^(b-1) en_j, the MFMA accumulator
    // start value that turns the dot product into the score; codes >= K get a huge negative FINITE
    // seed (they never win, and packing the register index into the low mantissa bits cannot turn
    // them into NaNs as it would for -inf); pad[32]]
    //   32x32x16 order:  [s < D/16][lane < 64][j < 8] = fp16(2^b E[32t + (lane & 31)][16 s + 8 (lane >> 5) + j])
    //   16x16x32 order (image "16"): fragment F = c2 * (D/32) + s' (c2 < 2 code halves, s' < D/32 k-steps of 32), lane l, j < 8:
    //                    fp16(2^b E[32t + 16 c2 + (l & 15)][32 s' + 8 (l >> 4) + j]); same seeds tail.
    const int KG = D / 8, S32 = D / 32;
    const size_t tile_bytes = (size_t)D * 64 + 256;
    char *t8 = img + (size_t)t * tile_bytes, *t16 = img16 + (size_t)t * tile_bytes;
    for (int u = tid; u < CPW * KG; u += 256) {
        const int cl = u / KG, o = u - cl * KG, c = sub * CPW + cl;
        const int code = t * 32 + c;
        f16x8 hv;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float v = (code < K) ? E[(size_t)code * D + 8 * o + j] * sb : 0.0f;
            const _Float16 hh = (_Float16)v;                 // round to nearest even
            hv[j] = hh;
            const float r = v - (float)hh;
            r2[cl * D + 8 * o + j] = r * r;
        }
        *(f16x8 *)(t8 + (((o >> 1) * 64 + 32 * (o & 1) + c) * 16)) = hv;
        *(f16x8 *)(t16 + ((((c >> 4) * S32 + (o >> 2)) * 64 + 16 * (o & 3) + (c & 15)) * 16)) = hv;
    }
    if (sub == 0 && tid < 64) {
        const int code = t * 32 + tid;
        float v = 0.0f;
        if (tid < 32) v = (code < K) ? fmaxf(-0.5f * sb * en_all[code], DVQ_SEED_PAD) : DVQ_SEED_PAD;
        ((float *)(t8 + (size_t)D * 64))[tid] = v;
        ((float *)(t16 + (size_t)D * 64))[tid] = v;
    }
    __syncthreads();
    // etamax = max_j || 2^b e_j - fp16(2^b e_j) ||_2 (each residual is exact in fp32), rounded up.  A wave per code.
    float best = 0.0f;
    for (int cl = wave; cl < CPW; cl += 4) {
        float sum = 0.0f;
        for (int k = lane; k < D; k += 64) sum += r2[cl * D + k];
        for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
        best = fmaxf(best, sum);
    }
    if (lane == 0 && best > 0.0f) {
        float v = sqrtf(best) * 1.001f;     // (the summation order differs from a sequential sum by a few ulp: inside the 0.1 % margin)
        atomicMax((int *)&meta->etamax, __float_as_int(v));       // positive floats order as ints
    }
}

// ---------------------------------------------------------------------------------------------
// audit aid (dvq_debug_filter_scores_f32, tools/bound_audit.py): pass 1's score arithmetic on a few tokens
// given as rows [n, D] -- same fp16 conversion, same seeded accumulator, same MFMA chain in the same order
// (v_mfma_f32_16x16x32_f16 over tile image "16"), same index packing, same threshold -- with every score
// written out instead of reduced to a top-2.  One wave per 32 tokens; A fragments straight from the prep image.
// (The tuning build can also dump best / second / 2W of the PRODUCTION kernel per token: g_dvq_tokdbg.)
// ---------------------------------------------------------------------------------------------
template <int D, bool FOLD>
__global__ __launch_bounds__(64) void filter_scores_debug_kernel(
    const float *__restrict__ tokens, int n, const char *__restrict__ img, const DvqF16Meta *__restrict__ meta,
    int K, float *__restrict__ G, float *__restrict__ thr2W_out, float *__restrict__ xn_out)
{
    constexpr int S16 = D / 16;
    constexpr int S32 = D / 32;
    constexpr int IMG_BYTES = S16 * 1024;
    constexpr int TILE_STRIDE = IMG_BYTES + 256;
    const int lane = threadIdx.x, c = lane & 31, h = lane >> 5;
    const int tok = blockIdx.x * 32 + c;
    const bool valid = tok < n;
    const float *zp = tokens + (size_t)(valid ? tok : n - 1) * D + 8 * h;
    const int T = dvq_num_tiles(K), Kpad = 32 * T;
    const float sB = meta->scale_b;
    float pa[2][8];
    float amax = 0.0f, zeta2 = 0.0f;
#pragma unroll
    for (int s = 0; s < S16; ++s) {
#pragma unroll
        for (int j2 = 0; j2 < 4; ++j2) {
            const float v0 = zp[16 * s + 2 * j2], v1 = zp[16 * s + 2 * j2 + 1];
            const float q0 = sq_rn(v0), q1 = sq_rn(v1);
            pa[s & 1][2 * j2] = (s < 2) ? q0 : __fadd_rn(pa[s & 1][2 * j2], q0);
            pa[s & 1][2 * j2 + 1] = (s < 2) ? q1 : __fadd_rn(pa[s & 1][2 * j2 + 1], q1);
            amax = vmax_abs(amax, v0);
            amax = vmax_abs(amax, v1);
            f32x2 vv = {v0, v1};
            f16x2 hh = __builtin_convertvector(vv, f16x2);
            const float r0 = v0 - (float)hh[0], r1 = v1 - (float)hh[1];
            zeta2 = __builtin_fmaf(r0, r0, zeta2);
            zeta2 = __builtin_fmaf(r1, r1, zeta2);
        }
    }
    float t8[8];
#pragma unroll
    for (int l = 0; l < 8; ++l) {
        float o0 = __shfl_xor(pa[0][l], 32), o1 = __shfl_xor(pa[1][l], 32);
        float a0_ = h == 0 ? pa[0][l] : o0, a1_ = h == 0 ? o0 : pa[0][l];
        float a2_ = h == 0 ? pa[1][l] : o1, a3_ = h == 0 ? o1 : pa[1][l];
        t8[l] = __fadd_rn(__fadd_rn(__fadd_rn(a0_, a1_), a2_), a3_);
    }
    float xn = t8[0];
#pragma unroll
    for (int l = 1; l < 8; ++l) xn = __fadd_rn(xn, t8[l]);
    amax = fmaxf(amax, __shfl_xor(amax, 32));
    zeta2 += __shfl_xor(zeta2, 32);
    const float thr2W = FOLD ? dvq_fold_threshold(xn, amax, zeta2, sB, (const DvqFoldMeta *)meta)
                             : dvq_filter_threshold(xn, amax, zeta2, sB, meta);
    if (valid && h == 0) { thr2W_out[tok] = thr2W; xn_out[tok] = xn; }
    // the 16x16x32 code loop of pass 1: lane (c16, q) holds tokens c16 / 16 + c16 of the block, k = 32 s' + 8 q + j --
    // the same fp16 values pass 1 permutes into this order
    const int c16 = lane & 15, q16 = lane >> 4;
    f16x8 zb[2][S32];
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2) {
        const int tk = blockIdx.x * 32 + 16 * t2 + c16;
        const float *zq_ = tokens + (size_t)(tk < n ? tk : n - 1) * D + 8 * q16;
#pragma unroll
        for (int sp = 0; sp < S32; ++sp) {
            u32x4 pk;
#pragma unroll
            for (int j2 = 0; j2 < 4; ++j2) {
                f32x2 vv = {zq_[32 * sp + 2 * j2], zq_[32 * sp + 2 * j2 + 1]};
                f16x2 hh = __builtin_convertvector(vv, f16x2);
                pk[j2] = __builtin_bit_cast(unsigned, hh);
            }
            zb[t2][sp] = __builtin_bit_cast(f16x8, pk);
        }
    }
    for (int t = 0; t < T; ++t) {
        const char *tile = img + (size_t)t * TILE_STRIDE;
        const float *seeds = (const float *)(tile + IMG_BYTES) + 4 * q16;
        f32x4 acc16[2][2];
#pragma unroll
        for (int c2 = 0; c2 < 2; ++c2) {
            const f32x4 e4 = *(const f32x4 *)(seeds + 16 * c2);
            acc16[c2][0] = e4;
            acc16[c2][1] = e4;
        }
#pragma unroll
        for (int F = 0; F < 2 * S32; ++F) {
            const f16x8 a = *(const f16x8 *)(tile + F * 1024 + lane * 16);
            acc16[F / S32][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, zb[0][F % S32], acc16[F / S32][0], 0, 0, 0);
            acc16[F / S32][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, zb[1][F % S32], acc16[F / S32][1], 0, 0, 0);
        }
#pragma unroll
        for (int t2 = 0; t2 < 2; ++t2) {
            const int tk = blockIdx.x * 32 + 16 * t2 + c16;
            if (tk < n) {
#pragma unroll
                for (int r = 0; r < 8; ++r) {
                    const int code = t * 32 + 16 * (r >> 2) + 4 * q16 + (r & 3);
                    G[(size_t)tk * Kpad + code] = __uint_as_float((__float_as_uint(acc16[r >> 2][t2][r & 3]) & 0xFFFFFFF0u) | (unsigned)r);
                }
            }
        }
    }
}

static inline size_t align256(size_t x) { return (x + 255) / 256 * 256; }

// the 16x16x32-order image follows the 32x32x16-order one (which the resolver reads)
static size_t dvq_img16_offset(int K, int D)
{
    const size_t tile = (size_t)(D / 16) * 1024 + 256;
    return ((size_t)dvq_num_tiles(K) * tile + 255) / 256 * 256;
}

// fold != 0: `prep` is the buffer of dvq_fold_prepare_f32, `tokens` the conv's inputs
int dvq_launch_filter_scores_debug(const float *tokens, int n, const void *prep, int D, int K, float *G,
                                   float *thr2W, float *xn, float *scale_b_out, hipStream_t st, int fold)
{
    char *base = (char *)prep + dvq_prep_f16_offset(K, D);
    base = (char *)(((uintptr_t)base + 255) / 256 * 256);
    if (fold) base = (char *)prep;
    const DvqF16Meta *meta = (const DvqF16Meta *)base;
    const char *im = base + 256 + dvq_img16_offset(K, D);
    const int blocks = (n + 31) / 32;
    if (fold) {
        switch (D) {
        case 64:  hipLaunchKernelGGL((filter_scores_debug_kernel<64, true>), dim3(blocks), dim3(64), 0, st, tokens, n, im, meta, K, G, thr2W, xn); break;
        case 128: hipLaunchKernelGGL((filter_scores_debug_kernel<128, true>), dim3(blocks), dim3(64), 0, st, tokens, n, im, meta, K, G, thr2W, xn); break;
        case 256: hipLaunchKernelGGL((filter_scores_debug_kernel<256, true>), dim3(blocks), dim3(64), 0, st, tokens, n, im, meta, K, G, thr2W, xn); break;
        default:  return -1000;
        }
    } else
    switch (D) {
    case 64:  hipLaunchKernelGGL((filter_scores_debug_kernel<64, false>), dim3(blocks), dim3(64), 0, st, tokens, n, im, meta, K, G, thr2W, xn); break;
    case 128: hipLaunchKernelGGL((filter_scores_debug_kernel<128, false>), dim3(blocks), dim3(64), 0, st, tokens, n, im, meta, K, G, thr2W, xn); break;
    case 256: hipLaunchKernelGGL((filter_scores_debug_kernel<256, false>), dim3(blocks), dim3(64), 0, st, tokens, n, im, meta, K, G, thr2W, xn); break;
    default:  return -1000;
    }
    if (scale_b_out != nullptr)
        (void)hipMemcpyAsync(scale_b_out, &meta->scale_b, sizeof(float), hipMemcpyDeviceToDevice, st);
    return (int)hipGetLastError();
}

// The op's counter block (dvq_common.h: DVQ_C_*) and the sliced resolver's chunk tickets.  In the steady state nobody launches
// this: every filter-path op puts its live words back to zero itself -- the list kernel's finishing workgroup the counter block,
// each chunk's last resolver slice its ticket pair -- and a caller that keeps track says so with DVQ_MODE_WS_CLEAN (dvq.h).
__global__ void zero_counters_kernel(int *__restrict__ counters, int nwords)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nwords; i += gridDim.x * blockDim.x) counters[i] = 0;
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
#ifdef DVQ_TUNING
// device buffer the tuning build's pass 1 writes its per-token diagnostics to (null = off): tokdbg [N][4] f32 = best, second,
// 2W, code; stamps [workgroup][8] u64 = stage times of the split form of pass 1 and of the resolver (null = off).  Every unit
// whose kernels read the pointers holds its own copy (dvq_pass1.h): set them all.
extern "C" __attribute__((visibility("default"))) int dvq_tuning_buffers(void *stamps, void *tokdbg)
{
    int (*const setters[])(void *, void *) = {dvq_tuning_set_pass1_d64, dvq_tuning_set_pass1_d64_res, dvq_tuning_set_pass1_d128,
                                              dvq_tuning_set_pass1_d128_res, dvq_tuning_set_pass1_d256, dvq_tuning_set_pass1_d256_res,
                                              dvq_tuning_set_resolve};
    for (auto set : setters) {
        const int rc = set(stamps, tokdbg);
        if (rc) return rc;
    }
    return 0;
}
#endif

// slots per shard (a multiple of RES_SLOTS); the whole record area holds DVQ_QSHARDS times that
static int shard_capacity(long N)
{
    long cap = N / 8;
    if (cap < 4096) cap = 4096;
    long per = (cap + DVQ_QSHARDS - 1) / DVQ_QSHARDS;
    per = (per + RES_SLOTS - 1) / RES_SLOTS * RES_SLOTS;
    return (int)per;
}

static int rec_capacity(long N) { return DVQ_QSHARDS * shard_capacity(N); }

bool dvq_filter_supported(int D, int HW, int K, long N)
{
    // D * HW < 2^29: pass 1 addresses a wave's loads / stores as a 32-bit byte offset from the wave's first token (buffer instructions)
    return (D == 64 || D == 128 || D == 256) && N < (1L << 31) && K < (1 << 20) && (long)D * HW < (1L << 29);
}

// ws_extra: [counters DVQ_COUNTER_BYTES][chunk ticket + overflow flag: 2 ints per resolver chunk]
//           [exact list N ints][records cap * rec_bytes]
// the split form of pass 1 (small batches): slices per token block, 1 = not taken.  As many as keep the grid within one workgroup
// per CU (256) and leave a slice two code tiles, at most 8.
static int split_slices(int K, long N)
{
    const long nb = (N + 127) / 128;
    if (nb > DVQ_SPLIT_MAX_BLOCKS) return 1;
    int ks = DVQ_SPLIT_MAX_SLICES;
    while (ks > 1 && (nb * ks > 256 || dvq_num_tiles(K) / ks < 2)) ks >>= 1;
    return ks;
}
static size_t split_bytes(long N)
{
    const long nb = (N + 127) / 128;
    return nb <= DVQ_SPLIT_MAX_BLOCKS ? align256((size_t)nb * DVQ_SPLIT_MAX_SLICES * 128 * sizeof(f32x4)) : 0;
}

size_t dvq_filter_ws_extra_bytes(int D, int HW, int K, long N)
{
    (void)HW; (void)K;
    return DVQ_COUNTER_BYTES + align256((size_t)rec_capacity(N) / RES_SLOTS * 2 * sizeof(int)) +
           align256((size_t)N * sizeof(int)) + align256((size_t)rec_capacity(N) * rec_bytes(D)) + split_bytes(N);
}

int dvq_launch_prep_f16(const float *E, int K, int D, void *prep, hipStream_t st)
{
    char *base = (char *)prep + dvq_prep_f16_offset(K, D);
    base = (char *)(((uintptr_t)base + 255) / 256 * 256);
    DvqF16Meta *meta = (DvqF16Meta *)base;
    char *img = base + 256;
    const float *en_all = (const float *)((char *)prep + dvq_prep_en_offset(K, D));
    const int T = dvq_num_tiles(K);
    char *img16 = img + dvq_img16_offset(K, D);
    if (dvq_prep_codes_per_workgroup(K) == 8)
        hipLaunchKernelGGL(codebook_prep_f16_kernel<8>, dim3(T * 4), dim3(256), 8 * D * sizeof(float), st, E, K, D, (const float *)prep, en_all, meta, img, img16);
    else
        hipLaunchKernelGGL(codebook_prep_f16_kernel<32>, dim3(T), dim3(256), 32 * D * sizeof(float), st, E, K, D, (const float *)prep, en_all, meta, img, img16);
    return (int)hipGetLastError();
}

// partials layout: [pass 1: np1 = its grid][resolver: cap/RES_SLOTS][exact list: min(ceil(N/128), DVQ_EXACT_LIST_BLOCKS)]
static int list_blocks(long N)
{
    long nb = (N + 127) / 128;
    return (int)(nb < DVQ_EXACT_LIST_BLOCKS ? nb : DVQ_EXACT_LIST_BLOCKS);
}

static FilterWs carve_ws(void *ws_extra, long N, int D)
{
    FilterWs w;
    w.counters = (int *)ws_extra;
    w.cap = rec_capacity(N);
    w.chunk_sync = (int *)((char *)ws_extra + DVQ_COUNTER_BYTES);
    const size_t sync_bytes = align256((size_t)w.cap / RES_SLOTS * 2 * sizeof(int));
    w.exact_list = (int *)((char *)ws_extra + DVQ_COUNTER_BYTES + sync_bytes);
    w.records = (char *)ws_extra + DVQ_COUNTER_BYTES + sync_bytes + align256((size_t)N * sizeof(int));
    w.split = split_bytes(N) ? (f32x4 *)(w.records + align256((size_t)w.cap * rec_bytes(D))) : nullptr;
    return w;
}

// SEL = 2 applies to the reference's grids: output rows of 32 positions, whole workgroups of 4 rows per image, and
// branch tensors the 16-byte DMA pieces can address
static bool staged_select_ok(const DvqRouted &rv)
{
    if (rv.Wout != 32 || rv.HWout % 128 != 0) return false;
    for (int g = 0; g < rv.G; ++g)
        if (((uintptr_t)rv.src[g] & 15) != 0) return false;
    return true;
}

// The form of pass 1: for the op, the first row that applies.  fold: the conv folded into the codebook (it takes precedence over
// conv); conv: the 1x1 conv as pass 1's prologue; routed: the select fused in; dense: none of these.  "Small batch":
// split_slices(K, N) > 1 and the workspace has the split area; "aligned": z and zq 16-byte aligned; "fits":
// N * D * 4 <= DVQ_CACHED_MAX_BYTES.
//   | op                          | condition, in order                             | kernel                                     |
//   |-----------------------------|-------------------------------------------------|--------------------------------------------|
//   | fold                        | small batch                                     | split, SEL = rv ? 1 : 0, FOLD              |
//   | fold, dense                 | HW == 1 and aligned                             | flat <D, FOLD = true>                      |
//   | fold, dense / staged routed | D == 256 and fits                               | cached <D, SEL in {0, 2}, true>            |
//   | fold                        | otherwise                                       | plain <D, SEL in {0, 1, 2}, false, true>   |
//   | conv (D = 256, else -1000)  | small batch                                     | split, SEL = rv ? 1 : 0, CONV              |
//   | conv                        | otherwise                                       | plain <256, rv ? 1 : 0, true, false>       |
//   | routed                      | small batch                                     | split, SEL = 1                             |
//   | routed                      | staged_select_ok                                | cached (D = 256, fits) else plain, SEL = 2 |
//   | routed                      | otherwise                                       | plain, SEL = 1                             |
//   | dense                       | D == 256 and (force_wide or K >= DVQ_WIDE_MIN_K | wide (checked BEFORE the small-batch test) |
//   |                             | and N >= 256 * 512)                             |                                            |
//   | dense                       | small batch                                     | split, FLAT = (HW == 1 and aligned)        |
//   | dense                       | HW == 1 and aligned                             | flat <D, false>                            |
//   | dense                       | D == 256 and fits                               | cached <D, 0, false>                       |
//   | dense                       | otherwise                                       | plain <D, 0, false, false>                 |
// 16-bit latents (xt != 0; dense only): always the x16 form -- the plain kernel on 2-byte accesses, for every HW (HW == 1: the
// row-major tensor, a lane per token) and every N: the wide, split, flat and cached forms do not exist for them, so a small
// batch runs unsplit.
static P1Plan pass1_plan(int D, int HW, int K, long N, bool aligned, const FilterWs &w, bool force_wide, const DvqRouted *rv,
                         bool conv, bool fold, int xt = 0)
{
    const bool dense = rv == nullptr && !conv && !fold;
    if (xt != 0) return {P1Form::x16, 0, false, false, false, 1, xt};
    if (dense && D == 256 && (force_wide || (K >= DVQ_WIDE_MIN_K && N >= 256L * 512)))   // large codebook and enough tokens to fill
        return {P1Form::wide, 0, false, false, false, 1};                                 // every CU with two 256-token workgroups
    const int ks = split_slices(K, N);
    if (ks > 1 && w.split != nullptr)                        // fewer token blocks than CUs: several workgroups per block
        return {P1Form::split, rv != nullptr ? 1 : 0, conv, fold, dense && HW == 1 && aligned, ks};
    if (conv) return {P1Form::plain, rv != nullptr ? 1 : 0, true, false, false, 1};
    const int sel = rv == nullptr ? 0 : (staged_select_ok(*rv) ? 2 : 1);
    // HW == 1 is a row-major [N, D] tensor: 16-byte accesses along a token's row (rows are 16-byte aligned: D % 16 == 0)
    if (sel == 0 && HW == 1 && aligned) return {P1Form::flat, 0, false, fold, true, 1};
    // a batch whose features fit the memory-side cache (with room for what else is live): plain loads instead of non-temporal ones
    if (sel != 1 && D == 256 && (size_t)N * D * sizeof(float) <= DVQ_CACHED_MAX_BYTES) return {P1Form::cached, sel, false, fold, false, 1};
    return {P1Form::plain, sel, false, fold, false, 1};
}

// pass 1 of a plan: the wide form, or the unit of (D, RES).  RES: a workgroup's code tiles (the split form: its largest slice)
// fit the seed table that pass1_body keeps in the seeds area, 32 tiles = 1024 codes; larger codebooks take the per-tile seed piece
static int launch_pass1(int D, const P1Plan &p, const P1Args &a)
{
    if (p.form == P1Form::wide) return D == 256 ? dvq_launch_pass1_wide(a) : -1000;
    const int tiles = dvq_num_tiles(a.K);
    const int per_wg = (p.form == P1Form::split) ? (tiles + p.ks - 1) / p.ks : tiles;
    const bool res = per_wg <= DVQ_SEED_TABLE_TILES && !p1_keeps_seed_piece(D, p.form, p.fold, p.flat);
    if (p.form == P1Form::x16)
        switch (D) {
        case 64:  return res ? dvq_launch_pass1_x16_d64_res(p, a) : dvq_launch_pass1_x16_d64(p, a);
        case 128: return res ? dvq_launch_pass1_x16_d128_res(p, a) : dvq_launch_pass1_x16_d128(p, a);
        case 256: return res ? dvq_launch_pass1_x16_d256_res(p, a) : dvq_launch_pass1_x16_d256(p, a);
        default:  return -1000;
        }
    switch (D) {
    case 64:  return res ? dvq_launch_pass1_d64_res(p, a) : dvq_launch_pass1_d64(p, a);
    case 128: return res ? dvq_launch_pass1_d128_res(p, a) : dvq_launch_pass1_d128(p, a);
    case 256: return res ? dvq_launch_pass1_d256_res(p, a) : dvq_launch_pass1_d256(p, a);
    default:  return -1000;
    }
}


// Dense op: z [B, D, HW].  Routed op (rv != nullptr): one token per output position of rv (the select fused into
// pass 1); N = B * HWout, mask = the codebook_mask pass 1 writes.
// Kernels of one op: [zero kernel unless ws_clean] -> pass 1 -> resolver -> list kernel (exact list, loss finalize, and its
// finishing workgroup puts the counter block back to zero: the op leaves its workspace clean).
// xt != 0 (dense op only): z and zq hold 16-bit latents of that type (dvq_common.h); every kernel of the chain widens them where
// it reads them and narrows z_q where it writes it.  The workspace, its carve and the counters are those of the fp32 op.
int dvq_launch_filter(const float *z, const void *prep, const float *E, const float *mask,
                      int D, int HW, int K, long N, float *zq, long long *codes, double *partials,
                      void *ws_extra, bool pass1_only, bool force_wide, float *loss, float beta,
                      const DvqRouted *rv, hipStream_t st, const DvqConv *cv, const DvqFold *fd, bool ws_clean, int xt)
{
    if (xt != 0 && (rv != nullptr || cv != nullptr || fd != nullptr || pass1_only || force_wide)) return -1000;
    char *base = (char *)prep + dvq_prep_f16_offset(K, D);
    base = (char *)(((uintptr_t)base + 255) / 256 * 256);
    // fd: pass 1 and the resolver's enumeration run on the folded codebook (same section layout); the exact chains, the
    // gathers and the exact-list kernel on the codebook itself
    const DvqF16Meta *meta = (fd != nullptr) ? (const DvqF16Meta *)fd->fprep : (const DvqF16Meta *)base;
    const char *img = (fd != nullptr) ? fd->fprep + 256 : base + 256;
    const float *en_all = (const float *)((const char *)prep + dvq_prep_en_offset(K, D));
    const FilterWs w = carve_ws(ws_extra, N, D);
    const bool routed = rv != nullptr;
    int rc;
    if (!ws_clean) {
        // A kernel rather than hipMemsetAsync: cheaper than the runtime's fill kernel, and the op stays a pure chain of
        // kernel nodes under hipGraph capture.
        const int nwords = DVQ_COUNTER_BYTES / 4 + (dvq_resolver_slices(K) > 1 ? w.cap / RES_SLOTS * 2 : 0);
        hipLaunchKernelGGL(zero_counters_kernel, dim3(nwords > 4096 ? 8 : 1), dim3(256), 0, st, w.counters, nwords);
        rc = (int)hipGetLastError();
        if (rc) return rc;
    }
    const int np1 = (int)((N + 127) / 128);
    const DvqConv *conv = fd != nullptr ? &fd->cv : cv;      // the conv folded into the codebook or computed by pass 1
    const bool aligned = (((uintptr_t)z | (uintptr_t)zq) & 15) == 0;
    const P1Plan plan = pass1_plan(D, HW, K, N, aligned, w, force_wide, rv, fd == nullptr && cv != nullptr, fd != nullptr, xt);
    const P1Args args = {z, img + dvq_img16_offset(K, D), meta, E, mask, HW, K, N, zq, codes, partials, w,
                         routed ? *rv : DvqRouted{}, conv != nullptr ? *conv : DvqConv{}, st};
    rc = launch_pass1(D, plan, args);                        // (pass 1's code loop runs on v_mfma_f32_16x16x32_f16: image "16")
    if (rc || pass1_only) return rc;
    const int HWout = routed ? rv->HWout : HW, Wout = routed ? rv->Wout : 0;
    rc = dvq_launch_resolver(D, img, meta, en_all, E, HWout, K, zq, codes, partials ? partials + np1 : nullptr,
                           w, Wout, nullptr, fd, st, partials, np1, xt);
    if (rc) return rc;
    double *partials3 = partials ? partials + np1 + w.cap / RES_SLOTS : nullptr;
    // the list kernel is the last of the op: it also sums the partials into loss[0..1] and cleans the counter block; the
    // resolver's partials already contain pass 1's (vq_resolve_kernel: p1_share)
    const DvqLossTail tail = {partials ? loss : nullptr, partials ? partials + np1 : nullptr, w.counters + DVQ_C_TICKET,
                              w.cap / RES_SLOTS + list_blocks(N),
                              1.0 / ((double)N * D), beta, w.counters, w.cap / DVQ_QSHARDS};
    const int *list_count = w.counters + DVQ_C_EXACT;
    // conv folded in or fused into pass 1: the list kernel computes its tokens' h itself, from the conv's input (dense z or the
    // branches) -- qconv.hip's arithmetic, what pass 1's prologue computes too (and with h_all it writes the h it scored over pass
    // 1's row of the token)
    return dvq_launch_exact_list(z, (const float *)prep, E, mask, D, HWout, K, N, zq, codes, partials3, w.exact_list, list_count,
                                 tail, rv, st, conv, xt);
}

// ---- routed op ---------------------------------------------------------------------------------
// filter mode: zero counters -> pass 1 with the select fused in (it derives the grain of every position's cell from the
// gate and writes indices / codebook_mask / gate_out itself: no prepass, no tables) -> resolver -> list + loss finalize.
// exact mode: a prepass writes indices / codebook_mask / gate_out, then every position by the exact chain.
int dvq_launch_routed(int G, int gate_mode, const void *gate, float thr, const float *h_coarse,
                      const float *h_median, const float *h_fine, const void *prep, const float *E,
                      int B, int D, int hc, int wc, int K, float beta, float *zq, long long *codes,
                      float *loss, long long *indices, float *cmask, long long *gate_out,
                      double *partials, void *ws_extra, bool exact, bool pass1_only, hipStream_t st, const DvqConv *cv,
                      const DvqFold *fd, bool ws_clean)
{
    const int SC = (G == 2) ? 2 : 4;
    const int Wout = SC * wc, HWout = SC * hc * Wout;
    const long N = (long)B * HWout;
    int rc = 0;
    if (exact) {
        rc = dvq_launch_routed_prepass(G, gate_mode, gate, thr, B, hc, wc, indices, cmask, gate_out, st);
        if (rc) return rc;
    }
    DvqRouted rv{};
    rv.G = G; rv.B = B; rv.D = D; rv.hc = hc; rv.wc = wc; rv.Wout = Wout; rv.HWout = HWout;
    rv.indices = indices; rv.gate = gate; rv.gate_mode = gate_mode; rv.thr = thr;
    if (!exact) { rv.indices_out = indices; rv.cmask_out = cmask; rv.gate_out = gate_out; }
    if (G == 2) {
        rv.src[0] = h_coarse; rv.src[1] = h_fine; rv.src[2] = nullptr;
        rv.sub[0] = 1; rv.sub[1] = 2; rv.sub[2] = 1;
        rv.rep[0] = 2; rv.rep[1] = 1; rv.rep[2] = 1;
    } else {
        rv.src[0] = h_coarse; rv.src[1] = h_median; rv.src[2] = h_fine;
        rv.sub[0] = 1; rv.sub[1] = 2; rv.sub[2] = 4;
        rv.rep[0] = 4; rv.rep[1] = 2; rv.rep[2] = 1;
    }
    if (exact) {
        rc = dvq_launch_exact(nullptr, (const float *)prep, E, cmask, D, HWout, K, N, zq, codes, partials, &rv, st);
        if (rc || loss == nullptr) return rc;
        return dvq_launch_loss_finalize(partials, (int)((N + 127) / 128), 1.0 / ((double)N * D), beta, loss, st);
    }
    return dvq_launch_filter(nullptr, prep, E, cmask, D, HWout, K, N, zq, codes, partials, ws_extra, pass1_only, false,
                             loss, beta, &rv, st, cv, fd, ws_clean, 0);
}
