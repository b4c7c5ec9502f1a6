// vq_resolve.hip -- the resolver of the fp16-filter assign (contract: header of vq_assign_filter.hip) and its launcher.
#include "dvq_pass1.h"

#ifdef DVQ_TUNING
// stage stamps of the resolver's workgroups, behind those of pass 1's split form: [4096 + workgroup][8]
#define DVQ_RSTAMP(i) do { if (g_dvq_stamps != nullptr && threadIdx.x == 0 && blockIdx.y == 0) g_dvq_stamps[(size_t)(4096 + blockIdx.x) * 8 + (i)] = wall_clock64(); } while (0)
#else
#define DVQ_RSTAMP(i) do { } while (0)
#endif

// ---------------------------------------------------------------------------------------------
// resolver: queued tokens, RES_SLOTS (= 32, one MFMA column set) per workgroup.  The queue is short
// (a few % of the tokens), so the work is spread for LATENCY: the four waves of a workgroup share
// the same 32 tokens and each takes every fourth code tile, reading its A fragments straight from
// the L2-resident prep image (no LDS ring, no barrier in the loop).
// One caller, vq_resolve_kernel (a launch of its own behind pass 1; large codebooks: sliced code
// tiles, the wide / pipe forms of pass 1).
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long order_key(float d, int code)
{
    d = d + 0.0f;                                 // -0 -> +0: equal distances tie on the index
    unsigned u = __float_as_uint(d);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);   // monotone map, finite d
    return ((unsigned long long)u << 32) | (unsigned)code;
}

#ifndef DVQ_RES_WAVES
#define DVQ_RES_WAVES 4          // waves per resolver workgroup (they split the code tiles)
#endif
// ATen-order sum of squares of v[0 .. D) (oracle/dvq_oracle.c: dvq_oracle_sumsq; D a multiple of 32)
__device__ __forceinline__ float aten_sumsq(const float *v, int D)
{
    float a[32];
#pragma unroll
    for (int m = 0; m < 32; ++m) a[m] = 0.0f;
    for (int k0 = 0; k0 < D; k0 += 32)
#pragma unroll
        for (int m = 0; m < 32; ++m) a[m] = __fadd_rn(a[m], sq_rn(v[k0 + m]));
    float s = 0.0f;
#pragma unroll
    for (int l = 0; l < 8; ++l) {
        const float tl = __fadd_rn(__fadd_rn(__fadd_rn(a[l], a[l + 8]), a[l + 16]), a[l + 24]);
        s = (l == 0) ? tl : __fadd_rn(s, tl);
    }
    return s;
}

// LDS of one resolver workgroup (statics of vq_resolve_kernel, a carve of pass 1's dynamic region for the consumers)
template <int D>
struct ResLds {
    static constexpr int RB = D * 4 + 32;                    // bytes per record (rec_bytes(D))
    static constexpr int SREC = 0;                           // [RES_SLOTS][RB] this workgroup's records
    static constexpr int CAND = SREC + RES_SLOTS * RB;       // [RES_CAND] unsigned
    static constexpr int BEST = CAND + RES_CAND * 4;         // [RES_SLOTS] u64
    static constexpr int REWR = BEST + RES_SLOTS * 8;        // [RES_SLOTS] int
    static constexpr int MISC = REWR + RES_SLOTS * 4;        // [8] int: 0 candidate count, 1 rewrite count, 2 last slice, 3 overflow flag,
                                                             //          4 live slots of the chunk, 5 chunk is the shard's last
    static constexpr int RED = MISC + 32;                    // [DVQ_RES_WAVES] double
    static constexpr int BYTES = RED + 8 * DVQ_RES_WAVES;
    static_assert(CAND % 16 == 0 && BEST % 8 == 0 && RED % 8 == 0, "carve alignment");
};

// One chunk: the records [base, base + nlive) (record indices; nlive <= RES_SLOTS), code tiles [t_begin, t_end).
// FOLD (vq_fold.hip): the records hold the conv's INPUT x and `img` / `meta` are the folded codebook: the enumeration below
// runs on x exactly as pass 1 scored it (its candidate set contains the reference's winner for every h inside the conv's
// tolerance); the workgroup then computes h = W x + bias for its 32 tokens -- qconv.hip's split-fp16 arithmetic, bit-identical
// to dvq_qconv_f32 -- in place over x, and the exact chains / the rewrite run on that h against the codebook itself.
// nslice > 1 (large codebooks): each slice resolves its candidates locally, merges its per-token best into the record with a
// 64-bit atomicMin, and the slice that arrives last at the chunk's ticket carries on (and puts the ticket back to zero).
// Returns (thread 0) the chunk's loss correction; *not_last is set for a slice that is not the chunk's last.
// HW = positions per image of the OUTPUT grid; a routed token (RecMeta.rep > 1) covers rep x rep positions, rows Wout apart,
// all rewritten with the same values.
// XT != 0 (dense op on 16-bit latents, dvq_common.h): zq holds that type; the rewritten row is narrowed at the store, from the fp32
// latents of the record (the widened input), its loss terms taken before.
template <int D, bool FOLD, int XT = 0>
__device__ __forceinline__ double resolve_chunk(
    char *__restrict__ L, const int base, const int nlive, const int t_begin, const int t_end,
    const char *__restrict__ img, const float *__restrict__ en_all, const float *__restrict__ E, int HW, int Wout,
    float *__restrict__ zq, long long *__restrict__ codes, int *__restrict__ counters, int *__restrict__ exact_list,
    char *__restrict__ records, int nslice, int *__restrict__ ticket, float *__restrict__ h_spill, const DvqConv &cv,
    const bool want_loss, bool *not_last)
{
    // h_spill (conv fused into pass 1; null otherwise): [B, D, HW] buffer the exact-list kernel reads its tokens' latents from.
    // Pass 1 spills the rows of ITS hand-offs; the tokens the resolver itself sends to that list (candidate overflow, no
    // candidate) get their row written here, from the record (which holds the conv's output).
    using LL = ResLds<D>;
    constexpr int S16 = D / 16;
    constexpr int IMG_BYTES = S16 * 1024;
    constexpr int TILE_STRIDE = IMG_BYTES + 256;
    constexpr int RW = DVQ_RES_WAVES;
    constexpr int RB = LL::RB;
    char *srec = L + LL::SREC;
    unsigned *cand = (unsigned *)(L + LL::CAND);
    unsigned long long *best = (unsigned long long *)(L + LL::BEST);
    int *rewrite = (int *)(L + LL::REWR);
    int *misc = (int *)(L + LL::MISC);
    double *red = (double *)(L + LL::RED);

    int tid = threadIdx.x, lane = tid & 63;                  // (re-derived after the enumeration loop, see there)
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int c = lane & 31, h = lane >> 5;
    *not_last = false;
    if (tid < RES_SLOTS) best[tid] = ~0ull;
    if (tid < 4) misc[tid] = 0;
    {
        // all of a thread's pieces are in flight before the first is stored (the rolled loop paid one memory latency per piece:
        // 4.3 of a chunk's 13 us)
        constexpr int NP = (RES_SLOTS * (RB / 16) + RW * 64 - 1) / (RW * 64);
        const int npieces = nlive * (RB / 16);
        f32x4 tmp[NP];
        const f32x4 *src = (const f32x4 *)(records + (size_t)base * RB);
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            const int i = tid + k * RW * 64;
            tmp[k] = src[i < npieces ? i : 0];
        }
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            const int i = tid + k * RW * 64;
            if (i < npieces) ((f32x4 *)srec)[i] = tmp[k];
        }
    }
    __syncthreads();
    DVQ_RSTAMP(2);
    const bool live = c < nlive;
    const char *rec = srec + (live ? c : 0) * RB;            // (FOLD: taken again after the enumeration loop)
    f16x8 zh[S16];
#pragma unroll
    for (int s = 0; s < S16; ++s) {                    // same RNE f32 -> f16 conversion as pass 1
        const f32x4 lo = *(const f32x4 *)(rec + (16 * s + 8 * h) * 4);
        const f32x4 hi = *(const f32x4 *)(rec + (16 * s + 8 * h + 4) * 4);
        u32x4 packed;
#pragma unroll
        for (int j2 = 0; j2 < 4; ++j2) {
            f32x2 vv = {j2 < 2 ? lo[2 * j2] : hi[2 * j2 - 4], j2 < 2 ? lo[2 * j2 + 1] : hi[2 * j2 - 3]};
            f16x2 hh = __builtin_convertvector(vv, f16x2);
            packed[j2] = __builtin_bit_cast(unsigned, hh);
        }
        zh[s] = __builtin_bit_cast(f16x8, packed);
    }
    const RecMeta rm = *(const RecMeta *)(rec + (size_t)D * 4);
    const float thr = live ? rm.thr : __builtin_inff();
    __syncthreads();
    // ---- enumerate: every code whose approximate score reaches best - 2W.  The A fragments of a tile come
    // straight from L2 (16 KiB per tile) and a workgroup is one latency chain (about one workgroup per CU is
    // active), so the next tile's sixteen loads are in flight while this tile's MFMAs run (two fragment sets;
    // same-box A/B: 31.9 -> 28.3 us at configs[2]; 64 tokens per workgroup instead: 35.5 us).
    {
        auto fetch = [&](int t, f16x8 (&a)[S16], f32x4 (&en4)[4]) {
            const char *tile = img + (size_t)t * TILE_STRIDE;
            const float *enr = (const float *)(tile + IMG_BYTES) + 4 * h;      // accumulator seeds of the tile
#pragma unroll
            for (int s = 0; s < S16; ++s) a[s] = *(const f16x8 *)(tile + s * 1024 + lane * 16);
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) en4[g4] = *(const f32x4 *)(enr + 8 * g4);   // rows 8g + 4h + q
        };
        auto score = [&](int t, const f16x8 (&a)[S16], const f32x4 (&en4)[4]) {
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
#pragma unroll
            for (int s = 0; s < S16; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[s], zh[s], acc, 0, 0, 0);
            unsigned hits = 0;
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    float g = acc[4 * g4 + q] + en4[g4][q];                            // padding: -3e38
                    hits |= (g >= thr) ? (1u << (4 * g4 + q)) : 0u;
                }
            while (hits) {
                int r = __builtin_ctz(hits);
                hits &= hits - 1;
                int code = t * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                int pos = atomicAdd(&misc[0], 1);
                if (pos < RES_CAND) cand[pos] = ((unsigned)c << 20) | (unsigned)code;
            }
        };
        // Two tiles in flight per wave.  Every fetch is UNCONDITIONAL (past the wave's last tile it re-reads that tile and the
        // result is not scored): with `if (t + RW < t_end) fetch(..)` the wait in front of a tile's first MFMA was computed over
        // both paths -- vmcnt(5): the just-issued prefetch had to land too, so no tile was ever fetched under another's MFMAs
        // (0.85 us per tile on an idle chip instead of the MFMA chain's 0.25).
        f16x8 a0[S16], a1[S16];
        f32x4 e0[4], e1[4];
        const int tw = t_begin + wave;
        if (tw < t_end) {
            const int tl = tw + (t_end - 1 - tw) / RW * RW;      // this wave's last tile
            auto clampt = [&](int t) { return t < tl ? t : tl; };
            // (sched_barrier: left alone the scheduler interleaves the two fetches, and the register the first MFMA needs is
            // then among the last loads issued)
            fetch(tw, a0, e0);
            __builtin_amdgcn_sched_barrier(0);
            fetch(clampt(tw + RW), a1, e1);
            __builtin_amdgcn_sched_barrier(0);
            for (int t = tw; t < t_end; t += 2 * RW) {
                score(t, a0, e0);
                __builtin_amdgcn_sched_barrier(0);
                fetch(clampt(t + 2 * RW), a0, e0);
                __builtin_amdgcn_sched_barrier(0);
                if (t + RW < t_end) score(t + RW, a1, e1);
                __builtin_amdgcn_sched_barrier(0);
                fetch(clampt(t + 3 * RW), a1, e1);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
    // the thread's ids from mbcnt instead of the registers that held them: kept live across the enumeration loop (256 registers,
    // every one in use) they were this kernel's spills (2 - 7 dwords of scratch per lane)
    lane = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    tid = wave * 64 + lane;
    c = lane & 31;
    h = lane >> 5;
    if constexpr (FOLD) {
        const char *rec = srec + (c < nlive ? c : 0) * RB;       // (shadows the first: the same address from the fresh ids)
        constexpr int T8 = D / 32, NT = (T8 + RW - 1) / RW;      // row tiles of the weight; this wave takes wave, wave + RW, ..
        constexpr int QIMG = S16 * 1024, QTILE = 2 * QIMG + 256;
        float amax = 0.0f;
#pragma unroll
        for (int s = 0; s < S16; ++s) {
            const f32x4 lo = *(const f32x4 *)(rec + (16 * s + 8 * h) * 4);
            const f32x4 hi = *(const f32x4 *)(rec + (16 * s + 8 * h + 4) * 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) { amax = vmax_abs(amax, lo[j]); amax = vmax_abs(amax, hi[j]); }
        }
        amax = fmaxf(amax, __shfl_xor(amax, 32));
        int ea = 0;                                              // per-token power-of-two scale, as qconv_kernel
        if (amax > 0.0f && amax < __builtin_inff()) { int e; (void)frexpf(amax, &e); ea = 14 - e; }
        ea = ea > 100 ? 100 : (ea < -100 ? -100 : ea);
        const float sa = ldexpf(1.0f, ea);
        const float unscale = ldexpf(cv.meta->inv_scale_w, -ea);
        // branch-free: a wave whose tile index runs past the last tile (D = 64: waves 2, 3) recomputes the last one and
        // writes the same values again.  The weight fragments come straight from L2, SB k-steps (SB * NT * 2 loads of 16 B per
        // lane) in flight at a time -- with a conditional per tile hipcc waited for every single load (12 us of the kernel).
        constexpr int SB = S16 < 8 ? S16 : 8;
        int tile_of[NT];
#pragma unroll
        for (int i = 0; i < NT; ++i) tile_of[i] = (wave + i * RW < T8) ? wave + i * RW : T8 - 1;
        f32x16 acc[NT];
#pragma unroll
        for (int i = 0; i < NT; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][r] = 0.0f;
#pragma unroll
        for (int s0 = 0; s0 < S16; s0 += SB) {
            f16x8 wh[SB][NT], wl[SB][NT];
#pragma unroll
            for (int q = 0; q < SB; ++q)
#pragma unroll
                for (int i = 0; i < NT; ++i) {
                    const char *wt = cv.wimg + (size_t)tile_of[i] * QTILE + (s0 + q) * 1024 + lane * 16;
                    wh[q][i] = *(const f16x8 *)wt;
                    wl[q][i] = *(const f16x8 *)(wt + QIMG);
                }
            __builtin_amdgcn_sched_barrier(0);                   // all of the batch's loads are issued before its first MFMA
#pragma unroll
            for (int q = 0; q < SB; ++q) {
                const int s = s0 + q;
                const f32x4 lo = *(const f32x4 *)(rec + (16 * s + 8 * h) * 4);
                const f32x4 hi = *(const f32x4 *)(rec + (16 * s + 8 * h + 4) * 4);
                u32x4 ph, pl;
#pragma unroll
                for (int j2 = 0; j2 < 4; ++j2) {
                    const float v0 = (j2 < 2 ? lo[2 * j2] : hi[2 * j2 - 4]) * sa, v1 = (j2 < 2 ? lo[2 * j2 + 1] : hi[2 * j2 - 3]) * sa;
                    const f32x2 vv = {v0, v1};
                    const f16x2 hh = __builtin_convertvector(vv, f16x2);
                    const f32x2 rr = {v0 - (float)hh[0], v1 - (float)hh[1]};
                    const f16x2 ll = __builtin_convertvector(rr, f16x2);
                    ph[j2] = __builtin_bit_cast(unsigned, hh);
                    pl[j2] = __builtin_bit_cast(unsigned, ll);
                }
                const f16x8 xh = __builtin_bit_cast(f16x8, ph), xl = __builtin_bit_cast(f16x8, pl);
#pragma unroll
                for (int i = 0; i < NT; ++i) {
                    acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl[q][i], xh, acc[i], 0, 0, 0);     // small terms first (qconv.hip)
                    acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[q][i], xl, acc[i], 0, 0, 0);
                    acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[q][i], xh, acc[i], 0, 0, 0);
                }
            }
        }
        __syncthreads();                                         // every wave has read x: h takes its place
        if (live) {
            float *hrow = (float *)(srec + c * RB);
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                const int t8 = tile_of[i];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int ch = 32 * t8 + 16 * (r >> 3) + 8 * h + (r & 7);     // qconv_row_channel's inverse
                    hrow[ch] = __builtin_fmaf(acc[i][r], unscale, cv.bias[ch]);
                }
            }
        }
        __syncthreads();
        // the reference's norm of h (ATen order: 32 partial sums a[i % 32], ((a[l] + a[l+8]) + a[l+16]) + a[l+24], then l = 0..7
        // left to right) for the exact chains: 8 lanes per token, lane l owns a[l], a[l+8], a[l+16], a[l+24]
        static_assert(RW * 64 >= RES_SLOTS * 8, "8 lanes per queued token");
        const int tk = (tid >> 3) < RES_SLOTS ? (tid >> 3) : RES_SLOTS - 1, l8 = tid & 7;   // (threads past the last token: idle repeats)
        const float *hv = (const float *)(srec + tk * RB);
        float a4[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int k0 = 0; k0 < D; k0 += 32)
#pragma unroll
            for (int g = 0; g < 4; ++g) a4[g] = __fadd_rn(a4[g], sq_rn(hv[k0 + l8 + 8 * g]));
        const float tl = __fadd_rn(__fadd_rn(__fadd_rn(a4[0], a4[1]), a4[2]), a4[3]);
        float sn = __shfl(tl, lane & ~7);
#pragma unroll
        for (int i = 1; i < 8; ++i) sn = __fadd_rn(sn, __shfl(tl, (lane & ~7) + i));
        if (l8 == 0 && (tid >> 3) < nlive) ((RecMeta *)(srec + tk * RB + (size_t)D * 4))->xn = sn;
        __syncthreads();
    }
    __syncthreads();
    const int ncand_raw = misc[0];
    bool overflow = ncand_raw > RES_CAND;             // hand the whole group to the exact list
    const int ncand = overflow ? 0 : ncand_raw;

    DVQ_RSTAMP(3);
    // ---- exact chains: one thread per (token, candidate)
    for (int i = tid; i < ncand; i += RW * 64) {
        const unsigned pc = cand[i];
        const int sl = (int)(pc >> 20), code = (int)(pc & 0xFFFFFu);
        const char *r2 = srec + sl * RB;
        const f32x4 *zv = (const f32x4 *)r2;
        const f32x4 *ev = (const f32x4 *)(E + (size_t)code * D);
        const float xn = ((const RecMeta *)(r2 + (size_t)D * 4))->xn;
        float acc = 0.0f;
        // the codebook row in batches of 16 x 16 B, the next batch in flight while this one feeds the (sequential) chain
        constexpr int CB = 16, NB = D / 4 / CB;
        f32x4 eb[2][CB];
#pragma unroll
        for (int q = 0; q < CB; ++q) eb[0][q] = ev[q];
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            if (b + 1 < NB) {
#pragma unroll
                for (int q = 0; q < CB; ++q) eb[(b + 1) & 1][q] = ev[(b + 1) * CB + q];
            }
#pragma unroll
            for (int q = 0; q < CB; ++q) {
                const f32x4 a = zv[b * CB + q], bb = eb[b & 1][q];
                acc = __builtin_fmaf(a[0], bb[0], acc);
                acc = __builtin_fmaf(a[1], bb[1], acc);
                acc = __builtin_fmaf(a[2], bb[2], acc);
                acc = __builtin_fmaf(a[3], bb[3], acc);
            }
        }
        float bias = __fadd_rn(xn, en_all[code]);
        float d = __builtin_fmaf(-2.0f, acc, bias);
        atomicMin(&best[sl], order_key(d, code));
    }
    __syncthreads();

    {
        if (nslice > 1) {
            // merge across slices through the records; the last slice of this chunk carries on
            int *oflag = ticket + 1;
            if (tid < nlive && best[tid] != ~0ull) {
                RecMeta *gm = (RecMeta *)(records + (size_t)(base + tid) * rec_bytes(D) + (size_t)D * 4);
                atomicMin(&gm->best, best[tid]);
            }
            if (overflow && tid == 0) atomicOr(oflag, 1);
            // everything handed over is an agent-scope atomic (and read back with agent-scope loads): what the ticket needs is
            // that every wave's atomics have COMPLETED before it is taken -- a counter wait per wave and the barrier, no cache
            // write-back / invalidate (a __threadfence() pair here cost 1.5 - 3 us per slice on a small batch)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (tid == 0)
                misc[2] = (__hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == nslice - 1);
            __syncthreads();
            if (!misc[2]) { *not_last = true; return 0.0; }   // not the last slice (its partial is written by the last)
            if (tid < nlive) {
                const RecMeta *gm = (const RecMeta *)(records + (size_t)(base + tid) * rec_bytes(D) + (size_t)D * 4);
                best[tid] = __hip_atomic_load(&gm->best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            if (tid == 0) {
                misc[3] = __hip_atomic_load(oflag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);       // every slice has been here: the
                __hip_atomic_store(ticket + 1, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // pair is clean for the next op
            }
            __syncthreads();
            overflow = misc[3] != 0;
        }
    }

    DVQ_RSTAMP(4);
    // ---- winners; slots whose winner differs from pass 1 are rewritten
    if (tid < nlive) {
        const char *r2 = srec + tid * RB;
        const RecMeta m2 = *(const RecMeta *)(r2 + (size_t)D * 4);
        if (overflow || best[tid] == ~0ull) {
            for (int ry = 0; ry < m2.rep; ++ry)               // cannot resolve here: full exact evaluation of every position
                for (int rx = 0; rx < m2.rep; ++rx) {         // the token stands for; pass 1's loss terms are taken back below
                    int pos = atomicAdd(&counters[DVQ_C_EXACT], 1);
                    exact_list[pos] = m2.n + ry * Wout + rx;
                }
            int pos = atomicAdd(&misc[1], 1);
            rewrite[pos] = (tid << 20) | 0xFFFFF;
        } else {
            int win = (int)(best[tid] & 0xFFFFFFFFu);
            if (win != m2.prov) {
                int pos = atomicAdd(&misc[1], 1);
                rewrite[pos] = (tid << 20) | win;
            }
        }
    }
    __syncthreads();
    const int nrew = misc[1];
    double dsum = 0.0;
    for (int i = wave; i < nrew; i += RW) {           // one wave per rewritten token, 4 channels per lane
        const int sl = rewrite[i] >> 20, win = rewrite[i] & 0xFFFFF;
        const bool take_back_only = win == 0xFFFFF;   // token went to the exact list
        const char *r2 = srec + sl * RB;
        const RecMeta m2 = *(const RecMeta *)(r2 + (size_t)D * 4);
        const long n = m2.n;
        const int rep = m2.rep;
        const long bimg = n / HW;
        const int hw = (int)(n - bimg * HW);
        const float m = m2.m;
        float delta = 0.0f;
        for (int k0 = lane * 4; k0 < D; k0 += 256) {
            f32x4 zv = *(const f32x4 *)(r2 + k0 * 4);
            if (take_back_only && h_spill != nullptr) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float *hp = h_spill + ((size_t)bimg * D + k0 + j) * HW + hw;
                    for (int ry = 0; ry < rep; ++ry)
                        for (int rx = 0; rx < rep; ++rx) hp[(size_t)ry * Wout + rx] = zv[j];
                }
            }
            f32x4 eo = *(const f32x4 *)(E + (size_t)m2.prov * D + k0);
            f32x4 en_ = take_back_only ? eo : *(const f32x4 *)(E + (size_t)win * D + k0);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float dn = __fsub_rn(en_[j], zv[j]), dold = __fsub_rn(eo[j], zv[j]);
                if (zq != nullptr && !take_back_only) {
                    typename DvqLat<XT>::T *zp = (typename DvqLat<XT>::T *)zq + ((size_t)bimg * D + k0 + j) * HW + hw;
                    // FOLD: z_q := e[code] as in pass 1 (the record holds h by now; fl(h + fl(e - h)) is within 1e-6 of it)
                    const float v = FOLD ? en_[j] : __fadd_rn(zv[j], dn);
                    for (int ry = 0; ry < rep; ++ry)
                        for (int rx = 0; rx < rep; ++rx) zp[(size_t)ry * Wout + rx] = dvq_narrow<XT>(v);
                }
                float tn = take_back_only ? 0.0f : __fmul_rn(__fmul_rn(dn, dn), m);
                delta += tn - __fmul_rn(__fmul_rn(dold, dold), m);
            }
        }
        if (lane == 0 && !take_back_only)
            for (int ry = 0; ry < rep; ++ry)
                for (int rx = 0; rx < rep; ++rx) codes[n + (long)ry * Wout + rx] = (long long)win;
        delta *= (float)(rep * rep);
        dsum += (double)delta;
    }
    DVQ_RSTAMP(5);
    double tot = 0.0;
    if (want_loss) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) dsum += __shfl_xor(dsum, off);
        if (lane == 0) red[wave] = dsum;
        __syncthreads();
        if (tid == 0) {
#pragma unroll
            for (int w = 0; w < RW; ++w) tot += red[w];
        }
    }
    return tot;
}

template <int D, bool FOLD, int XT = 0>
__global__ __launch_bounds__(DVQ_RES_WAVES * 64, DVQ_RES_WAVES > 4 ? 1 : 2) void vq_resolve_kernel(
    const char *__restrict__ img, const DvqF16Meta *__restrict__ meta, const float *__restrict__ en_all,
    const float *__restrict__ E, int HW, int K,
    float *__restrict__ zq, long long *__restrict__ codes, double *__restrict__ partials,
    int *__restrict__ counters, int *__restrict__ exact_list, char *__restrict__ records, int rec_cap,
    int nslice, int *__restrict__ chunk_sync, int Wout, float *__restrict__ h_spill, const DvqConv cv,
    const double *__restrict__ p1_partials, int np1)
{
    __shared__ __attribute__((aligned(16))) char L[ResLds<D>::BYTES];
    (void)meta;
    DVQ_RSTAMP(0);
    // The workgroup that writes chunk blockIdx.x's partial (also for an empty chunk) folds its share of pass 1's per-block loss
    // sums into it, in a fixed order: the list kernel's finishing workgroup then adds gridDim.x numbers instead of np1 more.
    auto p1_share = [&]() -> double {
        const int per = (np1 + (int)gridDim.x - 1) / (int)gridDim.x;
        const int i0 = (int)blockIdx.x * per, i1 = (i0 + per < np1) ? i0 + per : np1;
        double a = 0.0;
        for (int i = i0; i < i1; ++i) a += p1_partials[i];
        return a;
    };
    // block -> (shard, chunk): the first DVQ_QSHARDS blocks take chunk 0 of every shard, and so on
    const int shard = blockIdx.x & (DVQ_QSHARDS - 1), chunk = blockIdx.x / DVQ_QSHARDS;
    int total = counters[DVQ_QCOUNT0 + shard];
    total = total < rec_cap ? total : rec_cap;
    total += shard * rec_cap;                                   // end of this shard's filled run
    const int base = shard * rec_cap + chunk * RES_SLOTS;
    const int slice = blockIdx.y;
    if (base >= total) {
        if (partials != nullptr && threadIdx.x == 0 && slice == 0) partials[blockIdx.x] = p1_share();
        return;
    }
    const int T = dvq_num_tiles(K);
    int tps = (T + nslice - 1) / nslice;                        // tiles per slice, a multiple of 4
    tps = (tps + DVQ_RES_WAVES - 1) / DVQ_RES_WAVES * DVQ_RES_WAVES;
    const int t_begin = slice * tps, t_end = (t_begin + tps < T) ? t_begin + tps : T;
    const int nlive = (total - base < RES_SLOTS) ? total - base : RES_SLOTS;
    DVQ_RSTAMP(1);
    bool not_last;
    const int wave0 = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);   // (a scalar: thread 0 is found again below without
    const double tot = resolve_chunk<D, FOLD, XT>(L, base, nlive, t_begin, t_end, img, en_all, E, HW, Wout, zq, codes, counters,   // keeping threadIdx.x in a register)
                                              exact_list, records, nslice, chunk_sync + 2 * blockIdx.x, h_spill, cv,
                                              partials != nullptr, &not_last);
    const bool thread0 = wave0 == 0 && __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) == 0;
    if (!not_last && partials != nullptr && thread0) partials[blockIdx.x] = tot + p1_share();
    DVQ_RSTAMP(6);
}

// resolver slices over the code tiles: 1 up to 64 tiles (K <= 2048), then one per 64 tiles, at most 8
int dvq_resolver_slices(int K)
{
    int T = dvq_num_tiles(K);
    int ns = (T + 63) / 64;
    return ns < 1 ? 1 : (ns > 8 ? 8 : ns);
}

int dvq_launch_resolver(int D, const char *img, const DvqF16Meta *meta, const float *en_all, const float *E,
                        int HWout, int K, float *zq, long long *codes, double *partials,
                        const FilterWs &w, int Wout, float *h_spill, const DvqFold *fd, hipStream_t st,
                        const double *p1_partials, int np1, int xt)
{
    const bool fold = fd != nullptr;
    decltype(&vq_resolve_kernel<64, false>) kernel;
    if (xt != 0) {
        if (fold || (xt != 1 && xt != 2)) return -1000;
        switch (D) {
        case 64:  kernel = xt == 1 ? vq_resolve_kernel<64, false, 1> : vq_resolve_kernel<64, false, 2>; break;
        case 128: kernel = xt == 1 ? vq_resolve_kernel<128, false, 1> : vq_resolve_kernel<128, false, 2>; break;
        case 256: kernel = xt == 1 ? vq_resolve_kernel<256, false, 1> : vq_resolve_kernel<256, false, 2>; break;
        default:  return -1000;
        }
    } else
    switch (D) {
    case 64:  kernel = fold ? vq_resolve_kernel<64, true> : vq_resolve_kernel<64, false>; break;
    case 128: kernel = fold ? vq_resolve_kernel<128, true> : vq_resolve_kernel<128, false>; break;
    case 256: kernel = fold ? vq_resolve_kernel<256, true> : vq_resolve_kernel<256, false>; break;
    default:  return -1000;
    }
    const int nslice = dvq_resolver_slices(K);
    hipLaunchKernelGGL(kernel, dim3(w.cap / RES_SLOTS, nslice), dim3(DVQ_RES_WAVES * 64), 0, st, img, meta, en_all, E, HWout, K,
                       zq, codes, partials, w.counters, w.exact_list, w.records, w.cap / DVQ_QSHARDS, nslice, w.chunk_sync, Wout,
                       h_spill, fold ? fd->cv : DvqConv{}, p1_partials, np1);
    return (int)hipGetLastError();
}

#ifdef DVQ_TUNING
int dvq_tuning_set_resolve(void *stamps, void *tokdbg) { return dvq_tuning_set_unit(stamps, tokdbg); }
#endif
