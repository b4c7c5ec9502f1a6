// vq_pass1_wide.hip -- the two-blocks-per-wave form of pass 1 for large codebooks (D = 256) and its launcher.
#include "dvq_pass1.h"

// ---------------------------------------------------------------------------------------------
// pass 1, large codebooks ("wide" form, D = 256): a wave scores TWO blocks of 32 tokens against every
// code tile, so each A fragment read from LDS feeds two MFMAs and the ring DMA / barrier per tile are
// amortised over 32 MFMAs instead of 16.  There is no room left for the fp32 copy of z (the two blocks'
// fp16 fragments take 128 VGPRs): z is read again in the epilogue -- 2 KiB per token next to the
// >= 2 MiB of codebook every token is scored against.  Same top-2 tracking, same bound, same queue,
// records and outputs as vq_assign_filter_kernel.
// ---------------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(256, 2) void vq_assign_filter_wide_kernel(
    const float *__restrict__ z, const char *__restrict__ img, const DvqF16Meta *__restrict__ meta,
    const float *__restrict__ E, const float *__restrict__ mask,
    int HW, int K, long N, float *__restrict__ zq, long long *__restrict__ codes,
    double *__restrict__ partials, int *__restrict__ counters, int *__restrict__ exact_list,
    char *__restrict__ records, int rec_cap, int nparts_pass1)
{
    constexpr int NW = 4;
    constexpr int S16 = D / 16;
    static_assert(S16 == 16, "the wide form is written for D = 256");
    constexpr int IMG_BYTES = S16 * 1024;
    constexpr int TILE_STRIDE = IMG_BYTES + 256;
    constexpr int CPW = (S16 + NW - 1) / NW;
    constexpr int PER_TILE = CPW + 1;
    constexpr int NBUF = 4;
    static_assert(NBUF * IMG_BYTES + NBUF * NW * 64 * 4 + NW * 2048 == dvq_pass1_lds_bytes(D), "the launch's LDS is this carve");
    extern __shared__ __attribute__((aligned(16))) char lds[];
    float *enraw = (float *)(lds + NBUF * IMG_BYTES);        // [NBUF][NW][64] accumulator seeds, per-wave copy

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 31, h = lane >> 5;
    const int T = dvq_num_tiles(K);
    const float sB = meta->scale_b;

    auto issue_piece = [&](int t, int q) {
        const int tt = (t < T) ? t : T - 1;
        const char *src = img + (size_t)tt * TILE_STRIDE;
        if (q < CPW) {
            const char *s0 = src + wave * (CPW * 1024) + lane * 16;   // (one base + instruction offsets: vq_assign_filter_kernel)
            char *d0 = lds + (t & (NBUF - 1)) * IMG_BYTES + wave * (CPW * 1024);
            switch (q) {
            case 0: glds16_off<0>(s0, d0); break;
            case 1: glds16_off<1024>(s0, d0); break;
            case 2: glds16_off<2048>(s0, d0); break;
            default: glds16_off<3072>(s0, d0); break;
            }
        } else {
            glds4(src + IMG_BYTES + lane * 4, enraw + ((t & (NBUF - 1)) * NW + wave) * 64);
        }
    };
    auto issue = [&](int t) {
#pragma unroll
        for (int q = 0; q < PER_TILE; ++q) issue_piece(t, q);
    };
    issue(0);
    issue(1);
    issue(2);

    const int tile_id = xcd_swizzle(blockIdx.x, gridDim.x);
    int nn[2];                                               // token of this lane in block u, -1 = past the end
    size_t zbase[2];                                         // element offset of its channel 8h
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const long n_raw = ((long)tile_id * NW + wave) * 64 + 32 * u + c;
        nn[u] = (n_raw < N) ? (int)n_raw : -1;
        const long q = (nn[u] >= 0) ? nn[u] : N - 1;
        const long bimg = q / HW;
        zbase[u] = ((size_t)bimg * D + 8 * h) * HW + (size_t)(q - bimg * HW);
    }

    // ---- prologue: per block, z in batches of four k-steps -> fp16 fragments, exact-order norm, bound
    f16x8 zh[2][2];                                          // only the current pair of k-steps lives in the load layout
    f16x8 zb[2][2][S16 / 2];                                 // [block][token half][k-step of 32] in 16x16x32 operand order
    float xn[2], thr2W[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const float *zp = z + zbase[u];
        float pa[2][8];
        float amax = 0.0f, zeta2 = 0.0f;
        const float *zpb = zp;                              // advances by four k-steps per batch
#pragma unroll
        for (int sb = 0; sb < S16; sb += 4) {
            float zf[4][8];
            __builtin_amdgcn_s_setprio(2);
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int j = 0; j < 8; ++j) zf[q][j] = DVQ_LOAD_Z(zpb + (size_t)(16 * q + j) * HW);
            __builtin_amdgcn_s_setprio(0);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int s = sb + q;
                u32x4 packed;
#pragma unroll
                for (int j2 = 0; j2 < 4; ++j2) {
                    const float v0 = zf[q][2 * j2], v1 = zf[q][2 * j2 + 1];
                    const float q0 = sq_rn(v0), q1 = sq_rn(v1);
                    pa[s & 1][2 * j2] = (s < 2) ? q0 : __fadd_rn(pa[s & 1][2 * j2], q0);
                    pa[s & 1][2 * j2 + 1] = (s < 2) ? q1 : __fadd_rn(pa[s & 1][2 * j2 + 1], q1);
                    amax = vmax_abs(amax, v0);
                    amax = vmax_abs(amax, v1);
                    f32x2 vv = {v0, v1};
                    f16x2 hh = __builtin_convertvector(vv, f16x2);
                    packed[j2] = __builtin_bit_cast(unsigned, hh);
                    const float r0 = v0 - (float)hh[0], r1 = v1 - (float)hh[1];     // exact
                    zeta2 = __builtin_fmaf(r0, r0, zeta2);
                    zeta2 = __builtin_fmaf(r1, r1, zeta2);
                }
                zh[u][s & 1] = __builtin_bit_cast(f16x8, packed);
                if (s & 1) {                                 // same permutation as vq_assign_filter_kernel, per-wave LDS scratch
                    char *scr = lds + NBUF * IMG_BYTES + NBUF * NW * 64 * 4 + wave * 2048;
                    *(f16x8 *)(scr + lane * 16) = zh[u][0];
                    *(f16x8 *)(scr + 1024 + lane * 16) = zh[u][1];
#pragma unroll
                    for (int t2 = 0; t2 < 2; ++t2) {
                        const int srcl = 16 * t2 + (lane & 15) + 32 * ((lane >> 4) & 1);
                        zb[u][t2][s >> 1] = *(const f16x8 *)(scr + (lane >> 5) * 1024 + srcl * 16);
                    }
                }
            }
            // one batch of 32 loads at a time (register budget): the next batch's addresses depend,
            // opaquely, on this batch's last converted fragment
            zpb += (size_t)64 * HW;
            asm volatile("" : "+v"(zpb) : "v"(zb[u][1][(sb + 3) >> 1]));
        }
        float t8[8];
#pragma unroll
        for (int l = 0; l < 8; ++l) {
            float o0 = __shfl_xor(pa[0][l], 32), o1 = __shfl_xor(pa[1][l], 32);
            float a0_ = h == 0 ? pa[0][l] : o0;
            float a1_ = h == 0 ? o0 : pa[0][l];
            float a2_ = h == 0 ? pa[1][l] : o1;
            float a3_ = h == 0 ? o1 : pa[1][l];
            t8[l] = __fadd_rn(__fadd_rn(__fadd_rn(a0_, a1_), a2_), a3_);
        }
        float x = t8[0];
#pragma unroll
        for (int l = 1; l < 8; ++l) x = __fadd_rn(x, t8[l]);
        xn[u] = x;
        amax = fmaxf(amax, __shfl_xor(amax, 32));
        zeta2 += __shfl_xor(zeta2, 32);
        thr2W[u] = dvq_filter_threshold(x, amax, zeta2, sB, meta);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // tiles 0..2 (own DMA) landed during the prologue

    // ---- code loop
    int code[2];
    float thr[2];
    bool undecided[2], hopeless[2], valid[2];
    float bestv[2], secondv[2];
    {
        // 16x16x32 form: every A fragment (16 codes x 32 k) feeds four MFMAs (two blocks x two token halves)
        constexpr int S32 = S16 / 2;
        const int q16 = lane >> 4;
        float b1[2][2], b2[2][2];
        int bt[2][2];
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int t2 = 0; t2 < 2; ++t2) { b1[u][t2] = -__builtin_inff(); b2[u][t2] = -__builtin_inff(); bt[u][t2] = 0; }
        for (int t = 0; t < T; ++t) {
            const float *seeds = enraw + ((t & (NBUF - 1)) * NW + wave) * 64 + 4 * q16;
            f32x4 acc16[2][2][2];                            // [block][code half][token half]
#pragma unroll
            for (int c2 = 0; c2 < 2; ++c2) {
                const f32x4 e4 = *(const f32x4 *)(seeds + 16 * c2);
                acc16[0][c2][0] = e4; acc16[0][c2][1] = e4; acc16[1][c2][0] = e4; acc16[1][c2][1] = e4;
            }
            if (t > 0) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PER_TILE) : "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            const unsigned tile_a = (unsigned)(size_t)(const __attribute__((address_space(3))) char *)(
                                        lds + (t & (NBUF - 1)) * IMG_BYTES + lane * 16);
            f16x8 a0, a1, a2, a3;
            asm volatile("" : "+v"(acc16[0][0][0]), "+v"(acc16[0][0][1]), "+v"(acc16[0][1][0]), "+v"(acc16[0][1][1]),
                              "+v"(acc16[1][0][0]), "+v"(acc16[1][0][1]), "+v"(acc16[1][1][0]), "+v"(acc16[1][1][1]));
            __builtin_amdgcn_sched_barrier(0);
#define DVQ_RD(dst, S) asm volatile("ds_read_b128 %0, %1 offset:%c2" : "=v"(dst) : "v"(tile_a), "i"((S) * 1024))
#define DVQ_MM4(src, F, WAIT, NEXT)                                                                                       \
            asm volatile("s_waitcnt lgkmcnt(" #WAIT ")" ::: "memory");                                                       \
            __builtin_amdgcn_sched_barrier(0);                                                                               \
            acc16[0][(F) / S32][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(src, zb[0][0][(F) % S32], acc16[0][(F) / S32][0], 0, 0, 0); \
            acc16[0][(F) / S32][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(src, zb[0][1][(F) % S32], acc16[0][(F) / S32][1], 0, 0, 0); \
            acc16[1][(F) / S32][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(src, zb[1][0][(F) % S32], acc16[1][(F) / S32][0], 0, 0, 0); \
            acc16[1][(F) / S32][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(src, zb[1][1][(F) % S32], acc16[1][(F) / S32][1], 0, 0, 0); \
            __builtin_amdgcn_sched_barrier(0);                                                                               \
            if ((F) + 4 < S16) { DVQ_RD(src, ((F) + 4 < S16 ? (F) + 4 : 0)); }                                             \
            NEXT
            DVQ_RD(a0, 0); DVQ_RD(a1, 1); DVQ_RD(a2, 2); DVQ_RD(a3, 3);
            __builtin_amdgcn_s_setprio(1);
            DVQ_MM4(a0, 0, 3, ) DVQ_MM4(a1, 1, 3, issue_piece(t + 3, 0);) DVQ_MM4(a2, 2, 3, ) DVQ_MM4(a3, 3, 3, )
            DVQ_MM4(a0, 4, 3, issue_piece(t + 3, 1);) DVQ_MM4(a1, 5, 3, ) DVQ_MM4(a2, 6, 3, ) DVQ_MM4(a3, 7, 3, issue_piece(t + 3, 2);)
            DVQ_MM4(a0, 8, 3, ) DVQ_MM4(a1, 9, 3, ) DVQ_MM4(a2, 10, 3, issue_piece(t + 3, 3);) DVQ_MM4(a3, 11, 3, )
            DVQ_MM4(a0, 12, 3, ) DVQ_MM4(a1, 13, 2, issue_piece(t + 3, 4);) DVQ_MM4(a2, 14, 1, ) DVQ_MM4(a3, 15, 0, )
#undef DVQ_MM4
#undef DVQ_RD
            __builtin_amdgcn_s_setprio(0);
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int t2 = 0; t2 < 2; ++t2) {
                    const float om = b1[u][t2];
#pragma unroll
                    for (int r = 0; r < 8; r += 2) {
                        const float v0 = acc16[u][r >> 2][t2][r & 3], v1 = acc16[u][(r + 1) >> 2][t2][(r + 1) & 3];
                        float g0 = __uint_as_float((__float_as_uint(v0) & 0xFFFFFFF0u) | (unsigned)r);
                        float g1 = __uint_as_float((__float_as_uint(v1) & 0xFFFFFFF0u) | (unsigned)(r + 1));
                        float md = __builtin_amdgcn_fmed3f(b1[u][t2], g0, g1);
                        b1[u][t2] = vmax3_raw(b1[u][t2], g0, g1);
                        b2[u][t2] = vmax_raw(b2[u][t2], md);
                    }
                    bt[u][t2] = (b1[u][t2] != om) ? t : bt[u][t2];
                }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // surplus ring DMA
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            float rb[2], rs[2];
            int rc[2];
#pragma unroll
            for (int t2 = 0; t2 < 2; ++t2) {
                float mb = b1[u][t2], ms = b2[u][t2];
                int mt = bt[u][t2], mq = q16;
#pragma unroll
                for (int off = 16; off <= 32; off <<= 1) {
                    const float o1 = __shfl_xor(mb, off), o2 = __shfl_xor(ms, off);
                    const int ot = __shfl_xor(mt, off), oq = __shfl_xor(mq, off);
                    const bool other_wins = (o1 > mb) || (o1 == mb && ((lane ^ off) < lane));
                    ms = fmaxf(other_wins ? mb : o1, fmaxf(ms, o2));
                    mb = other_wins ? o1 : mb;
                    mt = other_wins ? ot : mt;
                    mq = other_wins ? oq : mq;
                }
                const int r = (int)(__float_as_uint(mb) & 15u);
                rb[t2] = mb; rs[t2] = ms;
                rc[t2] = mt * 32 + 16 * (r >> 2) + 4 * mq + (r & 3);
            }
            const int srcl = c & 15;
            const float x0 = __shfl(rb[0], srcl), x1 = __shfl(rb[1], srcl);
            const float y0 = __shfl(rs[0], srcl), y1 = __shfl(rs[1], srcl);
            const int c0 = __shfl(rc[0], srcl), c1 = __shfl(rc[1], srcl);
            bestv[u] = (c >> 4) ? x1 : x0;
            secondv[u] = (c >> 4) ? y1 : y0;
            code[u] = (c >> 4) ? c1 : c0;
        }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        thr[u] = bestv[u] - thr2W[u];
        const bool final_ok = (bestv[u] - secondv[u]) > thr2W[u];
        valid[u] = nn[u] >= 0;
        hopeless[u] = !(code[u] < K) || !(thr[u] == thr[u]);
        undecided[u] = valid[u] && !hopeless[u] && !final_ok;
    }
    const unsigned long long um0 = __ballot(undecided[0] && h == 0), um1 = __ballot(undecided[1] && h == 0);
    const int shard = blockIdx.x & (DVQ_QSHARDS - 1);
    int slot_raw = 0;
    const int nund = (int)__popcll(um0) + (int)__popcll(um1);
    if (nund != 0 && lane == 0) slot_raw = atomicAdd(&counters[DVQ_QCOUNT0 + shard], nund);
    int slot[2] = {-1, -1};
    if (nund != 0) {                                        // wave-uniform
        const int base = __shfl(slot_raw, 0);
        const unsigned long long lt = (1ull << c) - 1ull;
        slot[0] = undecided[0] ? base + (int)__popcll(um0 & lt) : -1;
        slot[1] = undecided[1] ? base + (int)__popcll(um0) + (int)__popcll(um1 & lt) : -1;
#pragma unroll
        for (int u = 0; u < 2; ++u)
            if (slot[u] >= rec_cap) { hopeless[u] = true; slot[u] = -1; }     // shard full -> exact list
    }
#pragma unroll
    for (int u = 0; u < 2; ++u)
        if (valid[u] && hopeless[u] && h == 0) {
            int pos = atomicAdd(&counters[DVQ_C_EXACT], 1);
            exact_list[pos] = nn[u];
        }

    // ---- epilogue per block: z again, chosen codebook row, z_q, loss term, record of a queued token
    float lsum = 0.0f;
    auto epilogue = [&](const int n, const bool active, const int cd, const size_t zb, const int sl,
                        const float xnu, const float thru) {
        if (!active) return;
        if (h == 0) codes[n] = (long long)cd;
        const float *zp = z + zb;
        const float *ep = E + (size_t)cd * D + 8 * h;
        const float m = (mask != nullptr) ? mask[n] : 1.0f;
        char *rec = (sl >= 0) ? records + ((size_t)shard * rec_cap + sl) * rec_bytes(D) : nullptr;
        auto finish = [&](auto store_tag) {
            constexpr bool STORE = decltype(store_tag)::value;
            float *zqp = STORE ? zq + zb : nullptr;
            const float *zpe = zp, *epe = ep;                // advance by two k-steps per batch
#pragma unroll
            for (int s0 = 0; s0 < S16; s0 += 2) {
                float zf[2][8];
                f32x4 eg[2][2];
#pragma unroll
                for (int q = 0; q < 2; ++q) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) zf[q][j] = DVQ_LOAD_Z(zpe + (size_t)(16 * q + j) * HW);
                    eg[q][0] = *(const f32x4 *)(epe + 16 * q);
                    eg[q][1] = *(const f32x4 *)(epe + 16 * q + 4);
                }
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    const int s = s0 + q;
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        float e = eg[q][j >> 2][j & 3];
                        float diff = __fsub_rn(e, zf[q][j]);
                        if (STORE) DVQ_STORE_ZQ(zqp + (size_t)(16 * s + j) * HW, __fadd_rn(zf[q][j], diff));
                        lsum = __fadd_rn(lsum, __fmul_rn(__fmul_rn(diff, diff), m));
                    }
                    if (rec != nullptr) {
                        f32x4 lo = {zf[q][0], zf[q][1], zf[q][2], zf[q][3]};
                        f32x4 hi = {zf[q][4], zf[q][5], zf[q][6], zf[q][7]};
                        *(f32x4 *)(rec + (16 * s + 8 * h) * 4) = lo;
                        *(f32x4 *)(rec + (16 * s + 8 * h + 4) * 4) = hi;
                    }
                }
                zpe += (size_t)32 * HW;
                epe += 32;
                asm volatile("" : "+v"(zpe), "+v"(epe) : "v"(lsum));     // next batch's loads wait for this one
            }
        };
        if (zq != nullptr) finish(std::true_type{});
        else finish(std::false_type{});
        if (rec != nullptr && h == 0) {
            RecMeta rm;
            rm.n = n; rm.xn = xnu; rm.thr = thru; rm.m = m; rm.prov = cd;
            rm.best = ~0ull; rm.rep = 1;
            *(RecMeta *)(rec + (size_t)D * 4) = rm;
        }
    };
    epilogue(nn[0], valid[0] && !hopeless[0], code[0], zbase[0], slot[0], xn[0], thr[0]);
    asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    epilogue(nn[1], valid[1] && !hopeless[1], code[1], zbase[1], slot[1], xn[1], thr[1]);
    if (partials != nullptr) {
        double dsum = (double)lsum;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) dsum += __shfl_xor(dsum, off);
        __syncthreads();
        double *red = (double *)lds;
        if (lane == 0) red[wave] = dsum;
        __syncthreads();
        if (tid == 0) {                                     // this grid is half the standard one: fill both slots
            partials[2 * blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
            if (2 * (int)blockIdx.x + 1 < nparts_pass1) partials[2 * blockIdx.x + 1] = 0.0;
        }
    }
}

int dvq_launch_pass1_wide(const P1Args &a)
{
    return dvq_launch_lds<vq_assign_filter_wide_kernel<256>>(dim3((unsigned)((a.N + 255) / 256)), dim3(256), dvq_pass1_lds_bytes(256), a.st,
                                                             a.z, a.img16, a.meta, a.E, a.mask, a.HW, a.K, a.N, a.zq, a.codes, a.partials,
                                                             a.w.counters, a.w.exact_list, a.w.records, a.w.cap / DVQ_QSHARDS,
                                                             (int)((a.N + 127) / 128));
}
