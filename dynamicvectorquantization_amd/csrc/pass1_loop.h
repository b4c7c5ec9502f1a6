// pass1_loop.h -- the 16x16x32 code loop of pass1_body (dvq_pass1.h), textually included there once per form:
// DVQ_NG = 2 scores both column groups of the wave (t2 = 0, 1), DVQ_NG = 1 the first one alone (the short form of SEL == 2: a wave
// whose second group holds only copies of coarser cells).  Everything the workgroup shares -- the counted vmcnt wait, the tile
// barrier, the DMA pieces of tile t + 3 at the same fragments, all 16 A-fragment reads and their counted waits -- is the same in
// both.  DVQ_NG = 0 (a wave of the workgroup-packed form, SEL == 2 at D = 256, with no column group to score) keeps the counted wait,
// the barrier and its DMA pieces, and nothing else.  Uses pass1_body's locals (b1, b2, bt, zb, lds, enraw, issue, issue_piece, T, q16, lane, wave) and no include guard.
#if DVQ_NG != 0
        f32x4 acc16[2][2];
        auto top2 = [&](int tt) {
#pragma unroll
            for (int t2 = 0; t2 < DVQ_NG; ++t2) {
                const float om = b1[t2];
#pragma unroll
                for (int r = 0; r < 8; r += 2) {             // r = 4 c2 + i
                    // running top-2 over the pair (g0, g1): with b2 <= b1 the new second-best is max(b2, med3(b1, g0, g1))
                    // and the new best max3(b1, g0, g1): 2.5 VALU ops per score; the register index rides in 4 mantissa bits
                    const float v0 = acc16[r >> 2][t2][r & 3], v1 = acc16[(r + 1) >> 2][t2][(r + 1) & 3];
                    float g0 = __uint_as_float((__float_as_uint(v0) & 0xFFFFFFF0u) | (unsigned)r);
                    float g1 = __uint_as_float((__float_as_uint(v1) & 0xFFFFFFF0u) | (unsigned)(r + 1));
                    float md = __builtin_amdgcn_fmed3f(b1[t2], g0, g1);
                    b1[t2] = vmax3_raw(b1[t2], g0, g1);
                    b2[t2] = vmax_raw(b2[t2], md);
                }
                bt[t2] = (b1[t2] != om) ? tt : bt[t2];
            }
        };
#endif
    for (int t = 0; t < T; ++t) {
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PER_TILE) : "memory");   // all but the youngest tile's DMA: tiles <= t + 1 landed
            __builtin_amdgcn_s_barrier();                    // tile t (everybody's DMA) landed; t-1 consumed
            asm volatile("" ::: "memory");
            if (S16 != 16) issue(t + 3);                     // D = 256: pieces ride between the MFMAs below
#if DVQ_NG == 0
            if (S16 == 16) issue(t + 3);                     // no column group: this wave's pieces of tile t + 3, at once
        }
#else
            // A fragments: hand-placed LDS reads, four k-steps ahead of the MFMA that consumes them
            // (ds_read returns in order: lgkmcnt(3) = "the oldest of my four reads has landed")
            const unsigned tile_a = (unsigned)(size_t)(const __attribute__((address_space(3))) char *)(
                                        lds + (t & (NBUF - 1)) * IMG_BYTES + lane * 16);
            f16x8 a0, a1, a2, a3;
#define DVQ_RD(dst, S) asm volatile("ds_read_b128 %0, %1 offset:%c2" : "=v"(dst) : "v"(tile_a), "i"((S) * 1024))
            DVQ_RD(a0, 0); DVQ_RD(a1, 1); DVQ_RD(a2, 2); DVQ_RD(a3, 3);
            __builtin_amdgcn_sched_barrier(0);
            if (t > 0) top2(t - 1);
            __builtin_amdgcn_sched_barrier(0);
            {
                // accumulator seeds of tile t, read behind the fragments: from the resident table (landed before tile 0's barrier),
                // or from this wave's own DMA copy (landed by the wait above)
                const unsigned seed_a = (unsigned)(size_t)(const __attribute__((address_space(3))) char *)(
                                            RES ? enraw + t * 32 + 4 * q16 : enraw + ((t & (NBUF - 1)) * NW + wave) * 64 + 4 * q16);
                f32x4 e0, e1;
                asm volatile("ds_read_b128 %0, %1" : "=v"(e0) : "v"(seed_a));
                asm volatile("ds_read_b128 %0, %1 offset:64" : "=v"(e1) : "v"(seed_a));
                asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(e0), "+v"(e1), "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3) :: "memory");
                acc16[0][0] = e0; if (DVQ_NG == 2) acc16[0][1] = e0;
                acc16[1][0] = e1; if (DVQ_NG == 2) acc16[1][1] = e1;
            }
            __builtin_amdgcn_sched_barrier(0);
#define DVQ_PIECE(Q) if constexpr ((Q) < PER_TILE) { issue_piece(t + 3, Q); }
#define DVQ_MM(src, F, WAIT, NEXT)                                                                             \
            asm volatile("s_waitcnt lgkmcnt(" #WAIT ")" ::: "memory");                                            \
            __builtin_amdgcn_sched_barrier(0);                                                                    \
            acc16[(F) / S32][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(src, zb[0][(F) % S32], acc16[(F) / S32][0], 0, 0, 0); \
            if (DVQ_NG == 2)                                                                                      \
            acc16[(F) / S32][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(src, zb[1][(F) % S32], acc16[(F) / S32][1], 0, 0, 0); \
            __builtin_amdgcn_sched_barrier(0);                                                                    \
            if ((F) + 4 < S16) { DVQ_RD(src, ((F) + 4 < S16 ? (F) + 4 : 0)); }                                  \
            NEXT
            __builtin_amdgcn_s_setprio(1);
            if (S16 == 16) {
                // the next ring tile's DMA pieces are issued between MFMAs: each ~100-cycle issue stall
                // then overlaps the MFMA already in the pipe instead of preceding the whole chain
                DVQ_MM(a0, 0, 0, ) DVQ_MM(a1, 1, 1, DVQ_PIECE(0)) DVQ_MM(a2, 2, 2, ) DVQ_MM(a3, 3, 3, )
                DVQ_MM(a0, 4, 3, DVQ_PIECE(1)) DVQ_MM(a1, 5, 3, ) DVQ_MM(a2, 6, 3, ) DVQ_MM(a3, 7, 3, DVQ_PIECE(2))
                DVQ_MM(a0, 8, 3, ) DVQ_MM(a1, 9, 3, ) DVQ_MM(a2, 10, 3, DVQ_PIECE(3)) DVQ_MM(a3, 11, 3, )
                DVQ_MM(a0, 12, 3, ) DVQ_MM(a1, 13, 2, DVQ_PIECE(4)) DVQ_MM(a2, 14, 1, ) DVQ_MM(a3, 15, 0, )
            } else if (S16 == 8) {
                DVQ_MM(a0, 0, 0, ) DVQ_MM(a1, 1, 1, ) DVQ_MM(a2, 2, 2, ) DVQ_MM(a3, 3, 3, )
                DVQ_MM(a0, 4, 3, ) DVQ_MM(a1, 5, 2, ) DVQ_MM(a2, 6, 1, ) DVQ_MM(a3, 7, 0, )
            } else {
                DVQ_MM(a0, 0, 0, ) DVQ_MM(a1, 1, 0, ) DVQ_MM(a2, 2, 0, ) DVQ_MM(a3, 3, 0, )
            }
#undef DVQ_MM
#undef DVQ_RD
#undef DVQ_PIECE
            __builtin_amdgcn_s_setprio(0);
        }
        top2(T - 1);
#endif
