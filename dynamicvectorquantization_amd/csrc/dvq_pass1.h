// dvq_pass1.h -- pass 1 of the fp16-filter assign (contract and error budget: header of vq_assign_filter.hip): the device body
// every form shares, the four kernel families around it, and the launch templates.  The kernels are instantiated, and launched,
// by one translation unit per (D, resident seed table) -- vq_pass1_d<D>[_res].hip, each a call of launch_pass1_res<D, RES> --
// so no kernel handle crosses an object boundary; the wide form (vq_pass1_wide.hip) and the resolver (vq_resolve.hip) are
// units of their own and take the host-side types from here.
// The code loop's text is pass1_loop.h, included by pass1_body once per form (two, one or no column group; the latter two: SEL == 2).
#pragma once
#include "dvq_filter.h"
#include <type_traits>

// z is read once and z_q written once per launch: stream them past L2 (nt) so that the codebook
// image and the fp32 codebook rows keep their lines
#define DVQ_LOAD_Z(p) __builtin_nontemporal_load(p)
#define DVQ_STORE_ZQ(p, v) __builtin_nontemporal_store((v), (p))
// the same through buffer instructions (resource = wave-uniform base, vector byte offset, scalar byte offset; aux 2 = nt)
#define DVQ_BUF_LOAD(rsrc, voff, soff, AUX) __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32((rsrc), (voff), (soff), (AUX)))
#define DVQ_BUF_STORE(v, rsrc, voff, soff) __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, (float)(v)), (rsrc), (voff), (soff), 2)
// 16-bit latents (XT = DVQ_DTYPE_F16 / DVQ_DTYPE_BF16, dvq_common.h): 2-byte buffer accesses, widened behind the load and narrowed
// (round-to-nearest-even) in front of the store -- the registers in between are the fp32 kernel's
#define DVQ_BUF_LOAD16(XT, rsrc, voff, soff, AUX) dvq_widen_bits<XT>(__builtin_amdgcn_raw_buffer_load_b16((rsrc), (voff), (soff), (AUX)))
#define DVQ_BUF_STORE16(XT, v, rsrc, voff, soff) __builtin_amdgcn_raw_buffer_store_b16(dvq_narrow_bits<XT>(v), (rsrc), (voff), (soff), 2)
// the per-lane select prologue (SEL = 1) reads lines of the coarser branches that neighbouring waves read again:
// plain loads keep them in L2
#define DVQ_LOAD_SEL(p) (*(p))
// (Round 3's timing-only ablation switches, the per-CU anti-phase lock, the early-DMA variant and the per-workgroup clock stamps
// left pass 1 in round 4: their results are in profiles/archive/r03_pass1_*.json and DESIGN.md section 5.1, the code in git history
// up to commit "Feature-router gate as a tiled GEMM".)

// ---------------------------------------------------------------------------------------------
// pass 1: 4-wave workgroups of 128 consecutive tokens, TWO per CU (<= 256 VGPRs).  A wave keeps its
// 32 tokens twice in registers -- fp32 (D/2 VGPRs, read once, reused for z_q and the resolver
// record: z is never re-read, HBM traffic = the algorithmic bytes) and fp16 MFMA fragments (D/4).
// The code loop runs on v_mfma_f32_16x16x32_f16 (tile image "16" of the prep buffer): the latents are
// converted in the load layout (lane = token, 8 consecutive channels) and permuted into the B-operand
// order through a 2-KiB per-wave LDS scratch; every A fragment (16 codes x 32 k) feeds two MFMAs.
//
// SEL: 0 = dense z.
//      1 = the router select fused in (DvqRouted, dense view): token n is output position n, its source
//          vector sits in the encoder branch that won its cell (per-lane source pointer and channel stride).
//      2 = the same for a 32-wide output grid (every reference config): the workgroup's four output rows
//          need exactly ONE 128-B line per channel of the 2x-coarser branch (dual: coarse; triple: median)
//          and one 32-B piece of the 4x-coarser one (triple: coarse).  Those are DMA'd ONCE per workgroup
//          into ring slots the code loop does not need yet and read back with ds_read_b32; the fine branch
//          is read by every lane with the dense kernel's load pattern.  With the per-lane form (SEL = 1) the
//          two / four waves that share a coarse line each fetched it (PMC: 2.1x the coarse bytes).
//
// CONV: the model's 1x1 quant_conv (qconv.hip) runs as the PROLOGUE: instead of loading its latents a wave computes them,
//       h = W x + bias for its 32 tokens, on v_mfma_f32_32x32x16_f16 at fp32 grade (x = hi + lo per token, W = hi + lo,
//       hi*hi + hi*lo + lo*hi; qconv.hip's arithmetic), streaming x in k-steps of 16 input channels (8 loads per lane, three
//       k-steps in flight) and the weight images through the code ring's four slots (16 KiB per k-step: 8 row tiles x hi / lo).
//       The rows of a weight tile are permuted (qconv_row_channel) so that the 128 accumulator registers of a lane ARE
//       zf[s][j] in the layout the rest of the kernel expects; h never goes to memory (except the rows of tokens handed to
//       the exact-list kernel, which reads them from cv.h_buf).  The per-token power-of-two scale of x follows the running
//       maximum: when a k-step brings a value that would leave the fp16 range the accumulators are rescaled (exact, a
//       workgroup-rare event), so no second pass over x is needed.
// ---------------------------------------------------------------------------------------------
#ifdef DVQ_TUNING
// diagnostic of the tuning build only: per-token (best, second, 2W, code) of the production arithmetic for the bound audit
// (tools/bound_audit.py --production).  Written to a buffer of its own; no output value is computed from it.
// Device code is not relocatable, so EVERY translation unit that includes this header holds its own copy of the two pointers: a
// unit whose kernels read them defines a setter around dvq_tuning_set_unit, and dvq_tuning_buffers (vq_assign_filter.hip)
// calls every one of them.  On the device each copy is the plain global it always was (same name, same addressing in the
// kernels); the host's handle to it is per unit (static), and the asm label keeps the name the host registers equal to the device's.
#ifdef __HIP_DEVICE_COMPILE__
#define DVQ_TUNING_PTR __device__
#else
#define DVQ_TUNING_PTR static __device__
#endif
DVQ_TUNING_PTR float *g_dvq_tokdbg __asm__("g_dvq_tokdbg") = nullptr;                  // [N][4]
// ... and stage stamps of the split form's workgroups (100-MHz wall clock): [workgroup][8] (tools/archive/split_timeline.py);
// the resolver's workgroups stamp behind those (vq_resolve.hip: DVQ_RSTAMP)
DVQ_TUNING_PTR unsigned long long *g_dvq_stamps __asm__("g_dvq_stamps") = nullptr;
#define DVQ_STAMP(i) do { if (SPLIT && g_dvq_stamps != nullptr && threadIdx.x == 0) g_dvq_stamps[(size_t)blockIdx.x * 8 + (i)] = wall_clock64(); } while (0)
static inline int dvq_tuning_set_unit(void *stamps, void *tokdbg)
{
    int rc = (int)hipMemcpyToSymbol(HIP_SYMBOL(g_dvq_stamps), &stamps, sizeof(void *));
    if (rc) return rc;
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_dvq_tokdbg), &tokdbg, sizeof(void *));
}
#else
#define DVQ_STAMP(i) do { } while (0)
#endif

// (Round 5 built the resolver INTO this launch -- consumer workgroups appended to the grid, records handed over with sc1
// write-through stores / stamps / sc1 loads, decisions through a rewrite list -- bit-exact and slower: the consumers get slots only
// when the last generation of token blocks retires, and what they do beside those blocks costs the blocks as much as it would cost
// afterwards: profiles/r05_fused_consumers_negative.json; the code is in git history, commit "Fused form of the filter path".)
// NT: the latents are read with the non-temporal hint (a launch streams more than the 256-MB memory-side cache holds: keep L2 for
// the code image and the codebook rows) or with plain loads (vq_assign_filter_cached_kernel: a batch whose features FIT that cache
// was just written by the encoder / read by the router gate, and plain loads are served from it: -6 % on the configs[3] per-GPU
// step, profiles/archive/r04_cache_policy.json)
// FLAT: the latents are ROW-MAJOR [N, D] (a token's channels contiguous: quantize2_list.py:153-170, channel_last inputs,
// VQEmbedding.forward) -- the same tensor as [B = N, D, HW = 1], but read and written as what it is: a lane's 8 channels of a
// k-step are 32 contiguous bytes = two 16-byte accesses (32 loads and 32 stores per lane instead of 128 each; with lane = token
// and 4-byte accesses at a stride of D * 4 bytes every wave-instruction touched 64 lines for 256 useful bytes).
// SPLIT (small batches: fewer token blocks than CUs; vq_assign_filter_split_kernel): `ksplit` workgroups share a token block, each
// scores it against its own slice of the code tiles -- a lone workgroup's code loop is an issue-bound ~1330 cycles per tile whoever
// else is on the chip, 20 of the 27 us the kernel takes for BASELINE configs[0] (1024 tokens on 8 of 256 CUs) -- and leaves
// (best, second, code) per token in `split`; the workgroup that takes a block's last ticket merges them (lower slice wins ties, as
// the lower tile does in the loop) and runs the epilogue of the whole block.  Everything downstream sees what one workgroup
// would have produced, up to which of two equal scores is called best (tokens that close are undecided either way).
// Dynamic LDS of every form of pass 1 (the wide kernel's too): 4 ring slots of a code tile's image (D / 16 KiB each), the slots'
// accumulator seeds per wave ([4][4 waves][64] floats) and a 2-KiB permutation scratch per wave -- the carve below
#define DVQ_SEED_TABLE_TILES 32   // code tiles whose seeds fit the seeds area as one table ([32 tiles][32] floats = its 4 KiB)
constexpr size_t dvq_pass1_lds_bytes(int D) { return 4 * (size_t)(D / 16) * 1024 + 4 * 4 * 64 * sizeof(float) + 4 * 2048; }

// XT != 0: z and zq hold 16-bit latents (passed through the float pointers; only their bytes are addressed).  The dense lane-per-token
// form alone has it (any HW; HW == 1 is the row-major tensor): the latents are widened where the loads land and z_q is narrowed
// at the stores, everything between -- fragments, bound, records, loss term -- is the fp32 kernel's on the widened values.
template <int D, int SEL, bool CONV, bool FOLD, bool NT, bool RES, bool FLAT = false, bool SPLIT = false, int XT = 0>
__device__ __forceinline__ void pass1_body(
    const float *__restrict__ z, const char *__restrict__ img, const DvqF16Meta *__restrict__ meta,
    const float *__restrict__ E, const float *__restrict__ mask,
    int HW, int K, long N, float *__restrict__ zq, long long *__restrict__ codes,
    double *__restrict__ partials, int *__restrict__ counters, int *__restrict__ exact_list,
    char *__restrict__ records, int rec_cap, const DvqRouted &rv, const DvqConv &cv,
    f32x4 *__restrict__ split = nullptr, int ksplit = 1)
{
    static_assert(!SPLIT || SEL != 2, "the split form: dense or per-lane select; plain, with the conv prologue, or on the folded codebook");
    static_assert(!(SPLIT && FLAT && SEL != 0), "row-major latents are a dense op");
    static_assert(!CONV || (D == 256 && SEL != 2), "the conv prologue exists for D = 256, dense or per-lane select");
    static_assert(!(CONV && FOLD), "the conv is either computed (CONV) or folded into the code image (FOLD)");
    static_assert(!FLAT || (SEL == 0 && !CONV), "the row-major form is a dense op");
    static_assert(XT == 0 || (SEL == 0 && !CONV && !FOLD && !FLAT && !SPLIT), "16-bit latents: the dense lane-per-token form only");
    constexpr int ZB = XT ? 2 : 4;                           // bytes per latent in memory
    constexpr int NW = 4;
    constexpr int S16 = D / 16;
    constexpr int S32 = S16 / 2;
    constexpr int IMG_BYTES = S16 * 1024;
    constexpr int TILE_STRIDE = IMG_BYTES + 256;
    constexpr int CPW = (S16 + NW - 1) / NW;
    static_assert(CPW * NW == S16 && CPW <= 4, "a wave's chunks of a code tile are contiguous and within the instruction offset");
    constexpr int NBUF = 4;
    // RES: the accumulator seeds of ALL of the workgroup's code tiles are resident in the seeds area ([T <= SEED_TILES][32] floats,
    // loaded once in the prologue; the launcher picks the form); else a tile's seeds travel with its image, a copy per wave
    constexpr int SEED_TILES = NBUF * NW * 64 / 32;
    static_assert(SEED_TILES == DVQ_SEED_TABLE_TILES, "the launcher's limit is the table's size");
    constexpr int PER_TILE = RES ? CPW : CPW + 1;            // DMA instructions per wave and ring tile
    // FLAT: the per-wave transposition image of half a row per token (see the prologue)
    constexpr int FLAT_RSH = D * 2 + 16;                     // bytes per token in the image
    constexpr int FLAT_TRW = 32 * FLAT_RSH;                  // bytes per wave
    constexpr int FLAT_LPT = D * 2 / 16;                     // lanes (16-byte pieces) per token-half
    constexpr int FLAT_TPI = 64 / FLAT_LPT;                  // tokens per wave-instruction
    constexpr int FLAT_IPH = 32 / FLAT_TPI;                  // wave-instructions per half
    static_assert(NBUF * IMG_BYTES + NBUF * NW * 64 * 4 + NW * 2048 == dvq_pass1_lds_bytes(D), "the launch's LDS is this carve");
    static_assert(!FLAT || NW * FLAT_TRW <= dvq_pass1_lds_bytes(D), "the images fit the kernel's LDS");
    extern __shared__ __attribute__((aligned(16))) char lds[];
    float *enraw = (float *)(lds + NBUF * IMG_BYTES);        // accumulator seeds: RES [SEED_TILES][32], else [NBUF][NW][64] (per-wave copies)
    DVQ_STAMP(0);

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 31, h = lane >> 5;
    // SPLIT: this workgroup's slice of the code tiles [t_lo, t_lo + T) -- the loop below runs on slice-relative tile numbers
    const int ks = SPLIT ? (int)(blockIdx.x % (unsigned)ksplit) : 0;
    const int t_lo = SPLIT ? (int)((long)dvq_num_tiles(K) * ks / ksplit) : 0;
    const int T = SPLIT ? (int)((long)dvq_num_tiles(K) * (ks + 1) / ksplit) - t_lo : dvq_num_tiles(K);
    if constexpr (SPLIT) img += (size_t)t_lo * TILE_STRIDE;
    const float sB = meta->scale_b;
    char *scr = lds + NBUF * IMG_BYTES + NBUF * NW * 64 * 4 + wave * 2048;   // this wave's permutation scratch

    // DMA of code tile t into its ring slot, in PER_TILE pieces (q < CPW: 1 KiB of the image; without the resident table
    // q == CPW: this wave's copy of the seeds).  Past the end: harmless repeat, so the counts stay constant.
    auto issue_piece = [&](int t, int q) {
        const int tt = (t < T) ? t : T - 1;
        const char *src = img + (size_t)tt * TILE_STRIDE;
        if (RES || q < CPW) {
            // this wave's CPW chunks are contiguous (S16 = NW * CPW for every supported D): one base, the chunk as the
            // instruction offset, which applies to the global and the LDS address alike
            const char *s0 = src + wave * (CPW * 1024) + lane * 16;
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
    // RES: the seed table, once per workgroup: the 32 seeds in use of every tile's 256-byte tail, gathered by the per-lane source
    // address (a wave-instruction = two tiles -> 256 contiguous LDS bytes; 4 instructions per wave; past the end: harmless
    // repeat).  Issued in FRONT of the first ring tile: the counted wait at the head of tile 0 (all but the youngest tile's
    // pieces) covers the older table pieces of this wave, the barrier behind it everybody's.
    auto issue_seeds = [&]() {
        if constexpr (RES) {
#pragma unroll
            for (int k = 0; k < SEED_TILES / 2 / NW; ++k) {
                // wave-uniform base (scalar registers) + one 32-bit lane offset: the pair's first tile, and its second one for the
                // upper lane half where that tile exists
                const int pair = wave * (SEED_TILES / 2 / NW) + k;
                const int t0 = (2 * pair < T) ? 2 * pair : T - 1;
                const unsigned voff = (unsigned)c * 4u + ((t0 + 1 < T) ? (unsigned)h * (unsigned)TILE_STRIDE : 0u);
                glds4(img + (size_t)t0 * TILE_STRIDE + IMG_BYTES + voff, enraw + pair * 64);
            }
        }
    };
    const int tile_id = SPLIT ? (int)(blockIdx.x / (unsigned)ksplit) : xcd_swizzle(blockIdx.x, gridDim.x);
    // SEL == 2 parks the coarser branches in the ring slots from `pre` on: 2 slots = D x 128 B for the 2x-coarser
    // branch (dual: slots 2, 3; triple: slots 1, 2), slot 3 for the triple's 4x-coarser branch (D x 32 B)
    // WGC (SEL == 2 at D = 256): the workgroup's real columns are packed over its four waves (below), and the B operands cross
    // waves through two 8-KiB exchange buffers: the four permutation scratches, and the first 8 KiB of the 2x-coarser branch's
    // image -- its channels 0 .. 63, which every wave has consumed once it has written the second k-step pair.  (Taking a ring slot
    // for the second buffer instead -- one code tile in flight through the dual's prologue, not two -- exposed that tile's DMA
    // latency in front of the loop: the kernel alone ran 2.7 us LONGER than the per-wave rule's, section 8.)
    constexpr bool WGC = (SEL == 2 && D == 256);
    const int pre = (SEL == 2) ? ((rv.G == 2) ? 2 : 1) : 3;  // code tiles in flight before the prologue
    char *const xbuf_a = lds + NBUF * IMG_BYTES + NBUF * NW * 64 * 4;
    char *xbuf_b = nullptr;
    if constexpr (WGC) xbuf_b = lds + pre * IMG_BYTES;       // (SEL == 2: the image sits in the slots from `pre` on)
    static_assert(!WGC || (64 * 128 == 8192 && S32 >= 4), "channels 0 .. 63 of the [D][32 floats] image are the second buffer");
    unsigned wgm0 = 0u, wgm1 = 0u, wgm2 = 0u, wgm3 = 0u;     // WGC: the four waves' copy masks (scalar registers through the loop)
    unsigned *wg_masks = nullptr;                            // ... and where they are exchanged: 16 bytes of static LDS
    if constexpr (WGC) {
        __shared__ unsigned s_wg_masks[4];
        wg_masks = s_wg_masks;
    }

    const int n_raw = (tile_id * NW + wave) * 32 + c;
    const int n = (n_raw < N) ? n_raw : -1;
    auto token_base = [&](int HW, int h) -> size_t {         // (HW and h as arguments: the epilogue passes re-derived copies, below)
        const long nn = (n >= 0) ? n : N - 1;
        if constexpr (FLAT) return (size_t)nn * D + 8 * h;
        const long bimg = nn / HW;
        const int hw = (int)(nn - bimg * HW);
        return ((size_t)bimg * D + 8 * h) * HW + hw;
    };
    // The 128 loads and 128 stores of a lane go through BUFFER instructions: a wave-uniform base (the resource: lane 0's token, the
    // smallest of the wave, or the image's base) + a 32-bit lane offset in ONE vector register + the channel's stride in a scalar
    // register -- no vector instruction per access (global_load / global_store took one 64-bit vector add each: 270 of a block's
    // ~8000 instructions).  D * HW < 2^29 (checked by the launcher) keeps every byte offset below 2^31.
    auto wave_base = [&](const float *p0, int hw, int hh) -> __amdgpu_buffer_rsrc_t {     // resource at p0 + (lane 0's token_base())
        const size_t tb = token_base(hw, hh);
        const size_t tb0 = ((size_t)(unsigned)__builtin_amdgcn_readfirstlane((int)(tb >> 32)) << 32) |
                           (size_t)(unsigned)__builtin_amdgcn_readfirstlane((int)(tb & 0xFFFFFFFFu));
        if constexpr (XT != 0) return __builtin_amdgcn_make_buffer_rsrc((void *)((const char *)p0 + tb0 * ZB), 0, -1, 0x00020000);
        else return __builtin_amdgcn_make_buffer_rsrc((void *)(p0 + tb0), 0, -1, 0x00020000);
    };
    auto lane_off = [&](int hw, int hh) -> unsigned {        // byte offset of this lane's token_base() from lane 0's
        const size_t tb = token_base(hw, hh);
        const size_t tb0 = ((size_t)(unsigned)__builtin_amdgcn_readfirstlane((int)(tb >> 32)) << 32) |
                           (size_t)(unsigned)__builtin_amdgcn_readfirstlane((int)(tb & 0xFFFFFFFFu));
        return (unsigned)(tb - tb0) * (XT ? 2u : 4u);
    };
    float zf[S16][8];
    float sel_mask = 1.0f;                                   // SEL: the codebook_mask value of this lane's cell (1 / rep^2), NEGATED for
                                                             // the copies of a coarser cell other than its first position (one register
                                                             // through the code loop instead of two)
    int sel_g = 0;                                           // SEL == 2: grain of this lane's cell
    unsigned stg_a = 0, stg_b = 0;                           // SEL == 2: LDS byte address of this lane's value of channel 8h in the
                                                             // image of the 2x-coarser / 4x-coarser branch
    // ---- CONV: h = W x + bias into zf (see the header).  zp = this lane's x at input channel 8h, st = channel stride.
    auto conv_prologue = [&](const float *zp, size_t st) __attribute__((always_inline)) {
        constexpr int QIMG = S16 * 1024;                     // one weight image (hi or lo) of a row tile
        constexpr int QTILE = 2 * QIMG + 256;
        float *bias_l = enraw;                               // [D] bias, channel order (the seeds area is idle until the code loop)
        // group k = the weight images of k-step k (4 pieces of 1 KiB per wave -> ring slot k & 3: [row tile][hi | lo]) and this
        // lane's 8 x values of it.  All of it asm / DMA with counted waits: 12 vector-memory operations per group and wave.
        float xr[3][8];
        const float *xp = zp;
        auto issue_w = [&](int k, int q) __attribute__((always_inline)) {       // weight piece q < 4 of group k
            const int i = 4 * wave + q;                      // piece: row tile i >> 1, hi / lo i & 1
            glds16(cv.wimg + (size_t)(i >> 1) * QTILE + (i & 1) * QIMG + k * 1024 + lane * 16,
                   lds + (k & 3) * IMG_BYTES + i * 1024);
        };
        auto issue_x = [&](int k, int j) __attribute__((always_inline)) {       // x value j < 8 of group k (in order j = 0 .. 7)
            asm volatile("global_load_dword %0, %1, off nt" : "=v"(xr[k % 3][j]) : "v"(xp) : "memory");
            xp += (j == 7) ? 9 * st : st;                    // after the last one: skip the other lane half's 8 channels
        };
        auto issue_group = [&](int k) __attribute__((always_inline)) {
#pragma unroll
            for (int q = 0; q < 4; ++q) issue_w(k, q);
#pragma unroll
            for (int j = 0; j < 8; ++j) issue_x(k, j);
        };
        glds4(cv.bias + wave * 64 + lane, bias_l + wave * 64);
        issue_group(0);
        issue_group(1);
        issue_group(2);
        f32x16 acc[8];
#pragma unroll
        for (int t8 = 0; t8 < 8; ++t8)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t8][r] = 0.0f;
        int ea = 100;                                        // x is scaled by 2^ea (per token; both lane halves agree)
        float sa = ldexpf(1.0f, 100);
        // group g has landed for this wave when at most the (up to two) younger groups are outstanding; its 8 values are scaled
        // and split into the hi / lo B fragments.  The scale follows the running maximum: a value that would reach 2^15 after
        // scaling moves it (exact rescale of the accumulators by a power of two; wave-uniform branch, rare after the first
        // k-steps).
        f16x8 xh, xl;
        auto take_group = [&](int g) __attribute__((always_inline)) {
            if (g <= S16 - 3) asm volatile("s_waitcnt vmcnt(24)" ::: "memory");
            else if (g == S16 - 2) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            float xv[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) { asm volatile("" : "+v"(xr[g % 3][j])); xv[j] = xr[g % 3][j]; }
            float m = 0.0f;
#pragma unroll
            for (int j = 0; j < 8; ++j) m = vmax_abs(m, xv[j]);
            m = fmaxf(m, __shfl_xor(m, 32));
            const bool grow = (m > 0.0f) && (m < __builtin_inff()) && (m * sa >= 32768.0f);
            if (__builtin_amdgcn_ballot_w64(grow) != 0ull) {
                int e;
                (void)frexpf(grow ? m : 1.0f, &e);
                int en = 14 - e;
                en = en > 100 ? 100 : (en < -100 ? -100 : en);
                en = grow ? en : ea;
                if (g > 0) {
                    const float f = ldexpf(1.0f, en - ea);
#pragma unroll
                    for (int t8 = 0; t8 < 8; ++t8)
#pragma unroll
                        for (int r = 0; r < 16; ++r) acc[t8][r] *= f;
                }
                ea = en;
                sa = ldexpf(1.0f, ea);
            }
            u32x4 ph, pl;
#pragma unroll
            for (int j2 = 0; j2 < 4; ++j2) {
                const float v0 = xv[2 * j2] * sa, v1 = xv[2 * j2 + 1] * sa;
                const f32x2 vv = {v0, v1};
                const f16x2 hh = __builtin_convertvector(vv, f16x2);
                const f32x2 rr = {v0 - (float)hh[0], v1 - (float)hh[1]};
                const f16x2 ll = __builtin_convertvector(rr, f16x2);
                ph[j2] = __builtin_bit_cast(unsigned, hh);
                pl[j2] = __builtin_bit_cast(unsigned, ll);
            }
            xh = __builtin_bit_cast(f16x8, ph);
            xl = __builtin_bit_cast(f16x8, pl);
        };
        take_group(0);
#pragma unroll
        for (int s = 0; s < S16; ++s) {
            __builtin_amdgcn_s_barrier();                    // k-step s of the weights landed (everybody's pieces); s - 1 consumed
            asm volatile("" ::: "memory");
            // group s + 3 (into the slot of k-step s - 1 and the x registers already converted) is issued piece by piece BETWEEN
            // the row tiles below: each of its 12 vector-memory instructions then issues in the shadow of MFMAs already in the pipe
            const f16x8 bh = xh, bl = xl;
            // the 16 weight fragments of the k-step (per row tile: lo, then hi) through three rotating registers, each read
            // CONV_AHEAD fragments before its MFMAs behind a counted lgkmcnt: left to hipcc every ds_read_b128 was followed by
            // a full LDS round trip (lgkmcnt(0)) in front of its MFMA -- 16 exposed round trips per 24 MFMAs
            const unsigned wa = (unsigned)(size_t)(const __attribute__((address_space(3))) char *)(lds + (s & 3) * IMG_BYTES) + lane * 16;
            f16x8 wf[3];
#define CV_OFF(Q) ((((Q) & 1) ? ((Q) - 1) : ((Q) + 1)) * 1024)      /* fragment Q: even = lo of tile Q / 2 (stored second), odd = hi */
#define CV_RD(Q) asm volatile("ds_read_b128 %0, %1 offset:%c2" : "=v"(wf[(Q) % 3]) : "v"(wa), "i"(CV_OFF(Q)))
#define CV_WAIT(N, Q) asm volatile("s_waitcnt lgkmcnt(" #N ")" : "+v"(wf[(Q) % 3]) :: "memory")
            CV_RD(0); CV_RD(1); CV_RD(2);
            __builtin_amdgcn_sched_barrier(0);
#define CV_TILE(T8, W0, W1)                                                                                              \
            CV_WAIT(W0, 2 * (T8));                                                                                        \
            __builtin_amdgcn_sched_barrier(0);                                                                            \
            acc[T8] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[(2 * (T8)) % 3], bh, acc[T8], 0, 0, 0);   /* small terms first (qconv.hip) */ \
            __builtin_amdgcn_sched_barrier(0);                                                                            \
            if (2 * (T8) + 3 < 16) { CV_RD(2 * (T8) + 3 < 16 ? 2 * (T8) + 3 : 0); }                                       \
            CV_WAIT(W1, 2 * (T8) + 1);                                                                                    \
            __builtin_amdgcn_sched_barrier(0);                                                                            \
            acc[T8] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[(2 * (T8) + 1) % 3], bl, acc[T8], 0, 0, 0);               \
            acc[T8] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[(2 * (T8) + 1) % 3], bh, acc[T8], 0, 0, 0);               \
            __builtin_amdgcn_sched_barrier(0);                                                                            \
            if (2 * (T8) + 4 < 16) { CV_RD(2 * (T8) + 4 < 16 ? 2 * (T8) + 4 : 0); }
            // outstanding reads at each wait: fragments Q .. min(Q + 2, 15); "all but the youngest N" = Q has landed
#define CV_W(Q) if (s + 3 < S16) { issue_w(s + 3, Q); __builtin_amdgcn_sched_barrier(0); }
#define CV_X(J) if (s + 3 < S16) { issue_x(s + 3, J); issue_x(s + 3, (J) + 1); __builtin_amdgcn_sched_barrier(0); }
            CV_TILE(0, 2, 2) CV_W(0) CV_TILE(1, 2, 2) CV_W(1) CV_TILE(2, 2, 2) CV_W(2) CV_TILE(3, 2, 2) CV_W(3)
            CV_TILE(4, 2, 2) CV_X(0) CV_TILE(5, 2, 2) CV_X(2) CV_TILE(6, 2, 2) CV_X(4) CV_TILE(7, 1, 0) CV_X(6)
#undef CV_W
#undef CV_X
#undef CV_TILE
#undef CV_WAIT
#undef CV_RD
#undef CV_OFF
            __builtin_amdgcn_sched_barrier(0);               // the MFMAs are issued; the next k-step's conversion runs under them
            if (s + 1 < S16) take_group(s + 1);
        }
        const float unscale = ldexpf(cv.meta->inv_scale_w, -ea);
#pragma unroll
        for (int s = 0; s < S16; ++s) {
            const f32x4 b0 = *(const f32x4 *)(bias_l + 16 * s + 8 * h), b1v = *(const f32x4 *)(bias_l + 16 * s + 8 * h + 4);
#pragma unroll
            for (int j = 0; j < 8; ++j)
                zf[s][j] = __builtin_fmaf(acc[s >> 1][8 * (s & 1) + j], unscale, (j < 4) ? b0[j & 3] : b1v[j & 3]);
            __builtin_amdgcn_sched_barrier(0);               // in place, one k-step's bias at a time (hoisted bias reads spill)
        }
        if (cv.h_all && n >= 0) {                            // tests: the conv's output for every token
            float *hp = cv.h_buf + token_base(HW, h);
#pragma unroll
            for (int s = 0; s < S16; ++s)
#pragma unroll
                for (int j = 0; j < 8; ++j) hp[(size_t)(16 * s + j) * HW] = zf[s][j];
        }
        __builtin_amdgcn_s_barrier();                        // every wave is done with the weight slots and the bias:
        asm volatile("" ::: "memory");                       // the ring and the seeds area go to the code tiles
        issue_seeds();
        for (int t = 0; t < 3; ++t) issue(t);
        __builtin_amdgcn_sched_barrier(0);                   // (the conversion below must not be hoisted over this: all of zf is ready)
    };
    if (SEL != 0) {
        // the router select, fused in: grain of this position's cell straight from the gate, source = the branch
        // that won the cell; indices / codebook_mask / the int64 gate are written here as by-products.
        // Ordinary loads whose values are used while an LDS-DMA is in flight make hipcc drain the whole vector-memory
        // queue (s_waitcnt vmcnt(0)), so: the gate is fetched BEFORE the first DMA is issued, and (SEL == 2) reduced only
        // after this wave's loads are on their way.
        const int nn = (n >= 0) ? n : (int)(N - 1);
        const int b = nn / HW, pos = nn - b * HW;
        const int y = pos / rv.Wout, x = pos - y * rv.Wout;
        const int SC = rv.sub[rv.G - 1];
        const size_t cell = (size_t)b * rv.hc * rv.wc + (y / SC) * rv.wc + x / SC;
        const DvqGateRaw graw = dvq_gate_fetch(rv.gate, rv.gate_mode, rv.G, cell);
        auto by_products = [&](int g) {
            const int rep_g = rv.rep[g];
            sel_mask = 1.0f / (float)(rep_g * rep_g);        // 1, 0.25, 0.0625: exact
            if (n >= 0 && h == 0 && rv.cmask_out != nullptr) {
                rv.cmask_out[n] = sel_mask;
                if (y % SC == 0 && x % SC == 0) {
                    rv.indices_out[cell] = g;
                    if (rv.gate_mode == 2 && rv.gate_out != nullptr) {
                        const float e = graw.f[0];
                        longlong2 gg; gg.x = (e <= rv.thr) ? 1 : 0; gg.y = (e > rv.thr) ? 1 : 0;
                        *(longlong2 *)(rv.gate_out + 2 * cell) = gg;
                    }
                }
            }
            if (!(y % rep_g == 0 && x % rep_g == 0)) sel_mask = -sel_mask;
        };
        if (SEL == 1) {
            const int g = dvq_gate_reduce(graw, rv.gate_mode, rv.G, rv.thr);
            by_products(g);
            int stride_l;
            const float *zp = dvq_dense_source(rv, b, y, x, g, stride_l) + (size_t)8 * h * stride_l;
            const size_t st = (size_t)stride_l;
            if constexpr (CONV) {
                conv_prologue(zp, st);
            } else {
            issue_seeds();
            for (int t = 0; t < pre; ++t) issue(t);
            __builtin_amdgcn_s_setprio(2);
#pragma unroll
            for (int s = 0; s < S16; ++s)
#pragma unroll
                for (int j = 0; j < 8; ++j) zf[s][j] = DVQ_LOAD_SEL(zp + (size_t)(16 * s + j) * st);
            __builtin_amdgcn_s_setprio(0);
            }
        } else {
            issue_seeds();
            for (int t = 0; t < pre; ++t) issue(t);
            // workgroup = output rows y0 .. y0 + 3 of image b (wave = row, lane = column); both are wave-uniform
            const int bw = __builtin_amdgcn_readfirstlane(b);
            const int y0 = __builtin_amdgcn_readfirstlane(y) - wave;
            char *img_a = lds + pre * IMG_BYTES;             // 2x-coarser branch [D][32 floats]
            char *img_b = lds + 3 * IMG_BYTES;               // 4x-coarser branch [D][8 floats] (triple only)
            {
                // branch G-2 (rep 2): rows y0/2, y0/2 + 1 of a 16-wide grid = 32 consecutive floats per channel;
                // a wave-instruction moves 8 channels x 8 pieces of 16 B
                const int ga = rv.G - 2;
                const int plane = rv.hc * rv.sub[ga] * 16;
                const float *src = rv.src[ga] + (size_t)bw * D * plane + (size_t)(y0 >> 1) * 16 + (lane & 7) * 4;
                for (int i = wave; i < D / 8; i += NW)
                    glds16(src + (size_t)(i * 8 + (lane >> 3)) * plane, img_a + i * 1024);
            }
            if (rv.G == 3) {
                // branch 0 (rep 4): row y0/4 of an 8-wide grid = 8 floats per channel; 32 channels x 2 pieces per instruction
                const int plane = rv.hc * 8;
                const float *src = rv.src[0] + (size_t)bw * D * plane + (size_t)(y0 >> 2) * 8 + (lane & 1) * 4;
                for (int i = wave; i < D / 32; i += NW)
                    glds16(src + (size_t)(i * 32 + (lane >> 1)) * plane, img_b + i * 1024);
            }
            stg_a = (unsigned)(size_t)(const __attribute__((address_space(3))) char *)img_a +
                    (unsigned)((8 * h) * 128 + (((wave >> 1) * 16 + (c >> 1)) << 2));
            stg_b = (unsigned)(size_t)(const __attribute__((address_space(3))) char *)img_b +
                    (unsigned)((8 * h) * 32 + ((c >> 2) << 2));
            const __amdgpu_buffer_rsrc_t zr = __builtin_amdgcn_make_buffer_rsrc((void *)(rv.src[rv.G - 1] + (size_t)bw * D * HW), 0,
                                                                                -1, 0x00020000);      // the image's plane stack
            const unsigned zo = (unsigned)(8 * h * HW + pos) * 4u;
            __builtin_amdgcn_s_setprio(2);
#pragma unroll
            for (int s = 0; s < S16; ++s)
#pragma unroll
                for (int j = 0; j < 8; ++j) zf[s][j] = DVQ_BUF_LOAD(zr, zo, (16 * s + j) * HW * 4, NT ? 2 : 0);
            __builtin_amdgcn_s_setprio(0);
            if constexpr (WGC) {
                // the wave's copy mask (bit c = column c is a copy: not its cell's first position) goes to the other waves through
                // LDS; the barrier behind the branch images publishes it
                sel_g = dvq_gate_reduce(graw, rv.gate_mode, rv.G, rv.thr);
                const int rep_g = rv.rep[sel_g];
                const unsigned cm = (unsigned)__builtin_amdgcn_ballot_w64(!(y % rep_g == 0 && x % rep_g == 0) && h == 0);
                if (lane == 0) wg_masks[wave] = cm;
                asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            } else
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's pieces of the branch images (and its loads) landed;
            __builtin_amdgcn_s_barrier();                      // the barrier makes that true for the other waves' pieces
            asm volatile("" ::: "memory");
            if constexpr (!WGC) sel_g = dvq_gate_reduce(graw, rv.gate_mode, rv.G, rv.thr);
            by_products(sel_g);
            if constexpr (WGC) {
                wgm0 = (unsigned)__builtin_amdgcn_readfirstlane((int)wg_masks[0]);
                wgm1 = (unsigned)__builtin_amdgcn_readfirstlane((int)wg_masks[1]);
                wgm2 = (unsigned)__builtin_amdgcn_readfirstlane((int)wg_masks[2]);
                wgm3 = (unsigned)__builtin_amdgcn_readfirstlane((int)wg_masks[3]);
            }
        }
    } else if constexpr (CONV) {
        conv_prologue(z + token_base(HW, h), (size_t)HW);
    } else if constexpr (FLAT) {
        // Row-major latents.  Read as what they are -- every wave-instruction fetches whole 128-byte lines (a token's HALF row,
        // D * 2 bytes, is contiguous: lane = 16-byte piece) -- and turned into the (token, 8 channels of a k-step) register
        // layout through a wave-private LDS image [32 tokens][D / 2 floats + 16 B pad] (the pad makes the b128 reads of lanes
        // c .. c + 7 hit distinct banks), one half of the channels at a time.  The image lives where the code ring will: the
        // first code tiles are DMA'd after a workgroup barrier, and land while the fragments are converted.
        // (The direct form -- lane = token, two 16-byte loads per k-step at a stride of D * 4 bytes -- touched every line from
        // eight instructions and ran at 2x the NCHW kernel's time; profiles/r05_flat.json.)
        char *tr = lds + wave * FLAT_TRW;
        const long n0 = ((long)tile_id * NW + wave) * 32;    // the wave's first token (its 32 tokens are consecutive rows)
        f32x4 tmp[2][FLAT_IPH];
#pragma unroll
        for (int h2 = 0; h2 < 2; ++h2)
#pragma unroll
            for (int i = 0; i < FLAT_IPH; ++i) {
                long tk = n0 + i * FLAT_TPI + lane / FLAT_LPT;
                tk = tk < N ? tk : N - 1;
                const f32x4 *src = (const f32x4 *)(z + (size_t)tk * D + h2 * (D / 2)) + (lane % FLAT_LPT);
                tmp[h2][i] = NT ? __builtin_nontemporal_load(src) : *src;
            }
#pragma unroll
        for (int h2 = 0; h2 < 2; ++h2) {
#pragma unroll
            for (int i = 0; i < FLAT_IPH; ++i)
                *(f32x4 *)(tr + (i * FLAT_TPI + lane / FLAT_LPT) * FLAT_RSH + (lane % FLAT_LPT) * 16) = tmp[h2][i];
#pragma unroll
            for (int sp = 0; sp < S16 / 2; ++sp) {
                const int s = h2 * (S16 / 2) + sp;
                const f32x4 lo = *(const f32x4 *)(tr + c * FLAT_RSH + (16 * sp + 8 * h) * 4);
                const f32x4 hi = *(const f32x4 *)(tr + c * FLAT_RSH + (16 * sp + 8 * h + 4) * 4);
#pragma unroll
                for (int j = 0; j < 4; ++j) { zf[s][j] = lo[j]; zf[s][4 + j] = hi[j]; }
            }
        }
        __syncthreads();                                     // every wave has read its image: the region becomes the code ring
        issue_seeds();                                       // (and the seeds area, which the images may cover)
        for (int t = 0; t < pre; ++t) issue(t);
    } else {
        issue_seeds();
        for (int t = 0; t < pre; ++t) issue(t);
        const __amdgpu_buffer_rsrc_t zr = wave_base(z, HW, h);
        const unsigned zo = lane_off(HW, h);
        __builtin_amdgcn_s_setprio(2);
#pragma unroll
        for (int s = 0; s < S16; ++s)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if constexpr (XT != 0) zf[s][j] = DVQ_BUF_LOAD16(XT, zr, zo, (16 * s + j) * HW * 2, NT ? 2 : 0);
                else zf[s][j] = DVQ_BUF_LOAD(zr, zo, (16 * s + j) * HW * 4, NT ? 2 : 0);
            }
        __builtin_amdgcn_s_setprio(0);
    }
    f16x8 zb[2][S32];                                        // B operands of the 16x16x32 loop, [token half][k-step of 32]
    float xn, thr2W;
    // SEL == 2, the order of a wave's columns: the real ones first (in column order), the copies of a coarser cell behind them.  A
    // column's scores depend on its B values and not on where it sits, so the order is free; with at most 16 real columns the
    // second column group (t2 = 1) holds copies only, whose results nobody reads, and the wave runs the code loop without it
    // (the short form, below).  copymask: bit c = column c is a copy (wave-uniform, in scalar registers through the loop).
    unsigned copymask = 0u;
    unsigned perm_off[2] = {0u, 0u};                         // scratch byte offset of the column at sorted position 16 t2 + (lane & 15)
    // WGC: the order is the WORKGROUP's: its real columns wave by wave, in column order; sorted position p is scored by wave p / 32
    // in column group (p / 16) & 1, and positions from nreal_wg on read a copy's (zero) operands.  The argument above carries over
    // from the wave to the workgroup, and wave w scores ng = clamp(ceil((nreal_wg - 32 w) / 16), 0, 2) groups: the long form of
    // the loop, the short one, or (ng = 0) the ring's protocol alone.
    int ng = 2;
    if constexpr (WGC) {
        const int nr0 = 32 - __builtin_popcount(wgm0), nr1 = 32 - __builtin_popcount(wgm1), nr2 = 32 - __builtin_popcount(wgm2);
        const int pf1 = nr0, pf2 = pf1 + nr1, pf3 = pf2 + nr2, nreal_wg = pf3 + 32 - __builtin_popcount(wgm3);
        const int left = nreal_wg - 32 * wave + 15;
        ng = __builtin_amdgcn_readfirstlane(left < 16 ? 0 : (left < 32 ? 1 : 2));
        // the first copy of the workgroup: its operands are zeros (no copy at all: nreal_wg = 128, and no position refers to it)
        const int wz = wgm0 ? 0 : (wgm1 ? 1 : (wgm2 ? 2 : 3));
        const unsigned mz = wgm0 ? wgm0 : (wgm1 ? wgm1 : (wgm2 ? wgm2 : wgm3));
        const int cz = mz ? __builtin_ctz(mz) : 0;
#pragma unroll
        for (int t2 = 0; t2 < 2; ++t2) {
            const int P = 32 * wave + 16 * t2 + (lane & 15);
            // the wave that holds the P-th real column, and the column: the k-th set bit of its real mask
            const int ws = (P >= pf3) ? 3 : ((P >= pf2) ? 2 : ((P >= pf1) ? 1 : 0));
            int k = P - ((P >= pf3) ? pf3 : ((P >= pf2) ? pf2 : ((P >= pf1) ? pf1 : 0)));
            const unsigned real = ~((ws == 3) ? wgm3 : ((ws == 2) ? wgm2 : ((ws == 1) ? wgm1 : wgm0)));
            int col = 0;
#pragma unroll
            for (int sh = 16; sh >= 1; sh >>= 1) {
                const int cnt = __builtin_popcount((real >> col) & ((1u << sh) - 1u));
                if (k >= cnt) { k -= cnt; col += sh; }
            }
            const bool past = P >= nreal_wg;
            const unsigned wsrc = past ? (unsigned)wz : (unsigned)ws, csrc = past ? (unsigned)cz : (unsigned)col;
            perm_off[t2] = wsrc * 2048u + (unsigned)(lane >> 5) * 1024u + (csrc + 32u * ((unsigned)(lane >> 4) & 1u)) * 16u;
        }
    } else
    if constexpr (SEL == 2) {
        copymask = (unsigned)__builtin_amdgcn_ballot_w64(sel_mask < 0.0f && h == 0);
        // column c sits at pos(c): a real column at its rank among the real ones, a copy at nreal + its rank among the copies.
        // The inverse (position -> column), 32 bytes, goes through the wave's scratch (idle until the first k-step pair; a wave's
        // LDS operations execute in order).  No copies: pos(c) = c, and the offsets are the ones the dense form computes.
        const int below = __builtin_popcount(copymask & ((1u << c) - 1u));
        const int p = (sel_mask < 0.0f) ? 32 - __builtin_popcount(copymask) + below : c - below;
        unsigned char *tab = (unsigned char *)scr;
        if (h == 0) tab[p] = (unsigned char)c;
#pragma unroll
        for (int t2 = 0; t2 < 2; ++t2) {
            const unsigned col = tab[16 * t2 + (lane & 15)];
            perm_off[t2] = (unsigned)(lane >> 5) * 1024u + (col + 32u * ((unsigned)(lane >> 4) & 1u)) * 16u;
        }
    }
    {
        float pa[2][8];
        float amax = 0.0f, zeta2 = 0.0f;
        f16x8 zprev = {};
#pragma unroll
        for (int s = 0; s < S16; ++s) {
            if (SEL == 2) {
                // lanes whose cell went to a coarser branch: its value of channel 16 s + 8 h + j replaces the fine one
                // (the LDS reads execute under the lanes' exec mask and land in the same registers: no select needed)
                if (sel_g == rv.G - 2) {
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        asm volatile("ds_read_b32 %0, %1 offset:%c2" : "+v"(zf[s][j]) : "v"(stg_a), "i"((16 * s + j) * 128));
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                }
                if (rv.G == 3 && sel_g == 0) {
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        asm volatile("ds_read_b32 %0, %1 offset:%c2" : "+v"(zf[s][j]) : "v"(stg_b), "i"((16 * s + j) * 32));
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) asm volatile("" : "+v"(zf[s][j]));
            }
            u32x4 packed;
#pragma unroll
            for (int j2 = 0; j2 < 4; ++j2) {
                const float v0 = zf[s][2 * j2], v1 = zf[s][2 * j2 + 1];
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
            if constexpr (SEL == 2) {
                // the copies of a coarser cell (every position but its first) score ZERO operands: their columns' results are
                // never used -- the lane that owns the cell computes the same (best, second, code) from the same vector and
                // hands them over behind the loop -- and a column of zeros costs the matrix cores less switching energy, which
                // under the socket's power cap is time (section 5.1).  Norm, bound and zf above are the real vector's.
                // (the empty asm ends the k-step's residual sums first, so that the words are replaced in place: selected while
                // the conversion's results were still needed they took eight more registers, and the D = 256 kernels spilled)
                asm volatile("" : "+v"(packed), "+v"(zeta2));
                if (sel_mask < 0.0f) packed = u32x4{0u, 0u, 0u, 0u};
            }
            const f16x8 zcur = __builtin_bit_cast(f16x8, packed);
            if (s & 1) {
                // tokens 16 t2 + (lane & 15), k = 32 s' + 8 (lane >> 4) + j  <-  lane (c, h) = (16 t2 + (lane & 15), (lane >> 4) & 1),
                // k-step 2 s' + (lane >> 5) of the load layout: through the per-wave LDS scratch (a wave's LDS
                // operations execute in order, so no barrier; 128 ds_bpermutes instead spilled 54 VGPRs)
                const int sp = s >> 1;
                if constexpr (WGC) {
                    // the same through the workgroup's exchange buffers, [wave][2 KiB]: the barrier publishes pair sp, and the wait
                    // in front of it has retired this wave's reads of pair sp - 1, so the buffer of pair sp - 1 may be written
                    // again behind it.  Pairs 0 and 1 both take the scratches (one more barrier between them: the image's head is
                    // still in use), from pair 2 on the image's head and the scratches alternate.  Every wave executes every one
                    // of these barriers.
                    char *xb = (sp >= 2 && !(sp & 1)) ? xbuf_b : xbuf_a;
                    if (sp == 1) {
                        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                        __builtin_amdgcn_s_barrier();
                        asm volatile("" ::: "memory");
                    }
                    *(f16x8 *)(xb + wave * 2048 + lane * 16) = zprev;
                    *(f16x8 *)(xb + wave * 2048 + 1024 + lane * 16) = zcur;
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    __builtin_amdgcn_s_barrier();
                    asm volatile("" ::: "memory");
#pragma unroll
                    for (int t2 = 0; t2 < 2; ++t2) zb[t2][sp] = *(const f16x8 *)(xb + perm_off[t2]);
                } else {
                *(f16x8 *)(scr + lane * 16) = zprev;
                *(f16x8 *)(scr + 1024 + lane * 16) = zcur;
#pragma unroll
                for (int t2 = 0; t2 < 2; ++t2) {
                    if constexpr (SEL == 2) {
                        zb[t2][sp] = *(const f16x8 *)(scr + perm_off[t2]);
                    } else {
                    const int srcl = 16 * t2 + (lane & 15) + 32 * ((lane >> 4) & 1);
                    zb[t2][sp] = *(const f16x8 *)(scr + (lane >> 5) * 1024 + srcl * 16);
                    }
                }
                }
            }
            zprev = zcur;
            if constexpr (CONV) __builtin_amdgcn_sched_barrier(0);   // zf is complete before the loop: keep the k-steps in order
        }
        float t8[8];
#pragma unroll
        for (int l = 0; l < 8; ++l) {
            float o0 = __shfl_xor(pa[0][l], 32), o1 = __shfl_xor(pa[1][l], 32);
            float a0 = h == 0 ? pa[0][l] : o0;
            float a1 = h == 0 ? o0 : pa[0][l];
            float a2 = h == 0 ? pa[1][l] : o1;
            float a3 = h == 0 ? o1 : pa[1][l];
            t8[l] = __fadd_rn(__fadd_rn(__fadd_rn(a0, a1), a2), a3);
        }
        xn = t8[0];
#pragma unroll
        for (int l = 1; l < 8; ++l) xn = __fadd_rn(xn, t8[l]);
        amax = fmaxf(amax, __shfl_xor(amax, 32));
        zeta2 += __shfl_xor(zeta2, 32);
        // FOLD: z is the conv's input, `img` / `meta` the folded codebook E W (vq_fold.hip), and the bound also covers the conv
        thr2W = FOLD ? dvq_fold_threshold(xn, amax, zeta2, sB, (const DvqFoldMeta *)meta)
                     : dvq_filter_threshold(xn, amax, zeta2, sB, meta);
    }
    if (SEL == 2) {
        if constexpr (WGC) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // ... and its operands of the last pair (slot buffer)
        __builtin_amdgcn_s_barrier();                        // every wave has read the branch images: the slots join the ring
        asm volatile("" ::: "memory");
    }
    for (int t = pre; t < 3; ++t) issue(t);                  // (SEL == 2) the code tiles that waited for those slots
    DVQ_STAMP(1);

    // ---- 16x16x32 code loop: fragment F = c2 * S32 + s' of the tile feeds two MFMAs (token halves t2 = 0, 1);
    // accumulator acc16[c2][t2][i] = code 16 c2 + 4 (lane >> 4) + i against token 16 t2 + (lane & 15)
    float best, second;
    int code;
    {
        const int q16 = lane >> 4;
        float b1[2] = {-__builtin_inff(), -__builtin_inff()}, b2[2] = {-__builtin_inff(), -__builtin_inff()};
        int bt[2] = {0, 0};
        // Per tile: barrier -> the first four A-fragment reads are issued -> the running top-2 is updated with the PREVIOUS
        // tile's scores (plain VALU work that hides the LDS latency of those reads) -> the accumulators are re-seeded ->
        // MFMA chain.  A wave's instruction ISSUE, not the matrix pipe, bounds this loop: about 1330 cycles per tile, of which
        // the pipe is busy 512; a workgroup alone on a CU takes as long as two sharing it (profiles/archive/r03_pass1_antiphase_ab.json,
        // r03_pass1_loop_ablation.json).  Moving the top-2 update into the shadow of the MFMAs (one code half behind them, no
        // second accumulator set) changed nothing, as that model predicts: 42.7k vs 42.6k cycles per loop
        // (profiles/archive/r03_pass1_half_tile_pipelining.json; git history has the code).
        // SEL == 2: a wave with at most 16 real columns runs the SHORT form of the loop: column group t2 = 0 alone -- half the MFMAs,
        // half the top-2 update, half the re-seed -- and everything the workgroup shares as in the long form: the counted vmcnt wait,
        // the tile barrier, the DMA pieces of tile t + 3 at the same fragments, all 16 A-fragment reads and their counted waits.
        // One scalar branch around the loop picks the form; no wave leaves the ring's protocol.
        // WGC: the form follows the wave's share of the workgroup's packed columns; a wave with none (ng = 0) performs the tile's
        // counted wait, the barrier and its DMA pieces, and nothing else.
        if constexpr (WGC) {
            if (ng == 0) {
#define DVQ_NG 0
#include "pass1_loop.h"
#undef DVQ_NG
            } else if (ng == 1) {
#define DVQ_NG 1
#include "pass1_loop.h"
#undef DVQ_NG
            } else {
#define DVQ_NG 2
#include "pass1_loop.h"
#undef DVQ_NG
            }
        } else
        if constexpr (SEL == 2) {
            if (__builtin_popcount(copymask) >= 16) {        // short wave: nreal <= 16 (wave-uniform, decided before the loop)
#define DVQ_NG 1
#include "pass1_loop.h"
#undef DVQ_NG
            } else {
#define DVQ_NG 2
#include "pass1_loop.h"
#undef DVQ_NG
            }
        } else {
#define DVQ_NG 2
#include "pass1_loop.h"
#undef DVQ_NG
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // surplus ring DMA
        // merge the four lane groups of a token column (lower lane wins ties), then hand the results to the lanes
        // that own the token in the (c, h) layout of the prologue / epilogue
        float rb[2], rs[2];
        int rc[2];
#pragma unroll
        for (int t2 = 0; t2 < 2; ++t2) {
            float mb = b1[t2], ms = b2[t2];
            int mt = bt[t2], mq = q16;
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
            rb[t2] = mb;
            rs[t2] = ms;
            rc[t2] = (mt + t_lo) * 32 + 16 * (r >> 2) + 4 * mq + (r & 3);
        }
        if constexpr (WGC) {
            // the triples go to a workgroup-wide table indexed by sorted position (the permutation scratches, idle since the
            // prologue; the surplus DMA has landed): groups the wave did not score leave entries nobody reads
            const int lane_t = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
            if (lane_t < 16) {
#pragma unroll
                for (int t2 = 0; t2 < 2; ++t2) {
                    const f32x4 mine = {rb[t2], rs[t2], __int_as_float(rc[t2]), 0.0f};
                    *(f32x4 *)(xbuf_a + (32 * wave + 16 * t2 + lane_t) * 16) = mine;
                }
            }
            best = 0.0f; second = 0.0f; code = 0;            // (taken from the table below)
        } else
        if constexpr (SEL == 2) {
            // the column's sorted position pos(c) again, from the mask and the lane id (nothing of the prologue's lives in a VGPR
            // through the loop).  A short wave's positions >= 16 are copies: what they pick from the unscored group is replaced by
            // their owner's triple below.
            unsigned cm = copymask;
            asm volatile("" : "+s"(cm));                     // (opaque: derived behind the loop, not kept from the prologue)
            const int c_p = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) & 31;
            const int below = __builtin_popcount(cm & ((1u << c_p) - 1u));
            const int pc = ((cm >> c_p) & 1u) ? 32 - __builtin_popcount(cm) + below : c_p - below;
            const int srcl = pc & 15;
            const float x0 = __shfl(rb[0], srcl), x1 = __shfl(rb[1], srcl);
            const float y0 = __shfl(rs[0], srcl), y1 = __shfl(rs[1], srcl);
            const int c0 = __shfl(rc[0], srcl), c1 = __shfl(rc[1], srcl);
            best = (pc >> 4) ? x1 : x0;
            second = (pc >> 4) ? y1 : y0;
            code = (pc >> 4) ? c1 : c0;
        } else {
        const int srcl = c & 15;
        const float x0 = __shfl(rb[0], srcl), x1 = __shfl(rb[1], srcl);
        const float y0 = __shfl(rs[0], srcl), y1 = __shfl(rs[1], srcl);
        const int c0 = __shfl(rc[0], srcl), c1 = __shfl(rc[1], srcl);
        best = (c >> 4) ? x1 : x0;
        second = (c >> 4) ? y1 : y0;
        code = (c >> 4) ? c1 : c0;
        }
    }
    DVQ_STAMP(2);
    if constexpr (SEL == 2) {
        // the copies scored zeros (prologue): they take the triple of the lane that owns their cell -- the cell's first position,
        // `y % rep` rows up and `x % rep` columns left, always in this workgroup (rows of 32 positions, four whole rows from a
        // multiple of four, rep in {1, 2, 4}: staged_select_ok) -- through the waves' permutation scratch, idle since the prologue.
        // A column's scores depend on its B values, the A fragments and the seeds, and the merge on the lane-group order, not on
        // which column it is: the owner's triple is bit for bit what the copy computed from the same vector.
        // Row, column and rep are re-derived here (wave = row, lane = column): nothing new lives in a VGPR through the loop.
        const int lane_e = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
        const int c_e = lane_e & 31;
        float am = __builtin_fabsf(sel_mask);
        asm volatile("" : "+v"(am));                         // (opaque: nothing derived from it is computed ahead of the loop)
        const int rm1 = (am == 1.0f) ? 0 : ((am == 0.25f) ? 1 : 3);             // rep - 1
        char *hand = lds + NBUF * IMG_BYTES + NBUF * NW * 64 * 4;               // [wave][2 KiB]: 32 columns x 16 B in use
        if constexpr (WGC) {
            // the owner (a real column: row wave_o, column c_o) sits at sorted position prefix(wave_o) + its rank among that wave's
            // real columns, re-derived from the four masks (scalar) and the lane id
            unsigned m0 = wgm0, m1 = wgm1, m2 = wgm2, m3 = wgm3;
            asm volatile("" : "+s"(m0), "+s"(m1), "+s"(m2), "+s"(m3));          // (opaque: derived behind the loop)
            const int wave_o = wave - (wave & rm1), c_o = c_e - (c_e & rm1);
            const int q1 = 32 - __builtin_popcount(m0), q2 = q1 + 32 - __builtin_popcount(m1), q3 = q2 + 32 - __builtin_popcount(m2);
            const unsigned m_o = (wave_o == 0) ? m0 : ((wave_o == 1) ? m1 : ((wave_o == 2) ? m2 : m3));
            const int pf_o = (wave_o == 0) ? 0 : ((wave_o == 1) ? q1 : ((wave_o == 2) ? q2 : q3));
            const int p_o = pf_o + __builtin_popcount(~m_o & ((1u << c_o) - 1u));
            __syncthreads();
            const f32x4 own = *(const f32x4 *)(hand + p_o * 16);
            best = own[0];
            second = own[1];
            code = __float_as_int(own[2]);
        } else {
        if (lane_e < 32) {
            const f32x4 mine = {best, second, __int_as_float(code), 0.0f};
            *(f32x4 *)(hand + wave * 2048 + c_e * 16) = mine;
        }
        __syncthreads();
        const f32x4 own = *(const f32x4 *)(hand + (wave - (wave & rm1)) * 2048 + (c_e - (c_e & rm1)) * 16);
        best = own[0];                                       // (a cell's first position reads back what it wrote)
        second = own[1];
        code = __float_as_int(own[2]);
        }
    }
    if constexpr (SPLIT) {
        // hand-off without fences (MI355X guide, inter-workgroup visibility: every payload store write-through (sc1) and drained by
        // its wave, the workgroup's barrier, ONE agent-scope add per workgroup; the workgroup whose add came last reads with sc1
        // loads after a barrier its adding wave joins).  A __threadfence() pair instead cost 3-70 us with the grid size.
        typedef __attribute__((address_space(1))) unsigned long long gu64;
        __shared__ int s_last;
        gu64 *mine = (gu64 *)(split + ((size_t)tile_id * ksplit) * 128 + wave * 32 + c);      // [block][slice][128 tokens] x 16 B
        if (h == 0) {
            gu64 *e = mine + (size_t)ks * 128 * 2;
            __hip_atomic_store(e, ((unsigned long long)__float_as_uint(second) << 32) | __float_as_uint(best), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(e + 1, (unsigned long long)(unsigned)code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        DVQ_STAMP(3);
        if (tid == 0) {
            const int old = __hip_atomic_fetch_add(&counters[DVQ_SPLIT_TICKET0 + tile_id], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            s_last = (old == ksplit - 1);
            if (old == ksplit - 1)                           // self-cleaning (DVQ_MODE_WS_CLEAN)
                __hip_atomic_store(&counters[DVQ_SPLIT_TICKET0 + tile_id], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();
        DVQ_STAMP(4);
        if (!s_last) return;
        float mb = -__builtin_inff(), ms = -__builtin_inff();
        int mc = 0;
        unsigned long long e0[DVQ_SPLIT_MAX_SLICES], e1[DVQ_SPLIT_MAX_SLICES];   // all slices' entries in flight at once (past the end: repeats)
#pragma unroll
        for (int k = 0; k < DVQ_SPLIT_MAX_SLICES; ++k) {
            const int kk = k < ksplit ? k : ksplit - 1;
            e0[k] = __hip_atomic_load(mine + (size_t)kk * 128 * 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            e1[k] = __hip_atomic_load(mine + (size_t)kk * 128 * 2 + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
#pragma unroll
        for (int k = 0; k < DVQ_SPLIT_MAX_SLICES; ++k) {
            const float eb = __uint_as_float((unsigned)e0[k]), es = __uint_as_float((unsigned)(e0[k] >> 32));
            const bool other_wins = k < ksplit && eb > mb;
            ms = (k < ksplit) ? fmaxf(other_wins ? mb : eb, fmaxf(ms, es)) : ms;
            mc = other_wins ? (int)(unsigned)e1[k] : mc;
            mb = other_wins ? eb : mb;
        }
        best = mb; second = ms; code = mc;
        DVQ_STAMP(5);
    }
    const float thr = best - thr2W;
    const bool final_ok = (best - second) > thr2W;
    const bool valid = n >= 0;
    bool hopeless = !(code < K) || !(thr == thr);
#ifdef DVQ_TUNING
    if (g_dvq_tokdbg != nullptr && valid && h == 0) {
        f32x4 dbg = {best, second, thr2W, (float)code};
        *(f32x4 *)(g_dvq_tokdbg + 4 * (size_t)n) = dbg;
    }
#endif
    // undecided tokens are queued for the resolver.  The slot comes from an atomic whose result is not
    // needed until the record is written, so: bump the shard counter now (one atomic per wave, lane 0,
    // by the number of undecided tokens), run the z_q / loss phase while it is in flight, and only then
    // read it back and dump the records.
    const bool undecided = valid && !hopeless && !final_ok;
    // routed op: the rep x rep output positions of a coarser cell are copies of ONE vector -- same scores, same bound, undecided
    // together -- so only the cell's first position queues a record (RecMeta.rep) and the resolver corrects all of them: 37 %
    // fewer records at a fine ratio of 0.5 (dual), and the resolver's chunks then fit one per CU
    const int sel_rep = (SEL == 0 || sel_mask < 0.0f) ? (SEL == 0 ? 1 : 0) : (sel_mask == 1.0f ? 1 : (sel_mask == 0.25f ? 2 : 4));
    const bool queued = undecided && sel_rep > 0;           // sel_rep: 0 for a copy, else positions per edge of the lane's cell
    const unsigned long long umask = __ballot(queued && h == 0);
    // (SPLIT: which workgroup merges a block varies from run to run -- the shard is a function of the tokens, per wave, so that the
    // queue's layout, the fallback counts and the resolver's chunks do not)
    const int shard = (SPLIT ? tile_id * NW + wave : (int)blockIdx.x) & (DVQ_QSHARDS - 1);
    int slot_raw = 0;
    if (umask != 0ull && lane == 0) slot_raw = atomicAdd(&counters[DVQ_QCOUNT0 + shard], (int)__popcll(umask));
    if (valid && hopeless && h == 0) {
        int pos = atomicAdd(&counters[DVQ_C_EXACT], 1);
        exact_list[pos] = n;
    }
    // (CONV: the exact-list kernel computes the conv output of its tokens itself, from the conv's input -- round 6; through round 5
    // pass 1 spilled their rows to a full-size [B, D, HW] scratch tensor, 256 MiB per stream at B = 256)
    float lsum = 0.0f;
    float m_tok = 1.0f;
    if (valid && !hopeless) {
        if (h == 0) codes[n] = (long long)code;
        m_tok = (SEL != 0) ? __builtin_fabsf(sel_mask) : ((mask != nullptr) ? mask[n] : 1.0f);
        if (zq != nullptr || partials != nullptr) {
            // (the lane half re-derived from the lane id: `8 * h` of the prologue does not live in a VGPR through the code loop)
            int h_e = h;                                     // (where it frees the register; elsewhere it costs some)
            if constexpr (FOLD || (FLAT && SPLIT) || SEL == 2) h_e =(int)(__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) >> 5);
            const float *ep = E + (size_t)code * D + 8 * h_e;
            // gathers per batch: 2 k-steps (A/B on MI355X: 2 beats 1, 4, 8 and a 3-deep pipeline) where other workgroups hide the
            // latency; the split form's merging workgroup is alone on its CU and takes 8 (two round trips instead of eight)
            constexpr int SB = SPLIT ? ((S16 < 8) ? S16 : 8) : ((S16 < 2) ? S16 : 2);
            // `zq != nullptr` is tested ONCE (a scalar branch on the kernel argument): with the test
            // inside the loop on the per-lane pointer every one of the 128 stores became its own
            // exec-masked branch to an out-of-line block.
            auto finish = [&](auto store_tag) {
                constexpr bool STORE = decltype(store_tag)::value;
                int hw_e = HW;                               // opaque: the token's offset is recomputed from it here (a division
                asm volatile("" : "+s"(hw_e));               // by HW, once) instead of keeping the prologue's reciprocal of HW in a
                const __amdgpu_buffer_rsrc_t qr = wave_base(STORE ? zq : (float *)E, hw_e, h_e);       // VGPR through the code loop
                const unsigned qo = lane_off(hw_e, h_e);
                int hw4 = HW * (XT ? 2 : 4);                 // opaque: the 128 scalar offsets are recomputed here (two scalar
                asm volatile("" : "+s"(hw4));                // instructions each) instead of living in spilled SGPRs since the prologue
#pragma unroll
                for (int s0 = 0; s0 < S16; s0 += SB) {
                    f32x4 eg[SB][2];
#pragma unroll
                    for (int q = 0; q < SB; ++q) {
                        eg[q][0] = *(const f32x4 *)(ep + 16 * (s0 + q));
                        eg[q][1] = *(const f32x4 *)(ep + 16 * (s0 + q) + 4);
                    }
#pragma unroll
                    for (int q = 0; q < SB; ++q) {
                        const int s = s0 + q;
#pragma unroll
                        for (int j = 0; j < 8; ++j) {
                            float e = eg[q][j >> 2][j & 3];
                            if constexpr (FOLD) {           // the registers hold the conv's INPUT: z_q := e[code] (within 1e-6 of
                                if (STORE) DVQ_BUF_STORE(e, qr, qo, (16 * s + j) * hw4);   // fl(h + fl(e - h))), no loss term
                            } else {
                            float diff = __fsub_rn(e, zf[s][j]);
                            if constexpr (XT != 0) {
                                if (STORE) DVQ_BUF_STORE16(XT, __fadd_rn(zf[s][j], diff), qr, qo, (16 * s + j) * hw4);
                            } else
                            if (STORE) DVQ_BUF_STORE(__fadd_rn(zf[s][j], diff), qr, qo, (16 * s + j) * hw4);
                            lsum = __builtin_fmaf(diff, diff, lsum);   // the token's loss weight is applied once, below
                            }
                        }
                    }
                }
            };
            if constexpr (!FLAT) {
                if (zq != nullptr) finish(std::true_type{});
                else finish(std::false_type{});
                lsum *= m_tok;
            }
        }
    }
    if constexpr (FLAT) {
        // Row-major z_q: the lanes' values go through the wave's LDS image (one half of the channels at a time) and leave as
        // whole 128-byte lines, 16 bytes per lane -- the prologue's path backwards.  The image overlays the code ring: every wave
        // is past its last tile (barrier) and its surplus DMA has landed (the wait after the loop).
        char *flat_tr = lds + wave * FLAT_TRW;
        const bool store = zq != nullptr;                    // kernel argument: uniform
        if (store) __syncthreads();
        const bool mine = valid && !hopeless && (store || partials != nullptr);
        const unsigned long long okmask = __ballot(valid && !hopeless && h == 0);
        const long n0 = ((long)tile_id * NW + wave) * 32;
        const float *ep = E + (size_t)(mine ? code : 0) * D + 8 * h;
#pragma unroll
        for (int h2 = 0; h2 < 2; ++h2) {
            if (mine) {
                constexpr int SB = (S16 / 2 < 2) ? S16 / 2 : 2;
#pragma unroll
                for (int sp0 = 0; sp0 < S16 / 2; sp0 += SB) {
                    f32x4 eg[SB][2];
#pragma unroll
                    for (int q = 0; q < SB; ++q) {
                        eg[q][0] = *(const f32x4 *)(ep + 16 * (h2 * (S16 / 2) + sp0 + q));
                        eg[q][1] = *(const f32x4 *)(ep + 16 * (h2 * (S16 / 2) + sp0 + q) + 4);
                    }
#pragma unroll
                    for (int q = 0; q < SB; ++q) {
                        const int sp = sp0 + q, s = h2 * (S16 / 2) + sp;
                        f32x4 o[2];
#pragma unroll
                        for (int j = 0; j < 8; ++j) {
                            const float e = eg[q][j >> 2][j & 3];
                            if constexpr (FOLD) {
                                o[j >> 2][j & 3] = e;           // z_q := e[code] (see the NCHW form)
                            } else {
                                const float diff = __fsub_rn(e, zf[s][j]);
                                o[j >> 2][j & 3] = __fadd_rn(zf[s][j], diff);
                                lsum = __builtin_fmaf(diff, diff, lsum);
                            }
                        }
                        if (store) {
                            *(f32x4 *)(flat_tr + c * FLAT_RSH + (16 * sp + 8 * h) * 4) = o[0];
                            *(f32x4 *)(flat_tr + c * FLAT_RSH + (16 * sp + 8 * h + 4) * 4) = o[1];
                        }
                    }
                }
            }
            if (store) {
#pragma unroll
                for (int i = 0; i < FLAT_IPH; ++i) {
                    const int tk = i * FLAT_TPI + lane / FLAT_LPT;
                    const f32x4 v = *(const f32x4 *)(flat_tr + tk * FLAT_RSH + (lane % FLAT_LPT) * 16);
                    if ((okmask >> tk) & 1ull)              // (hopeless tokens: the exact-list kernel writes their rows)
                        __builtin_nontemporal_store(v, (f32x4 *)(zq + (size_t)(n0 + tk) * D + h2 * (D / 2)) + (lane % FLAT_LPT));
                }
            }
        }
        lsum *= m_tok;
    }
    DVQ_STAMP(6);
    if (umask != 0ull) {                                    // wave-uniform
        const int base = __shfl(slot_raw, 0);
        int slot = base + (int)__popcll(umask & ((1ull << c) - 1ull));   // rank among the wave's queued tokens
        slot = queued ? slot : -1;
        if (queued && slot >= rec_cap) {                    // shard full: full exact evaluation instead; the
            if (h == 0) {                                   // provisional code / z_q written above are overwritten
                const int rr = sel_rep > 0 ? sel_rep : 1;   // by the exact-list kernel, the loss term is dropped here
                for (int ry = 0; ry < rr; ++ry)
                    for (int rx = 0; rx < rr; ++rx) {
                        int pos = atomicAdd(&counters[DVQ_C_EXACT], 1);
                        exact_list[pos] = n + ry * rv.Wout + rx;
                    }
            }
            lsum = -(float)(sel_rep * sel_rep - 1) * lsum;  // ... for every copy of the cell (their terms equal this lane's bit for bit)
            slot = -1;
        }
        if (slot >= 0) {
            char *rec = records + ((size_t)shard * rec_cap + slot) * rec_bytes(D);
#pragma unroll
            for (int s = 0; s < S16; ++s) {
                f32x4 lo = {zf[s][0], zf[s][1], zf[s][2], zf[s][3]};
                f32x4 hi = {zf[s][4], zf[s][5], zf[s][6], zf[s][7]};
                *(f32x4 *)(rec + (16 * s + 8 * h) * 4) = lo;
                *(f32x4 *)(rec + (16 * s + 8 * h + 4) * 4) = hi;
            }
            if (h == 0) {
                RecMeta rm;
                rm.n = n; rm.xn = xn; rm.thr = thr; rm.m = m_tok; rm.prov = code;
                rm.best = ~0ull; rm.rep = sel_rep > 0 ? sel_rep : 1;
                *(RecMeta *)(rec + (size_t)D * 4) = rm;
            }
        }
    }
    if (partials != nullptr) {
        double dsum = (double)lsum;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) dsum += __shfl_xor(dsum, off);
        __syncthreads();
        double *red = (double *)lds;
        if (lane == 0) red[wave] = dsum;
        __syncthreads();
        if (tid == 0) partials[SPLIT ? tile_id : (int)blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
    }
    DVQ_STAMP(7);
}

// RES (every form below): pass1_body's resident seed table, for launches whose workgroups take at most 32 code tiles each
template <int D, int SEL, bool CONV, bool FOLD, bool RES>
__global__ __launch_bounds__(256, 2) void vq_assign_filter_kernel(
    const float *__restrict__ z, const char *__restrict__ img, const DvqF16Meta *__restrict__ meta,
    const float *__restrict__ E, const float *__restrict__ mask,
    int HW, int K, long N, float *__restrict__ zq, long long *__restrict__ codes,
    double *__restrict__ partials, int *__restrict__ counters, int *__restrict__ exact_list,
    char *__restrict__ records, int rec_cap, const DvqRouted rv, const DvqConv cv)
{
    pass1_body<D, SEL, CONV, FOLD, true, RES>(z, img, meta, E, mask, HW, K, N, zq, codes, partials, counters, exact_list, records, rec_cap, rv, cv);
}

// row-major latents [N, D] (FLAT, see pass1_body)
template <int D, bool FOLD, bool RES>
__global__ __launch_bounds__(256, 2) void vq_assign_filter_flat_kernel(
    const float *__restrict__ z, const char *__restrict__ img, const DvqF16Meta *__restrict__ meta,
    const float *__restrict__ E, const float *__restrict__ mask,
    int HW, int K, long N, float *__restrict__ zq, long long *__restrict__ codes,
    double *__restrict__ partials, int *__restrict__ counters, int *__restrict__ exact_list,
    char *__restrict__ records, int rec_cap, const DvqRouted rv, const DvqConv cv)
{
    pass1_body<D, 0, false, FOLD, true, RES, true>(z, img, meta, E, mask, HW, K, N, zq, codes, partials, counters, exact_list, records, rec_cap, rv, cv);
}

// small batches: `ksplit` workgroups per token block, each on its slice of the code tiles (SPLIT, see pass1_body).  Dense (FLAT:
// row-major latents), with the router select fused in (per-lane form, SEL = 1: every slice's workgroup writes the same indices /
// codebook_mask / gate), with the 1x1 conv as the prologue (CONV: every slice's workgroup computes the block's h itself,
// 3 x 8.4 MFLOP, nothing to share; the conv's inputs are read with the non-temporal hint) or on the conv-folded codebook (FOLD:
// loss-free inference / stage-2 tokenisation of single images)
template <int D, int SEL, bool CONV, bool FOLD, bool FLAT, bool RES>
__global__ __launch_bounds__(256, 2) void vq_assign_filter_split_kernel(
    const float *__restrict__ z, const char *__restrict__ img, const DvqF16Meta *__restrict__ meta,
    const float *__restrict__ E, const float *__restrict__ mask,
    int HW, int K, long N, float *__restrict__ zq, long long *__restrict__ codes,
    double *__restrict__ partials, int *__restrict__ counters, int *__restrict__ exact_list,
    char *__restrict__ records, int rec_cap, const DvqRouted rv, const DvqConv cv, f32x4 *__restrict__ split, int ksplit)
{
    pass1_body<D, SEL, CONV, FOLD, CONV, RES, FLAT, true>(z, img, meta, E, mask, HW, K, N, zq, codes, partials, counters, exact_list, records,
                                                     rec_cap, rv, cv, split, ksplit);
}

// the same kernel with plain loads of the latents, for batches that fit the memory-side cache (dense or staged select, no conv)
template <int D, int SEL, bool FOLD, bool RES>
__global__ __launch_bounds__(256, 2) void vq_assign_filter_cached_kernel(
    const float *__restrict__ z, const char *__restrict__ img, const DvqF16Meta *__restrict__ meta,
    const float *__restrict__ E, const float *__restrict__ mask,
    int HW, int K, long N, float *__restrict__ zq, long long *__restrict__ codes,
    double *__restrict__ partials, int *__restrict__ counters, int *__restrict__ exact_list,
    char *__restrict__ records, int rec_cap, const DvqRouted rv, const DvqConv cv)
{
    pass1_body<D, SEL, false, FOLD, false, RES>(z, img, meta, E, mask, HW, K, N, zq, codes, partials, counters, exact_list, records, rec_cap, rv, cv);
}

// 16-bit latents (XT: dvq_common.h), dense, any HW: the plain form's kernel on 2-byte loads and stores
template <int D, bool RES, int XT>
__global__ __launch_bounds__(256, 2) void vq_assign_filter_x16_kernel(
    const void *__restrict__ z, const char *__restrict__ img, const DvqF16Meta *__restrict__ meta,
    const float *__restrict__ E, const float *__restrict__ mask,
    int HW, int K, long N, void *__restrict__ zq, long long *__restrict__ codes,
    double *__restrict__ partials, int *__restrict__ counters, int *__restrict__ exact_list,
    char *__restrict__ records, int rec_cap)
{
    static_assert(XT == 1 || XT == 2, "f16 or bf16");
    pass1_body<D, 0, false, false, true, RES, false, false, XT>((const float *)z, img, meta, E, mask, HW, K, N, (float *)zq, codes, partials,
                                                                counters, exact_list, records, rec_cap, DvqRouted{}, DvqConv{});
}

// ---------------------------------------------------------------------------------------------
// host side: the workspace carve, the plan and the arguments of one launch (made by vq_assign_filter.hip)
// ---------------------------------------------------------------------------------------------
struct FilterWs {
    int *counters, *chunk_sync, *exact_list;
    char *records;
    int cap;
    f32x4 *split;                                            // [token block][slice < 8][128] of the split form (small batches), else null
};

// The forms of pass 1 (one kernel family each) and the plan of one launch
enum class P1Form { plain, cached, flat, split, wide, x16 };
struct P1Plan {
    P1Form form;
    int sel;                                                 // pass1_body's SEL
    bool conv, fold, flat;                                   // ... CONV, FOLD and FLAT
    int ks;                                                  // the split form's workgroups per token block
    int xt;                                                  // form x16: the latents' type (DVQ_DTYPE_F16 / DVQ_DTYPE_BF16); else 0
};

// two row-major forms at D = 256 keep the per-tile seed piece at every K: with the table their register allocation spills
// 2 - 3 dwords more (flat FOLD 6 -> 9, split flat 7 -> 9).  Their kernels exist in the unit without the table only.
constexpr bool p1_keeps_seed_piece(int D, P1Form form, bool fold, bool flat)
{
    return D == 256 && ((form == P1Form::flat && fold) || (form == P1Form::split && flat));
}

struct P1Args {
    const float *z;
    const char *img16;
    const DvqF16Meta *meta;
    const float *E, *mask;
    int HW, K;
    long N;
    float *zq;
    long long *codes;
    double *partials;
    const FilterWs &w;
    DvqRouted rv;
    DvqConv cv;
    hipStream_t st;
};

// One launch site per kernel family.  `if constexpr` keeps to the kernels the plans use: 20 plain, 4 cached, 6 flat, 17 split, each
// with and without the resident seed table (RES; but see p1_keeps_seed_piece).  The wide form: vq_pass1_wide.hip.
template <int D, int SEL, bool CONV, bool FOLD, bool FLAT, bool RES>
static int launch_pass1_form(const P1Plan &p, const P1Args &a)
{
    const unsigned nb = (unsigned)((a.N + 127) / 128);
    const size_t lds = dvq_pass1_lds_bytes(D);
#define DVQ_P1_ARGS a.z, a.img16, a.meta, a.E, a.mask, a.HW, a.K, a.N, a.zq, a.codes, a.partials, a.w.counters, a.w.exact_list, \
                    a.w.records, a.w.cap / DVQ_QSHARDS
    switch (p.form) {
    case P1Form::plain:
        if constexpr (!FLAT)
            return dvq_launch_lds<vq_assign_filter_kernel<D, SEL, CONV, FOLD, RES>>(dim3(nb), dim3(256), lds, a.st, DVQ_P1_ARGS, a.rv, a.cv);
        break;
    case P1Form::cached:
        if constexpr (D == 256 && SEL != 1 && !CONV && !FLAT)
            return dvq_launch_lds<vq_assign_filter_cached_kernel<D, SEL, FOLD, RES>>(dim3(nb), dim3(256), lds, a.st, DVQ_P1_ARGS, a.rv, a.cv);
        break;
    case P1Form::flat:
        if constexpr (FLAT && !(RES && p1_keeps_seed_piece(D, P1Form::flat, FOLD, FLAT)))
            return dvq_launch_lds<vq_assign_filter_flat_kernel<D, FOLD, RES>>(dim3(nb), dim3(256), lds, a.st, DVQ_P1_ARGS, a.rv, a.cv);
        break;
    case P1Form::split:
        if constexpr (SEL != 2 && !(FLAT && FOLD) && !(RES && p1_keeps_seed_piece(D, P1Form::split, FOLD, FLAT)))
            return dvq_launch_lds<vq_assign_filter_split_kernel<D, SEL, CONV, FOLD, FLAT, RES>>(dim3(nb * p.ks), dim3(256), lds, a.st,
                                                                                         DVQ_P1_ARGS, a.rv, a.cv, a.w.split, p.ks);
        break;
    case P1Form::wide:
    case P1Form::x16:                                        // launch_pass1_x16, below
        break;
    }
#undef DVQ_P1_ARGS
    return -1000;
}

// the plan's flags as template arguments.  RES: a workgroup's code tiles (the split form: its largest slice) fit the seed table that
// pass1_body keeps in the seeds area, 32 tiles = 1024 codes; larger codebooks take the per-tile seed piece
template <int D, bool RES>
static int launch_pass1_res(const P1Plan &p, const P1Args &a)
{
    if (p.conv) {
        if constexpr (D == 256)
            return p.sel ? launch_pass1_form<D, 1, true, false, false, RES>(p, a) : launch_pass1_form<D, 0, true, false, false, RES>(p, a);
        return -1000;
    }
    if (p.flat) return p.fold ? launch_pass1_form<D, 0, false, true, true, RES>(p, a) : launch_pass1_form<D, 0, false, false, true, RES>(p, a);
    switch (p.sel) {
    case 0:  return p.fold ? launch_pass1_form<D, 0, false, true, false, RES>(p, a) : launch_pass1_form<D, 0, false, false, false, RES>(p, a);
    case 1:  return p.fold ? launch_pass1_form<D, 1, false, true, false, RES>(p, a) : launch_pass1_form<D, 1, false, false, false, RES>(p, a);
    default: return p.fold ? launch_pass1_form<D, 2, false, true, false, RES>(p, a) : launch_pass1_form<D, 2, false, false, false, RES>(p, a);
    }
}

// the 16-bit form: one unit per (D, RES) as well (vq_pass1_x16_d<D>[_res].hip), both types in it
template <int D, bool RES>
static int launch_pass1_x16(const P1Plan &p, const P1Args &a)
{
    const unsigned nb = (unsigned)((a.N + 127) / 128);
    const size_t lds = dvq_pass1_lds_bytes(D);
    if (p.form != P1Form::x16) return -1000;
    if (p.xt == 1)
        return dvq_launch_lds<vq_assign_filter_x16_kernel<D, RES, 1>>(dim3(nb), dim3(256), lds, a.st, (const void *)a.z, a.img16, a.meta, a.E,
                                                                      a.mask, a.HW, a.K, a.N, (void *)a.zq, a.codes, a.partials,
                                                                      a.w.counters, a.w.exact_list, a.w.records, a.w.cap / DVQ_QSHARDS);
    if (p.xt == 2)
        return dvq_launch_lds<vq_assign_filter_x16_kernel<D, RES, 2>>(dim3(nb), dim3(256), lds, a.st, (const void *)a.z, a.img16, a.meta, a.E,
                                                                      a.mask, a.HW, a.K, a.N, (void *)a.zq, a.codes, a.partials,
                                                                      a.w.counters, a.w.exact_list, a.w.records, a.w.cap / DVQ_QSHARDS);
    return -1000;
}

// the six pass-1 units (vq_pass1_d<D>[_res].hip), the wide form (vq_pass1_wide.hip; D = 256) and the resolver (vq_resolve.hip)
int dvq_launch_pass1_d64(const P1Plan &p, const P1Args &a);
int dvq_launch_pass1_d64_res(const P1Plan &p, const P1Args &a);
int dvq_launch_pass1_d128(const P1Plan &p, const P1Args &a);
int dvq_launch_pass1_d128_res(const P1Plan &p, const P1Args &a);
int dvq_launch_pass1_d256(const P1Plan &p, const P1Args &a);
int dvq_launch_pass1_d256_res(const P1Plan &p, const P1Args &a);
int dvq_launch_pass1_wide(const P1Args &a);
int dvq_launch_pass1_x16_d64(const P1Plan &p, const P1Args &a);
int dvq_launch_pass1_x16_d64_res(const P1Plan &p, const P1Args &a);
int dvq_launch_pass1_x16_d128(const P1Plan &p, const P1Args &a);
int dvq_launch_pass1_x16_d128_res(const P1Plan &p, const P1Args &a);
int dvq_launch_pass1_x16_d256(const P1Plan &p, const P1Args &a);
int dvq_launch_pass1_x16_d256_res(const P1Plan &p, const P1Args &a);
int dvq_resolver_slices(int K);
// xt != 0: zq holds 16-bit latents of that type (dense op only)
int dvq_launch_resolver(int D, const char *img, const DvqF16Meta *meta, const float *en_all, const float *E,
                        int HWout, int K, float *zq, long long *codes, double *partials,
                        const FilterWs &w, int Wout, float *h_spill, const DvqFold *fd, hipStream_t st,
                        const double *p1_partials, int np1, int xt = 0);
#ifdef DVQ_TUNING
int dvq_tuning_set_pass1_d64(void *stamps, void *tokdbg);
int dvq_tuning_set_pass1_d64_res(void *stamps, void *tokdbg);
int dvq_tuning_set_pass1_d128(void *stamps, void *tokdbg);
int dvq_tuning_set_pass1_d128_res(void *stamps, void *tokdbg);
int dvq_tuning_set_pass1_d256(void *stamps, void *tokdbg);
int dvq_tuning_set_pass1_d256_res(void *stamps, void *tokdbg);
int dvq_tuning_set_resolve(void *stamps, void *tokdbg);
#endif
