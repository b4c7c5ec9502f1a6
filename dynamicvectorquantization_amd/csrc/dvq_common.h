// dvq_common.h -- shared device helpers and the codebook "prep" buffer layout (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

#define DVQ_CODE_TILE 32  // codes per MFMA tile (rows of a 32x32 MFMA)

// ---------------------------------------------------------------------------------------------
// 16-bit latents (the *_x16 entry points of dvq.h; XT = DVQ_DTYPE_F16 / DVQ_DTYPE_BF16, 0 = float32).  Only the storage type of
// latent-shaped tensors (z, z_q, g_zq, g_z) changes: a value is widened to fp32 where it enters registers (exact: f16 -> f32 is
// the hardware convert, subnormals included; bf16 -> f32 a 16-bit shift) and narrowed once, round-to-nearest-even, where it
// leaves them (f32 -> f16: v_cvt_f16_f32, overflow -> inf; f32 -> bf16: gfx950's v_cvt_pk_bf16_f32; NaN stays NaN) -- the
// bits of torch's `.float()` and `.to(dtype)`.  All arithmetic in between is the fp32 op's.
// ---------------------------------------------------------------------------------------------
template <int XT> struct DvqLat { typedef float T; };
template <> struct DvqLat<1> { typedef _Float16 T; };
template <> struct DvqLat<2> { typedef __bf16 T; };
template <int XT> __device__ __forceinline__ float dvq_widen(typename DvqLat<XT>::T v) { return (float)v; }
template <int XT> __device__ __forceinline__ typename DvqLat<XT>::T dvq_narrow(float v) { return (typename DvqLat<XT>::T)v; }
// the same on the raw 16 bits a buffer instruction moves (zero-extended in / low half out)
template <int XT> __device__ __forceinline__ float dvq_widen_bits(unsigned short u)
{
    if constexpr (XT == 2) return __builtin_bit_cast(float, (unsigned)u << 16);
    else return (float)__builtin_bit_cast(_Float16, u);
}
template <int XT> __device__ __forceinline__ unsigned short dvq_narrow_bits(float v)
{
    return __builtin_bit_cast(unsigned short, dvq_narrow<XT>(v));
}

// ---------------------------------------------------------------------------------------------
// Prep buffer (built once per codebook by dvq_codebook_prepare_f32), all offsets in bytes,
// T = ceil(K/32) code tiles:
//   [f32 tile images]  T x (32*D + 64) floats.  Image of tile t:
//        img[kg][c][p], kg < D/8, c < 32, p < 8  =  E[32t + c][8kg + 2(p&3) + (p>>2)]
//        (lane (c, h) of a wave reads its 4 next f32-MFMA A operands k = 8kg + {0,2,4,6} + h with
//         one ds_read_b128 at float offset (kg*32 + c)*8 + 4h), then en[32] (exact ATen-order
//        squared norms of the tile's codes; 0 for padded codes) and 32 floats of padding (no kernel reads them; the build parks
//        its partial maxima there: vq_assign_exact.hip, codebook_prep_f32_kernel).  tests/test_codebook_prep.py restates every section.
//   [en]               Kpad floats (Kpad = 32T): all squared norms, same values.
//   [f16 section]      used by the filter kernel, see vq_assign_filter.hip.
// ---------------------------------------------------------------------------------------------
__host__ __device__ inline int dvq_num_tiles(int K) { return (K + DVQ_CODE_TILE - 1) / DVQ_CODE_TILE; }
__host__ __device__ constexpr size_t dvq_tile_floats(int D) { return (size_t)32 * D + 64; }
__host__ __device__ inline size_t dvq_prep_f32_tiles_bytes(int K, int D)
{
    return (size_t)dvq_num_tiles(K) * dvq_tile_floats(D) * sizeof(float);
}
__host__ __device__ inline size_t dvq_prep_en_offset(int K, int D) { return dvq_prep_f32_tiles_bytes(K, D); }
__host__ __device__ inline size_t dvq_prep_f16_offset(int K, int D)
{
    return dvq_prep_en_offset(K, D) + (size_t)dvq_num_tiles(K) * 32 * sizeof(float);
}

// XCD-aware block remap (bijective for any grid size): consecutive tiles go to ONE XCD, so the
// adjacent pieces of a DRAM row / the shared operands are requested close together in time by
// one L2.  blockIdx % 8 labels the blocks that share an XCD (dispatch is round-robin); this is a
// speed heuristic only -- any placement gives the same results.
__device__ __forceinline__ int xcd_swizzle(int bid, int nblk)
{
    const int q = nblk >> 3, r = nblk & 7;
    const int xcd = bid & 7, idx = bid >> 3;
    const int start = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return start + idx;
}

// async global -> LDS copy, 16 B per lane; LDS destination = wave-uniform base + lane*16
__device__ __forceinline__ void glds16(const void *gsrc_lane, void *lds_wave_base)
{
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) void *)gsrc_lane,
        (__attribute__((address_space(3))) void *)lds_wave_base, 16, 0, 0);
}
// the same with an instruction offset OFF (bytes, < 4096): it is added to BOTH addresses -- global gsrc_lane + OFF, LDS
// lds_wave_base + OFF + lane*16 (measured: tools/micro/glds_offset.hip) -- so the pieces of one contiguous copy share one
// address register pair and one M0 value
template <int OFF>
__device__ __forceinline__ void glds16_off(const void *gsrc_lane, void *lds_wave_base)
{
    static_assert(OFF >= 0 && OFF < 4096, "13-bit signed instruction offset");
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) void *)gsrc_lane,
        (__attribute__((address_space(3))) void *)lds_wave_base, 16, OFF, 0);
}
__device__ __forceinline__ void glds4(const void *gsrc_lane, void *lds_wave_base)
{
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) void *)gsrc_lane,
        (__attribute__((address_space(3))) void *)lds_wave_base, 4, 0, 0);
}

// ATen-order squared norm pieces (see oracle/dvq_oracle.c): explicit roundings, never contracted.
__device__ __forceinline__ float sq_rn(float x) { return __fmul_rn(x, x); }

// torch CPU argmin step over candidates visited in ascending index:
// take if d < best, or d is NaN and best is not.
__device__ __forceinline__ bool argmin_take(float d, float best)
{
    return !(d >= best) && (best == best);
}

// merge two (distance, index) candidates of disjoint ascending scans
__device__ __forceinline__ void argmin_merge(float &d, int &i, float d2, int i2)
{
    bool n1 = d != d, n2 = d2 != d2;
    bool other;
    if (n1 || n2)
        other = n2 && (!n1 || i2 < i);
    else
        other = (d2 < d) || (d2 == d && i2 < i);
    if (other) { d = d2; i = i2; }
}

// torch argmax step over candidates visited in ascending index (vq_sample.hip, vq_gumbel.hip): take if v > best, or v is NaN and
// best is not
__device__ __forceinline__ bool argmax_take(float v, float best)
{
    return !(v <= best) && (best == best);
}

// merge two (value, index) candidates of disjoint ascending scans
__device__ __forceinline__ void argmax_merge(float &v, int &i, float v2, int i2)
{
    const bool n1 = v != v, n2 = v2 != v2;
    bool other;
    if (n1 || n2)
        other = n2 && (!n1 || i2 < i);
    else
        other = (v2 > v) || (v2 == v && i2 < i);
    if (other) { v = v2; i = i2; }
}

// (value, index) argmax of the draws argmax(p / q) and argmax(p) (sample.hip, vq_soft.hip's phase B), any visiting order: the
// smallest index among equal maxima; a NaN never wins (argmax_take / argmax_merge above are torch.argmax: there a NaN is the maximum)
__device__ __forceinline__ void argmax_pair(float &v, int &i, float ov, int oi)
{
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}

// Loss finalize fused into the last kernel of the filter path (vq_assign_exact_kernel in list
// mode): the block that draws the last ticket sums partials[0 .. nparts) and writes loss[0..1].
struct DvqLossTail {
    float *loss;              // nullptr = no fused loss finalize
    const double *partials;
    int *ticket;              // zeroed at the start of the op
    int nparts;
    double inv_numel;
    float beta;
    int *counters;            // nullptr = no queue bookkeeping; else counters[0] = total queued tokens
    int shard_cap;
};
#define DVQ_QSHARDS 64        // the pass-1 -> resolver queue is sharded this many ways (power of two)
#define DVQ_QCOUNT0 8         // counters[DVQ_QCOUNT0 + shard] = tokens queued in that shard
#define DVQ_COUNTER_BYTES 1024
// The counter block (ints) at the start of the filter path's workspace.  "report" words are only ever overwritten (what
// dvq_vq_assign_fallback_count_offset points at); "live" words are zero between ops: the list kernel's finishing workgroup puts
// them back (so does each chunk's last resolver slice with its ticket pair), and the zero kernel in front of the op is only
// launched for a caller that does not declare the workspace clean (DVQ_MODE_WS_CLEAN).
#define DVQ_C_QUEUED   0      // report: tokens queued for the resolver
#define DVQ_C_NEXACT   1      // report: tokens handed to the exact list
#define DVQ_C_EXACT    2      // live: exact-list append counter
#define DVQ_C_TICKET   4      // live: finalize ticket of the list kernel
#define DVQ_C_PREPASS  5
#define DVQ_SPLIT_TICKET0 128     // live: counters[DVQ_SPLIT_TICKET0 + token block] = slices done (split form of pass 1, small batches)
#ifndef DVQ_SPLIT_MAX_SLICES
#define DVQ_SPLIT_MAX_SLICES 8    // slices per token block at most (a power of two; 16: no faster at B = 4, 16 x 16, and the merge spills)
#endif
#define DVQ_SPLIT_MAX_BLOCKS 64   // ... which serves up to this many token blocks of 128 (beyond: no gain measured, profiles/r05_small_batch.json)
// Cache policy of the streaming reads of a batch's latents / branch features: up to this many bytes of the FINEST tensor (the coarser
// branches add a third) they are read with plain loads -- the 256-MB memory-side cache then serves what the producer wrote or the router
// gate just read -- above it with the non-temporal hint.  profiles/archive/r04_cache_policy.json: one batch at a time, plain loads pay up to
// ~150 MB (configs[1] -2.4 %, the gate op -5 %); with three batches in flight on three streams (how bench.py and a serving loop drive
// the op) they pay only while all three working sets fit the cache together, hence 64 MiB (B = 64 at 32 x 32 x 256); B = 128 under
// three streams loses 3 % with plain loads, B = 256 3 - 6 % even alone.
#ifndef DVQ_CACHED_MAX_BYTES
#define DVQ_CACHED_MAX_BYTES ((size_t)64 << 20)
#endif
#define DVQ_EXACT_LIST_BLOCKS 512   // grid of the list-mode exact kernel (2 per CU; it walks the list in chunks)

// Launch of a kernel with more than 64 KiB of dynamic LDS: the per-device opt-in to OPTIN bytes (0 = the launch's `lds`) is
// applied once per kernel and device -- a bitmask per kernel, one bit per device ordinal, so a process driving several GPUs opts
// in on each; relaxed atomics: two host threads may both apply the attribute, which is idempotent.  Returns the HIP error of the
// opt-in or of the launch (0 = ok).
template <auto Kernel>
static unsigned long long dvq_lds_done = 0;

template <auto Kernel, int OPTIN = 0, class... A>
static inline int dvq_launch_lds(dim3 grid, dim3 block, size_t lds, hipStream_t st, A... args)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev > 63) dev = 63;     // shared bit: always re-apply
    if (dev == 63 || !((__atomic_load_n(&dvq_lds_done<Kernel>, __ATOMIC_RELAXED) >> dev) & 1ull)) {
        const hipError_t rc = hipFuncSetAttribute((const void *)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                  OPTIN ? OPTIN : (int)lds);
        if (rc != hipSuccess) return (int)rc;
        if (dev != 63) __atomic_fetch_or(&dvq_lds_done<Kernel>, 1ull << dev, __ATOMIC_RELAXED);
    }
    hipLaunchKernelGGL(Kernel, grid, block, lds, st, args...);
    return (int)hipGetLastError();
}

// per-launch host-side error plumbing (dvq_abi.hip)
void dvq_set_error(const char *fmt, ...);

// training-mode routing tail (router_train.hip): arguments of one forward or backward call, branches coarse -> fine
struct DvqRouteTrain {
    int nb, B, C, hc, wc, groups;  // groups == 0: no normalisation
    float eps;
    const float *h[3], *gn_w[3], *gn_b[3];
    const float *w1, *b1, *w2, *b2;
    int hid, act;                  // hid == 0: single Linear (w2 = that layer)
    const float *gumbels;          // nullptr: no-gumbel mode (gate = logits, no scale)
    float tau;
    float *h_out, *cmask, *gate;   // forward outputs
    long long *indices;
    const float *g_out, *g_gate;   // backward inputs (nullable)
    float *dh[3], *dgn_w[3], *dgn_b[3], *dw1, *db1, *dw2, *db2;
    void *ws;
};

// exclusive prefix count of `flag` over the 256 threads of the block (4 waves); `total` = the block's count.
// wave_tot: 4 ints of LDS.  Used by the stream compactions of permute.hip and sample.hip.
__device__ __forceinline__ int block_excl_scan_256(int flag, int *wave_tot, int &total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long m = __ballot(flag);
    const int in_wave = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wave_tot[wave] = __popcll(m);
    __syncthreads();
    int off = 0;
    for (int w = 0; w < wave; ++w) off += wave_tot[w];
    total = wave_tot[0] + wave_tot[1] + wave_tot[2] + wave_tot[3];
    __syncthreads();
    return off + in_wave;
}
