// sample.hip -- the token-level glue of stage-2 generation (gfx950): one sampling step of
// Dualformer.sample_from_scratch and the coarse -> fine position transfer.
//
// Replaces (reference models/stage2_dynamic/dqtransformer_class.py and its two variants):
//   sampling head  :313-330 and the three other position / content blocks of sample_from_scratch:
//                  `[:, -1, :] / temperature`, avoid_* (:518-557, one Python loop over the batch with
//                  3-4 indexed writes per row), top_k_logits, softmax, top_p_logits (models/stage2/utils.py:22-40:
//                  sort, cumsum, scatter, renormalise) and torch.multinomial / torch.topk
//   transfer       transfer_sampled_coarse_position_to_{remain,sampled}_fine_position (:464-516): a double
//                  Python loop with one device->host read per coarse step, then pad_sequence
//
// Head: one workgroup of 256 threads per row, the row (V <= 8192) in LDS.
//   top-k      exact k-th largest by a radix select (4 x 8-bit digits) over order-preserving uint32 keys;
//              integer histograms, so the threshold is exact and ties above it are all kept (as `out < v[-1]`)
//   softmax    max, expf(x - max), one fixed-order sum (per-thread strided sums, then a shuffle tree per wave,
//              then the 4 wave totals in order), a true division per element
//   top-p      the kept set is a prefix of the order (p descending, index ascending).  Its last element X is
//              found by a radix descent (6 x 8-bit digits) over the 43-bit key (0x3F800000 - bits(p)) << 13 | j,
//              choosing at each digit the largest one whose "mass strictly before" stays < p.  The masses are
//              sums of p_j in 48-bit fixed point (integer LDS atomics: order-independent, hence deterministic;
//              truncation error < V * 2^-48).  Kept: renormalised by a fixed-order float sum.
//   draw       argmax(p / q) (torch.multinomial's own algorithm, q = Exp(1) draws given by the caller) or
//              argmax(p); first index on ties.
// Transfer: count + fill kernels like permute.hip (ballot scan of the marked cells; ranks in LDS for row-first).
#include "launchers.h"

constexpr int SAMPLE_MAX_V = 8192;
constexpr int SAMPLE_MAX_CELLS = 1024;

struct SampleRules { long long pad, ban_a, ban_from, restore, ban_b, ban_from_post, flag_code; };

// order-preserving float <-> uint32 key (a larger float has a larger key; -inf is below every finite value)
__device__ __forceinline__ unsigned f2key(float f)
{
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key2f(unsigned k)
{
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// inclusive prefix sum over the 256 threads of the block (thread order); wtot: 4 words of LDS
__device__ __forceinline__ unsigned long long block_incl_scan_u64(unsigned long long v, unsigned long long *wtot)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long n = __shfl_up(v, off);
        if (lane >= off) v += n;
    }
    if (lane == 63) wtot[wave] = v;
    __syncthreads();
    unsigned long long base = 0;
    for (int w = 0; w < wave; ++w) base += wtot[w];
    __syncthreads();
    return base + v;
}

// fixed-order block reductions: a shuffle tree within each wave, then the 4 wave results in wave order
__device__ __forceinline__ float block_sum_f32(float v, float *red)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const float s = ((red[0] + red[1]) + red[2]) + red[3];
    __syncthreads();
    return s;
}
__device__ __forceinline__ float block_max_f32(float v, float *red)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const float m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    return m;
}
__global__ __launch_bounds__(256) void sample_head_kernel(
    const float *__restrict__ logits, long long lstride, int V, float temperature, SampleRules r,
    const long long *__restrict__ hist, long long hstride, int hlen, float *__restrict__ flag,
    int top_k, float top_p, int sample, const float *__restrict__ q,
    long long *__restrict__ tokens, long long tstride, float *__restrict__ out_logits, float *__restrict__ out_probs)
{
    __shared__ float val[SAMPLE_MAX_V];
    __shared__ unsigned banned[SAMPLE_MAX_V / 32];
    __shared__ unsigned long long bins[256];
    __shared__ unsigned long long wtot[4];
    __shared__ float red[4];
    __shared__ unsigned long long pick[2];
    __shared__ int redi[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float NEG_INF = -__builtin_inff();
    const float *lrow = logits + (size_t)b * lstride;
    const bool flagged = flag[b] != 0.0f;
    const bool use_hist = !flagged && hlen > 0;

    // 1. logits / temperature (IEEE division: this file is built without fast-math and with -ffp-contract=off)
    for (int j = tid; j < V; j += 256) val[j] = lrow[j] / temperature;
    if (use_hist) {
        for (int w = tid; w < (V + 31) / 32; w += 256) banned[w] = 0u;
        __syncthreads();
        const long long *h = hist + (size_t)b * hstride;
        for (int k = tid; k < hlen; k += 256) {
            const long long c = h[k];
            if (c >= 0 && c < V) atomicOr(&banned[c >> 5], 1u << (c & 31));
        }
    }
    __syncthreads();

    // 2. the mask rule of the step kind (include/dvq.h: dvq_sample_head_f32)
    for (int j = tid; j < V; j += 256) {
        const float x = val[j];
        float v;
        if (flagged) {
            v = (j == r.pad) ? x : NEG_INF;
        } else {
            const bool ban = (use_hist && ((banned[j >> 5] >> (j & 31)) & 1u)) || j == r.pad || j == r.ban_a ||
                             (r.ban_from >= 0 && j >= r.ban_from);
            v = ban ? NEG_INF : x;
            if (j == r.restore) v = x;
            if (j == r.ban_b || (r.ban_from_post >= 0 && j >= r.ban_from_post)) v = NEG_INF;
        }
        val[j] = v;
    }
    __syncthreads();

    // 3. top_k_logits: the k-th largest key, MSB digit first
    if (top_k > 0) {
        unsigned prefix = 0;
        unsigned long long krem = (unsigned long long)top_k;
        for (int shift = 24; shift >= 0; shift -= 8) {
            bins[tid] = 0;
            __syncthreads();
            const unsigned hmask = (shift == 24) ? 0u : (0xffffffffu << (shift + 8));
            for (int j = tid; j < V; j += 256) {
                const unsigned k = f2key(val[j]);
                if ((k & hmask) == (prefix & hmask)) atomicAdd(&bins[(k >> shift) & 255u], 1ull);
            }
            __syncthreads();
            const int d = 255 - tid;                               // digits in descending order
            const unsigned long long c = bins[d];
            const unsigned long long incl = block_incl_scan_u64(c, wtot);   // matching elements with digit >= d
            if (incl >= krem && incl - c < krem) { pick[0] = (unsigned long long)d; pick[1] = krem - (incl - c); }
            __syncthreads();
            prefix |= (unsigned)pick[0] << shift;
            krem = pick[1];
            __syncthreads();
        }
        const float thr = key2f(prefix);
        for (int j = tid; j < V; j += 256) {
            const float v = val[j];
            if (v < thr) val[j] = NEG_INF;
        }
        __syncthreads();
    }
    if (out_logits)
        for (int j = tid; j < V; j += 256) out_logits[(size_t)b * V + j] = val[j];

    // 4. softmax
    float m = NEG_INF;
    for (int j = tid; j < V; j += 256) m = fmaxf(m, val[j]);
    m = block_max_f32(m, red);
    float s = 0.0f;
    for (int j = tid; j < V; j += 256) {
        const float e = expf(val[j] - m);
        val[j] = e;
        s += e;
    }
    s = block_sum_f32(s, red);
    for (int j = tid; j < V; j += 256) val[j] = val[j] / s;
    __syncthreads();

    // 5. top_p_logits: keep j iff the mass strictly before j in (p desc, index asc) order is < p
    if (top_p > 0.0f) {
        const double scale = 281474976710656.0;                 // 2^48
        unsigned long long P = (unsigned long long)((double)top_p * scale);
        if (P == 0) P = 1;
        unsigned long long prefix = 0, below = 0;
        for (int shift = 40; shift >= 0; shift -= 8) {
            bins[tid] = 0;
            __syncthreads();
            for (int j = tid; j < V; j += 256) {
                const float p = val[j];
                const unsigned long long key = ((unsigned long long)(0x3F800000u - __float_as_uint(p)) << 13) | (unsigned)j;
                if ((key >> (shift + 8)) == (prefix >> (shift + 8)))
                    atomicAdd(&bins[(key >> shift) & 255ull], (unsigned long long)((double)p * scale));
            }
            __syncthreads();
            const unsigned long long w = bins[tid];
            const unsigned long long incl = block_incl_scan_u64(w, wtot), excl = incl - w;
            if (below + excl < P && (tid == 255 || below + incl >= P)) { pick[0] = (unsigned long long)tid; pick[1] = below + excl; }
            __syncthreads();
            prefix |= pick[0] << shift;
            below = pick[1];
            __syncthreads();
        }
        float ks = 0.0f;
        for (int j = tid; j < V; j += 256) {
            const float p = val[j];
            const unsigned long long key = ((unsigned long long)(0x3F800000u - __float_as_uint(p)) << 13) | (unsigned)j;
            const float kept = (key <= prefix) ? p : 0.0f;
            val[j] = kept;
            ks += kept;
        }
        ks = block_sum_f32(ks, red);
        for (int j = tid; j < V; j += 256) val[j] = val[j] / ks;
        __syncthreads();
    }
    if (out_probs)
        for (int j = tid; j < V; j += 256) out_probs[(size_t)b * V + j] = val[j];

    // 6. the draw: argmax(p / q) or argmax(p), first index on ties
    const float *qrow = sample ? q + (size_t)b * V : nullptr;
    float bv = NEG_INF;
    int bi = 0x7fffffff;
    for (int j = tid; j < V; j += 256) argmax_pair(bv, bi, sample ? val[j] / qrow[j] : val[j], j);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) argmax_pair(bv, bi, __shfl_xor(bv, off), __shfl_xor(bi, off));
    if ((tid & 63) == 0) { red[tid >> 6] = bv; redi[tid >> 6] = bi; }
    __syncthreads();
    if (tid == 0) {
        float v = red[0];
        int ix = redi[0];
        for (int w = 1; w < 4; ++w) argmax_pair(v, ix, red[w], redi[w]);
        if (ix == 0x7fffffff) ix = 0;                            // every ratio NaN: not reached by a finite row
        tokens[(size_t)b * tstride] = ix;
        if (r.flag_code >= 0 && ix == r.flag_code) flag[b] = flag[b] + 1.0f;
    }
}

// coarse cells sampled before the first coarse EOS of the row: mark[c] = 1 (columns 1.. of the row; column 0 is the sos)
__device__ void transfer_mark(const long long *__restrict__ row, int Lc, int ncell, long long ceos, int *mark, int *eos_at)
{
    for (int c = threadIdx.x; c < ncell; c += 256) mark[c] = 0;
    if (threadIdx.x == 0) *eos_at = Lc - 1;
    __syncthreads();
    for (int l = 1 + threadIdx.x; l < Lc; l += 256) if (row[l] == ceos) atomicMin(eos_at, l - 1);
    __syncthreads();
    const int n = *eos_at;
    for (int l = threadIdx.x; l < n; l += 256) {
        const long long c = row[1 + l];
        if (c >= 0 && c < ncell) mark[c] = 1;                    // repeated positions mark the same cell
    }
    __syncthreads();
}

__global__ __launch_bounds__(256) void transfer_count_kernel(const long long *__restrict__ cp, long long cstride, int Lc,
                                                             int ncell, long long ceos, int remain, int *__restrict__ counts,
                                                             int *__restrict__ maxes)
{
    __shared__ int mark[SAMPLE_MAX_CELLS];
    __shared__ int eos_at, tot;
    transfer_mark(cp + (size_t)blockIdx.x * cstride, Lc, ncell, ceos, mark, &eos_at);
    if (threadIdx.x == 0) tot = 0;
    __syncthreads();
    int n = 0;
    for (int c = threadIdx.x; c < ncell; c += 256) n += (mark[c] != remain);
    for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off);
    if ((threadIdx.x & 63) == 0) atomicAdd(&tot, n);
    __syncthreads();
    if (threadIdx.x == 0) {
        counts[blockIdx.x] = tot;
        atomicMax(maxes, tot);
    }
}

__global__ __launch_bounds__(256) void transfer_fill_kernel(const long long *__restrict__ cp, long long cstride, int Lc,
                                                            int hc, long long ceos, int remain, int row_first, int sos_mode,
                                                            long long sos, long long feos, long long fpad, int L,
                                                            long long *__restrict__ out)
{
    __shared__ int mark[SAMPLE_MAX_CELLS];
    __shared__ int rank_f[SAMPLE_MAX_CELLS + 1];
    __shared__ int wave_tot[4];
    __shared__ int eos_at;
    const int b = blockIdx.x, ncell = hc * hc, W = 2 * hc;
    const long long *row = cp + (size_t)b * cstride;
    transfer_mark(row, Lc, ncell, ceos, mark, &eos_at);
    const int off = sos_mode ? 1 : 0;
    long long *o = out + (size_t)b * L + off;
    const int Lo = L - off;
    int base = 0;
    for (int c0 = 0; c0 < ncell; c0 += 256) {
        const int ci = c0 + threadIdx.x;
        const bool sel = ci < ncell && mark[ci] != remain;
        int tot;
        const int rf = block_excl_scan_256(sel, wave_tot, tot) + base;
        if (ci < ncell) rank_f[ci] = rf;
        if (sel && !row_first) {                                 // region-first: the 4 fine positions of the cell together
            const int cy = ci / hc, cx = ci - cy * hc;
#pragma unroll
            for (int qd = 0; qd < 4; ++qd) {
                const int k = 4 * rf + qd;
                if (k < Lo) o[k] = (long long)(2 * cy + (qd >> 1)) * W + 2 * cx + (qd & 1);
            }
        }
        base += tot;
    }
    if (threadIdx.x == 0) rank_f[ncell] = base;
    __syncthreads();
    if (row_first) {                                             // fine pixels in row-major order
        for (int ci = threadIdx.x; ci < ncell; ci += 256) {
            if (mark[ci] == remain) continue;
            const int cy = ci / hc, cx = ci - cy * hc;
            const int row0 = rank_f[cy * hc], rowcnt = rank_f[(cy + 1) * hc] - row0, within = rank_f[ci] - row0;
#pragma unroll
            for (int qd = 0; qd < 4; ++qd) {
                const int dy = qd >> 1, dx = qd & 1;
                const int k = 4 * row0 + dy * 2 * rowcnt + 2 * within + dx;
                if (k < Lo) o[k] = (long long)(2 * cy + dy) * W + 2 * cx + dx;
            }
        }
    }
    for (int k = 4 * base + threadIdx.x; k < Lo; k += 256) o[k] = (k == 4 * base) ? feos : fpad;
    if (sos_mode && threadIdx.x == 0) out[(size_t)b * L] = (sos_mode == 1) ? sos : row[0];
}

__global__ void transfer_zero_max_kernel(int *__restrict__ maxes)
{
    if (threadIdx.x == 0) maxes[0] = 0;
}

int dvq_launch_sample_head(const float *logits, long long lstride, int B, int V, float temperature, const long long *rules,
                           const long long *hist, long long hstride, int hlen, float *flag, int top_k, float top_p,
                           int sample, const float *q, long long *tokens, long long tstride, float *out_logits,
                           float *out_probs, hipStream_t st)
{
    SampleRules r = {rules[0], rules[1], rules[2], rules[3], rules[4], rules[5], rules[6]};
    hipLaunchKernelGGL(sample_head_kernel, dim3(B), dim3(256), 0, st, logits, lstride, V, temperature, r, hist, hstride, hlen,
                       flag, top_k, top_p, sample, q, tokens, tstride, out_logits, out_probs);
    return (int)hipGetLastError();
}

int dvq_launch_transfer_count(const long long *cp, long long cstride, int B, int Lc, int hc, long long ceos, int remain,
                              int *counts, int *maxes, hipStream_t st)
{
    // zeroed by a kernel, not hipMemsetAsync (as permute.hip: memset nodes misbehave under hipGraph replay)
    hipLaunchKernelGGL(transfer_zero_max_kernel, dim3(1), dim3(64), 0, st, maxes);
    hipLaunchKernelGGL(transfer_count_kernel, dim3(B), dim3(256), 0, st, cp, cstride, Lc, hc * hc, ceos, remain, counts, maxes);
    return (int)hipGetLastError();
}

int dvq_launch_transfer_fill(const long long *cp, long long cstride, int B, int Lc, int hc, long long ceos, int remain,
                             int row_first, int sos_mode, long long sos, long long feos, long long fpad, int L, long long *out,
                             hipStream_t st)
{
    hipLaunchKernelGGL(transfer_fill_kernel, dim3(B), dim3(256), 0, st, cp, cstride, Lc, hc, ceos, remain, row_first, sos_mode,
                       sos, feos, fpad, L, out);
    return (int)hipGetLastError();
}

int dvq_sample_max_vocab(void) { return SAMPLE_MAX_V; }
int dvq_sample_max_cells(void) { return SAMPLE_MAX_CELLS; }
