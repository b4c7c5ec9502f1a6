// code_stats.hip -- code-usage statistics of a batch of int64 codes for gfx950: the histogram, the number of codes in use, the
// perplexity of the histogram and (optionally) the dense one-hot matrix the taming quantizers return.
//
// Replaces, in VectorQuantizer / EMAVectorQuantizer (reference modules/vector_quantization/quantize_vqgan.py:58-60, 84-85 and
// :434-436): `zeros(N, K)` + `scatter_` (or F.one_hot + a dtype cast), `mean(0)`, `log`, `sum`, `exp` -- four or five passes over
// an [N, K] fp32 matrix (1 GiB at N = 262144, K = 1024) -- and the host-side Python sets of scripts/tools/codebook_usage*.py.
// Here ONE sweep over the codes: a workgroup owns a contiguous range of rows, counts their codes in LDS (32-bit counters, K <=
// 16384: 64 KiB), writes their one-hot rows exactly once (16-byte non-temporal stores when K % 4 == 0 and the buffer is 16-byte
// aligned: every quad then lies inside one row; 4-byte stores otherwise) and flushes its non-zero counters with 64-bit integer
// atomics.  Larger K, or a workgroup with fewer than K / 16 codes to count: the counts go to global memory directly.  No float atomics anywhere: the counts are exact, and the
// perplexity is a pure function of them (one workgroup, a fixed summation order), so it is the same bits on every run.
// The one-hot write is a pure HBM write stream: its bound is N * K * 4 bytes over the write bandwidth.
//
// Grain form: codes [B, H, W] of a dual / triple granularity model with its grain map [B, hc, wc] (0 = coarsest): every REGION is
// counted once, into the row of its grain -- position (y, x) counts iff y and x are multiples of s = (H / hc) >> grain, which is
// the position the permuter emits for that region.
#include "launchers.h"

#define CS_NT 256
#define CS_LDS_MAX_FLAT 16384              // counters in LDS, flat form: 64 KiB, two workgroups per CU still stream the one-hot
#define CS_LDS_MAX_GRAIN 36860             // ... grain form (no stream behind it): up to 144 KiB of the CU's 160

__global__ __launch_bounds__(CS_NT) void code_stats_zero_kernel(unsigned long long *__restrict__ a, size_t na,
                                                                unsigned long long *__restrict__ b, size_t nb)
{
    const size_t stride = (size_t)gridDim.x * CS_NT, i0 = (size_t)blockIdx.x * CS_NT + threadIdx.x;
    for (size_t i = i0; i < na; i += stride) a[i] = 0ull;
    for (size_t i = i0; i < nb; i += stride) b[i] = 0ull;
}

// one counted code: all lanes of the wave on ONE code (a collapsed codebook, the copies of a coarse cell) is one add of the
// lane count instead of 64 adds that serialise on one address
template <bool LDS>
__device__ __forceinline__ void count_code(bool ok, int idx, unsigned *__restrict__ hist, unsigned long long *__restrict__ counts)
{
    const unsigned long long act = __ballot(ok);
    if (act == 0ull) return;
    const int first = __builtin_amdgcn_readlane(idx, __builtin_ctzll(act));
    const unsigned long long same = __ballot(ok && idx == first);
    if (same == act) {
        if ((int)(threadIdx.x & 63) == __builtin_ctzll(act)) {
            if (LDS) atomicAdd(&hist[first], (unsigned)__popcll(act));
            else atomicAdd(&counts[first], (unsigned long long)__popcll(act));
        }
        return;
    }
    if (ok) {
        if (LDS) atomicAdd(&hist[idx], 1u);
        else atomicAdd(&counts[idx], 1ull);
    }
}

// flat form: workgroup b owns rows [b * rpb, min(N, (b + 1) * rpb))
template <bool LDS, int ONEHOT>            // ONEHOT: 0 none, 1 four-byte stores, 4 sixteen-byte stores (K % 4 == 0, aligned buffer)
__global__ __launch_bounds__(CS_NT) void code_stats_kernel(const long long *__restrict__ codes, long N, int K, long rpb,
                                                           unsigned long long *__restrict__ counts, float *__restrict__ onehot)
{
    extern __shared__ unsigned cs_hist[];
    const int tid = threadIdx.x;
    const long r0 = (long)blockIdx.x * rpb;
    const long r1 = r0 + rpb < N ? r0 + rpb : N;
    if (LDS) {
        for (int j = tid; j < K; j += CS_NT) cs_hist[j] = 0u;
        __syncthreads();
    }
    for (long rb = r0; rb < r1; rb += CS_NT) {                           // (whole waves enter: count_code ballots)
        const long r = rb + tid;
        const long long c = r < r1 ? codes[r] : -1;
        const bool ok = c >= 0 && c < K;
        count_code<LDS>(ok, ok ? (int)c : 0, cs_hist, counts);
    }
    if (ONEHOT != 0) {
        // the rows' elements as one flat range [r0 K, r1 K); a thread's position is kept as (row, column) and advanced by the
        // workgroup's step with one 32-bit division (column + step < 2^31: K < 2^20, step = 1024 at most)
        constexpr unsigned V = ONEHOT, STEP = CS_NT * V;
        long row = r0;
        unsigned col = (unsigned)tid * V;
        if (col >= (unsigned)K) { const unsigned q = col / (unsigned)K; row += q; col -= q * (unsigned)K; }
        while (row < r1) {
            const long long c = codes[row];
            const size_t e = (size_t)row * (size_t)K + col;
            if (V == 4) {
                const long long d = c - (long long)col;                   // 0 .. 3: the one falls into this quad
                f32x4 v;
                v.x = d == 0 ? 1.0f : 0.0f;
                v.y = d == 1 ? 1.0f : 0.0f;
                v.z = d == 2 ? 1.0f : 0.0f;
                v.w = d == 3 ? 1.0f : 0.0f;
                __builtin_nontemporal_store(v, (f32x4 *)(onehot + e));
            } else {
                __builtin_nontemporal_store(c == (long long)col ? 1.0f : 0.0f, onehot + e);
            }
            col += STEP;
            if (col >= (unsigned)K) { const unsigned q = col / (unsigned)K; row += q; col -= q * (unsigned)K; }
        }
    }
    if (LDS) {
        __syncthreads();
        for (int j = tid; j < K; j += CS_NT) {
            const unsigned c = cs_hist[j];
            if (c != 0u) atomicAdd(&counts[j], (unsigned long long)c);
        }
    }
}

// grain form: counts [G, K], n_tokens [G]; LDS layout: [G * K] counters, then [G] token counters
template <bool LDS>
__global__ __launch_bounds__(CS_NT) void code_stats_grain_kernel(const long long *__restrict__ codes,
                                                                 const long long *__restrict__ grain, long N, int H, int W,
                                                                 int hc, int wc, int G, int K, long ppb,
                                                                 unsigned long long *__restrict__ counts,
                                                                 unsigned long long *__restrict__ n_tokens)
{
    extern __shared__ unsigned cs_hist[];
    const int tid = threadIdx.x;
    const int GK = G * K;
    const long p0 = (long)blockIdx.x * ppb;
    const long p1 = p0 + ppb < N ? p0 + ppb : N;
    if (LDS) {
        for (int j = tid; j < GK + G; j += CS_NT) cs_hist[j] = 0u;
        __syncthreads();
    }
    const int S = H / hc;                                                // = W / wc = 2^(G - 1), checked by the caller
    const long HWl = (long)H * W;
    for (long pb = p0; pb < p1; pb += CS_NT) {
        const long p = pb + tid;
        bool tok = false, ok = false;
        int idx = 0, g = 0;
        if (p < p1) {
            const long b = p / HWl;
            const int rem = (int)(p - b * HWl);
            const int y = rem / W, x = rem - y * W;
            const long long gl = grain[(b * hc + y / S) * wc + x / S];
            if (gl >= 0 && gl < G) {
                g = (int)gl;
                const int s = S >> g;
                if (y % s == 0 && x % s == 0) {
                    tok = true;
                    const long long c = codes[p];
                    ok = c >= 0 && c < K;
                    idx = ok ? g * K + (int)c : 0;
                }
            }
        }
        count_code<LDS>(ok, idx, cs_hist, counts);
        count_code<LDS>(tok, LDS ? GK + g : g, cs_hist, n_tokens);
    }
    if (LDS) {
        __syncthreads();
        for (int j = tid; j < GK + G; j += CS_NT) {
            const unsigned c = cs_hist[j];
            if (c != 0u) atomicAdd(j < GK ? &counts[j] : &n_tokens[j - GK], (unsigned long long)c);
        }
    }
}

// workgroup g: n_used[g] and perplexity[g] of counts[g, :].  p_j = fl(count_j) / fl(n) (one fp32 division -- bit for bit the
// reference's mean(one_hot, 0)), t_j = p_j * logf(p_j + 1e-10f), H = the sum of the t_j in double: a thread adds a contiguous
// index range in index order, thread 0 adds the 256 partial sums in thread order -- one fixed order, a pure function of the counts.
__global__ __launch_bounds__(CS_NT) void code_stats_finalize_kernel(const unsigned long long *__restrict__ counts, int K,
                                                                    const unsigned long long *__restrict__ n_tokens, long n_flat,
                                                                    long long *__restrict__ n_used, float *__restrict__ perplexity)
{
    __shared__ double part[CS_NT];
    __shared__ int used[CS_NT];
    const int tid = threadIdx.x, g = blockIdx.x;
    const unsigned long long *cnt = counts + (size_t)g * K;
    const unsigned long long n = n_tokens != nullptr ? n_tokens[g] : (unsigned long long)n_flat;
    const float nf = (float)n;
    const int per = (K + CS_NT - 1) / CS_NT;
    const int j0 = tid * per, j1 = j0 + per < K ? j0 + per : K;
    double h = 0.0;
    int u = 0;
    for (int j = j0; j < j1; ++j) {
        const unsigned long long c = cnt[j];
        if (c != 0ull) {                                                 // (a zero count adds 0 * logf(1e-10f) = -0.0: nothing)
            ++u;
            const float p = (float)c / nf;
            h += (double)__fmul_rn(p, logf(__fadd_rn(p, 1e-10f)));
        }
    }
    part[tid] = h;
    used[tid] = u;
    __syncthreads();
    if (tid == 0) {
        double hs = 0.0;
        long long us = 0;
        for (int t = 0; t < CS_NT; ++t) { hs += part[t]; us += used[t]; }
        n_used[g] = n == 0ull ? 0 : us;
        perplexity[g] = n == 0ull ? 1.0f : expf((float)(-hs));           // no tokens: exp(-0), never 0 / 0
    }
}

template <auto Kernel, class... A>
static inline int cs_launch_plain(dim3 grid, hipStream_t st, A... args)      // no dynamic LDS: nothing to opt in to
{
    hipLaunchKernelGGL(Kernel, grid, dim3(CS_NT), 0, st, args...);
    return (int)hipGetLastError();
}

static unsigned zero_grid(size_t n)
{
    size_t b = (n + CS_NT - 1) / CS_NT;
    return (unsigned)(b < 1 ? 1 : (b > 1024 ? 1024 : b));
}

// three launches: zero, sweep (not for N == 0), finalize.  Zeroed by a kernel, not a memset node (ema_update.hip).
int dvq_launch_code_stats(const long long *codes, long N, int K, long long *counts, long long *n_used, float *perplexity,
                          float *onehot, hipStream_t st)
{
    unsigned long long *cnt = (unsigned long long *)counts;
    hipLaunchKernelGGL(code_stats_zero_kernel, dim3(zero_grid((size_t)K)), dim3(CS_NT), 0, st, cnt, (size_t)K, cnt, (size_t)0);
    if (N > 0) {
        // rows per workgroup: at least 256 KiB of one-hot (or 2048 codes without one), at most ~2048 workgroups
        long rpb = onehot != nullptr ? (65536 + K - 1) / K : 2048;
        const long spread = (N + 2047) / 2048;
        if (rpb < spread) rpb = spread;
        const unsigned grid = (unsigned)((N + rpb - 1) / rpb);
        // the LDS histogram costs a workgroup 2 K / 256 LDS operations per lane (zero, flush) whatever it counts: it is taken when the
        // workgroup has at least K / 16 codes to count, else the few codes go to the global counters directly (K = 16384 with the
        // one-hot: 4 rows per workgroup)
        const bool lds = K <= CS_LDS_MAX_FLAT && rpb * 16 >= K;
        const size_t shm = lds ? (size_t)K * sizeof(unsigned) : 0;
        const int oh = onehot == nullptr ? 0 : (((K & 3) == 0 && ((uintptr_t)onehot & 15) == 0) ? 4 : 1);
        int rc;
        // (the opt-in is applied once per kernel and device: always to the family's limit, not to the first call's size)
#define CS_LAUNCH(O) (lds ? dvq_launch_lds<code_stats_kernel<true, O>, CS_LDS_MAX_FLAT * 4>(dim3(grid), dim3(CS_NT), shm, st, codes, N, K, rpb, cnt, onehot) \
                         : cs_launch_plain<code_stats_kernel<false, O>>(dim3(grid), st, codes, N, K, rpb, cnt, onehot))
        rc = oh == 4 ? CS_LAUNCH(4) : (oh == 1 ? CS_LAUNCH(1) : CS_LAUNCH(0));
#undef CS_LAUNCH
        if (rc != 0) return rc;
    }
    hipLaunchKernelGGL(code_stats_finalize_kernel, dim3(1), dim3(CS_NT), 0, st, cnt, K, (const unsigned long long *)nullptr, N,
                       n_used, perplexity);
    return (int)hipGetLastError();
}

int dvq_launch_code_stats_grain(const long long *codes, const long long *grain, int B, int H, int W, int hc, int wc, int G, int K,
                                long long *counts, long long *n_tokens, long long *n_used, float *perplexity, hipStream_t st)
{
    unsigned long long *cnt = (unsigned long long *)counts, *ntk = (unsigned long long *)n_tokens;
    const size_t GK = (size_t)G * K;
    hipLaunchKernelGGL(code_stats_zero_kernel, dim3(zero_grid(GK)), dim3(CS_NT), 0, st, cnt, GK, ntk, (size_t)G);
    const long N = (long)B * H * W;
    if (N > 0) {
        long ppb = 2048;
        const long spread = (N + 1023) / 1024;
        if (ppb < spread) ppb = spread;
        const bool lds = GK + G <= CS_LDS_MAX_GRAIN;
        if (lds && ppb < (long)(GK + G)) ppb = (long)(GK + G);          // at least as many positions as counters to zero and flush
        const unsigned grid = (unsigned)((N + ppb - 1) / ppb);
        int rc;
        if (lds)                                                         // opt-in to the family's limit, whatever this call's size
            rc = dvq_launch_lds<code_stats_grain_kernel<true>, CS_LDS_MAX_GRAIN * 4>(dim3(grid), dim3(CS_NT), (GK + G) * sizeof(unsigned), st, codes, grain, N,
                                                               H, W, hc, wc, G, K, ppb, cnt, ntk);
        else
            rc = cs_launch_plain<code_stats_grain_kernel<false>>(dim3(grid), st, codes, grain, N, H, W, hc, wc, G, K, ppb, cnt, ntk);
        if (rc != 0) return rc;
    }
    hipLaunchKernelGGL(code_stats_finalize_kernel, dim3(G), dim3(CS_NT), 0, st, cnt, K, (const unsigned long long *)ntk, 0L, n_used,
                       perplexity);
    return (int)hipGetLastError();
}
