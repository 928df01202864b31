// score_topk.hip — 1:N identification: per query the k best gallery rows by inner product, WITHOUT the N x M score matrix (gfx950).
//
// Order (svhip.h, svhip_score_topk): score descending, equal scores by the lower gallery index, NaN below every number.  All three kernels
// compare ONE composite key, (okey(score) << 32) | ~index, with okey an order-preserving map of the floats in which NaN is the smallest
// key and -0 is +0: a total order, no tie case anywhere.
//
//   score_topk_kernel   the gallery walk of score_walk.h (shared with score_above.hip: a lane is handed 16 gallery scores of ONE query per
//                       block of 32 gallery rows, in ascending index; grid: query tiles x gallery slices) with the selection as its
//                       epilogue, which is lane-local.  Every lane keeps the k best of the rows it saw in a list of (score bits, index)
//                       pairs in handle-owned scratch (L2): a score above the lane's threshold is appended; when a list cannot take
//                       another block the wave selects that list's k-th key (32-step bitwise search), compacts the list to k entries in
//                       place and raises the threshold.  A lane meets its rows in ascending index order and the compaction is stable, so
//                       "equal score, later" is always "equal score, higher index": the threshold test is on the score alone, strict,
//                       and nothing at or above a list's own k-th composite key is ever dropped.  FEW deals the slice's blocks to the
//                       four waves round robin: each wave has lists of its own, their order does not matter to the merge.
//   score_topk_merge    one workgroup per query: the k largest composite keys of all its lists, in order (k rounds of a block-wide max
//                       below the previous one).
//   score_topk_rows     the slab route's row kernel: the same k rounds over one row of a score slab.
//   score_topk_coef     svhip_score_topk_norm only: the (a, b) pairs of queries and gallery rows, once per call.  The NORM instances of
//                       score_topk_kernel and score_topk_rows select on t = fmaf(s, aq + ag, -(bq + bg)) instead of s.
#include "common.h"
#include "kernels.h"
#include "score_select.h"
#include "score_walk.h"

namespace svhip {

namespace {

// order-preserving key of a score: NaN -> 1 (below every number), numbers -> fkey + 1 (>= 0x00800000); 0 is no score at all
__device__ __forceinline__ uint32_t okey(float v) { return v != v ? 1u : fkey(v + 0.0f) + 1u; }
__device__ __forceinline__ float okey_inv(uint32_t k) { return k <= 1u ? __builtin_nanf("") : fkey_inv(k - 1u); }
__device__ __forceinline__ unsigned long long composite(float v, uint32_t idx) { return ((unsigned long long)okey(v) << 32) | (uint32_t)~idx; }

constexpr int TK_NQ = 5;            // registers per lane of a list held by a wave: cap <= 64 * TK_NQ

// The wave compacts the list of every lane in `need` to its k best entries, in place and in list order, and sets that lane's threshold
// to the list's k-th score key.  Called by the whole wave (wave-uniform control flow); a list in `need` holds more than k entries.
// (NQ: registers per lane that hold a list, 64 NQ >= its capacity.)  The lists are private to the wave, and a wave's memory operations
// go through its CU's one vector L1, which a store of that CU updates: the appends of one lane are visible to the loads of the others
// once they have completed (workgroup-scope fence: a wait, no cache maintenance; an agent-scope fence here cost several times the MFMAs)
template <int NQ>
__device__ __forceinline__ void compact_lists(unsigned long long need, uint2* lbase, int& cnt, uint32_t& thr, int k, int lane) {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    const unsigned long long lt = (1ull << lane) - 1ull;
    while (need) {
        const int src = __ffsll((long long)need) - 1;
        need &= need - 1;
        uint2* base = reinterpret_cast<uint2*>(__shfl(reinterpret_cast<unsigned long long>(lbase), src, 64));
        const int n = __shfl(cnt, src, 64);
        uint2 ent[NQ];
        uint32_t key[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int e = lane + 64 * q;
            ent[q] = make_uint2(0u, 0u);
            if (e < n) ent[q] = base[e];
            key[q] = e < n ? okey(__uint_as_float(ent[q].x)) : 0u;
        }
        uint32_t prefix = 0;
        for (int bit = 31; bit >= 0; --bit) {
            const uint32_t cand = prefix | (1u << bit);
            int c = 0;
#pragma unroll
            for (int q = 0; q < NQ; ++q) c += __popcll(__ballot(key[q] >= cand));
            if (c >= k) prefix = cand;
        }
        int cgt = 0;
#pragma unroll
        for (int q = 0; q < NQ; ++q) cgt += __popcll(__ballot(key[q] > prefix));
        const int need_eq = k - cgt;            // of the entries AT the k-th key the first need_eq stay: the lowest indices
        int outpos = 0, eqseen = 0;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const bool live = lane + 64 * q < n;
            const bool eq = live && key[q] == prefix;
            const unsigned long long meq = __ballot(eq);
            const bool keep = live && (key[q] > prefix || (eq && eqseen + __popcll(meq & lt) < need_eq));
            const unsigned long long mk = __ballot(keep);
            if (keep) base[outpos + __popcll(mk & lt)] = ent[q];       // (every slot was read above; an entry only ever moves down)
            outpos += __popcll(mk);
            eqseen += __popcll(meq);
        }
        if (lane == src) { cnt = outpos; thr = prefix; }
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
}

// The walk's epilogue (score_walk.h): a lane keeps the k best of the scores it is handed in its list.  NORM: the lists hold t in place of s.
template <int D, bool FEW, bool NORM>
__global__ __launch_bounds__(256, 2) void score_topk_kernel(ScoreTopkParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const ScoreLane g(FEW, p.N);
    const int lane = g.lane, h = g.h;
    const bool valid = g.valid;

    // this lane's list: one per (slice, [wave,] half) of its query
    const int lid = FEW ? ((int)blockIdx.y * 4 + g.wave) * 2 + h : (int)blockIdx.y * 2 + h;
    const int64_t lslot = (valid ? g.row : 0) * p.nlists + lid;
    uint2* lbase = p.lists + lslot * p.cap;
    int cnt = 0;
    uint32_t thr = 0;                               // a score is appended while its key is above thr (0: fewer than k seen, everything is)

    auto compact = [&](unsigned long long need) {
        if (p.cap <= 64) compact_lists<1>(need, lbase, cnt, thr, p.k, lane);
        else compact_lists<TK_NQ>(need, lbase, cnt, thr, p.k, lane);
    };
    auto process = [&](const f32x16& a, int b) {
        // Most blocks append nothing once the thresholds have risen: one maximum over the lane's 16 scores against the threshold as a
        // float decides that for the whole wave.  (thr <= 1: fewer than k numbers seen, NaN scores still count; the maximum skips NaN.)
        float m = a[0];
#pragma unroll
        for (int r = 1; r < 16; ++r) m = fmaxf(m, a[r]);
        if (!__ballot(valid && (thr <= 1u || m > okey_inv(thr)))) return;
        const unsigned long long full = __ballot(valid && cnt > p.cap - 16);
        if (full) compact(full);
        const int64_t kb = (int64_t)b * 32 + 4 * h;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t i = kb + (r & 3) + 8 * (r >> 2);
            const float v = a[r] + 0.0f;
            if (valid && i < p.M && okey(v) > thr) {
                lbase[cnt] = make_uint2(__float_as_uint(v), (uint32_t)i);
                ++cnt;
            }
        }
    };
    score_walk<D, FEW, NORM, false>(g, p.Q, p.N, p.G, p.M, p.per, p.qcoef, p.gcoef, smem, process);
    // what the merge reads: at most k entries per list
    const unsigned long long over = __ballot(valid && cnt > p.k);
    if (over) compact(over);
    if (valid) p.cnt[lslot] = cnt;
}

// block-wide maximum of a 64-bit key (256 threads); sm: 8 words, `parity` alternates between consecutive calls (one barrier per call)
__device__ __forceinline__ unsigned long long block_max_u64(unsigned long long v, unsigned long long* sm, int parity) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(v, off, 64);
        v = o > v ? o : v;
    }
    if ((threadIdx.x & 63) == 0) sm[parity * 4 + (threadIdx.x >> 6)] = v;
    __syncthreads();
    const unsigned long long a = sm[parity * 4], b = sm[parity * 4 + 1], c = sm[parity * 4 + 2], d = sm[parity * 4 + 3];
    const unsigned long long ab = a > b ? a : b, cd = c > d ? c : d;
    return ab > cd ? ab : cd;
}

constexpr int MERGE_PER = 8;        // composite keys a thread keeps in registers; what lies beyond is read again every round

// the k largest of a workgroup's composite keys, best first: k rounds of a block-wide maximum below the previous one.  A thread holds
// MERGE_PER keys in c (0: none); tail(prev, best) folds in the keys it does not hold (read again every round)
template <typename Tail>
__device__ __forceinline__ void emit_topk(const unsigned long long (&c)[MERGE_PER], int k, Tail tail, unsigned long long* sm,
                                          float* __restrict__ out_score, int32_t* __restrict__ out_index) {
    unsigned long long prev = ~0ull;
    for (int i = 0; i < k; ++i) {
        unsigned long long best = 0ull;
#pragma unroll
        for (int u = 0; u < MERGE_PER; ++u)
            if (c[u] < prev && c[u] > best) best = c[u];
        best = block_max_u64(tail(prev, best), sm, i & 1);
        if (threadIdx.x == 0) {
            out_score[i] = okey_inv((uint32_t)(best >> 32));
            out_index[i] = (int32_t)~(uint32_t)best;
        }
        prev = best;
    }
}

// one workgroup per query: the k largest composite keys of its nlists lists (each <= k entries, M >= k of them in all), best first
__global__ __launch_bounds__(256) void score_topk_merge_kernel(const uint2* __restrict__ lists, const int32_t* __restrict__ cnt, int nlists, int cap,
                                                               int k, float* __restrict__ out_score, int32_t* __restrict__ out_index) {
    __shared__ unsigned long long sm[8];
    const int64_t row = blockIdx.x;
    const int tid = threadIdx.x;
    const int total = nlists * k;
    const uint2* lrow = lists + row * nlists * cap;
    const int32_t* crow = cnt + row * nlists;
    auto load = [&](int t) -> unsigned long long {
        const int l = t / k, e = t - l * k;
        if (e >= crow[l]) return 0ull;
        const uint2 x = lrow[(int64_t)l * cap + e];
        return composite(__uint_as_float(x.x), x.y);
    };
    unsigned long long c[MERGE_PER];
#pragma unroll
    for (int u = 0; u < MERGE_PER; ++u) {
        const int t = tid + 256 * u;
        c[u] = t < total ? load(t) : 0ull;
    }
    emit_topk(c, k, [&](unsigned long long prev, unsigned long long best) {
        for (int t = tid + 256 * MERGE_PER; t < total; t += 256) {
            const unsigned long long x = load(t);
            if (x < prev && x > best) best = x;
        }
        return best;
    }, sm, out_score + row * k, out_index + row * k);
}

// The slab route: one workgroup per row of a score slab.  Pass 1: every thread's largest key over its strided share of the row; the k-th
// largest of those 256 maxima, T, is a lower bound of the row's k-th key (k <= min(M, 256) shares are not empty, and k keys are >= T).
// Pass 2 (the row comes from L2): the keys >= T go to an LDS list — about 2 k of them on scores without structure — and the k rounds run
// over that list in registers.  A row that fills the list (its large scores share a few threads' strides) takes the k rounds over the row.
// NORM: every read of s[t] goes through the statement's fmaf with the row's (aq, bq) and the gallery's pair of column t, so all passes
// see the identical value.
constexpr int ROWS_CAND = 256 * MERGE_PER;
template <bool NORM>
__global__ __launch_bounds__(256) void score_topk_rows_kernel(const float* __restrict__ S, int64_t M, int64_t ld, int k, float* __restrict__ out_score,
                                                              int32_t* __restrict__ out_index, const float2* __restrict__ qcoef,
                                                              const float2* __restrict__ gcoef) {
    __shared__ unsigned long long sm[8];
    __shared__ unsigned long long cand[ROWS_CAND];
    __shared__ int ncand;
    const int64_t row = blockIdx.x;
    const int tid = threadIdx.x;
    const float* __restrict__ sraw = S + row * ld;
    float aq = 0.0f, bq = 0.0f;
    if (NORM) {
        const float2 c = qcoef[row];
        aq = c.x; bq = c.y;
    }
    struct Row {
        const float* __restrict__ s;
        const float2* __restrict__ g;
        float aq, bq;
        __device__ __forceinline__ float operator[](int64_t t) const {
            if (!NORM) return s[t];
            const float2 c = g[t];
            return __builtin_fmaf(s[t], aq + c.x, -(bq + c.y));
        }
    };
    const Row s{sraw, gcoef, aq, bq};
    unsigned long long mx = 0ull;
    for (int64_t t = tid; t < M; t += 256) {
        const unsigned long long x = composite(s[t], (uint32_t)t);
        mx = x > mx ? x : mx;
    }
    unsigned long long T = ~0ull;
    for (int i = 0; i < k; ++i) T = block_max_u64(mx < T ? mx : 0ull, sm, i & 1);
    if (tid == 0) ncand = 0;
    __syncthreads();
    for (int64_t t = tid; t < M; t += 256) {
        const unsigned long long x = composite(s[t], (uint32_t)t);
        if (x >= T) {
            const int pos = atomicAdd(&ncand, 1);
            if (pos < ROWS_CAND) cand[pos] = x;
        }
    }
    __syncthreads();
    const int n = ncand;
    unsigned long long c[MERGE_PER];
    if (n <= ROWS_CAND) {                       // (workgroup-uniform)
#pragma unroll
        for (int u = 0; u < MERGE_PER; ++u) c[u] = tid + 256 * u < n ? cand[tid + 256 * u] : 0ull;
        emit_topk(c, k, [](unsigned long long, unsigned long long best) { return best; }, sm, out_score + row * k, out_index + row * k);
        return;
    }
#pragma unroll
    for (int u = 0; u < MERGE_PER; ++u) {
        const int64_t t = tid + 256 * u;
        c[u] = t < M ? composite(s[t], (uint32_t)t) : 0ull;
    }
    emit_topk(c, k, [&](unsigned long long prev, unsigned long long best) {
        for (int64_t t = tid + 256 * MERGE_PER; t < M; t += 256) {
            const unsigned long long x = composite(s[t], (uint32_t)t);
            if (x < prev && x > best) best = x;
        }
        return best;
    }, sm, out_score + row * k, out_index + row * k);
}

// the coefficients of the statement, one IEEE operation each: a = 0.5f / sigma, b = mu * a, as interleaved pairs per query and per
// gallery row; the gallery's table runs to Mpad = whole blocks of 32 rows, the entries past M repeat row M - 1
__global__ __launch_bounds__(256) void score_topk_coef_kernel(const float* __restrict__ q_mu, const float* __restrict__ q_sigma, int64_t N,
                                                              const float* __restrict__ g_mu, const float* __restrict__ g_sigma, int64_t M,
                                                              int64_t Mpad, float2* __restrict__ qcoef, float2* __restrict__ gcoef) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N + Mpad) return;
    const bool isq = i < N;
    const int64_t src = isq ? i : min(i - N, M - 1);
    const float mu = isq ? q_mu[src] : g_mu[src], sigma = isq ? q_sigma[src] : g_sigma[src];
    const float a = 0.5f / sigma;
    const float b = mu * a;
    (isq ? qcoef + i : gcoef + (i - N))[0] = make_float2(a, b);
}

template <int D, bool FEW, bool NORM>
hipError_t launch_topk_d(const ScoreTopkParams& p, const dim3& grid, hipStream_t stream) {
    static DeviceOnce attr;
    constexpr int lds = score_walk_lds_bytes(D, FEW, NORM);
    if (!FEW)
        if (hipError_t e = set_max_dynamic_lds(attr, reinterpret_cast<const void*>(score_topk_kernel<D, FEW, NORM>), lds)) return e;
    hipLaunchKernelGGL((score_topk_kernel<D, FEW, NORM>), grid, dim3(256), lds, stream, p);
    return hipGetLastError();
}

template <int D, bool NORM>
hipError_t launch_topk_form(const ScoreTopkParams& p, bool few, const dim3& grid, hipStream_t stream) {
    return few ? launch_topk_d<D, true, NORM>(p, grid, stream) : launch_topk_d<D, false, NORM>(p, grid, stream);
}

}  // namespace

int64_t score_topk_coef_rows(int64_t M) { return (M + 31) / 32 * 32; }

hipError_t launch_score_topk_coef(const float* q_mu, const float* q_sigma, int64_t N, const float* g_mu, const float* g_sigma, int64_t M,
                                  float2* qcoef, float2* gcoef, hipStream_t stream) {
    if (N <= 0) return hipSuccess;
    if (!q_mu || !q_sigma || !g_mu || !g_sigma || !qcoef || !gcoef || M < 1 || M >= ((int64_t)1 << 31)) return hipErrorInvalidValue;
    const int64_t Mpad = score_topk_coef_rows(M);
    const int64_t blocks = (N + Mpad + 255) / 256;
    if (blocks >= ((int64_t)1 << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(score_topk_coef_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, q_mu, q_sigma, N, g_mu, g_sigma, M, Mpad, qcoef, gcoef);
    return hipGetLastError();
}

bool score_topk_fused_supported(int D) { return D == 192 || D == 256; }

// slots per list: a list must take one more block (16 scores per lane) whenever it holds no more than cap - 16, and a compaction leaves k
int score_topk_cap(int k) { return (2 * k + 32 + 63) / 64 * 64; }

hipError_t launch_score_topk(const ScoreTopkParams& p, int D, bool few, int slices, hipStream_t stream) {
    if (p.N <= 0) return hipSuccess;
    if (!p.lists || !p.cnt) return hipErrorInvalidValue;
    if (p.k < 1 || p.k > SCORE_TOPK_MAX_K || p.k > p.M) return hipErrorInvalidValue;
    if (p.cap != score_topk_cap(p.k) || p.cap > 64 * TK_NQ || p.cap < p.k + 17) return hipErrorInvalidValue;
    if (p.nlists != slices * (few ? 8 : 2)) return hipErrorInvalidValue;
    dim3 grid;
    if (hipError_t e = score_walk_launch(D, p.Q, p.N, p.G, p.M, p.per, p.qcoef, p.gcoef, few, slices, &grid)) return e;
    if (p.qcoef) return D == 192 ? launch_topk_form<192, true>(p, few, grid, stream) : launch_topk_form<256, true>(p, few, grid, stream);
    return D == 192 ? launch_topk_form<192, false>(p, few, grid, stream) : launch_topk_form<256, false>(p, few, grid, stream);
}

hipError_t launch_score_topk_merge(const uint2* lists, const int32_t* cnt, int64_t rows, int nlists, int cap, int k, float* out_score,
                                   int32_t* out_index, hipStream_t stream) {
    if (rows <= 0) return hipSuccess;
    if (!lists || !cnt || !out_score || !out_index || nlists < 1 || k < 1 || k > cap || (int64_t)nlists * k >= ((int64_t)1 << 31) ||
        rows >= ((int64_t)1 << 31))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(score_topk_merge_kernel, dim3((unsigned)rows), dim3(256), 0, stream, lists, cnt, nlists, cap, k, out_score, out_index);
    return hipGetLastError();
}

hipError_t launch_score_topk_rows(const float* S, int64_t rows, int64_t M, int64_t ld, int k, float* out_score, int32_t* out_index, hipStream_t stream,
                                  const float2* qcoef, const float2* gcoef) {
    if (rows <= 0) return hipSuccess;
    if (!S || !out_score || !out_index || k < 1 || k > M || M >= ((int64_t)1 << 31) || ld < M || rows >= ((int64_t)1 << 31)) return hipErrorInvalidValue;
    if (!qcoef != !gcoef) return hipErrorInvalidValue;
    if (qcoef)
        hipLaunchKernelGGL(score_topk_rows_kernel<true>, dim3((unsigned)rows), dim3(256), 0, stream, S, M, ld, k, out_score, out_index, qcoef, gcoef);
    else
        hipLaunchKernelGGL(score_topk_rows_kernel<false>, dim3((unsigned)rows), dim3(256), 0, stream, S, M, ld, k, out_score, out_index, qcoef, gcoef);
    return hipGetLastError();
}

}  // namespace svhip
