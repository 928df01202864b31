// score_cluster.hip — speaker clustering: the connected components of the graph "rows i < j are linked iff v(i, j) >= thr" over ONE set of
// rows, WITHOUT an edge list and without the N x N score matrix (gfx950; svhip.h, svhip_cluster_above).
//
//   cluster_init        parent[i] = i
//   cluster_seed        the joint forest of a two-set call (svhip_cluster_join): parent[i] = the seed of row i where a side brings a known
//                       grouping, i otherwise
//   cluster_link        the gallery walk of score_walk.h (Q = G = E, the masks of score_above_kernel in UPPER mode, so v has the bits
//                       score_above gives the pair) with a third epilogue: every surviving pair is unioned at once in a lock-free
//                       disjoint-set forest that lives in the out_root buffer itself.  One MFMA pass over the upper half plane: a
//                       workgroup whose gallery slice ends at or below its first query row returns before the walk (no pair j > i lies
//                       there; workgroup-uniform, and no score's bits change).
//   cluster_link_rows   the slab route: one workgroup per row of a score slab, four columns per thread, the columns above the row's own index
//   cluster_join_link / cluster_join_rows   the same two bodies for svhip_cluster_join, with an index offset for the query side and one for
//                       the gallery side of a link: CLUSTER_LINK_SIDE keeps the upper mask and the diagonal skip (the self-join of one
//                       side of the joint numbering), CLUSTER_LINK_CROSS has no mask (the rectangle A x B).  They are instantiations of
//                       their own: cluster_above's kernels keep their parameters and their instruction stream.
//   cluster_flatten     root[i] = the representative of i, in place, behind the kernel boundary
//   cluster_count / _scan / _rank / _assign   dense ids: the roots are flagged (root[i] == i), counted per block of 1024 rows, ONE block
//                       scans the block counts, the roots take their rank, every other row takes its root's: clusters are numbered in
//                       order of their smallest member.  Integers only: the ids depend on root[] alone.
//
// The forest (the ECL-CC / Jayanti-Tarjan scheme).  parent[x] <= x always; x is a ROOT while parent[x] == x.  To link (u, v): climb from both
// to nodes that look like roots; if they are one node, done; otherwise hook the LARGER under the smaller with
// atomicCAS(&parent[hi], hi, lo).  The CAS succeeds only while hi really is a root; when it fails it returns the value that was there,
// which is strictly smaller than hi, and the link goes on from it: every step moves to a smaller index, so the loop ends without waiting
// for any other wave.  While climbing, a node's parent may be lowered to its grandparent (atomicMin): the only other write there is.
//   Invariant.  Rows form SETS (the unions made so far).  A set has exactly one root, which is its smallest member (a hook puts the root
//   of one set under a member lo < hi of the other, whose root is <= lo: the smaller of the two minima stays root), and every value ever
//   stored in parent[x] is a member of x's set that is <= x (a hook stores a member of the merged set; atomicMin stores what was read as
//   the parent of the parent: sets only ever grow).
//   Staleness.  Per-XCD L2s and per-CU L1s are not coherent, so inside cluster_link every access to parent[] is an agent-scope atomic:
//   atomicCAS to hook, __hip_atomic_load(relaxed, agent) to climb, atomicMin to shorten; there is no plain store to it.  Even so a load
//   may return an OLDER value of parent[x].  That is harmless by construction: an older value is x itself or a member of x's set below x
//   (the invariant), so a climb through stale values still ends at a member of the start's set, and a node that only LOOKS like a root
//   is caught by the CAS, which is the arbiter: it compares with the value memory holds.  Two climbs that meet in one node started in one
//   set, whatever they read on the way.  When the kernel has ended every link (u, v) has either met or hooked, so u and v are in one set;
//   no two rows without a chain of links ever are.  The root of every set is then the smallest index of its component, whatever order the
//   hardware met the links in: the result is a function of the data only.
// No spin-waits, no cross-lane operation inside the divergent link loop, no inline assembly: plain C++ and HIP atomics.
#include "block_scan.h"
#include "common.h"
#include "kernels.h"
#include "score_walk.h"

namespace svhip {

namespace {

__device__ __forceinline__ int32_t forest_load(const int32_t* parent, int32_t x) {
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// a node above x that looks like a root; on the way a node's parent is lowered to its grandparent
__device__ __forceinline__ int32_t forest_climb(int32_t* parent, int32_t x) {
    int32_t p = forest_load(parent, x);
    while (p != x) {
        const int32_t g = forest_load(parent, p);
        if (g != p) atomicMin(parent + x, g);       // (x is no root: its parent only ever moves down inside its set)
        x = p;
        p = g;
    }
    return x;
}

__device__ __forceinline__ void forest_link(int32_t* parent, int32_t u, int32_t v) {
    for (;;) {
        u = forest_climb(parent, u);
        v = forest_climb(parent, v);
        if (u == v) return;
        const int32_t hi = u > v ? u : v, lo = u > v ? v : u;
        const int32_t was = atomicCAS(parent + hi, hi, lo);
        if (was == hi) return;
        u = was;                                    // hi was hooked meanwhile: go on below it (was < hi)
        v = lo;
    }
}

// The link epilogue over the walk.  FORM (kernels.h): CLUSTER_LINK_SET is cluster_above's launch (q_off and g_off are not read);
// CLUSTER_LINK_SIDE the same masks with both ends of a link moved by the side's offset; CLUSTER_LINK_CROSS every pair of the rectangle.
template <int D, bool FEW, bool NORM, int FORM>
__device__ __forceinline__ void cluster_link_body(const ClusterLinkParams& p, int64_t q_off, int64_t g_off, char* smem) {
    // the diagonal skip: the slice's last gallery row lies at or below the workgroup's first query row (workgroup-uniform)
    const int64_t tile_first_row = FEW ? 0 : (int64_t)blockIdx.x * 128;
    if (FORM != CLUSTER_LINK_CROSS && ((int64_t)blockIdx.y + 1) * p.per * 32 <= p.row_base + tile_first_row) return;
    const ScoreLane g(FEW, p.N);
    const int h = g.h;
    // a link's gallery index lies in [lo, M): score_above_kernel's UPPER mask (CROSS: the whole gallery)
    const int64_t first = FORM == CLUSTER_LINK_CROSS ? 0 : p.row_base + g.row + 1;
    const uint32_t lo = g.valid && first < (int64_t)0xffffffffu ? (uint32_t)first : 0xffffffffu, hi = (uint32_t)p.M;
    const int32_t me = (int32_t)((FORM == CLUSTER_LINK_SET ? 0 : q_off) + p.row_base + (g.valid ? g.row : 0));
    const int32_t g0 = FORM == CLUSTER_LINK_SET ? 0 : (int32_t)g_off;

    auto process = [&](const f32x16& a, int b) {
        const uint32_t kb = (uint32_t)b * 32u + 4u * h;
        uint32_t hits = 0;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const uint32_t i = kb + (r & 3) + 8 * (r >> 2);
            if (i >= lo && i < hi && a[r] >= p.thr) hits |= 1u << r;                    // (a NaN score links nothing)
        }
        while (hits) {                                                                  // (divergent: most lanes hold no hit)
            const int r = __ffs(hits) - 1;
            hits &= hits - 1;
            forest_link(p.parent, me, g0 + (int32_t)(kb + (r & 3) + 8 * (r >> 2)));
        }
    };
    score_walk<D, FEW, NORM, true>(g, p.Q, p.N, p.G, p.M, p.per, p.qcoef, p.gcoef, smem, process);
}

template <int D, bool FEW, bool NORM>
__global__ __launch_bounds__(256, 2) void cluster_link_kernel(ClusterLinkParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    cluster_link_body<D, FEW, NORM, CLUSTER_LINK_SET>(p, 0, 0, smem);
}

// svhip_cluster_join: a link is (q_off + the query's row, g_off + the gallery row); every index lies below the forest's size (the launcher)
template <int D, bool FEW, bool NORM, int FORM>
__global__ __launch_bounds__(256, 2) void cluster_join_link_kernel(ClusterLinkParams p, int64_t q_off, int64_t g_off) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    cluster_link_body<D, FEW, NORM, FORM>(p, q_off, g_off, smem);
}

// The slab route: one workgroup per row of a score slab, four consecutive columns per thread and round (score_above_rows_kernel's reads),
// from the round that holds the first column above the row's own index (CROSS: from column 0, every column).
template <bool NORM, int FORM>
__device__ __forceinline__ void cluster_link_rows_body(const float* __restrict__ S, int64_t M, int64_t ld, float thr, int64_t row_base,
                                                       const float2* __restrict__ qcoef, const float2* __restrict__ gcoef, int32_t* parent,
                                                       int64_t q_off, int64_t g_off) {
    const int64_t row = blockIdx.x;
    const int tid = threadIdx.x;
    const float* __restrict__ s = S + row * ld;
    float aq = 0.0f, bq = 0.0f;
    if (NORM) {
        const float2 c = qcoef[row];
        aq = c.x; bq = c.y;
    }
    const int64_t above = row_base + row;
    const int32_t me = (int32_t)((FORM == CLUSTER_LINK_SET ? 0 : q_off) + above);
    const int64_t g0 = FORM == CLUSTER_LINK_SET ? 0 : g_off;
    for (int64_t c0 = FORM == CLUSTER_LINK_CROSS ? 0 : (above + 1) & ~(int64_t)1023; c0 < M; c0 += 1024) {
        const int64_t t0 = c0 + 4 * tid;
        if (t0 >= M) continue;                                         // (ld % 4 == 0: the four columns lie inside the row's stride)
        const f32x4 x = *reinterpret_cast<const f32x4*>(s + t0);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            float v = x[u];
            if (NORM && t0 + u < M) {
                const float2 g = gcoef[t0 + u];
                v = __builtin_fmaf(x[u], aq + g.x, -(bq + g.y));
            }
            if (t0 + u < M && (FORM == CLUSTER_LINK_CROSS || t0 + u > above) && v >= thr) forest_link(parent, me, (int32_t)(g0 + t0 + u));
        }
    }
}

template <bool NORM>
__global__ __launch_bounds__(256) void cluster_link_rows_kernel(const float* __restrict__ S, int64_t M, int64_t ld, float thr, int64_t row_base,
                                                                const float2* __restrict__ qcoef, const float2* __restrict__ gcoef, int32_t* parent) {
    cluster_link_rows_body<NORM, CLUSTER_LINK_SET>(S, M, ld, thr, row_base, qcoef, gcoef, parent, 0, 0);
}

template <bool NORM, int FORM>
__global__ __launch_bounds__(256) void cluster_join_rows_kernel(const float* __restrict__ S, int64_t M, int64_t ld, float thr, int64_t row_base,
                                                                const float2* __restrict__ qcoef, const float2* __restrict__ gcoef, int32_t* parent,
                                                                int64_t q_off, int64_t g_off) {
    cluster_link_rows_body<NORM, FORM>(S, M, ld, thr, row_base, qcoef, gcoef, parent, q_off, g_off);
}

__global__ __launch_bounds__(256) void cluster_init_kernel(int32_t* __restrict__ parent, int64_t N) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < N) parent[i] = (int32_t)i;
}

// The joint forest of svhip_cluster_join: rows 0 .. NA - 1 are A's, NA .. NA + NB - 1 are B's; a side's seed (NULL: none) is in the side's own
// numbering.  Plain stores: a kernel boundary lies before the first link launch, and nothing else runs on the buffer meanwhile.
//   Termination.  forest_climb and cluster_flatten walk x -> parent[x] and end only because parent[x] <= x holds for EVERY x, with equality
//   exactly at the roots: every step strictly lowers a non-negative index.  cluster_init gives parent[x] = x; hooks and shortenings store
//   members below x (the invariant above).  A seed is foreign data, so it goes through cluster_seed_parent (kernels.h), which returns a value
//   in [0, i] for every input: an entry above i, or a negative one, is read as i (the row starts alone) and can neither point upwards - a
//   cycle, hence a hang - nor outside the buffer.  A's values lie in [0, i], B's in [NA, NA + j]: parent[x] <= x for both, so the forest
//   the link kernels meet is as well-founded as cluster_init's, and it encodes exactly the seed links (i, root[i]).
__global__ __launch_bounds__(256) void cluster_seed_kernel(const int32_t* __restrict__ root_a, int64_t NA, const int32_t* __restrict__ root_b,
                                                           int64_t NB, int32_t* __restrict__ parent) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= NA + NB) return;
    if (i < NA) {
        parent[i] = root_a ? cluster_seed_parent(root_a[i], i) : (int32_t)i;
    } else {
        const int64_t j = i - NA;
        parent[i] = (int32_t)(NA + (root_b ? cluster_seed_parent(root_b[j], j) : (int32_t)j));
    }
}

// In place: a row climbs to its root and stores it.  Rows are rewritten while others still climb through them: what a climb reads is an
// older or a newer ancestor, and a root is never rewritten to anything but itself - the accesses stay agent-scope atomics all the same.
__global__ __launch_bounds__(256) void cluster_flatten_kernel(int32_t* root, int64_t N) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    int32_t x = (int32_t)i, p = forest_load(root, x);
    if (p == x) return;
    while (p != x) {
        x = p;
        p = forest_load(root, x);
    }
    __hip_atomic_store(root + i, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- dense ids: blocks of 1024 rows, four consecutive rows per thread ------------------------------------------------------------------
constexpr int CLUSTER_BLOCK = 1024;

// the roots among the thread's four rows, as a mask
__device__ __forceinline__ uint32_t root_flags(const int32_t* __restrict__ root, int64_t N, int64_t i0) {
    uint32_t f = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u)
        if (i0 + u < N && root[i0 + u] == (int32_t)(i0 + u)) f |= 1u << u;
    return f;
}

// (block_exclusive, the workgroup scan of the kernels below: block_scan.h)

__global__ __launch_bounds__(256) void cluster_count_kernel(const int32_t* __restrict__ root, int64_t N, int32_t* __restrict__ bcnt) {
    __shared__ int ws[4];
    int all;
    block_exclusive(__popc(root_flags(root, N, (int64_t)blockIdx.x * CLUSTER_BLOCK + 4 * threadIdx.x)), ws, &all);
    if (threadIdx.x == 0) bcnt[blockIdx.x] = all;
}

// ONE workgroup: bcnt[b] <- the roots of the blocks before b, 256 blocks a round; *out_n = the number of roots
__global__ __launch_bounds__(256) void cluster_scan_kernel(int32_t* __restrict__ bcnt, int64_t nb, int64_t* __restrict__ out_n) {
    __shared__ int ws[4];
    int64_t carry = 0;
    for (int64_t b0 = 0; b0 < nb; b0 += 256) {
        const int64_t b = b0 + threadIdx.x;
        const int n = b < nb ? bcnt[b] : 0;
        int all;
        const int before = block_exclusive(n, ws, &all);
        if (b < nb) bcnt[b] = (int32_t)(carry + before);               // (fewer than 2^31 rows: fewer roots)
        carry += all;
    }
    if (threadIdx.x == 0) *out_n = carry;
}

// a root's id: the roots before it
__global__ __launch_bounds__(256) void cluster_rank_kernel(const int32_t* __restrict__ root, int64_t N, const int32_t* __restrict__ boff,
                                                           int32_t* __restrict__ cluster) {
    __shared__ int ws[4];
    const int64_t i0 = (int64_t)blockIdx.x * CLUSTER_BLOCK + 4 * threadIdx.x;
    const uint32_t f = root_flags(root, N, i0);
    int all;
    int rank = boff[blockIdx.x] + block_exclusive(__popc(f), ws, &all);
#pragma unroll
    for (int u = 0; u < 4; ++u)
        if ((f >> u) & 1u) cluster[i0 + u] = rank++;
}

// every other row: its root's id (the roots' entries were written by the launch before and are not written here)
__global__ __launch_bounds__(256) void cluster_assign_kernel(const int32_t* __restrict__ root, int64_t N, int32_t* cluster) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int32_t r = root[i];
    if (r != (int32_t)i) cluster[i] = cluster[r];
}

template <int D, bool FEW, bool NORM>
hipError_t launch_link_d(const ClusterLinkParams& p, const dim3& grid, hipStream_t stream) {
    static DeviceOnce attr;
    constexpr int lds = score_walk_lds_bytes(D, FEW, NORM);
    if (!FEW)
        if (hipError_t e = set_max_dynamic_lds(attr, reinterpret_cast<const void*>(cluster_link_kernel<D, FEW, NORM>), lds)) return e;
    hipLaunchKernelGGL((cluster_link_kernel<D, FEW, NORM>), grid, dim3(256), lds, stream, p);
    return hipGetLastError();
}

template <int D>
hipError_t launch_link_form(const ClusterLinkParams& p, bool few, const dim3& grid, hipStream_t stream) {
    if (p.qcoef) return few ? launch_link_d<D, true, true>(p, grid, stream) : launch_link_d<D, false, true>(p, grid, stream);
    return few ? launch_link_d<D, true, false>(p, grid, stream) : launch_link_d<D, false, false>(p, grid, stream);
}

template <int D, bool FEW, bool NORM, int FORM>
hipError_t launch_join_link_d(const ClusterLinkParams& p, int64_t q_off, int64_t g_off, const dim3& grid, hipStream_t stream) {
    static DeviceOnce attr;
    constexpr int lds = score_walk_lds_bytes(D, FEW, NORM);
    if (!FEW)
        if (hipError_t e = set_max_dynamic_lds(attr, reinterpret_cast<const void*>(cluster_join_link_kernel<D, FEW, NORM, FORM>), lds)) return e;
    hipLaunchKernelGGL((cluster_join_link_kernel<D, FEW, NORM, FORM>), grid, dim3(256), lds, stream, p, q_off, g_off);
    return hipGetLastError();
}

template <int D, int FORM>
hipError_t launch_join_link_form(const ClusterLinkParams& p, int64_t q_off, int64_t g_off, bool few, const dim3& grid, hipStream_t stream) {
    if (p.qcoef)
        return few ? launch_join_link_d<D, true, true, FORM>(p, q_off, g_off, grid, stream) : launch_join_link_d<D, false, true, FORM>(p, q_off, g_off, grid, stream);
    return few ? launch_join_link_d<D, true, false, FORM>(p, q_off, g_off, grid, stream) : launch_join_link_d<D, false, false, FORM>(p, q_off, g_off, grid, stream);
}

// what both join launchers ask of the offsets: every index a link touches lies in [0, forest)
inline bool join_offsets_ok(int form, int64_t row_base, int64_t rows, int64_t M, int64_t q_off, int64_t g_off, int64_t forest) {
    if (form != CLUSTER_LINK_SIDE && form != CLUSTER_LINK_CROSS) return false;
    if (row_base < 0 || q_off < 0 || g_off < 0 || forest < 1 || forest >= ((int64_t)1 << 31)) return false;
    if (q_off + row_base + rows > forest || g_off + M > forest) return false;
    // a side's self-join: its queries are rows of its own gallery, and both ends move by the one offset
    if (form == CLUSTER_LINK_SIDE && (q_off != g_off || row_base + rows > M)) return false;
    return true;
}

inline unsigned blocks_of(int64_t N, int per) { return (unsigned)((N + per - 1) / per); }

}  // namespace

hipError_t launch_cluster_init(int32_t* parent, int64_t N, hipStream_t stream) {
    if (N <= 0) return hipSuccess;
    if (!parent || N >= ((int64_t)1 << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(cluster_init_kernel, dim3(blocks_of(N, 256)), dim3(256), 0, stream, parent, N);
    return hipGetLastError();
}

hipError_t launch_cluster_seed(const int32_t* root_a, int64_t NA, const int32_t* root_b, int64_t NB, int32_t* parent, hipStream_t stream) {
    if (NA < 0 || NB < 0) return hipErrorInvalidValue;
    if (NA + NB == 0) return hipSuccess;
    if (!parent || NA + NB >= ((int64_t)1 << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(cluster_seed_kernel, dim3(blocks_of(NA + NB, 256)), dim3(256), 0, stream, root_a, NA, root_b, NB, parent);
    return hipGetLastError();
}

hipError_t launch_cluster_join_link(const ClusterLinkParams& p, int D, bool few, int slices, int form, int64_t q_off, int64_t g_off, int64_t forest,
                                    hipStream_t stream) {
    if (p.N <= 0) return hipSuccess;
    if (!p.parent || p.thr != p.thr || !join_offsets_ok(form, p.row_base, p.N, p.M, q_off, g_off, forest)) return hipErrorInvalidValue;
    dim3 grid;
    if (hipError_t e = score_walk_launch(D, p.Q, p.N, p.G, p.M, p.per, p.qcoef, p.gcoef, few, slices, &grid)) return e;
    if (form == CLUSTER_LINK_SIDE)
        return D == 192 ? launch_join_link_form<192, CLUSTER_LINK_SIDE>(p, q_off, g_off, few, grid, stream)
                        : launch_join_link_form<256, CLUSTER_LINK_SIDE>(p, q_off, g_off, few, grid, stream);
    return D == 192 ? launch_join_link_form<192, CLUSTER_LINK_CROSS>(p, q_off, g_off, few, grid, stream)
                    : launch_join_link_form<256, CLUSTER_LINK_CROSS>(p, q_off, g_off, few, grid, stream);
}

hipError_t launch_cluster_join_rows(const float* S, int64_t rows, int64_t M, int64_t ld, float thr, int64_t row_base, const float2* qcoef,
                                    const float2* gcoef, int32_t* parent, int form, int64_t q_off, int64_t g_off, int64_t forest, hipStream_t stream) {
    if (rows <= 0) return hipSuccess;
    if (!S || !parent || thr != thr || M < 1 || M >= ((int64_t)1 << 31) || ld < M || (ld & 3) || (reinterpret_cast<uintptr_t>(S) & 15) ||
        !join_offsets_ok(form, row_base, rows, M, q_off, g_off, forest))
        return hipErrorInvalidValue;
    if (!qcoef != !gcoef) return hipErrorInvalidValue;
    const dim3 grid((unsigned)rows), block(256);
#define SVHIP_JOIN_ROWS(NORM, FORM) \
    hipLaunchKernelGGL((cluster_join_rows_kernel<NORM, FORM>), grid, block, 0, stream, S, M, ld, thr, row_base, qcoef, gcoef, parent, q_off, g_off)
    if (form == CLUSTER_LINK_SIDE) { if (qcoef) SVHIP_JOIN_ROWS(true, CLUSTER_LINK_SIDE); else SVHIP_JOIN_ROWS(false, CLUSTER_LINK_SIDE); }
    else { if (qcoef) SVHIP_JOIN_ROWS(true, CLUSTER_LINK_CROSS); else SVHIP_JOIN_ROWS(false, CLUSTER_LINK_CROSS); }
#undef SVHIP_JOIN_ROWS
    return hipGetLastError();
}

hipError_t launch_cluster_link(const ClusterLinkParams& p, int D, bool few, int slices, hipStream_t stream) {
    if (p.N <= 0) return hipSuccess;
    // every index a link touches lies in [0, M): the queries of the launch are the rows row_base .. row_base + N - 1 of the gallery
    if (!p.parent || p.thr != p.thr || p.row_base < 0 || p.row_base + p.N > p.M) return hipErrorInvalidValue;
    dim3 grid;
    if (hipError_t e = score_walk_launch(D, p.Q, p.N, p.G, p.M, p.per, p.qcoef, p.gcoef, few, slices, &grid)) return e;
    return D == 192 ? launch_link_form<192>(p, few, grid, stream) : launch_link_form<256>(p, few, grid, stream);
}

hipError_t launch_cluster_link_rows(const float* S, int64_t rows, int64_t M, int64_t ld, float thr, int64_t row_base, const float2* qcoef,
                                    const float2* gcoef, int32_t* parent, hipStream_t stream) {
    if (rows <= 0) return hipSuccess;
    if (!S || !parent || thr != thr || M < 1 || M >= ((int64_t)1 << 31) || ld < M || (ld & 3) || (reinterpret_cast<uintptr_t>(S) & 15) ||
        row_base < 0 || row_base + rows > M)
        return hipErrorInvalidValue;
    if (!qcoef != !gcoef) return hipErrorInvalidValue;
    if (qcoef) hipLaunchKernelGGL(cluster_link_rows_kernel<true>, dim3((unsigned)rows), dim3(256), 0, stream, S, M, ld, thr, row_base, qcoef, gcoef, parent);
    else hipLaunchKernelGGL(cluster_link_rows_kernel<false>, dim3((unsigned)rows), dim3(256), 0, stream, S, M, ld, thr, row_base, qcoef, gcoef, parent);
    return hipGetLastError();
}

hipError_t launch_cluster_flatten(int32_t* root, int64_t N, hipStream_t stream) {
    if (N <= 0) return hipSuccess;
    if (!root || N >= ((int64_t)1 << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(cluster_flatten_kernel, dim3(blocks_of(N, 256)), dim3(256), 0, stream, root, N);
    return hipGetLastError();
}

int64_t cluster_id_blocks(int64_t N) { return (N + CLUSTER_BLOCK - 1) / CLUSTER_BLOCK; }

hipError_t launch_cluster_ids(const int32_t* root, int64_t N, int32_t* bcnt, int32_t* cluster, int64_t* out_n, hipStream_t stream) {
    if (N <= 0) return hipSuccess;
    if (!root || !bcnt || !out_n || N >= ((int64_t)1 << 31)) return hipErrorInvalidValue;
    const int64_t nb = cluster_id_blocks(N);
    hipLaunchKernelGGL(cluster_count_kernel, dim3((unsigned)nb), dim3(256), 0, stream, root, N, bcnt);
    hipLaunchKernelGGL(cluster_scan_kernel, dim3(1), dim3(256), 0, stream, bcnt, nb, out_n);
    if (cluster) {
        hipLaunchKernelGGL(cluster_rank_kernel, dim3((unsigned)nb), dim3(256), 0, stream, root, N, bcnt, cluster);
        hipLaunchKernelGGL(cluster_assign_kernel, dim3(blocks_of(N, 256)), dim3(256), 0, stream, root, N, cluster);
    }
    return hipGetLastError();
}

}  // namespace svhip
