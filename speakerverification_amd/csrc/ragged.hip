// ragged.hip — the two kernels that only a ragged batch has (gfx950): the row -> utterance table and the SE gate over packed rows.
//
// n utterances of T_u frames are packed back to back into the frame-major workspace: row0[u] is the first row of utterance u,
// row0[n] the row count M, utt[m] the utterance of row m (rag_rows_kernel fills it from row0).  The reductions over time — the
// front-end's log-mel mean and instance norm, the SE squeeze, the ASP statistics, softmax and pooling — are not here: they are the
// RAG instances of the fixed-length kernels (colstats_kernel, asp_pool_kernel in elementwise.hip) and the packed entries around the
// prologue's shared bodies (prologue_stats_row, prologue_apply_tile in fbank.hip),
// one workgroup per (utterance, channel block) that walks the utterance's own frames, and the small linear layers are
// rowvec_linear_small_kernel.  The two forms share one body, so the order of every sum is fixed by the frame index alone, never by the
// tile or row-group boundaries of the packed matrix, an utterance's values do not depend on what it is packed with or where, and the
// fixed-length kernels' error bars carry over.  Nothing holds an utterance's time axis in LDS: a 60 s file (12 001 frames) is just a
// longer loop.  All HBM-bound: 16-byte accesses along the channel axis.
#include "common.h"
#include "kernels.h"

namespace svhip {

namespace {

// utt[m] = u for the rows of utterance u: grid (ceil(maxT / 256), n)
__global__ __launch_bounds__(256) void rag_rows_kernel(const int* __restrict__ row0, int* __restrict__ utt) {
    const int u = blockIdx.y;
    const int r0 = row0[u], Tn = row0[u + 1] - r0;
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < Tn) utt[r0 + t] = u;
}

// SE gate + residual over the packed rows, the gate looked up per row.  grid ceil(M / RAG_SE_ROWS), block 256: a thread keeps one
// 16-byte column chunk and walks the block's rows four at a time; the gate row is re-read only where the utterance changes.
// (Not an instance of se_apply_kernel, which gives a workgroup the rows of ONE utterance and writes the S32 side output.)
constexpr int RAG_SE_ROWS = 32;
template <typename T>
__global__ __launch_bounds__(256) void rag_se_apply_kernel(const T* __restrict__ h, int ldh, const float* __restrict__ s, const T* __restrict__ x,
                                                           int ldx, T* __restrict__ out, int ldo, const int* __restrict__ utt, int M, int C) {
    constexpr int VEC = Vec16<T>::N;
    const int cpr = C / VEC;
    const int m0 = blockIdx.x * RAG_SE_ROWS, m1 = min(m0 + RAG_SE_ROWS, M);
    for (int cc = threadIdx.x; cc < cpr * 4; cc += 256) {
        const int fl = cc / cpr, c = (cc - fl * cpr) * VEC;
        int ucur = -1;
        float g[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) g[j] = 0.0f;
        for (int m = m0 + fl; m < m1; m += 4) {
            const int u = utt[m];
            if (u != ucur) {
                ucur = u;
#pragma unroll
                for (int j = 0; j < VEC; ++j) g[j] = s[(int64_t)u * C + c + j];
            }
            const Vec16<T> hv = ld_nt(h + (int64_t)m * ldh + c);
            const Vec16<T> xv = ld_nt(x + (int64_t)m * ldx + c);
            Vec16<T> o;
#pragma unroll
            for (int j = 0; j < VEC; ++j) o.set(j, fmaf(hv.get(j), g[j], xv.get(j)));
            *reinterpret_cast<Vec16<T>*>(out + (int64_t)m * ldo + c) = o;
        }
    }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

hipError_t launch_rag_rows(const int* row0, int n, int maxT, int* utt, hipStream_t stream) {
    if (!row0 || !utt || n <= 0 || maxT <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rag_rows_kernel, dim3((maxT + 255) / 256, n), dim3(256), 0, stream, row0, utt);
    return hipGetLastError();
}

hipError_t launch_rag_se_apply(const void* h, int ldh, const float* s, const void* x, int ldx, void* out, int ldo, bool bf16,
                               const int* utt, int M, int C, hipStream_t stream) {
    const int vec = bf16 ? 8 : 4;
    if (!h || !s || !x || !out || !utt || M <= 0 || C % vec || ldh % vec || ldx % vec || ldo % vec) return hipErrorInvalidValue;
    if (!aligned16(h) || !aligned16(x) || !aligned16(out)) return hipErrorInvalidValue;
    const dim3 grid((M + RAG_SE_ROWS - 1) / RAG_SE_ROWS), block(256);
    if (bf16) hipLaunchKernelGGL(rag_se_apply_kernel<bf16_t>, grid, block, 0, stream, (const bf16_t*)h, ldh, s, (const bf16_t*)x, ldx, (bf16_t*)out, ldo, utt, M, C);
    else hipLaunchKernelGGL(rag_se_apply_kernel<float>, grid, block, 0, stream, (const float*)h, ldh, s, (const float*)x, ldx, (float*)out, ldo, utt, M, C);
    return hipGetLastError();
}

}  // namespace svhip
