// scoring_host.h — what the host files of the scoring entry points share: api_scoring.hip (which defines all of it), api_asnorm.hip,
// api_search.hip, api_audit.hip and api_metrics.hip.  Internal and host-only: no other file includes it.
#pragma once
#include <algorithm>
#include <functional>

#include "handle.h"

namespace svhip {

// a scratch slot of at least `bytes` (grown by half again; the old block is freed only after the stream has drained)
int scratch(svhip_handle* h, int slot, size_t bytes, void** out);
void release_big_scratch(svhip_handle* h, bool staged_host);

// the 16-byte alignment the vector-load routes ask of their operands
inline bool aligned16(const void* a, const void* b = nullptr) { return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) == 0; }

// A scratch layout, written once: each take() is one region and returns its offset, the total goes to scratch(), a pointer is base + offset.
struct Bump {
    size_t size = 0;
    size_t take(size_t bytes, size_t align = 1) {       // align: a power of two; rounds the region's start up (take(0, align): the total)
        const size_t at = (size + align - 1) & ~(align - 1);
        size = at + bytes;
        return at;
    }
};
template <typename T>
T* at(void* base, size_t offset) { return reinterpret_cast<T*>(static_cast<char*>(base) + offset); }

// The operands of one call and its ending.  The constructor selects the handle's device; in() / out() hand back device pointers: the
// caller's own where the flags say they are device pointers, else a scratch slot of the handle (in: with the copy enqueued).  The first
// failure stays in `rc` and turns the later in() / out() into no-ops: a call stages all its operands, then returns `rc` if it is set.
// out() remembers what it staged, and finish() copies it back.
struct Staged {
    svhip_handle* h;
    bool din, dout, async;
    int rc;
    struct Out { void* host; void* dev; size_t bytes; } outs[4] = {};     // (four: the most outputs a call has; no allocation on the call path)
    int n_outs = 0;
    Staged(svhip_handle* hh, int32_t flags);
    int stage(int slot, size_t bytes, const void* host_src, void** dev);      // the slot at `bytes`; host_src: copied into it
    // from_host: `src` is host memory whatever the flags say (a table the call made itself)
    template <typename T>
    const T* in(int slot, const T* src, size_t bytes, bool from_host = false) {
        void* d = const_cast<T*>(src);
        if (!rc && (!din || from_host)) rc = stage(slot, bytes, src, &d);
        return static_cast<const T*>(d);
    }
    template <typename T>
    T* out(int slot, T* dst, size_t bytes) {
        void* d = dst;
        if (!rc && !dout) rc = stage(slot, bytes, nullptr, &d);
        if (!rc) outs[n_outs++] = {dst, d, bytes};
        return static_cast<T*>(d);
    }
    // The end of a call whose work is enqueued (res: what the call came to so far): copy the staged outputs back, wait unless the call is
    // asynchronous, report what the stream reports under the call's name and, with `release`, free the scratch that is not kept between
    // calls.  `release` keeps each call's retention as it was when the endings were written per call (asnorm_stats, the search calls and
    // group_audit release, the rest never did); one policy for all of them would be a change of behaviour, not of this helper.
    int finish(const char* name, int res, bool release);
};

// out (Na, Nb) = A @ B^T.  The route is decided ONCE (split_b and score_gemm used to re-derive it from different predicates):
//   SCORE_H3W     rows of A in registers, B streamed past them as half planes (score_h3w.hip; D = 192 / 256, aligned operands);
//                 the kernel's launcher fills the planes itself (and scales both operands by exact powers of two)
//   SCORE_WORDS   the tiled GEMM with B as (hi half << 16 | lo half) words, A split in registers (gemm_pw's x3 form)
//   SCORE_F32MFMA the exact fp32 MFMA GEMM (option score_f32mfma, or shapes gemm_pw's split form does not take)
// The split forms run as three fp16 MFMAs per product on every handle since round 4 (a score of unit vectors within ~4e-8 of the float64
// oracle, the exact fp32 MFMA 3.5e-8) at twice the fp32 matrix rate.
enum ScoreRoute { SCORE_F32MFMA = 0, SCORE_WORDS = 1, SCORE_H3W = 2 };
ScoreRoute score_route(const svhip_handle* h, const float* dA, int64_t Na, const float* dB, int64_t Nb, int D);
int score_gemm(svhip_handle* h, const char* label, const float* dA, int64_t Na, const float* dB, int64_t Nb, int D, float* dO, int64_t ldo,
               ScoreRoute route, const void* dBsplit);
// the split operand of the chosen route in a scratch slot of the handle: half planes (filled by the row-streaming kernel's own launcher:
// [2][Nb][D] halves + its scale word) or split words (filled here)
int split_b(svhip_handle* h, ScoreRoute route, const float* dB, int64_t Nb, int D, void** out);

// The slab route of asnorm_stats, score_topk and score_above: A @ B^T goes through an HBM scratch (SCR_SLAB) in slabs of A's rows - at most
// 2 GiB, at least 128 rows, row stride ldk - and a row kernel consumes each slab.  open() decides everything once per call, pass() walks.
struct SlabWalk {
    svhip_handle* h;
    const float* dA; int64_t N;
    const float* dB; int64_t M;
    int D;
    int64_t ldk = 0, slab_rows = 0;
    ScoreRoute route = SCORE_F32MFMA;
    void *bsplit = nullptr, *slab = nullptr;
    // name: the call that refuses, in its own words, an M no 128-row slab holds (NULL: no refusal, as asnorm_stats always ran)
    int open(const char* name);
    // per slab: score_gemm under `label` (gemm = false: the call's one slab still holds its scores), then rows_fn(r0, rows, slab, ldk)
    int pass(const char* label, bool gemm, const std::function<int(int64_t, int64_t, const float*, int64_t)>& rows_fn);
};

}  // namespace svhip
