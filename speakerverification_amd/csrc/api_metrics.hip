// api_metrics.hip — the verification metrics of libsvhip (see include/svhip.h; kernels: metrics.hip).
#include <cstring>

#include "scoring_host.h"

using namespace svhip;

namespace {
// shared front half: stage scores / labels, sort, scan.  Labels must be 0 / 1 (host labels are checked).
struct MetricsRun {
    svhip_handle* h;
    Staged s;
    void* ws = nullptr;
    size_t ws_bytes = 0;
    MetricsRun(svhip_handle* hh, int32_t flags) : h(hh), s(hh, flags & ~SVHIP_ASYNC) {}       // the metric calls have always waited, SVHIP_ASYNC or not
    int start(const float* scores, const int32_t* labels, int64_t P, bool nan_to_num, const char* label) {
        if (P >= ((int64_t)1 << 31)) SV_FAIL(h, SVHIP_ERR_UNSUPPORTED, "trial lists are limited to 2^31 - 1 entries");
        if (!s.din)
            for (int64_t i = 0; i < P; ++i)
                if (labels[i] != 0 && labels[i] != 1) SV_FAIL(h, SVHIP_ERR_INVALID, "label %lld of trial %lld is not 0 / 1", (long long)labels[i], (long long)i);
        const float* dS = s.in(svhip_handle::SCR_IN0, scores, (size_t)P * 4);
        const int32_t* dL = s.in(svhip_handle::SCR_IN1, labels, (size_t)P * 4);
        if (s.rc) return s.rc;
        ws_bytes = metrics_workspace_bytes(P);
        if (int rc = scratch(h, svhip_handle::SCR_WS, ws_bytes, &ws)) return rc;
        return run(h, label, 0, [&]() { return metrics_sort_scan(dS, dL, P, nan_to_num, ws, ws_bytes, h->stream); });
    }
};
}  // namespace

extern "C" {

int svhip_roc_points(svhip_handle* h, const float* scores, const int32_t* labels, int64_t P, int64_t* n_out, float* thr, int64_t* fps,
                     int64_t* tps, int32_t flags) {
    if (!h || !scores || !labels || !n_out || !thr || !fps || !tps || P <= 0) return SVHIP_ERR_INVALID;
    MetricsRun m(h, flags);
    int rc;
    if ((rc = m.start(scores, labels, P, true, "metrics_sort"))) return rc;
    float* dT = m.s.out(svhip_handle::SCR_OUT0, thr, (size_t)P * 4);
    int64_t* dF = m.s.out(svhip_handle::SCR_OUT1, fps, (size_t)P * 8);
    int64_t* dP = m.s.out(svhip_handle::SCR_OUT2, tps, (size_t)P * 8);
    if (m.s.rc) return m.s.rc;
    int32_t* n_dev = nullptr;
    if ((rc = run(h, "metrics_roc", 0, [&]() { return metrics_roc_points(P, m.ws, m.ws_bytes, dT, dF, dP, &n_dev, h->stream); }))) return rc;
    int32_t n32 = 0;
    SV_HIP(h, hipMemcpyAsync(&n32, n_dev, 4, hipMemcpyDeviceToHost, h->stream));
    SV_HIP(h, hipStreamSynchronize(h->stream));
    *n_out = n32;
    // its own copy-back: n32 points, not the P the outputs were staged for (the stream has just been waited for, so the copies block)
    if (!m.s.dout) {
        SV_HIP(h, hipMemcpy(thr, dT, (size_t)n32 * 4, hipMemcpyDeviceToHost));
        SV_HIP(h, hipMemcpy(fps, dF, (size_t)n32 * 8, hipMemcpyDeviceToHost));
        SV_HIP(h, hipMemcpy(tps, dP, (size_t)n32 * 8, hipMemcpyDeviceToHost));
    }
    return SVHIP_OK;
}

int svhip_error_rates(svhip_handle* h, const float* scores, const int32_t* labels, int64_t P, double* fnrs, double* fprs, float* thresholds,
                      int32_t flags) {
    if (!h || !scores || !labels || !fnrs || !fprs || !thresholds || P <= 0) return SVHIP_ERR_INVALID;
    MetricsRun m(h, flags);
    int rc;
    if ((rc = m.start(scores, labels, P, false, "metrics_sort"))) return rc;
    double* dA = m.s.out(svhip_handle::SCR_OUT0, fnrs, (size_t)P * 8);
    double* dB = m.s.out(svhip_handle::SCR_OUT1, fprs, (size_t)P * 8);
    float* dC = m.s.out(svhip_handle::SCR_OUT2, thresholds, (size_t)P * 4);
    if (m.s.rc) return m.s.rc;
    return m.s.finish("error_rates", run(h, "metrics_rates", 0, [&]() { return metrics_error_rates(P, m.ws, m.ws_bytes, dA, dB, dC, h->stream); }), false);
}

int svhip_min_dcf(svhip_handle* h, const float* scores, const int32_t* labels, int64_t P, double p_target, double c_miss, double c_fa,
                  double* min_dcf, float* threshold, int32_t flags) {
    if (!h || !scores || !labels || !min_dcf || !threshold || P <= 0) return SVHIP_ERR_INVALID;
    MetricsRun m(h, flags);
    int rc;
    if ((rc = m.start(scores, labels, P, false, "metrics_sort"))) return rc;
    // both results are host values and leave the device as one 16-byte block: its own copy-back
    void* res = nullptr;
    if ((rc = scratch(h, svhip_handle::SCR_OUT0, 16, &res))) return rc;
    rc = run(h, "metrics_min_dcf", 0, [&]() { return metrics_min_dcf(P, m.ws, m.ws_bytes, p_target, c_miss, c_fa, (double*)res, (float*)((char*)res + 8), h->stream); });
    char host[16];
    hipError_t e = rc ? hipSuccess : hipMemcpyAsync(host, res, 16, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (rc) return rc;
    SV_HIP(h, e);
    memcpy(min_dcf, host, 8);
    memcpy(threshold, host + 8, 4);
    return SVHIP_OK;
}

}  // extern "C"
