// api_ragged.hip — what the ragged calls of ECAPA-TDNN, RawNet3, the Conformer and TitaNet share on the host: the refusal texts, the table ring
// (RagTables) and the mel input of a pack.  Each model's own rules, table layout and forward stay in its api_<model>.hip.
#include <cstdarg>

#include "handle.h"

namespace svhip {

int refuse(std::string& err, int code, const char* fmt, ...) {
    char b[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(b, sizeof(b), fmt, ap);
    va_end(ap);
    err = b;
    return code;
}

int rag_rows_fit(std::string& err, int i, int64_t rows, int64_t cap, const char* frames_name) {
    if (rows <= cap) return SVHIP_OK;
    return refuse(err, SVHIP_ERR_INVALID, "utterance %d: the pack reaches %lld frames, over the handle's capacity of max_batch * %s = %lld rows", i,
                  (long long)rows, frames_name, (long long)cap);
}

// ---- the table ring --------------------------------------------------------------------------------------
// `dev` is set last: non-null means that everything is there, and it is the one guard of the models' ragged allocation.  Each part is
// allocated only while null, here and in the models, so a call after one that failed halfway allocates nothing twice
int RagTables::alloc(svhip_handle* h, size_t table_bytes, size_t wav_floats) {
    if (dev) return SVHIP_OK;
    int rc;
    if (!wav && (rc = dev_alloc(h, &wav, wav_floats))) return rc;
    for (auto& sl : slot) {
        if (!sl.host) SV_HIP(h, hipHostMalloc((void**)&sl.host, table_bytes, hipHostMallocDefault));
        if (!sl.done) SV_HIP(h, hipEventCreateWithFlags(&sl.done, hipEventDisableTiming));
    }
    return dev_alloc(h, &dev, table_bytes);
}

int RagTables::acquire(svhip_handle* h, char** host) {
    cur = &slot[next];
    next = (next + 1) & 3;
    if (cur->busy) { SV_HIP(h, hipEventSynchronize(cur->done)); cur->busy = false; }
    *host = cur->host;
    return SVHIP_OK;
}

int RagTables::commit(svhip_handle* h, size_t bytes) {
    SV_HIP(h, hipMemcpyAsync(dev, cur->host, bytes, hipMemcpyHostToDevice, h->stream));
    SV_HIP(h, hipEventRecord(cur->done, h->stream));
    cur->busy = true;
    return SVHIP_OK;
}

RagTables::~RagTables() {
    for (auto& sl : slot) {
        if (sl.host) (void)hipHostFree(sl.host);
        if (sl.done) (void)hipEventDestroy(sl.done);
    }
}

// ---- the mel input of a pack (ECAPA-TDNN, Conformer, TitaNet) ---------------------------------------------------------
int rag_mel_input(svhip_handle* h, RagTables& rag, const float* in, bool in_host, bool is_wave, const int64_t* in_off, const int32_t* lengths,
                  int n, const int* mel0, int64_t* feat_off, const float** d_feat) {
    const svhip_config& c = h->cfg;
    int rc;
    h->cur = h->stream;
    *d_feat = h->d_feat;
    h->feat_is_stale = false;
    if (is_wave) {
        // the mel power of every utterance, (n_mels, T_u) blocks back to back in d_feat.  The DFT kernel is launched once per utterance
        // (a workgroup of it sees one utterance's samples only, so its values do not depend on the pack)
        int64_t pos = 0;
        for (int u = 0; u < n; ++u) {
            const int L = lengths[u], T = mel0[u + 1] - mel0[u];
            const float* w = in + in_off[u];
            if (in_host) {
                SV_HIP(h, hipMemcpyAsync(rag.wav + pos, w, (size_t)L * 4, hipMemcpyHostToDevice, h->stream));
                w = rag.wav + pos;
                pos += L;
            }
            float* mel = h->d_feat + (size_t)mel0[u] * c.n_mels;
            if ((rc = run(h, "fbank", 0, [&]() { return launch_fbank(h->fb, w, 1, L, T, mel, h->stream); }))) return rc;
            feat_off[u] = (int64_t)mel0[u] * c.n_mels;
        }
    } else if (in_host) {
        for (int u = 0; u < n; ++u) {
            feat_off[u] = (int64_t)mel0[u] * c.n_mels;
            SV_HIP(h, hipMemcpyAsync(h->d_feat + feat_off[u], in + in_off[u] * c.n_mels, (size_t)lengths[u] * c.n_mels * 4, hipMemcpyHostToDevice, h->stream));
        }
    } else {
        for (int u = 0; u < n; ++u) feat_off[u] = in_off[u] * c.n_mels;
        *d_feat = in;
        h->feat_is_stale = true;            // (d_feat does not hold this forward's mel power)
    }
    return SVHIP_OK;
}

}  // namespace svhip
