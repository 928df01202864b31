// api_ragged.hip — what the ragged calls of ECAPA-TDNN, RawNet2 'conv', RawNet3, the Conformer, TitaNet and ResNetSE34V2 share on the host: the refusal texts and the
// rules of the mel models, the table ring (RagTables), the one table layout, and the driver that turns a call's arrays into a RagPack
// (allocation, the row loop, the input, the upload).  A model's api_<model>.hip keeps its RagRule, its own rules and its forward.
#include <algorithm>
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

int rag_mel_check(const svhip_config& c, const int32_t* lengths, int n, bool is_wave, std::string& err, bool cfg_extra_ok, const char* cfg_names,
                  int min_frames, const char* why, RagUttRule* more, int64_t bound, int row_unit) {
    if (c.hop_length <= 0 || c.max_batch <= 0 || c.samples < c.n_fft || !cfg_extra_ok) return refuse(err, SVHIP_ERR_INVALID, "bad %s", cfg_names);
    const int64_t cap = (int64_t)c.max_batch * mel_frames(c, c.samples, true);
    int64_t rows = 0;
    for (int i = 0; i < n; ++i) {
        if (is_wave && lengths[i] < c.n_fft)
            return refuse(err, SVHIP_ERR_INVALID, "utterance %d: %lld samples, fewer than n_fft=%d", i, (long long)lengths[i], c.n_fft);
        const int64_t T = mel_frames(c, lengths[i], is_wave);
        if (T < min_frames) return refuse(err, SVHIP_ERR_INVALID, "utterance %d: %lld frames, fewer than %d%s", i, (long long)T, min_frames, why);
        int rc;
        if (more && (rc = more(bound, i, T, err))) return rc;
        if ((rc = rag_rows_fit(err, i, rows += (T + row_unit - 1) / row_unit * row_unit, cap, "T"))) return rc;
    }
    return SVHIP_OK;
}

// ---- the table ring --------------------------------------------------------------------------------------
// `dev` is set last: non-null means that everything is there, and it is the one guard of a handle's ragged allocation.  Each part is
// allocated only while null, here, in rag_pack and in the models, so a call after one that failed halfway allocates nothing twice
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

// ---- the mel input of a pack (ECAPA-TDNN, Conformer, TitaNet, ResNetSE) ---------------------------------------------------------
// mel0: the n + 1 first mel frames on the host.  Waveforms go through the staging buffer and one fbank launch per utterance into
// h->d_feat, host features are copied there, device features are read in place; fills feat_off, *d_feat is the array they index
static int rag_mel_input(svhip_handle* h, RagTables& rag, const float* in, bool in_host, bool is_wave, const int64_t* in_off, const int32_t* lengths,
                  int n, const int* mel0, int64_t* feat_off, const float** d_feat) {
    const svhip_config& c = h->cfg;
    int rc;
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

// ---- a call's arrays -> a pack ------------------------------------------------------------------------------------------
namespace {

struct RagView { int64_t* off; int32_t* len; int* row0[RAG_LEVELS]; };      // the typed tables of a block, on the device or in a pinned slot

size_t rag_tab_bytes(size_t B, int levels) { return B * 8 + B * 4 + (size_t)levels * (B + 1) * 4; }

RagView rag_view(char* base, size_t B, int levels) {
    RagView v{reinterpret_cast<int64_t*>(base), reinterpret_cast<int32_t*>(base + B * 8), {}};
    for (int l = 0; l < levels; ++l) v.row0[l] = v.len + B + l * (B + 1);
    return v;
}

}  // namespace

int rag_pack(svhip_handle* h, RagTables& rag, const RagRule& rule, const size_t utt_cap[RAG_LEVELS], const float* in, bool in_host, bool is_wave,
             const int64_t* in_off, const int32_t* lengths, int n, RagPack& pk) {
    const svhip_config& c = h->cfg;
    const size_t B = c.max_batch, bytes = rag_tab_bytes(B, rule.levels);
    int rc;
    if (!rag.dev) {
        for (int l = 0; l < rule.levels; ++l)
            if (utt_cap[l] && !rag.utt[l] && (rc = dev_alloc(h, &rag.utt[l], utt_cap[l]))) return rc;
        // (RawNet3: a pack of n <= B utterances within B T0 frames holds at most 10 B T0 + 250 n <= B (samples + 9) samples;
        //  RawNet2 'conv': at most 3 sum T1_u + 2 n <= B (samples + 2) samples, since L_u <= 3 T1_u + 2 and sum T1_u <= B floor(samples / 3))
        if ((rc = rag.alloc(h, bytes, B * ((size_t)c.samples + (rule.mel ? c.hop_length : 16))))) return rc;
    }
    char* slot = nullptr;
    if ((rc = rag.acquire(h, &slot))) return rc;
    const RagView host = rag_view(slot, B, rule.levels), dev = rag_view(rag.dev, B, rule.levels);
    pk = RagPack{};
    pk.n = n; pk.levels = rule.levels;
    pk.off = dev.off; pk.len = dev.len;
    for (int u = 0; u < n; ++u) {
        int T[RAG_LEVELS] = {};
        rule.frames(c, lengths[u], is_wave, T);
        for (int l = 0; l < rule.levels; ++l) {
            Seg& g = pk.lv[l];
            host.row0[l][u] = g.M;
            g.M += T[l];
            g.maxT = std::max(g.maxT, T[l]);
        }
        host.len[u] = lengths[u];
    }
    for (int l = 0; l < rule.levels; ++l) {
        Seg& g = pk.lv[l];
        host.row0[l][n] = g.M;
        g.row0 = dev.row0[l]; g.utt = rag.utt[l]; g.hrow0 = host.row0[l];
    }
    h->cur = h->stream;
    if (rule.mel) {
        if ((rc = rag_mel_input(h, rag, in, in_host, is_wave, in_off, lengths, n, host.row0[0], host.off, &pk.in))) return rc;
    } else {
        // the waveforms as they are: a host array's utterances back to back in the staging buffer
        int64_t pos = 0;
        for (int u = 0; u < n; ++u) {
            host.off[u] = in_off[u];
            if (in_host) {
                SV_HIP(h, hipMemcpyAsync(rag.wav + pos, in + in_off[u], (size_t)lengths[u] * 4, hipMemcpyHostToDevice, h->stream));
                host.off[u] = pos;
                pos += lengths[u];
            }
        }
        pk.in = in_host ? rag.wav : in;
    }
    return rag.commit(h, bytes);
}

}  // namespace svhip
