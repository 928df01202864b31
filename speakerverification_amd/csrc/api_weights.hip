// api_weights.hip — weight loading of libsvhip: front-end tables, expected weight names / shapes, weight packing, the workspace.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <thread>

#include "handle.h"

namespace svhip {

static inline uint16_t f32_to_f16_rne(float f) {      // IEEE half, round to nearest even (the host compiler's _Float16 conversion)
    const _Float16 hv = static_cast<_Float16>(f);
    uint16_t u;
    memcpy(&u, &hv, 2);
    return u;
}

static inline uint16_t f32_to_bf16_rne(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);   // NaN stays NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

// host twin of common.h's x3_hi / x3_lo: a weight as (hi << 16) | lo in the planes' type (IEEE half; bf16 under -DSVHIP_X3_BF16)
static inline uint32_t x3_split_word(float v) {
#ifdef SVHIP_X3_BF16
    const uint16_t hi = f32_to_bf16_rne(v);
    uint32_t hu = (uint32_t)hi << 16;
    float hf; memcpy(&hf, &hu, 4);
    return hu | f32_to_bf16_rne(v - hf);
#else
    const _Float16 h = static_cast<_Float16>(v);                 // (plain conversions: overflow -> inf, NaN stays NaN — common.h, RANGE)
    const _Float16 l = static_cast<_Float16>(v - static_cast<float>(h));
    uint16_t hb, lb;
    memcpy(&hb, &h, 2); memcpy(&lb, &l, 2);
    return ((uint32_t)hb << 16) | lb;
#endif
}

// a weight in the handle's 16-bit storage type
static inline uint16_t to_h16(const svhip_handle* h, float f) { return h->f16 ? f32_to_f16_rne(f) : f32_to_bf16_rne(f); }

// ---- front-end tables (oracle/fbank.py restates the same constants) --------------------------------
static double hz_to_mel(double f) {
    const double f_sp = 200.0 / 3, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = std::log(6.4) / 27.0;
    return f >= min_log_hz ? min_log_mel + std::log(f / min_log_hz) / logstep : f / f_sp;
}
static double mel_to_hz(double m) {
    const double f_sp = 200.0 / 3, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = std::log(6.4) / 27.0;
    return m >= min_log_mel ? min_log_hz * std::exp(logstep * (m - min_log_mel)) : f_sp * m;
}

int build_fbank_tables(svhip_handle* h) {
    const svhip_config& c = h->cfg;
    FbankTables& fb = h->fb;
    fb.n_fft = c.n_fft; fb.win_length = c.win_length; fb.hop = c.hop_length; fb.n_mels = c.n_mels;
    fb.n_bins = c.n_fft / 2 + 1;
    fb.lpad = (c.n_fft - c.win_length) / 2;
    fb.n_pairs = (fb.n_bins + 31) / 32;
    fb.n_q = c.win_length / 8;
    fb.preemph = c.preemph;
    if (c.win_length % 8 != 0 || c.hop_length % 4 != 0 || fb.n_pairs > 9 || c.win_length > c.n_fft)
        SV_FAIL(h, SVHIP_ERR_UNSUPPORTED, "fbank geometry n_fft=%d win=%d hop=%d not supported", c.n_fft, c.win_length, c.hop_length);
    const double PI = 3.14159265358979323846;
    // periodic Hamming (scipy get_window('hamming', win, fftbins=True)), cast to float32
    std::vector<float> win(c.win_length);
    for (int k = 0; k < c.win_length; ++k) win[k] = (float)(0.54 - 0.46 * std::cos(2.0 * PI * k / c.win_length));
    // basis[q][pair][part][lane] float4: tap = 8q + 4h + j, bin = 32*pair + r (lane = 32h + r); part 0 = cos, 1 = sin
    std::vector<float> basis((size_t)fb.n_q * fb.n_pairs * 2 * 64 * 4, 0.0f);
    for (int q = 0; q < fb.n_q; ++q)
        for (int pr = 0; pr < fb.n_pairs; ++pr)
            for (int part = 0; part < 2; ++part)
                for (int lane = 0; lane < 64; ++lane)
                    for (int j = 0; j < 4; ++j) {
                        const int r = lane & 31, hh = lane >> 5;
                        const int tap = 8 * q + 4 * hh + j, bin = 32 * pr + r;
                        float v = 0.0f;
                        if (bin < fb.n_bins) {
                            const double ang = 2.0 * PI * (double)bin * (double)(fb.lpad + tap) / (double)c.n_fft;
                            const float tr = (float)(part == 0 ? std::cos(ang) : std::sin(ang));
                            v = tr * win[tap];                       // float32 product, as nnAudio's kernel * window mask
                        }
                        basis[((((size_t)q * fb.n_pairs + pr) * 2 + part) * 64 + lane) * 4 + j] = v;
                    }
    // bf16x3 tables: the same windowed taps split into bf16 hi + lo, k-steps of 16 (zero padded)
    fb.n_k16 = (c.win_length + 15) / 16;
    fb.split_bf16 = (h->bf16 && c.hop_length % 8 == 0) ? 1 : 0;
    fb.split6 = (h->x3 && c.hop_length % 8 == 0) ? 1 : 0;          // F32X3 handles: the exact three-way split, six products
    if (fb.split_bf16 || fb.split6) {
        std::vector<uint16_t> bhi((size_t)fb.n_k16 * fb.n_pairs * 2 * 64 * 8, 0), blo(bhi.size(), 0), bl3(bhi.size(), 0);
        for (int kk = 0; kk < fb.n_k16; ++kk)
            for (int pr = 0; pr < fb.n_pairs; ++pr)
                for (int part = 0; part < 2; ++part)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int j = 0; j < 8; ++j) {
                            const int r = lane & 31, hh = lane >> 5;
                            const int tap = 16 * kk + 8 * hh + j, bin = 32 * pr + r;
                            float v = 0.0f;
                            if (bin < fb.n_bins && tap < c.win_length) {
                                const double ang = 2.0 * PI * (double)bin * (double)(fb.lpad + tap) / (double)c.n_fft;
                                v = (float)(part == 0 ? std::cos(ang) : std::sin(ang)) * win[tap];
                            }
                            const uint16_t hi = f32_to_bf16_rne(v);
                            uint32_t hu = (uint32_t)hi << 16;
                            float hf; memcpy(&hf, &hu, 4);
                            const size_t idx = ((((size_t)kk * fb.n_pairs + pr) * 2 + part) * 64 + lane) * 8 + j;
                            bhi[idx] = hi;
                            blo[idx] = f32_to_bf16_rne(v - hf);
                            uint32_t mu = (uint32_t)blo[idx] << 16;
                            float mf; memcpy(&mf, &mu, 4);
                            bl3[idx] = f32_to_bf16_rne((v - hf) - mf);
                        }
        uint16_t *dh, *dl;
        int rc2;
        if ((rc2 = dev_upload(h, &dh, bhi))) return rc2;
        if ((rc2 = dev_upload(h, &dl, blo))) return rc2;
        fb.basis_hi = dh; fb.basis_lo = dl;
        if (fb.split6) {
            uint16_t* d3;
            if ((rc2 = dev_upload(h, &d3, bl3))) return rc2;
            fb.basis_l3 = d3;
        }
    }
    // the fused front-end of bf16 handles (fbank.hip, round 6): the window is symmetric about tap win / 2, so Re X_k / Im X_k are products of
    // K = win / 2 + 1 taps with w_m cos(2 pi k m / n_fft) / w_m sin(2 pi k m / n_fft), m = 0 .. win / 2 (slot win / 2 carries the unpaired tap 0)
    if (h->bf16 && c.n_fft == 512 && c.win_length == 200 && c.hop_length == 80) {
        const int half = c.win_length / 2, nks = 7, npr = 8;
        std::vector<uint16_t> shi((size_t)nks * npr * 2 * 64 * 8, 0), slo(shi.size(), 0);
        for (int kk = 0; kk < nks; ++kk)
            for (int pr = 0; pr < npr; ++pr)
                for (int part = 0; part < 2; ++part)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int j = 0; j < 8; ++j) {
                            const int r = lane & 31, hh = lane >> 5;
                            const int m = 16 * kk + 8 * hh + j, bin = 32 * pr + r;
                            float v = 0.0f;
                            if (m <= half && bin < fb.n_bins) {
                                const float w = m < half ? win[half + m] : win[0];
                                const double ang = 2.0 * PI * (double)bin * (double)m / (double)c.n_fft;
                                v = (float)(part == 0 ? std::cos(ang) : std::sin(ang)) * w;
                            }
                            const uint16_t hi = f32_to_bf16_rne(v);
                            uint32_t hu = (uint32_t)hi << 16;
                            float hf; memcpy(&hf, &hu, 4);
                            const size_t idx = ((((size_t)kk * npr + pr) * 2 + part) * 64 + lane) * 8 + j;
                            shi[idx] = hi;
                            slo[idx] = f32_to_bf16_rne(v - hf);
                        }
        uint16_t *dh, *dl;
        int rc2;
        if ((rc2 = dev_upload(h, &dh, shi))) return rc2;
        if ((rc2 = dev_upload(h, &dl, slo))) return rc2;
        fb.sym_hi = dh; fb.sym_lo = dl;
    }
    // Slaney mel bank (librosa 0.7 filters.mel(htk=False, norm=1)) in double, stored float32, sparse rows
    const double sr = c.fb_sr;
    const double fmax = c.fmax > 0 ? c.fmax : sr / 2;
    const int nm = c.n_mels, nb = fb.n_bins;
    std::vector<double> mel_f(nm + 2), fftf(nb);
    for (int i = 0; i < nb; ++i) fftf[i] = (sr / 2) * i / (double)(nb - 1);
    const double m0 = hz_to_mel(c.fmin), m1 = hz_to_mel(fmax);
    for (int i = 0; i < nm + 2; ++i) mel_f[i] = mel_to_hz(m0 + (m1 - m0) * i / (double)(nm + 1));
    std::vector<float> mw;
    std::vector<int> mstart(nm), mlen(nm), moff(nm);
    for (int i = 0; i < nm; ++i) {
        const double fd0 = mel_f[i + 1] - mel_f[i], fd1 = mel_f[i + 2] - mel_f[i + 1];
        const double enorm = 2.0 / (mel_f[i + 2] - mel_f[i]);
        int first = -1, last = -1;
        std::vector<float> row(nb);
        for (int k = 0; k < nb; ++k) {
            const double lower = -(mel_f[i] - fftf[k]) / fd0, upper = (mel_f[i + 2] - fftf[k]) / fd1;
            const float w32 = (float)std::fmax(0.0, std::fmin(lower, upper));
            row[k] = (float)((double)w32 * enorm);
            if (row[k] != 0.0f) { if (first < 0) first = k; last = k; }
        }
        if (first < 0) { first = 0; last = -1; }
        mstart[i] = first; mlen[i] = last - first + 1; moff[i] = (int)mw.size();
        for (int k = first; k <= last; ++k) mw.push_back(row[k]);
    }
    if (mw.empty()) mw.push_back(0.0f);
    float* d_basis; float* d_mw; int *d_ms, *d_ml, *d_mo;
    int rc;
    if ((rc = dev_upload(h, &d_basis, basis))) return rc;
    if ((rc = dev_upload(h, &d_mw, mw))) return rc;
    if ((rc = dev_upload(h, &d_ms, mstart))) return rc;
    if ((rc = dev_upload(h, &d_ml, mlen))) return rc;
    if ((rc = dev_upload(h, &d_mo, moff))) return rc;
    fb.n_melw = (int)mw.size();
    fb.mel_max_bin = 0;
    for (int i = 0; i < nm; ++i) fb.mel_max_bin = std::max(fb.mel_max_bin, mstart[i] + mlen[i] - 1);
    fb.basis = d_basis; fb.mel_w = d_mw; fb.mel_start = d_ms; fb.mel_len = d_ml; fb.mel_off = d_mo;
    return SVHIP_OK;
}

// ---- expected weight names / shapes ----------------------------------------------------------------
const int ECAPA_K[5] = {5, 3, 3, 3, 1};
const int ECAPA_D[5] = {1, 2, 3, 4, 1};

static void ecapa_spec(const svhip_config& c, std::map<std::string, std::vector<int64_t>>& spec) {
    const int64_t C = c.channels, C3 = 3 * C, nm = c.n_mels;
    auto bn = [&](const std::string& p, int64_t n) {
        spec[p + ".weight"] = {n}; spec[p + ".bias"] = {n}; spec[p + ".running_mean"] = {n};
        spec[p + ".running_var"] = {n}; spec[p + ".num_batches_tracked"] = {};
    };
    auto tdnn = [&](const std::string& p, int64_t cin, int64_t cout, int64_t k) {
        spec[p + ".conv.conv.weight"] = {cout, cin, k}; spec[p + ".conv.conv.bias"] = {cout};
        bn(p + ".norm.norm", cout);
    };
    if (c.input_norm) { spec["instance_norm.weight"] = {nm}; spec["instance_norm.bias"] = {nm}; }
    tdnn("blocks.0", nm, C, ECAPA_K[0]);
    for (int i = 1; i <= 3; ++i) {
        const std::string p = "blocks." + std::to_string(i);
        tdnn(p + ".tdnn1", C, C, 1);
        for (int j = 0; j < 7; ++j) tdnn(p + ".res2net_block.blocks." + std::to_string(j), C / 8, C / 8, ECAPA_K[i]);
        tdnn(p + ".tdnn2", C, C, 1);
        spec[p + ".se_block.conv1.conv.weight"] = {128, C, 1}; spec[p + ".se_block.conv1.conv.bias"] = {128};
        spec[p + ".se_block.conv2.conv.weight"] = {C, 128, 1}; spec[p + ".se_block.conv2.conv.bias"] = {C};
    }
    tdnn("mfa", C3, C3, 1);
    tdnn("asp.tdnn", 3 * C3, 128, 1);
    spec["asp.conv.conv.weight"] = {C3, 128, 1}; spec["asp.conv.conv.bias"] = {C3};
    bn("asp_bn.norm", 2 * C3);
    spec["fc.conv.weight"] = {(int64_t)c.embed_dim, 2 * C3, 1}; spec["fc.conv.bias"] = {(int64_t)c.embed_dim};
}

const int RN_LAYERS[6] = {1, 1, 1, 2, 1, 2};                   // RawNet2_custom.py:231

const int RN_FILTERS[6] = {128, 128, 256, 256, 512, 512};      // RawNet2_custom.py:232

static void rawnet2_spec(const svhip_config& c, std::map<std::string, std::vector<int64_t>>& spec) {
    auto bn = [&](const std::string& p, int64_t n) {
        spec[p + ".weight"] = {n}; spec[p + ".bias"] = {n}; spec[p + ".running_mean"] = {n};
        spec[p + ".running_var"] = {n}; spec[p + ".num_batches_tracked"] = {};
    };
    if (c.model == SVHIP_MODEL_RAWNET2_CONV) {          // conv1 = Conv1d(1, 128, 3, stride=3) with bias (RawNet2_custom.py:45-52)
        spec["conv1.weight"] = {128, 1, 3}; spec["conv1.bias"] = {128};
    } else {
        spec["ln.gamma"] = {(int64_t)c.samples}; spec["ln.beta"] = {(int64_t)c.samples};
        spec["first_conv.low_hz_"] = {128, 1}; spec["first_conv.band_hz_"] = {128, 1};
        bn("first_bn", 128);
    }
    int64_t inpl = 128;
    for (int li = 0; li < 6; ++li)
        for (int b = 0; b < RN_LAYERS[li]; ++b) {
            const std::string p = "layer" + std::to_string(li + 1) + "." + std::to_string(b);
            const int64_t planes = RN_FILTERS[li];
            bn(p + ".bn1", inpl);
            spec[p + ".conv1.weight"] = {planes, inpl, 3};
            bn(p + ".bn2", planes);
            spec[p + ".conv2.weight"] = {planes, planes, 3};
            spec[p + ".afms.alpha"] = {planes, 1};
            spec[p + ".afms.fc.weight"] = {planes, planes}; spec[p + ".afms.fc.bias"] = {planes};
            if (inpl != planes) spec[p + ".shortcut.0.weight"] = {planes, inpl, 1};
            inpl = planes;
        }
    if (rn_is_gru(c.model)) {                        // aggregate='gru' (RawNet2_custom.py:84-95): fc is built too, and never used (:196-207)
        const int64_t G = 3 * RN_GRU_HIDDEN;
        bn("bn_before_gru", 512);
        spec["gru.weight_ih_l0"] = {G, 512}; spec["gru.weight_hh_l0"] = {G, RN_GRU_HIDDEN};
        spec["gru.bias_ih_l0"] = {G}; spec["gru.bias_hh_l0"] = {G};
        spec["fc_after_gru.weight"] = {(int64_t)c.embed_dim, RN_GRU_HIDDEN}; spec["fc_after_gru.bias"] = {(int64_t)c.embed_dim};
    } else {
        bn("bn_before_agg", 512);
        spec["attention.0.weight"] = {128, 512, 1}; spec["attention.0.bias"] = {128};
        bn("attention.2", 128);
        spec["attention.3.weight"] = {512, 128, 1}; spec["attention.3.bias"] = {512};
    }
    spec["fc.weight"] = {(int64_t)c.embed_dim, 1024}; spec["fc.bias"] = {(int64_t)c.embed_dim};
}

// RawNet3.MainModel's defaults (RawNet3.py:172-186): the 234 names of its state dict, the unused bn1.*, bn6.* and the pre-emphasis
// buffer included (the filterbank's window_ / n_ buffers are read: the checkpoint's values are the ones the filters are built from)
static void rawnet3_spec(const svhip_config& c, std::map<std::string, std::vector<int64_t>>& spec) {
    auto bn = [&](const std::string& p, int64_t n) {
        spec[p + ".weight"] = {n}; spec[p + ".bias"] = {n}; spec[p + ".running_mean"] = {n};
        spec[p + ".running_var"] = {n}; spec[p + ".num_batches_tracked"] = {};
    };
    const int64_t C = 1024, W = C / 8, D = 1536, nOut = c.embed_dim;
    spec["preprocess.0.flipped_filter"] = {1, 1, 2}; spec["preprocess.1.weight"] = {1}; spec["preprocess.1.bias"] = {1};
    spec["conv1.filterbank.low_hz_"] = {C / 8, 1}; spec["conv1.filterbank.band_hz_"] = {C / 8, 1};
    spec["conv1.filterbank.window_"] = {125}; spec["conv1.filterbank.n_"] = {1, 125};
    bn("bn1", C / 4);
    for (int li = 1; li <= 3; ++li) {
        const std::string p = "layer" + std::to_string(li);
        const int64_t cin = li == 1 ? C / 4 : C;
        spec[p + ".conv1.weight"] = {C, cin, 1}; spec[p + ".conv1.bias"] = {C};
        bn(p + ".bn1", C);
        for (int i = 0; i < 7; ++i) {
            spec[p + ".convs." + std::to_string(i) + ".weight"] = {W, W, 3}; spec[p + ".convs." + std::to_string(i) + ".bias"] = {W};
            bn(p + ".bns." + std::to_string(i), W);
        }
        spec[p + ".conv3.weight"] = {C, C, 1}; spec[p + ".conv3.bias"] = {C};
        bn(p + ".bn3", C);
        spec[p + ".afms.alpha"] = {C, 1}; spec[p + ".afms.fc.weight"] = {C, C}; spec[p + ".afms.fc.bias"] = {C};
        if (cin != C) spec[p + ".residual.0.weight"] = {C, cin, 1};
    }
    spec["layer4.weight"] = {D, 3 * C, 1}; spec["layer4.bias"] = {D};
    spec["attention.0.weight"] = {128, 3 * D, 1}; spec["attention.0.bias"] = {128};
    bn("attention.2", 128);
    spec["attention.3.weight"] = {1, 128, 1}; spec["attention.3.bias"] = {1};
    bn("bn5", 2 * D);
    spec["fc6.weight"] = {nOut, 2 * D}; spec["fc6.bias"] = {nOut};
    bn("bn6", nOut);
}

// TitaNet.MainModel (TitaNet.py:124-159,202-318,321-431): the names of its state dict for SVHIP_TITANET_MAX_BLOCKS mega-blocks; a checkpoint
// holds the first n of them (finalize_titanet)
static void tn_block_spec(int64_t H, int64_t k, const std::string& p, std::map<std::string, std::vector<int64_t>>& spec);
static void titanet_spec(const svhip_config& c, std::map<std::string, std::vector<int64_t>>& spec) {
    auto bn = [&](const std::string& p, int64_t n) {
        spec[p + ".weight"] = {n}; spec[p + ".bias"] = {n}; spec[p + ".running_mean"] = {n};
        spec[p + ".running_var"] = {n}; spec[p + ".num_batches_tracked"] = {};
    };
    const int64_t H = c.channels, k = tn_kernel_size(c.channels), D = 1536, nOut = c.embed_dim;
    spec["encoder.prolog.conv_block.0.weight"] = {H, (int64_t)c.n_mels, 3}; spec["encoder.prolog.conv_block.0.bias"] = {H};
    bn("encoder.prolog.conv_block.1", H);
    for (int i = 0; i < SVHIP_TITANET_MAX_BLOCKS; ++i) tn_block_spec(H, k, "encoder.mega_blocks." + std::to_string(i) + ".", spec);
    spec["encoder.epilog.conv_block.0.weight"] = {D, H, 1}; spec["encoder.epilog.conv_block.0.bias"] = {D};
    bn("encoder.epilog.conv_block.1", D);
    spec["decoder.pool.0.in_linear.weight"] = {128, D}; spec["decoder.pool.0.in_linear.bias"] = {128};
    spec["decoder.pool.0.out_linear.weight"] = {D, 128}; spec["decoder.pool.0.out_linear.bias"] = {D};
    bn("decoder.pool.1", 2 * D);
    spec["decoder.linear.0.weight"] = {nOut, 2 * D}; spec["decoder.linear.0.bias"] = {nOut};
    bn("decoder.linear.1", nOut);
}
static void tn_block_spec(int64_t H, int64_t k, const std::string& p, std::map<std::string, std::vector<int64_t>>& spec) {
    auto bn = [&](const std::string& q, int64_t n) {
        spec[q + ".weight"] = {n}; spec[q + ".bias"] = {n}; spec[q + ".running_mean"] = {n};
        spec[q + ".running_var"] = {n}; spec[q + ".num_batches_tracked"] = {};
    };
    for (int j = 0; j < 3; ++j) {
        const std::string q = p + "sub_blocks." + std::to_string(j) + ".conv_block.";
        spec[q + "0.conv.0.weight"] = {H, 1, k}; spec[q + "0.conv.0.bias"] = {H};
        spec[q + "0.conv.1.weight"] = {H, H, 1}; spec[q + "0.conv.1.bias"] = {H};
        bn(q + "1", H);
    }
    spec[p + "sub_blocks.3.excitation.0.weight"] = {H / 16, H}; spec[p + "sub_blocks.3.excitation.2.weight"] = {H, H / 16};
    spec[p + "skip_connection.0.weight"] = {H, H, 1}; spec[p + "skip_connection.0.bias"] = {H};
    bn(p + "skip_connection.1", H);
}

// Conformer.MainModel (models/Conformer.py:13-97 with models/conformer/conformer/encoder.py's ConformerEncoder(n_mels, 256, 6 layers,
// 4 heads, FF x 4, conv kernel 15)): the 278 names of its state dict.  asp.* / asp_bn.* are in it but never called (Conformer.py:144-148)
static void cf_block_spec(const std::string& p, std::map<std::string, std::vector<int64_t>>& spec) {
    const int64_t D = CF_D;
    auto ln = [&](const std::string& q) { spec[q + ".weight"] = {D}; spec[q + ".bias"] = {D}; };
    auto ff = [&](const std::string& q) {
        ln(q + "module.sequential.0");
        spec[q + "module.sequential.1.linear.weight"] = {4 * D, D}; spec[q + "module.sequential.1.linear.bias"] = {4 * D};
        spec[q + "module.sequential.4.linear.weight"] = {D, 4 * D}; spec[q + "module.sequential.4.linear.bias"] = {D};
    };
    ff(p + "sequential.0.");
    const std::string a = p + "sequential.1.module.";
    spec[a + "positional_encoding.pe"] = {1, CF_MAX_T, D};
    ln(a + "layer_norm");
    spec[a + "attention.u_bias"] = {4, 64}; spec[a + "attention.v_bias"] = {4, 64};
    for (const char* q : {"query_proj", "key_proj", "value_proj", "out_proj"}) {
        spec[a + "attention." + q + ".linear.weight"] = {D, D}; spec[a + "attention." + q + ".linear.bias"] = {D};
    }
    spec[a + "attention.pos_proj.linear.weight"] = {D, D};
    const std::string cv = p + "sequential.2.module.sequential.";
    ln(cv + "0");
    spec[cv + "2.conv.weight"] = {2 * D, D, 1}; spec[cv + "2.conv.bias"] = {2 * D};
    spec[cv + "4.conv.weight"] = {D, 1, 15};
    spec[cv + "5.weight"] = {D}; spec[cv + "5.bias"] = {D}; spec[cv + "5.running_mean"] = {D}; spec[cv + "5.running_var"] = {D};
    spec[cv + "5.num_batches_tracked"] = {};
    spec[cv + "7.conv.weight"] = {D, D, 1}; spec[cv + "7.conv.bias"] = {D};
    ff(p + "sequential.3.");
    ln(p + "sequential.4");
}
static void conformer_spec(const svhip_config& c, std::map<std::string, std::vector<int64_t>>& spec) {
    auto bn = [&](const std::string& p, int64_t n) {
        spec[p + ".weight"] = {n}; spec[p + ".bias"] = {n}; spec[p + ".running_mean"] = {n};
        spec[p + ".running_var"] = {n}; spec[p + ".num_batches_tracked"] = {};
    };
    const int64_t D = CF_D, nm = c.n_mels, F2 = cf_sub(cf_sub((int)nm)), nOut = c.embed_dim;
    spec["instance_norm.weight"] = {nm}; spec["instance_norm.bias"] = {nm};
    const std::string s = "conformer_block.conv_subsample.sequential.";
    spec[s + "0.weight"] = {D, 1, 3, 3}; spec[s + "0.bias"] = {D};
    spec[s + "2.weight"] = {D, D, 3, 3}; spec[s + "2.bias"] = {D};
    spec["conformer_block.input_projection.0.linear.weight"] = {D, D * F2}; spec["conformer_block.input_projection.0.linear.bias"] = {D};
    for (int i = 0; i < CF_LAYERS; ++i) cf_block_spec("conformer_block.layers." + std::to_string(i) + ".", spec);
    spec["asp.tdnn.conv.conv.weight"] = {128, 3 * D, 1}; spec["asp.tdnn.conv.conv.bias"] = {128};
    bn("asp.tdnn.norm.norm", 128);
    spec["asp.conv.weight"] = {D, 128, 1}; spec["asp.conv.bias"] = {D};
    bn("asp_bn.norm", 2 * D);
    spec["attention.0.weight"] = {128, D, 1}; spec["attention.0.bias"] = {128};
    bn("attention.2", 128);
    spec["attention.3.weight"] = {D, 128, 1}; spec["attention.3.bias"] = {D};
    bn("attention_norm", 2 * D);
    spec["fc.conv.weight"] = {nOut, 2 * D, 1}; spec["fc.conv.bias"] = {nOut};
}

void model_spec(const svhip_config& c, std::map<std::string, std::vector<int64_t>>& spec) {
    if (c.model == SVHIP_MODEL_ECAPA) ecapa_spec(c, spec);
    else if (is_rawnet2(c.model)) rawnet2_spec(c, spec);
    else if (c.model == SVHIP_MODEL_RAWNET3) rawnet3_spec(c, spec);
    else if (c.model == SVHIP_MODEL_TITANET) titanet_spec(c, spec);
    else if (c.model == SVHIP_MODEL_CONFORMER) conformer_spec(c, spec);
}

static const HostTensor* getw(svhip_handle* h, const std::string& name) {
    auto it = h->host_w.find(name);
    return it == h->host_w.end() ? nullptr : &it->second;
}

// fold BatchNorm1d(eval, eps=1e-5) into scale / shift (double arithmetic on the host)
static int make_bn(svhip_handle* h, const std::string& p, int n, float** scale, float** shift) {
    const HostTensor *w = getw(h, p + ".weight"), *b = getw(h, p + ".bias"), *rm = getw(h, p + ".running_mean"),
                     *rv = getw(h, p + ".running_var");
    if (!w || !b || !rm || !rv) SV_FAIL(h, SVHIP_ERR_MISSING, "missing BatchNorm tensors for %s", p.c_str());
    std::vector<float> sc(n), sh(n);
    for (int i = 0; i < n; ++i) {
        const double s = (double)w->data[i] / std::sqrt((double)rv->data[i] + 1e-5);
        sc[i] = (float)s;
        sh[i] = (float)((double)b->data[i] - (double)rm->data[i] * s);
    }
    int rc;
    if ((rc = dev_upload(h, scale, sc))) return rc;
    return dev_upload(h, shift, sh);
}

// pack conv weight (N, cin, taps) columns [c_lo, c_hi) -> [Np][Kp], k = tap*cin' + c
static int make_conv(svhip_handle* h, ConvLayer& L, const std::string& wname, const std::string& bname, const std::string& bnname,
                     int dil, int c_lo = 0, int c_hi = -1) {
    const HostTensor* w = getw(h, wname);
    if (!w) SV_FAIL(h, SVHIP_ERR_MISSING, "missing tensor %s", wname.c_str());
    const int N = (int)w->shape[0], cin_full = (int)w->shape[1], taps = w->shape.size() > 2 ? (int)w->shape[2] : 1;      // (a Linear: 1 tap)
    if (c_hi < 0) c_hi = cin_full;
    const int cin = c_hi - c_lo;
    const int bk = gemm_bk(h->bf16);
    L.N = N; L.taps = taps; L.dil = dil; L.cin = cin; L.K = taps * cin;
    L.Kp = round_up(L.K, bk); L.Np = round_up(N, GEMM_BN);
    L.flops_per_row = 2.0 * N * L.K;
    std::vector<float> packed((size_t)L.Np * L.Kp, 0.0f);
    for (int n = 0; n < N; ++n)
        for (int t = 0; t < taps; ++t)
            for (int c = 0; c < cin; ++c)
                packed[(size_t)n * L.Kp + t * cin + c] = w->data[((size_t)n * cin_full + (c_lo + c)) * taps + t];
    int rc;
    if (h->bf16) {
        std::vector<uint16_t> pb(packed.size());
        for (size_t i = 0; i < packed.size(); ++i) pb[i] = to_h16(h, packed[i]);
        uint16_t* d;
        if ((rc = dev_upload(h, &d, pb))) return rc;
        L.W = d;
    } else {
        float* d;
        if ((rc = dev_upload(h, &d, packed))) return rc;
        L.W = d;
        if (h->x3) {
            std::vector<uint32_t> ws(packed.size());
            for (size_t i = 0; i < packed.size(); ++i) ws[i] = x3_split_word(packed[i]);      // (hi plane << 16) | lo plane, x3_t of common.h
            uint32_t* dsplit;
            if ((rc = dev_upload(h, &dsplit, ws))) return rc;
            L.Wsplit = dsplit;
            // pointwise GELU layers (gemm_pw3's X3 form) and the Res2Net convolutions (its R2 form: N == cin, k = 3)
            if ((taps == 1 && N % 256 == 0 && L.K == L.Kp && L.K % 64 == 0 && L.K >= 128) ||
                (taps == 3 && N == cin && (cin == 64 || cin == 128) && L.K == L.Kp) ||
                // RawNet2's convolutions and projection shortcuts (r2_step.hip, modes 1 / 2)
                (is_rawnet2(h->cfg.model) && (taps == 1 || taps == 3) && N % 128 == 0 && cin % 32 == 0 && L.K == L.Kp && L.K == taps * cin)) {
                std::vector<uint16_t> s32((size_t)N * L.K * 2);
                for (int n = 0; n < N; ++n)
                    for (int k = 0; k < L.K; ++k) {
                        const uint32_t wv = ws[(size_t)n * L.Kp + k];
                        const size_t o = (size_t)n * L.K * 2 + (size_t)(k >> 5) * 64 + (k & 31);
                        s32[o] = (uint16_t)(wv >> 16);
                        s32[o + 32] = (uint16_t)(wv & 0xffffu);
                    }
                uint16_t* d32;
                if ((rc = dev_upload(h, &d32, s32))) return rc;
                L.Ws32 = d32;
            }
            if (taps >= 3 && taps <= 7 && (taps & 1) && N % 256 == 0 && N != cin) {      // the conv-gather X3 form (gemm_pw3cv)
                const int ccv = round_up(cin, 32), kcv = round_up(taps * ccv, 64);
                // the first convolution of the network meets features of whatever magnitude the checkpoint was trained on: weights fitted to
                // int16-scaled mel power are ~1e-10 — below the half planes' resolution.  Outside the ordinary range the planes hold sw * W,
                // sw an exact power of two (max |w| -> [64, 128)); the kernel multiplies back together with the input's scale (GemmParams::in_scale)
                float wmax = 0.0f;
                for (int n = 0; n < N; ++n)
                    for (int k = 0; k < L.K; ++k) { const float a = std::fabs(packed[(size_t)n * L.Kp + k]); if (std::isfinite(a) && a > wmax) wmax = a; }
                float sw = 1.0f;
                if (wmax > 0.0f && !(wmax >= 0x1p-8f && wmax < 0x1p13f)) { int e2; (void)std::frexp(wmax, &e2); sw = std::ldexp(1.0f, 7 - e2); }
                L.cv_wscale = sw;
                std::vector<uint16_t> s32((size_t)N * kcv * 2, 0);
                for (int n = 0; n < N; ++n)
                    for (int t = 0; t < taps; ++t)
                        for (int c = 0; c < cin; ++c) {
                            const uint32_t wv = sw == 1.0f ? ws[(size_t)n * L.Kp + t * cin + c] : x3_split_word(packed[(size_t)n * L.Kp + t * cin + c] * sw);
                            const int k = t * ccv + c;
                            const size_t o = (size_t)n * kcv * 2 + (size_t)(k >> 5) * 64 + (k & 31);
                            s32[o] = (uint16_t)(wv >> 16);
                            s32[o + 32] = (uint16_t)(wv & 0xffffu);
                        }
                uint16_t* dcv;
                if ((rc = dev_upload(h, &dcv, s32))) return rc;
                L.Wcv = dcv; L.cv_cin = ccv; L.cv_Kp = kcv;
            }
        }
    }
    if (!bname.empty()) {
        const HostTensor* b = getw(h, bname);
        if (!b) SV_FAIL(h, SVHIP_ERR_MISSING, "missing tensor %s", bname.c_str());
        if ((rc = dev_upload(h, &L.bias, b->data))) return rc;
    }
    if (!bnname.empty()) return make_bn(h, bnname, N, &L.scale, &L.shift);
    return SVHIP_OK;
}

static int make_tdnn(svhip_handle* h, ConvLayer& L, const std::string& p, int dil) {
    return make_conv(h, L, p + ".conv.conv.weight", p + ".conv.conv.bias", p + ".norm.norm", dil);
}

// fp32 linear from a (N, K, 1) or (N, K) tensor, optional column range
static int make_linear(svhip_handle* h, LinearLayer& L, const std::string& wname, const std::string& bname, int c_lo = 0, int c_hi = -1) {
    const HostTensor* w = getw(h, wname);
    if (!w) SV_FAIL(h, SVHIP_ERR_MISSING, "missing tensor %s", wname.c_str());
    const int N = (int)w->shape[0], Kfull = (int)w->shape[1];
    if (c_hi < 0) c_hi = Kfull;
    L.N = N; L.K = c_hi - c_lo;
    std::vector<float> m((size_t)N * L.K);
    for (int n = 0; n < N; ++n)
        for (int k = 0; k < L.K; ++k) m[(size_t)n * L.K + k] = w->data[(size_t)n * Kfull + c_lo + k];
    int rc;
    if ((rc = dev_upload(h, &L.W, m))) return rc;
    if (!bname.empty()) {
        const HostTensor* b = getw(h, bname);
        if (!b) SV_FAIL(h, SVHIP_ERR_MISSING, "missing tensor %s", bname.c_str());
        if ((rc = dev_upload(h, &L.bias, b->data))) return rc;
    }
    return SVHIP_OK;
}

int finalize_ecapa(svhip_handle* h) {
    const int C = h->cfg.channels, C3 = 3 * C;
    int rc;
    if ((rc = make_tdnn(h, h->blocks0, "blocks.0", ECAPA_D[0]))) return rc;
    for (int i = 1; i <= 3; ++i) {
        const std::string p = "blocks." + std::to_string(i);
        if ((rc = make_tdnn(h, h->tdnn1[i - 1], p + ".tdnn1", 1))) return rc;
        for (int j = 0; j < 7; ++j)
            if ((rc = make_tdnn(h, h->res2[i - 1][j], p + ".res2net_block.blocks." + std::to_string(j), ECAPA_D[i]))) return rc;
        if ((rc = make_tdnn(h, h->tdnn2[i - 1], p + ".tdnn2", 1))) return rc;
        if ((rc = make_linear(h, h->se1[i - 1], p + ".se_block.conv1.conv.weight", p + ".se_block.conv1.conv.bias"))) return rc;
        if ((rc = make_linear(h, h->se2[i - 1], p + ".se_block.conv2.conv.weight", p + ".se_block.conv2.conv.bias"))) return rc;
        {
            const HostTensor* w2 = getw(h, p + ".se_block.conv2.conv.weight");      // (C, 128, 1)
            std::vector<float> t((size_t)128 * C);
            for (int c = 0; c < C; ++c)
                for (int n = 0; n < 128; ++n) t[(size_t)n * C + c] = w2->data[(size_t)c * 128 + n];
            if ((rc = dev_upload(h, &h->se2T[i - 1], t))) return rc;
            if (h->bf16) {
                const HostTensor* w1 = getw(h, p + ".se_block.conv1.conv.weight");  // (128, C, 1)
                std::vector<uint16_t> b1v((size_t)128 * C), b2v((size_t)128 * C);
                for (size_t k = 0; k < b1v.size(); ++k) { b1v[k] = f32_to_bf16_rne(w1->data[k]); b2v[k] = f32_to_bf16_rne(t[k]); }
                for (int which = 0; which < 2; ++which) {
                    void* d = nullptr;
                    SV_HIP(h, hipMalloc(&d, b1v.size() * 2));
                    h->allocs.push_back(d);
                    SV_HIP(h, hipMemcpy(d, which ? b2v.data() : b1v.data(), b1v.size() * 2, hipMemcpyHostToDevice));
                    (which ? h->se2T_bf[i - 1] : h->se1_bf[i - 1]) = d;
                }
            }
        }
    }
    if ((rc = make_tdnn(h, h->mfa, "mfa", 1))) return rc;
    // asp.tdnn over cat[x, mean, std]: the x columns go through the GEMM, the time-constant columns
    // become a per-utterance bias (ctx) computed by a small linear layer.
    if ((rc = make_conv(h, h->asp_tdnn, "asp.tdnn.conv.conv.weight", "", "asp.tdnn.norm.norm", 1, 0, C3))) return rc;
    if ((rc = make_linear(h, h->asp_ctx, "asp.tdnn.conv.conv.weight", "asp.tdnn.conv.conv.bias", C3, 3 * C3))) return rc;
    if ((rc = make_conv(h, h->asp_conv, "asp.conv.conv.weight", "asp.conv.conv.bias", "", 1))) return rc;
    if ((rc = make_bn(h, "asp_bn.norm", 2 * C3, &h->aspbn_scale, &h->aspbn_shift))) return rc;
    if ((rc = make_linear(h, h->fc, "fc.conv.weight", "fc.conv.bias"))) return rc;
    if (h->cfg.input_norm) {
        const HostTensor *w = getw(h, "instance_norm.weight"), *b = getw(h, "instance_norm.bias");
        if (!w || !b) SV_FAIL(h, SVHIP_ERR_MISSING, "missing instance_norm tensors");
        if ((rc = dev_upload(h, &h->in_w, w->data))) return rc;
        if ((rc = dev_upload(h, &h->in_b, b->data))) return rc;
    }
    // algorithmic FLOPs per utterance: 2 x MACs of every conv / linear (SURVEY §8d counts the same)
    const double T = h->T;
    double f = T * h->blocks0.flops_per_row + T * h->mfa.flops_per_row + T * h->asp_conv.flops_per_row;
    f += T * 2.0 * 128 * (3.0 * C3);                                  // asp.tdnn over the full 9C input, as the reference computes it
    for (int i = 0; i < 3; ++i) {
        f += T * (h->tdnn1[i].flops_per_row + h->tdnn2[i].flops_per_row);
        for (int j = 0; j < 7; ++j) f += T * h->res2[i][j].flops_per_row;
        f += 2.0 * h->se1[i].N * h->se1[i].K + 2.0 * h->se2[i].N * h->se2[i].K;
    }
    f += 2.0 * h->fc.N * h->fc.K;
    h->flops_per_utt = f;
    return SVHIP_OK;
}

static int upload_f32(svhip_handle* h, const std::string& name, float** dst) {
    const HostTensor* t = getw(h, name);
    if (!t) SV_FAIL(h, SVHIP_ERR_MISSING, "missing tensor %s", name.c_str());
    return dev_upload(h, dst, t->data);
}

// sinc band-pass filters baked once per weight load (RawNet_baseline.py:313-318,339-357), float32 arithmetic
static int bake_sinc(svhip_handle* h) {
    const HostTensor *lo = getw(h, "first_conv.low_hz_"), *bd = getw(h, "first_conv.band_hz_");
    if (!lo || !bd) SV_FAIL(h, SVHIP_ERR_MISSING, "missing sinc parameters");
    const int NF = 128, KS = 251, HALF = 125;
    const float sr = 16000.0f, min_low = 50.0f, min_band = 50.0f;
    const float PI = 3.14159265358979323846f;
    std::vector<float> win(HALF), n_(HALF);
    for (int i = 0; i < HALF; ++i) {
        const float n_lin = (float)(124.5 * i / 124.0);                         // torch.linspace(0, 124.5, 125)
        win[i] = 0.54f - 0.46f * std::cos(2.0f * PI * n_lin / (float)KS);
        n_[i] = 2.0f * PI * (float)(-125 + i) / sr;                             // 2*pi*arange(-125, 0)/16000
    }
    std::vector<float> filt((size_t)NF * KS);
    for (int f = 0; f < NF; ++f) {
        const float low = min_low + std::fabs(lo->data[f]);
        float high = low + min_band + std::fabs(bd->data[f]);
        high = std::fmin(std::fmax(high, min_low), sr / 2);
        const float band = high - low;
        for (int i = 0; i < HALF; ++i) {
            const float left = ((std::sin(high * n_[i]) - std::sin(low * n_[i])) / (n_[i] / 2.0f)) * win[i];
            filt[(size_t)f * KS + i] = left / (2.0f * band);
            filt[(size_t)f * KS + (KS - 1 - i)] = left / (2.0f * band);
        }
        filt[(size_t)f * KS + HALF] = (2.0f * band) / (2.0f * band);
    }
    int rc;
    if (h->bf16) {
        std::vector<uint16_t> pk((size_t)NF * 256, 0);
        for (int f = 0; f < NF; ++f)
            for (int k = 0; k < KS; ++k) pk[(size_t)f * 256 + k] = to_h16(h, filt[(size_t)f * KS + k]);
        uint16_t* d;
        if ((rc = dev_upload(h, &d, pk))) return rc;
        h->rn_filt = d;
        if (h->f16) {
            // the symmetric form (rawnet2.hip, SYM): slot k' = 2 + m carries h[125 + m] (the centre tap halved: its operand is x[c] + x[c]),
            // slots 0 and 1 are zero; right and left halves of a filter are the same numbers by construction (checked here)
            bool symmetric = true;
            for (int f = 0; f < NF && symmetric; ++f)
                for (int i = 0; i < HALF; ++i) symmetric = symmetric && filt[(size_t)f * KS + i] == filt[(size_t)f * KS + (KS - 1 - i)];
            if (symmetric) {
                std::vector<uint16_t> ps((size_t)NF * 128, 0);
                for (int f = 0; f < NF; ++f) {
                    ps[(size_t)f * 128 + 2] = to_h16(h, 0.5f * filt[(size_t)f * KS + HALF]);
                    for (int m = 1; m <= HALF; ++m) ps[(size_t)f * 128 + 2 + m] = to_h16(h, filt[(size_t)f * KS + HALF + m]);
                }
                uint16_t* ds;
                if ((rc = dev_upload(h, &ds, ps))) return rc;
                h->rn_filt_sym = ds;
            }
        }
    } else {
        std::vector<float> pk((size_t)NF * 252, 0.0f);
        for (int f = 0; f < NF; ++f)
            for (int k = 0; k < KS; ++k) pk[(size_t)f * 252 + k] = filt[(size_t)f * KS + k];
        float* d;
        if ((rc = dev_upload(h, &d, pk))) return rc;
        h->rn_filt = d;
        if (h->x3) {        // the split front-end (rn_sinc_x3): hi and lo half planes, k contiguous, zero beyond the 251 taps
            std::vector<uint16_t> pl((size_t)2 * NF * 256, 0);
            for (int f = 0; f < NF; ++f)
                for (int k = 0; k < KS; ++k) {
                    const uint32_t w = x3_split_word(filt[(size_t)f * KS + k]);
                    pl[(size_t)f * 256 + k] = (uint16_t)(w >> 16);
                    pl[(size_t)(NF + f) * 256 + k] = (uint16_t)(w & 0xffffu);
                }
            uint16_t* dx;
            if ((rc = dev_upload(h, &dx, pl))) return rc;
            h->rn_filt_x3 = dx;
        }
    }
    return SVHIP_OK;
}

// the 'conv' front-end's constants: conv1.weight (128, 1, 3) and conv1.bias as [w0 | w1 | w2 | bias] x 128 floats
static int make_conv3_front(svhip_handle* h) {
    const HostTensor *w = getw(h, "conv1.weight"), *b = getw(h, "conv1.bias");
    if (!w || !b) SV_FAIL(h, SVHIP_ERR_MISSING, "missing tensor %s", !w ? "conv1.weight" : "conv1.bias");
    std::vector<float> cw(4 * 128);
    for (int c = 0; c < 128; ++c) {
        for (int k = 0; k < 3; ++k) cw[k * 128 + c] = w->data[c * 3 + k];
        cw[3 * 128 + c] = b->data[c];
    }
    return dev_upload(h, &h->rn_cw, cw);
}

// aggregate='gru' (RawNet2_custom.py:84-95,196-207): bn_before_gru is the pass block 7's AFMS pass applies (rn_agg_scale / shift); the input
// projection W_ih is a 1 x 1 conv layer whose bias folds b_ih + [b_hr | b_hz | 0] (b_hn stays inside r * (W_hn h + b_hn)); W_hh is packed
// gate-interleaved (gru.hip) in the compute type; fc_after_gru is a small linear.  fc.* is loaded and not used, as in the reference.
static int finalize_rawnet2_gru(svhip_handle* h) {
    const int H = RN_GRU_HIDDEN, G = 3 * H;
    int rc;
    if ((rc = make_bn(h, "bn_before_gru", 512, &h->rn_agg_scale, &h->rn_agg_shift))) return rc;
    const HostTensor *whh = getw(h, "gru.weight_hh_l0"), *bih = getw(h, "gru.bias_ih_l0"), *bhh = getw(h, "gru.bias_hh_l0");
    if (!whh || !bih || !bhh) SV_FAIL(h, SVHIP_ERR_MISSING, "missing GRU tensors (gru.weight_hh_l0, gru.bias_ih_l0, gru.bias_hh_l0)");
    if ((rc = make_conv(h, h->rn_gru_ih, "gru.weight_ih_l0", "", "", 1))) return rc;
    std::vector<float> bias(G), bhn(H);
    for (int j = 0; j < G; ++j) bias[j] = j < 2 * H ? (float)((double)bih->data[j] + (double)bhh->data[j]) : bih->data[j];
    for (int j = 0; j < H; ++j) bhn[j] = bhh->data[2 * H + j];
    if ((rc = dev_upload(h, &h->rn_gru_ih.bias, bias))) return rc;
    if ((rc = dev_upload(h, &h->rn_gru_bhn, bhn))) return rc;
    // packed row ut * 48 + g * 16 + j = W_hh row g * H + ut * 16 + j
    std::vector<float> pk((size_t)G * H);
    for (int ut = 0; ut < H / 16; ++ut)
        for (int g = 0; g < 3; ++g)
            for (int j = 0; j < 16; ++j)
                memcpy(&pk[((size_t)ut * 48 + g * 16 + j) * H], &whh->data[((size_t)g * H + ut * 16 + j) * H], (size_t)H * 4);
    if (h->bf16) {
        std::vector<uint16_t> pb(pk.size());
        for (size_t i = 0; i < pk.size(); ++i) pb[i] = to_h16(h, pk[i]);
        uint16_t* d;
        if ((rc = dev_upload(h, &d, pb))) return rc;
        h->rn_gru_whh = d;
    } else {
        float* d;
        if ((rc = dev_upload(h, &d, pk))) return rc;
        h->rn_gru_whh = d;
    }
    return make_linear(h, h->rn_gru_fc, "fc_after_gru.weight", "fc_after_gru.bias");
}

int finalize_rawnet2(svhip_handle* h) {
    int rc;
    const bool conv = h->cfg.model == SVHIP_MODEL_RAWNET2_CONV;
    if (conv) {
        if ((rc = make_conv3_front(h))) return rc;
    } else {
        if ((rc = upload_f32(h, "ln.gamma", &h->rn_gamma))) return rc;
        if ((rc = upload_f32(h, "ln.beta", &h->rn_beta))) return rc;
        if ((rc = bake_sinc(h))) return rc;
        if ((rc = make_bn(h, "first_bn", 128, &h->rn_fbn_scale, &h->rn_fbn_shift))) return rc;
    }
    int inpl = 128, bi = 0;
    int T = h->rn_T1;
    double fl = conv ? 2.0 * 128 * 3 * (double)T : 2.0 * 128 * 251 * (double)(h->cfg.samples - 250);
    for (int li = 0; li < 6; ++li)
        for (int b = 0; b < RN_LAYERS[li]; ++b, ++bi) {
            svhip_handle::RnBlock& B = h->rn_blocks[bi];
            const std::string p = "layer" + std::to_string(li + 1) + "." + std::to_string(b);
            const int planes = RN_FILTERS[li];
            B.cin = inpl; B.cout = planes; B.downsample = (b == RN_LAYERS[li] - 1); B.has_shortcut = inpl != planes;
            if ((rc = make_bn(h, p + ".bn1", inpl, &B.bn1_scale, &B.bn1_shift))) return rc;
            if ((rc = make_conv(h, B.conv1, p + ".conv1.weight", "", p + ".bn2", 1))) return rc;
            if ((rc = make_conv(h, B.conv2, p + ".conv2.weight", "", "", 1))) return rc;
            if (B.has_shortcut && (rc = make_conv(h, B.shortcut, p + ".shortcut.0.weight", "", "", 1))) return rc;
            if (B.has_shortcut && h->bf16 && B.conv2.K % 64 == 0 && inpl % 64 == 0) {
                // conv2 and the shortcut share their output: [conv2 columns (tap-major) | shortcut columns] as one K axis
                const HostTensor* w2 = getw(h, p + ".conv2.weight");           // (planes, planes, 3)
                const HostTensor* ws = getw(h, p + ".shortcut.0.weight");      // (planes, inpl, 1)
                const int K2 = B.conv2.K, Kt = K2 + inpl, Np = B.conv2.Np;
                std::vector<uint16_t> pk((size_t)Np * Kt, 0);
                for (int n = 0; n < planes; ++n) {
                    for (int t = 0; t < 3; ++t)
                        for (int c = 0; c < planes; ++c) pk[(size_t)n * Kt + t * planes + c] = to_h16(h, w2->data[((size_t)n * planes + c) * 3 + t]);
                    for (int c = 0; c < inpl; ++c) pk[(size_t)n * Kt + K2 + c] = to_h16(h, ws->data[(size_t)n * inpl + c]);
                }
                uint16_t* d;
                if ((rc = dev_upload(h, &d, pk))) return rc;
                B.conv2sc_W = d;
            }
            if ((rc = upload_f32(h, p + ".afms.alpha", &B.alpha))) return rc;
            if ((rc = make_linear(h, B.afms_fc, p + ".afms.fc.weight", p + ".afms.fc.bias"))) return rc;
            {
                const HostTensor* fw = getw(h, p + ".afms.fc.weight");                  // (planes, planes)
                std::vector<float> t((size_t)planes * planes);
                for (int n = 0; n < planes; ++n)
                    for (int c = 0; c < planes; ++c) t[(size_t)c * planes + n] = fw->data[(size_t)n * planes + c];
                if ((rc = dev_upload(h, &B.afms_fcT, t))) return rc;
            }
            fl += (double)T * (B.conv1.flops_per_row + B.conv2.flops_per_row + (B.has_shortcut ? B.shortcut.flops_per_row : 0.0));
            fl += 2.0 * planes * planes;
            if (B.downsample) T /= 3;
            inpl = planes;
        }
    if (rn_is_gru(h->cfg.model)) {
        if ((rc = finalize_rawnet2_gru(h))) return rc;
        fl += (double)T * (h->rn_gru_ih.flops_per_row + 2.0 * 3 * RN_GRU_HIDDEN * RN_GRU_HIDDEN) + 2.0 * h->rn_gru_fc.N * h->rn_gru_fc.K;
        h->flops_per_utt = fl;
        return SVHIP_OK;
    }
    if ((rc = make_bn(h, "bn_before_agg", 512, &h->rn_agg_scale, &h->rn_agg_shift))) return rc;
    if ((rc = make_conv(h, h->rn_att0, "attention.0.weight", "attention.0.bias", "attention.2", 1))) return rc;
    if ((rc = make_conv(h, h->rn_att3, "attention.3.weight", "attention.3.bias", "", 1))) return rc;
    if ((rc = make_linear(h, h->rn_fc, "fc.weight", "fc.bias"))) return rc;
    fl += (double)T * (h->rn_att0.flops_per_row + h->rn_att3.flops_per_row) + 2.0 * h->rn_fc.N * h->rn_fc.K;
    h->flops_per_utt = fl;
    return SVHIP_OK;
}

// ParamSincFB(256, 251).filters() (asteroid-filterbanks 0.4; its cos half is RawNet_baseline.py:339-357's formula) from the
// checkpoint's low_hz_, band_hz_, window_ and n_, in fp64, stored tap-major [251][256]: cos filters 0..127, sin filters 128..255
static int bake_sinc3(svhip_handle* h) {
    const HostTensor *lo = getw(h, "conv1.filterbank.low_hz_"), *bd = getw(h, "conv1.filterbank.band_hz_"),
                     *win = getw(h, "conv1.filterbank.window_"), *nn = getw(h, "conv1.filterbank.n_");
    if (!lo || !bd || !win || !nn) SV_FAIL(h, SVHIP_ERR_MISSING, "missing conv1.filterbank tensors");
    const int NF = RN3_FILTERS / 2, HK = 125;
    std::vector<double> f((size_t)RN3_TAPS * RN3_FILTERS);
    for (int i = 0; i < NF; ++i) {
        const double low = 50.0 + std::fabs((double)lo->data[i]);
        const double high = std::min(std::max(low + 50.0 + std::fabs((double)bd->data[i]), 50.0), 8000.0);
        const double band = high - low;
        for (int k = 0; k < HK; ++k) {
            const double n = nn->data[k], w = win->data[k];
            const double c = (std::sin(high * n) - std::sin(low * n)) / (n / 2) * w;     // cos half, left side
            const double s = (std::cos(low * n) - std::cos(high * n)) / (n / 2) * w;     // sin half, left side
            f[(size_t)k * RN3_FILTERS + i] = c / (2 * band);
            f[(size_t)(RN3_TAPS - 1 - k) * RN3_FILTERS + i] = c / (2 * band);
            f[(size_t)k * RN3_FILTERS + NF + i] = s / (2 * band);
            f[(size_t)(RN3_TAPS - 1 - k) * RN3_FILTERS + NF + i] = -s / (2 * band);
        }
        f[(size_t)HK * RN3_FILTERS + i] = 2 * band / (2 * band);
        f[(size_t)HK * RN3_FILTERS + NF + i] = 0.0;
    }
    if (!h->bf16) {
        double* d;
        int rc = dev_upload(h, &d, f);
        h->rn3_filt = d;
        return rc;
    }
    std::vector<float> ff(f.begin(), f.end());
    float* d;
    int rc = dev_upload(h, &d, ff);
    h->rn3_filt = d;
    return rc;
}

int finalize_rawnet3(svhip_handle* h) {
    int rc;
    const HostTensor* pf = getw(h, "preprocess.0.flipped_filter");
    if (!pf) SV_FAIL(h, SVHIP_ERR_MISSING, "missing tensor preprocess.0.flipped_filter");
    h->rn3_pre[0] = pf->data[0]; h->rn3_pre[1] = pf->data[1];
    if ((rc = upload_f32(h, "preprocess.1.weight", &h->rn3_in_w))) return rc;
    if ((rc = upload_f32(h, "preprocess.1.bias", &h->rn3_in_b))) return rc;
    if ((rc = bake_sinc3(h))) return rc;
    const int T0 = h->rn3_T0;
    double fl = 2.0 * RN3_FILTERS * RN3_TAPS * T0;
    const int dil[3] = {2, 3, 4}, pool[3] = {5, 3, 1};
    int T = T0;
    for (int li = 0; li < 3; ++li) {
        svhip_handle::Rn3Layer& Ly = h->rn3[li];
        const std::string p = "layer" + std::to_string(li + 1);
        if ((rc = make_conv(h, Ly.conv1, p + ".conv1.weight", p + ".conv1.bias", p + ".bn1", 1))) return rc;
        for (int i = 0; i < 7; ++i)
            if ((rc = make_conv(h, Ly.convs[i], p + ".convs." + std::to_string(i) + ".weight", p + ".convs." + std::to_string(i) + ".bias",
                                p + ".bns." + std::to_string(i), dil[li]))) return rc;
        if ((rc = make_conv(h, Ly.conv3, p + ".conv3.weight", p + ".conv3.bias", p + ".bn3", 1))) return rc;
        Ly.has_residual = li == 0;
        if (Ly.has_residual && (rc = make_conv(h, Ly.residual, p + ".residual.0.weight", "", "", 1))) return rc;
        if ((rc = upload_f32(h, p + ".afms.alpha", &Ly.alpha))) return rc;
        if ((rc = make_linear(h, Ly.afms_fc, p + ".afms.fc.weight", p + ".afms.fc.bias"))) return rc;
        double per_row = Ly.conv1.flops_per_row + 7 * Ly.convs[0].flops_per_row + Ly.conv3.flops_per_row + (Ly.has_residual ? Ly.residual.flops_per_row : 0.0);
        fl += (double)T * per_row + 2.0 * 1024 * 1024;
        T /= pool[li];
    }
    if ((rc = make_conv(h, h->rn3_l4, "layer4.weight", "layer4.bias", "", 1))) return rc;
    if ((rc = make_conv(h, h->rn3_att, "attention.0.weight", "", "attention.2", 1, 0, 1536))) return rc;
    if ((rc = make_linear(h, h->rn3_att_ctx, "attention.0.weight", "attention.0.bias", 1536, 3 * 1536))) return rc;
    if ((rc = upload_f32(h, "attention.3.weight", &h->rn3_w2))) return rc;
    if ((rc = upload_f32(h, "attention.3.bias", &h->rn3_b2))) return rc;
    if ((rc = make_bn(h, "bn5", 2 * 1536, &h->rn3_bn5_scale, &h->rn3_bn5_shift))) return rc;
    if ((rc = make_linear(h, h->rn3_fc6, "fc6.weight", "fc6.bias"))) return rc;
    fl += (double)T * (h->rn3_l4.flops_per_row + h->rn3_att.flops_per_row + 2.0 * 128) + 2.0 * 128 * 3072 + 2.0 * h->rn3_fc6.N * h->rn3_fc6.K;
    h->flops_per_utt = fl;
    return SVHIP_OK;
}

// ---- TitaNet ---------------------------------------------------------------------------------------------
int titanet_blocks_loaded(const svhip_handle* h) {
    int n = 0;
    while (n < SVHIP_TITANET_MAX_BLOCKS) {
        const std::string p = "encoder.mega_blocks." + std::to_string(n) + ".";
        auto it = h->host_w.lower_bound(p);
        if (it == h->host_w.end() || it->first.compare(0, p.size(), p) != 0) break;
        ++n;
    }
    return n;
}

// conv (N, cin, taps) + bias followed directly by BatchNorm1d(eval, eps 1e-5): the BN folded into the conv, W' = s W, b' = s b + t (double
// arithmetic on the host), packed as a plain conv layer
static int make_conv_bn(svhip_handle* h, ConvLayer& L, const std::string& conv, const std::string& bnp) {
    const HostTensor *w = getw(h, conv + ".weight"), *b = getw(h, conv + ".bias");
    const HostTensor *g = getw(h, bnp + ".weight"), *be = getw(h, bnp + ".bias"), *rm = getw(h, bnp + ".running_mean"), *rv = getw(h, bnp + ".running_var");
    if (!w || !b) SV_FAIL(h, SVHIP_ERR_MISSING, "missing tensor %s.%s", conv.c_str(), !w ? "weight" : "bias");
    if (!g || !be || !rm || !rv) SV_FAIL(h, SVHIP_ERR_MISSING, "missing BatchNorm tensors for %s", bnp.c_str());
    const int64_t N = w->shape[0], per = w->numel() / N;
    HostTensor fw = *w, fb = *b;
    for (int64_t n = 0; n < N; ++n) {
        const double sc = (double)g->data[n] / std::sqrt((double)rv->data[n] + 1e-5);
        for (int64_t i = 0; i < per; ++i) fw.data[n * per + i] = (float)(sc * (double)w->data[n * per + i]);
        fb.data[n] = (float)(sc * (double)b->data[n] + ((double)be->data[n] - (double)rm->data[n] * sc));
    }
    const std::string fwn = "#fold." + conv + ".weight", fbn = "#fold." + conv + ".bias";
    h->host_w[fwn] = std::move(fw);
    h->host_w[fbn] = std::move(fb);
    int rc = make_conv(h, L, fwn, fbn, "", 1);
    h->host_w.erase(fwn);
    h->host_w.erase(fbn);
    L.scale = h->d_ones;          // (an identity affine: the persistent 16-bit GEMM takes layers that carry all three vectors)
    L.shift = h->d_zeros;
    return rc;
}

// a [rows][cols] fp32 matrix in the handle's storage type (bf16 handles: bf16, else null)
static int upload_h16(svhip_handle* h, const std::vector<float>& m, void** dst) {
    std::vector<uint16_t> v(m.size());
    for (size_t i = 0; i < m.size(); ++i) v[i] = f32_to_bf16_rne(m[i]);
    uint16_t* d;
    int rc = dev_upload(h, &d, v);
    *dst = d;
    return rc;
}

int finalize_titanet(svhip_handle* h) {
    const svhip_config& c = h->cfg;
    const int H = c.channels, k = tn_kernel_size(H), Hh = H / 16, D = 1536, nOut = c.embed_dim, T = h->T;
    const int nb = titanet_blocks_loaded(h);
    if (nb == 0) SV_FAIL(h, SVHIP_ERR_MISSING, "no mega-block was loaded (encoder.mega_blocks.0.*)");
    for (auto& kv : h->host_w)          // a gap: tensors of a block beyond the contiguous run
        if (kv.first.rfind("encoder.mega_blocks.", 0) == 0 && atoi(kv.first.c_str() + 20) >= nb)
            SV_FAIL(h, SVHIP_ERR_MISSING, "%s is loaded but mega-block %d is missing (blocks are counted contiguously from 0)", kv.first.c_str(), nb);
    {
        std::map<std::string, std::vector<int64_t>> bspec;
        for (int i = 0; i < nb; ++i) tn_block_spec(H, k, "encoder.mega_blocks." + std::to_string(i) + ".", bspec);
        for (auto& kv : bspec)
            if (!h->host_w.count(kv.first) && kv.first.find("num_batches_tracked") == std::string::npos)
                SV_FAIL(h, SVHIP_ERR_MISSING, "tensor %s was never loaded (mega-block count %d)", kv.first.c_str(), nb);
    }
    h->tn_k = k;
    h->tn.assign(nb, svhip_handle::TnBlock{});
    int rc;
    if ((rc = make_conv_bn(h, h->tn_prolog, "encoder.prolog.conv_block.0", "encoder.prolog.conv_block.1"))) return rc;
    double fl = h->tn_prolog.flops_per_row;
    for (int i = 0; i < nb; ++i) {
        svhip_handle::TnBlock& Bk = h->tn[i];
        const std::string p = "encoder.mega_blocks." + std::to_string(i) + ".";
        for (int j = 0; j < 3; ++j) {
            const std::string q = p + "sub_blocks." + std::to_string(j) + ".conv_block.";
            const HostTensor* dw = getw(h, q + "0.conv.0.weight");            // (H, 1, k)
            if (!dw || dw->shape.size() != 3 || dw->shape[2] != k) SV_FAIL(h, SVHIP_ERR_INVALID, "%s0.conv.0.weight: depthwise kernel size must be %d", q.c_str(), k);
            std::vector<float> tw((size_t)k * H);
            for (int cch = 0; cch < H; ++cch)
                for (int t = 0; t < k; ++t) tw[(size_t)t * H + cch] = dw->data[(size_t)cch * k + t];
            if ((rc = dev_upload(h, &Bk.dw_w[j], tw))) return rc;
            if ((rc = upload_f32(h, q + "0.conv.0.bias", &Bk.dw_b[j]))) return rc;
            if ((rc = make_conv_bn(h, Bk.pw[j], q + "0.conv.1", q + "1"))) return rc;
            fl += Bk.pw[j].flops_per_row + 2.0 * k * H;
        }
        if ((rc = make_conv_bn(h, Bk.skip, p + "skip_connection.0", p + "skip_connection.1"))) return rc;
        fl += Bk.skip.flops_per_row;
        const HostTensor *w1 = getw(h, p + "sub_blocks.3.excitation.0.weight"), *w2 = getw(h, p + "sub_blocks.3.excitation.2.weight");
        std::vector<float> m1(w1->data), m2((size_t)Hh * H);
        for (int cch = 0; cch < H; ++cch)
            for (int n = 0; n < Hh; ++n) m2[(size_t)n * H + cch] = w2->data[(size_t)cch * Hh + n];
        if ((rc = dev_upload(h, &Bk.se1, m1))) return rc;
        if ((rc = dev_upload(h, &Bk.se2T, m2))) return rc;
        if (h->bf16) {
            if ((rc = upload_h16(h, m1, &Bk.se1_bf))) return rc;
            if ((rc = upload_h16(h, m2, &Bk.se2T_bf))) return rc;
        }
    }
    if ((rc = make_conv_bn(h, h->tn_epilog, "encoder.epilog.conv_block.0", "encoder.epilog.conv_block.1"))) return rc;
    if ((rc = make_conv(h, h->tn_att_in, "decoder.pool.0.in_linear.weight", "decoder.pool.0.in_linear.bias", "", 1))) return rc;
    if ((rc = make_conv(h, h->tn_att_out, "decoder.pool.0.out_linear.weight", "decoder.pool.0.out_linear.bias", "", 1))) return rc;
    if ((rc = make_bn(h, "decoder.pool.1", 2 * D, &h->tn_pbn_scale, &h->tn_pbn_shift))) return rc;
    {
        // decoder.linear = Linear(3072, nOut) + BatchNorm1d(nOut): folded into one fp32 linear
        const HostTensor *w = getw(h, "decoder.linear.0.weight"), *b = getw(h, "decoder.linear.0.bias");
        const HostTensor *g = getw(h, "decoder.linear.1.weight"), *be = getw(h, "decoder.linear.1.bias");
        const HostTensor *rm = getw(h, "decoder.linear.1.running_mean"), *rv = getw(h, "decoder.linear.1.running_var");
        std::vector<float> fw((size_t)nOut * 2 * D), fb(nOut);
        for (int n = 0; n < nOut; ++n) {
            const double sc = (double)g->data[n] / std::sqrt((double)rv->data[n] + 1e-5);
            for (int i = 0; i < 2 * D; ++i) fw[(size_t)n * 2 * D + i] = (float)(sc * (double)w->data[(size_t)n * 2 * D + i]);
            fb[n] = (float)(sc * (double)b->data[n] + ((double)be->data[n] - (double)rm->data[n] * sc));
        }
        h->tn_fc.N = nOut; h->tn_fc.K = 2 * D;
        if ((rc = dev_upload(h, &h->tn_fc.W, fw))) return rc;
        if ((rc = dev_upload(h, &h->tn_fc.bias, fb))) return rc;
    }
    fl += h->tn_epilog.flops_per_row + h->tn_att_in.flops_per_row + h->tn_att_out.flops_per_row;
    h->flops_per_utt = (double)T * fl + 2.0 * nOut * 2 * D;
    return SVHIP_OK;
}

// ---- Conformer -------------------------------------------------------------------------------------------
// a host tensor under a temporary name, packed by make_conv as a plain (N, K) layer, then dropped
static int make_conv_from(svhip_handle* h, ConvLayer& L, const std::string& tag, std::vector<float> w, std::vector<int64_t> shape,
                          const std::string& bname, std::vector<float>* bias = nullptr) {
    const std::string wn = "#cf." + tag + ".weight", bn = "#cf." + tag + ".bias";
    h->host_w[wn] = HostTensor{std::move(w), std::move(shape)};
    if (bias) h->host_w[bn] = HostTensor{*bias, {(int64_t)bias->size()}};
    int rc = make_conv(h, L, wn, bias ? bn : bname, "", 1);
    h->host_w.erase(wn);
    h->host_w.erase(bn);
    return rc;
}

int finalize_conformer(svhip_handle* h) {
    const svhip_config& c = h->cfg;
    const int D = CF_D, Tp = h->cf_Tp, F2 = h->cf_F2, nOut = c.embed_dim;
    int rc;
    if ((rc = upload_f32(h, "instance_norm.weight", &h->in_w))) return rc;
    if ((rc = upload_f32(h, "instance_norm.bias", &h->in_b))) return rc;
    const std::string s = "conformer_block.conv_subsample.sequential.";
    {
        const HostTensor* w = getw(h, s + "0.weight");         // (256, 1, 3, 3) -> tap-major [9][256]
        if (!w) SV_FAIL(h, SVHIP_ERR_MISSING, "missing tensor %s0.weight", s.c_str());
        std::vector<float> tw(9 * D);
        for (int ch = 0; ch < D; ++ch)
            for (int t = 0; t < 9; ++t) tw[(size_t)t * D + ch] = w->data[(size_t)ch * 9 + t];
        if ((rc = dev_upload(h, &h->cf_c1_w, tw))) return rc;
        if ((rc = upload_f32(h, s + "0.bias", &h->cf_c1_b))) return rc;
    }
    {
        const HostTensor* w = getw(h, s + "2.weight");         // (256, 256, 3, 3) [n][c][dt][df] -> [n][dt * 768 + df * 256 + c]
        if (!w) SV_FAIL(h, SVHIP_ERR_MISSING, "missing tensor %s2.weight", s.c_str());
        std::vector<float> pw((size_t)D * 9 * D);
        for (int n = 0; n < D; ++n)
            for (int ch = 0; ch < D; ++ch)
                for (int t = 0; t < 9; ++t) pw[(size_t)n * 9 * D + (size_t)(t / 3) * 3 * D + (t % 3) * D + ch] = w->data[((size_t)n * D + ch) * 9 + t];
        if ((rc = make_conv_from(h, h->cf_c2, "c2", std::move(pw), {D, 9 * D, 1}, s + "2.bias"))) return rc;
        std::vector<int> so((size_t)Tp * F2);
        for (int t = 0; t < Tp; ++t)
            for (int f = 0; f < F2; ++f) so[(size_t)t * F2 + f] = ((2 * t) * h->cf_F1 + 2 * f) * D;
        if ((rc = dev_upload(h, &h->cf_seg_off, so))) return rc;
    }
    {
        const std::string p = "conformer_block.input_projection.0.linear.";
        const HostTensor* w = getw(h, p + "weight");           // (256, 256 F2), column c F2 + f -> f 256 + c (the GEMM writes (b, t, f) rows)
        if (!w) SV_FAIL(h, SVHIP_ERR_MISSING, "missing tensor %sweight", p.c_str());
        std::vector<float> pw((size_t)D * D * F2);
        for (int n = 0; n < D; ++n)
            for (int ch = 0; ch < D; ++ch)
                for (int f = 0; f < F2; ++f) pw[(size_t)n * D * F2 + (size_t)f * D + ch] = w->data[(size_t)n * D * F2 + (size_t)ch * F2 + f];
        if ((rc = make_conv_from(h, h->cf_proj, "proj", std::move(pw), {D, D * F2}, p + "bias"))) return rc;
    }
    double fl = 2.0 * 9 * D * h->cf_T1 * h->cf_F1 + (double)Tp * F2 * h->cf_c2.flops_per_row + (double)Tp * h->cf_proj.flops_per_row;
    h->cf.assign(CF_LAYERS, svhip_handle::CfBlock{});
    for (int i = 0; i < CF_LAYERS; ++i) {
        svhip_handle::CfBlock& K = h->cf[i];
        const std::string p = "conformer_block.layers." + std::to_string(i) + ".";
        for (int j = 0; j < 2; ++j) {
            const std::string q = p + (j == 0 ? "sequential.0." : "sequential.3.") + "module.sequential.";
            if ((rc = upload_f32(h, q + "0.weight", &K.ff_g[j]))) return rc;
            if ((rc = upload_f32(h, q + "0.bias", &K.ff_b[j]))) return rc;
            if ((rc = make_conv(h, K.ff1[j], q + "1.linear.weight", q + "1.linear.bias", "", 1))) return rc;
            if ((rc = make_conv(h, K.ff2[j], q + "4.linear.weight", q + "4.linear.bias", "", 1))) return rc;
            fl += (double)Tp * (K.ff1[j].flops_per_row + K.ff2[j].flops_per_row);
        }
        const std::string a = p + "sequential.1.module.";
        if ((rc = upload_f32(h, a + "layer_norm.weight", &K.att_g))) return rc;
        if ((rc = upload_f32(h, a + "layer_norm.bias", &K.att_b))) return rc;
        {
            std::vector<float> w, b;
            for (const char* q : {"query_proj", "key_proj", "value_proj"}) {
                const HostTensor *wq = getw(h, a + "attention." + q + ".linear.weight"), *bq = getw(h, a + "attention." + q + ".linear.bias");
                if (!wq || !bq) SV_FAIL(h, SVHIP_ERR_MISSING, "missing tensor %sattention.%s.linear.*", a.c_str(), q);
                w.insert(w.end(), wq->data.begin(), wq->data.end());
                b.insert(b.end(), bq->data.begin(), bq->data.end());
            }
            if ((rc = make_conv_from(h, K.qkv, "qkv", std::move(w), {3 * D, D}, "", &b))) return rc;
        }
        if ((rc = make_conv(h, K.out, a + "attention.out_proj.linear.weight", a + "attention.out_proj.linear.bias", "", 1))) return rc;
        if ((rc = upload_f32(h, a + "attention.u_bias", &K.u))) return rc;
        if ((rc = upload_f32(h, a + "attention.v_bias", &K.v))) return rc;
        {
            // P = pe[:T'] pos_proj^T in double: the positional term depends on T' only
            const HostTensor *pe = getw(h, a + "positional_encoding.pe"), *wp = getw(h, a + "attention.pos_proj.linear.weight");
            if (!pe || !wp) SV_FAIL(h, SVHIP_ERR_MISSING, "missing tensor %s%s", a.c_str(), !pe ? "positional_encoding.pe" : "attention.pos_proj.linear.weight");
            std::vector<float> P((size_t)Tp * D);
            auto rows = [&](int t0, int t1) {
                for (int t = t0; t < t1; ++t) {
                    const float* pr = pe->data.data() + (size_t)t * D;
                    for (int n = 0; n < D; ++n) {
                        const float* wr = wp->data.data() + (size_t)n * D;
                        double acc = 0.0;
                        for (int k = 0; k < D; ++k) acc += (double)pr[k] * (double)wr[k];
                        P[(size_t)t * D + n] = (float)acc;
                    }
                }
            };
            // (rows split over up to 16 host threads: 6 x 655 M multiply-adds at T' = 10^4; every row is the same sum whatever the split)
            const int nt = std::max(1, std::min({16, (int)std::thread::hardware_concurrency(), (Tp + 63) / 64}));
            std::vector<std::thread> pool;
            for (int q = 1; q < nt; ++q) pool.emplace_back(rows, (int)((int64_t)Tp * q / nt), (int)((int64_t)Tp * (q + 1) / nt));
            rows(0, Tp / nt);
            for (auto& th : pool) th.join();
            if ((rc = dev_upload(h, &K.P, P))) return rc;
        }
        fl += (double)Tp * (K.qkv.flops_per_row + K.out.flops_per_row) + 4.0 * Tp * (double)Tp * 3 * 2 * 64;
        const std::string cv = p + "sequential.2.module.sequential.";
        if ((rc = upload_f32(h, cv + "0.weight", &K.cv_g))) return rc;
        if ((rc = upload_f32(h, cv + "0.bias", &K.cv_b))) return rc;
        if ((rc = make_conv(h, K.pw1, cv + "2.conv.weight", cv + "2.conv.bias", "", 1))) return rc;
        if ((rc = make_conv(h, K.pw2, cv + "7.conv.weight", cv + "7.conv.bias", "", 1))) return rc;
        {
            // depthwise (256, 1, 15), no bias, then BatchNorm(256) (eval, eps 1e-5): w' = s w, b' = beta - mean s (double on the host)
            const HostTensor *dw = getw(h, cv + "4.conv.weight"), *g = getw(h, cv + "5.weight"), *be = getw(h, cv + "5.bias");
            const HostTensor *rm = getw(h, cv + "5.running_mean"), *rv = getw(h, cv + "5.running_var");
            if (!dw || !g || !be || !rm || !rv) SV_FAIL(h, SVHIP_ERR_MISSING, "missing depthwise / BatchNorm tensors of %s", cv.c_str());
            std::vector<float> tw((size_t)15 * D), tb(D);
            for (int ch = 0; ch < D; ++ch) {
                const double sc = (double)g->data[ch] / std::sqrt((double)rv->data[ch] + 1e-5);
                for (int t = 0; t < 15; ++t) tw[(size_t)t * D + ch] = (float)(sc * (double)dw->data[(size_t)ch * 15 + t]);
                tb[ch] = (float)((double)be->data[ch] - (double)rm->data[ch] * sc);
            }
            if ((rc = dev_upload(h, &K.dw_w, tw))) return rc;
            if ((rc = dev_upload(h, &K.dw_b, tb))) return rc;
        }
        fl += (double)Tp * (K.pw1.flops_per_row + K.pw2.flops_per_row + 2.0 * 15 * D);
        if ((rc = upload_f32(h, p + "sequential.4.weight", &K.fin_g))) return rc;
        if ((rc = upload_f32(h, p + "sequential.4.bias", &K.fin_b))) return rc;
    }
    // pooling: attention.0 + ReLU with attention.2 (BatchNorm1d(128)) as the epilogue affine, attention.3 to fp32 logits
    if ((rc = make_conv(h, h->cf_att0, "attention.0.weight", "attention.0.bias", "attention.2", 1))) return rc;
    if ((rc = make_conv(h, h->cf_att3, "attention.3.weight", "attention.3.bias", "", 1))) return rc;
    if ((rc = make_bn(h, "attention_norm", 2 * D, &h->cf_pbn_scale, &h->cf_pbn_shift))) return rc;
    if ((rc = make_linear(h, h->cf_fc, "fc.conv.weight", "fc.conv.bias"))) return rc;
    if (h->cf_fc.N != nOut || h->cf_fc.K != 2 * D) SV_FAIL(h, SVHIP_ERR_INVALID, "fc.conv.weight must be (%d, %d, 1)", nOut, 2 * D);
    {
        std::vector<float> half(D, 0.5f);
        if ((rc = dev_upload(h, &h->cf_half, half))) return rc;
    }
    fl += (double)Tp * (h->cf_att0.flops_per_row + h->cf_att3.flops_per_row) + 2.0 * nOut * 2 * D;
    h->flops_per_utt = fl;
    return SVHIP_OK;
}

int alloc_workspace(svhip_handle* h) {
    const svhip_config& c = h->cfg;
    const size_t B = c.max_batch, T = h->T, M = B * T, C = c.channels, C3 = 3 * C, e = h->esz;
    int rc;
    if ((rc = dev_alloc(h, &h->d_wav, B * (size_t)c.samples))) return rc;
    if ((rc = dev_alloc(h, &h->d_feat, B * c.n_mels * T))) return rc;
    if ((rc = dev_alloc(h, &h->d_pstats, B * c.n_mels * 2))) return rc;
    if (h->x3 && (rc = dev_alloc(h, &h->d_xscale, 2 * (4 + 256)))) return rc;       // (one set per lane slice)
    if (h->fb.sym_hi) {
        if ((rc = dev_alloc(h, &h->d_logmel, B * c.n_mels * T))) return rc;
        if ((rc = dev_alloc(h, &h->d_fpart, B * c.n_mels * ((T + 63) / 64)))) return rc;
    }
    if ((rc = dev_alloc(h, &h->d_zero, 64))) return rc;
    SV_HIP(h, hipMemset(h->d_zero, 0, 256));
    {
        std::vector<float> one(4096, 1.0f), zero(4096, 0.0f);
        if ((rc = dev_upload(h, &h->d_ones, one))) return rc;
        if ((rc = dev_upload(h, &h->d_zeros, zero))) return rc;
    }
    if ((rc = dev_alloc(h, &h->d_emb, B * (size_t)c.embed_dim))) return rc;
    if ((rc = dev_alloc(h, &h->d_status, 4))) return rc;
    SV_HIP(h, hipMemset(h->d_status, 0, 16));
    SV_HIP(h, hipHostMalloc((void**)&h->host_flag, 64, hipHostMallocMapped));
    *h->host_flag = 0;
    SV_HIP(h, hipHostGetDevicePointer((void**)&h->host_flag_dev, h->host_flag, 0));
    if (is_rawnet2(c.model)) {
        const bool conv = c.model == SVHIP_MODEL_RAWNET2_CONV;
        h->rn_T1 = conv ? (c.samples - 3) / 3 + 1 : (c.samples - 250) / 3;       // conv1 (kernel 3, stride 3) | sinc (251 taps) + max_pool1d(3)
        const size_t per_utt = (size_t)h->rn_T1 * 128;           // largest activation: (T1, 128); later stages shrink 3x per doubling
        h->rn_buf_bytes = B * per_utt * e;
        for (int i = 0; i < 6; ++i) {
            char* q;
            if ((rc = dev_alloc(h, &q, B * per_utt * e + 256))) return rc;
            h->rn_buf[i] = q;
            SV_HIP(h, hipMemset(q + h->rn_buf_bytes, 0, 256));          // the zero tail (no kernel writes past the payload)
        }
        if (!conv && (rc = dev_alloc(h, &h->rn_stats, B * 2))) return rc;
        if (!conv && (h->bf16 || h->x3)) {                                  // LayerNorm output in 16 bits, zero-tailed rows (operand of the 16-bit / split sinc kernels)
            h->rn_Lp = (int)round_up(c.samples + RN_XN_TAIL, 64);
            uint16_t* q;
            if ((rc = dev_alloc(h, &q, (h->x3 ? 4 : 2) * B * (size_t)h->rn_Lp))) return rc;      // (F32X3: hi and lo parts of both copies)
            h->rn_xn = q;
        }
        if ((rc = dev_alloc(h, &h->rn_part, B * (size_t)(rn_block128_ntiles(h->rn_T1) + 1) * 4 * 128))) return rc;
        if ((rc = dev_alloc(h, &h->rn_mean, B * 512))) return rc;
        if ((rc = dev_alloc(h, &h->rn_scratch, B * 16 * 512))) return rc;
        if ((rc = dev_alloc(h, &h->rn_s, B * 512 * 2))) return rc;
        int tf = h->rn_T1;
        for (int i = 0; i < 6; ++i) tf /= 3;                      // six max_pool1d(3) stages follow the front-end
        if (tf < 1) SV_FAIL(h, SVHIP_ERR_INVALID, "utterance too short for RawNet2 (%d samples)", c.samples);
        if ((rc = dev_alloc(h, &h->rn_logits, B * (size_t)tf * 512))) return rc;
        if (rn_is_gru(c.model)) {                                 // (256 x 14 frames: 11 MB of gate inputs)
            h->rn_gru_T = tf;
            if ((rc = dev_alloc(h, &h->rn_gru_gi, B * (size_t)tf * 3 * RN_GRU_HIDDEN))) return rc;
            for (int i = 0; i < 2; ++i) if ((rc = dev_alloc(h, &h->rn_gru_hbuf[i], B * (size_t)RN_GRU_HIDDEN))) return rc;
        }
        if ((rc = dev_alloc(h, &h->rn_pooled, B * 1024))) return rc;
        if (h->bf16) {          // K-slice partials of fc (K = 1 024: four slices of 256) at full batches, 16-bit handles
            h->lin_part_per_utt = (size_t)4 * (size_t)std::max(128, c.embed_dim);
            if ((rc = dev_alloc(h, &h->d_lin_part, B * h->lin_part_per_utt))) return rc;
        }
    }
    if (c.model == SVHIP_MODEL_RAWNET3) {
        // three (B T0, 1024) activation buffers carry layer1 (RawNet3 forward, api_rawnet3.hip); the later stages reuse them
        h->rn3_T0 = rn3_frames(c.samples);
        const size_t M0 = B * (size_t)h->rn3_T0, T2 = (size_t)(h->rn3_T0 / 5 / 3);
        if (T2 < 2) SV_FAIL(h, SVHIP_ERR_INVALID, "utterance too short for RawNet3 (%d samples)", c.samples);
        for (int i = 0; i < 3; ++i) {
            char* q;
            if ((rc = dev_alloc(h, &q, M0 * 1024 * e + 256))) return rc;
            h->rn3_buf[i] = q;
        }
        char* q;
        if ((rc = dev_alloc(h, &q, B * T2 * 3072 * e + 256))) return rc;
        h->rn3_cat = q;
        if ((rc = dev_alloc(h, &q, M0 * RN3_FILTERS * e + 256))) return rc;
        h->rn3_x0 = q;
        if ((rc = dev_alloc(h, &h->rn3_stats, B * 2))) return rc;
        if ((rc = dev_alloc(h, &h->rn3_mean, B * 1024))) return rc;
        if ((rc = dev_alloc(h, &h->rn3_gate, B * 1024))) return rc;
        if ((rc = dev_alloc(h, &h->rn3_tstat, B * 3072))) return rc;
        if ((rc = dev_alloc(h, &h->rn3_ctx, B * 128))) return rc;
        if ((rc = dev_alloc(h, &h->rn3_logit, B * T2))) return rc;
        if ((rc = dev_alloc(h, &h->rn3_pooled, B * 3072))) return rc;
    }
    if (c.model == SVHIP_MODEL_TITANET) {
        // (TitaNet forward, api_titanet.hip): six (B T, H) activation buffers, the encoder output, the attention activation and energies
        const size_t H = C;
        char* p;
        auto actbuf = [&](void** dst, size_t elems) -> int {
            int r = dev_alloc(h, &p, elems * e + 256);
            *dst = p;
            return r;
        };
        if ((rc = actbuf(&h->X_in, M * c.n_mels))) return rc;
        for (int i = 0; i < 6; ++i) if ((rc = actbuf(&h->tn_buf[i], M * H))) return rc;
        if ((rc = actbuf(&h->tn_enc, M * 1536))) return rc;
        if ((rc = actbuf(&h->tn_att, M * 128))) return rc;
        if ((rc = dev_alloc(h, &h->tn_logits, M * 1536))) return rc;
        if ((rc = dev_alloc(h, &h->tn_mean, B * H))) return rc;
        if ((rc = dev_alloc(h, &h->tn_gate, B * H))) return rc;
        if ((rc = dev_alloc(h, &h->tn_pool_raw, B * 3072))) return rc;
        if ((rc = dev_alloc(h, &h->tn_pool, B * 3072))) return rc;
        if (h->bf16) {          // the third pointwise GEMM's column-sum partials (the SE squeeze)
            h->colsum_region = (int64_t)((M + 255) / 256 + 2) * 16 * H;
            if ((rc = dev_alloc(h, &h->d_colsum, (size_t)2 * h->colsum_region))) return rc;
        }
    }
    if (c.model == SVHIP_MODEL_CONFORMER) {
        // (Conformer forward, api_conformer.hip): the subsampling slice buffers, eleven (B T', <= 1024) activations, logits, pooled rows
        h->cf_T1 = cf_sub(h->T); h->cf_F1 = cf_sub(c.n_mels);
        h->cf_Tp = cf_sub(h->cf_T1); h->cf_F2 = cf_sub(h->cf_F1);
        const size_t Tp = h->cf_Tp, Mp = B * Tp, D = CF_D;
        const size_t per_utt = (size_t)h->cf_T1 * h->cf_F1 * D * e;          // conv1 output bytes of one utterance
        h->cf_chunk = (int)std::max<size_t>(1, std::min<size_t>(B, ((size_t)256 << 20) / per_utt));
        char* p;
        auto actbuf = [&](void** dst, size_t elems) -> int {
            int r = dev_alloc(h, &p, elems * e + 256);
            *dst = p;
            return r;
        };
        if ((rc = actbuf(&h->X_in, M * c.n_mels))) return rc;
        if ((rc = actbuf(&h->cf_c1, (size_t)h->cf_chunk * h->cf_T1 * h->cf_F1 * D))) return rc;
        if ((rc = actbuf(&h->cf_s2, (size_t)h->cf_chunk * Tp * h->cf_F2 * D))) return rc;
        void** bufs[] = {&h->cf_in, &h->cf_b0, &h->cf_x[0], &h->cf_x[1], &h->cf_r, &h->cf_ln, &h->cf_ln2, &h->cf_ctx, &h->cf_attn0, &h->cf_last};
        for (void** b : bufs) if ((rc = actbuf(b, Mp * D))) return rc;
        if ((rc = actbuf(&h->cf_hid, Mp * 4 * D))) return rc;
        if ((rc = dev_alloc(h, &h->cf_logits, Mp * D))) return rc;
        if ((rc = dev_alloc(h, &h->cf_pool_raw, B * 2 * D))) return rc;
        if ((rc = dev_alloc(h, &h->cf_pool, B * 2 * D))) return rc;
    }
    if (c.model == SVHIP_MODEL_ECAPA) {
        char* p;
        auto actbuf = [&](void** dst, size_t elems) -> int {
            int r = dev_alloc(h, &p, elems * e + 256);
            *dst = p;
            return r;
        };
        if ((rc = actbuf(&h->X_in, M * c.n_mels))) return rc;
        if ((rc = actbuf(&h->X0, M * C))) return rc;
        if ((rc = actbuf(&h->H1, M * C))) return rc;
        if ((rc = actbuf(&h->H2, M * C))) return rc;
        if ((rc = actbuf(&h->H3, M * C))) return rc;
        if ((rc = actbuf(&h->CAT, M * C3))) return rc;
        if ((rc = actbuf(&h->MFA, M * C3))) return rc;
        if ((rc = actbuf(&h->ATT, M * 128))) return rc;
        if ((rc = dev_alloc(h, &h->LOGITS, M * C3))) return rc;
        if ((rc = dev_alloc(h, &h->d_mean, B * C))) return rc;
        if ((rc = dev_alloc(h, &h->d_s1, B * 128))) return rc;
        if ((rc = dev_alloc(h, &h->d_s2, B * C))) return rc;
        if ((rc = dev_alloc(h, &h->d_gstats, B * 2 * C3))) return rc;
        if ((rc = dev_alloc(h, &h->d_ctx, B * 128))) return rc;
        h->lin_part_per_utt = (size_t)((2 * C3 + 383) / 384) * (size_t)std::max(128, c.embed_dim);
        if ((rc = dev_alloc(h, &h->d_lin_part, B * h->lin_part_per_utt))) return rc;
        if ((rc = dev_alloc(h, &h->d_pool_raw, B * 2 * C3))) return rc;
        if ((rc = dev_alloc(h, &h->d_pool_bn, B * 2 * C3))) return rc;
        if (h->x3 && (rc = dev_alloc(h, reinterpret_cast<char**>(&h->s32_buf), M * C3 * 4 + 256))) return rc;
        if (h->x3 && C % 32 == 0 && (rc = dev_alloc(h, reinterpret_cast<char**>(&h->cat_s32), M * C3 * 4 + 256))) return rc;
        if (h->x3 && (C == 512 || C == 1024)) {
            if ((rc = dev_alloc(h, reinterpret_cast<char**>(&h->h2_s32), M * C * 4 + 256))) return rc;
            for (int i = 0; i < 2; ++i) if ((rc = dev_alloc(h, reinterpret_cast<char**>(&h->u_s32[i]), M * (C / 8) * 4 + 256))) return rc;
        }
        h->colsum_region = (int64_t)((M + 255) / 256 + 2) * 16 * C3;
        if ((rc = dev_alloc(h, &h->d_colsum, (size_t)4 * h->colsum_region))) return rc;
    }
    return SVHIP_OK;
}

}  // namespace svhip
