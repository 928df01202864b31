// api_weights.hip — what the models of libsvhip share when a handle is created and its weights are loaded: front-end tables, 16-bit and
// split conversions, weight packing, the common workspace.  Each model's own names, packing and buffers are in its api_<model>.hip.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "handle.h"

namespace svhip {

static inline uint16_t f32_to_f16_rne(float f) {      // IEEE half, round to nearest even (the host compiler's _Float16 conversion)
    const _Float16 hv = static_cast<_Float16>(f);
    uint16_t u;
    memcpy(&u, &hv, 2);
    return u;
}

uint16_t f32_to_bf16_rne(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);   // NaN stays NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

// host twin of common.h's x3_hi / x3_lo: a weight as (hi << 16) | lo in the planes' type (IEEE half; bf16 under -DSVHIP_X3_BF16)
uint32_t x3_split_word(float v) {
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

uint16_t to_h16(const svhip_handle* h, float f) { return h->f16 ? f32_to_f16_rne(f) : f32_to_bf16_rne(f); }

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
    // an odd n_fft: the reference pads n_fft / 2 samples on both sides, one sample less than a frame in all, and so has (L - 1) / hop + 1
    // frames where every buffer of the library is sized for L / hop + 1
    if (c.n_fft % 2 != 0)
        SV_FAIL(h, SVHIP_ERR_UNSUPPORTED, "fbank geometry n_fft=%d win=%d hop=%d not supported: n_fft must be even", c.n_fft, c.win_length, c.hop_length);
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
    // the kernels' sample buffer grows with the hop: what launch_fbank will ask for must fit one workgroup's LDS on this device
    int dev_lds = 0;
    if (hipDeviceGetAttribute(&dev_lds, hipDeviceAttributeMaxSharedMemoryPerBlock, c.device) != hipSuccess) dev_lds = 64 * 1024;
    const size_t need = fbank_lds_needed(fb), have = std::min((size_t)dev_lds, fbank_lds_limit());
    if (need > have)
        SV_FAIL(h, SVHIP_ERR_UNSUPPORTED, "fbank geometry n_fft=%d win=%d hop=%d n_mels=%d not supported: its tile needs %zu bytes of LDS, a workgroup has %zu",
                c.n_fft, c.win_length, c.hop_length, c.n_mels, need, have);
    return SVHIP_OK;
}

// ---- shared weight helpers ---------------------------------------------------------------------------
const HostTensor* getw(svhip_handle* h, const std::string& name) {
    auto it = h->host_w.find(name);
    return it == h->host_w.end() ? nullptr : &it->second;
}

int needw(svhip_handle* h, const std::string& name, const HostTensor*& t) {
    if (!(t = getw(h, name))) SV_FAIL(h, SVHIP_ERR_MISSING, "missing tensor %s", name.c_str());
    return SVHIP_OK;
}

void spec_bn(WeightSpec& spec, const std::string& p, int64_t n) {
    spec[p + ".weight"] = {n}; spec[p + ".bias"] = {n}; spec[p + ".running_mean"] = {n};
    spec[p + ".running_var"] = {n}; spec[p + ".num_batches_tracked"] = {};
}

int bn_fold(svhip_handle* h, const std::string& p, int n, std::vector<double>& s, std::vector<double>& t) {
    const HostTensor *w = getw(h, p + ".weight"), *b = getw(h, p + ".bias"), *rm = getw(h, p + ".running_mean"),
                     *rv = getw(h, p + ".running_var");
    if (!w || !b || !rm || !rv) SV_FAIL(h, SVHIP_ERR_MISSING, "missing BatchNorm tensors for %s", p.c_str());
    s.resize(n); t.resize(n);
    for (int i = 0; i < n; ++i) {
        s[i] = (double)w->data[i] / std::sqrt((double)rv->data[i] + 1e-5);
        t[i] = (double)b->data[i] - (double)rm->data[i] * s[i];
    }
    return SVHIP_OK;
}

int make_bn(svhip_handle* h, const std::string& p, int n, float** scale, float** shift) {
    std::vector<double> s, t;
    int rc;
    if ((rc = bn_fold(h, p, n, s, t))) return rc;
    if ((rc = dev_upload(h, scale, std::vector<float>(s.begin(), s.end())))) return rc;
    return dev_upload(h, shift, std::vector<float>(t.begin(), t.end()));
}

int make_conv(svhip_handle* h, ConvLayer& L, const HostTensor& w, const std::vector<float>* bias, int dil, int c_lo, int c_hi, bool rn_s32) {
    const int N = (int)w.shape[0], cin_full = (int)w.shape[1], taps = w.shape.size() > 2 ? (int)w.shape[2] : 1;      // (a Linear: 1 tap)
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
                packed[(size_t)n * L.Kp + t * cin + c] = w.data[((size_t)n * cin_full + (c_lo + c)) * taps + t];
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
                (rn_s32 && (taps == 1 || taps == 3) && N % 128 == 0 && cin % 32 == 0 && L.K == L.Kp && L.K == taps * cin)) {
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
    if (bias && (rc = dev_upload(h, &L.bias, *bias))) return rc;
    return SVHIP_OK;
}

int make_conv(svhip_handle* h, ConvLayer& L, const std::string& wname, const std::string& bname, const std::string& bnname, int dil,
              int c_lo, int c_hi, bool rn_s32) {
    const HostTensor *w, *b = nullptr;
    int rc;
    if ((rc = needw(h, wname, w)) || (!bname.empty() && (rc = needw(h, bname, b)))) return rc;
    if ((rc = make_conv(h, L, *w, b ? &b->data : nullptr, dil, c_lo, c_hi, rn_s32))) return rc;
    return bnname.empty() ? SVHIP_OK : make_bn(h, bnname, L.N, &L.scale, &L.shift);
}

// fp32 linear from a (N, K, 1) or (N, K) tensor, optional column range
int make_linear(svhip_handle* h, LinearLayer& L, const std::string& wname, const std::string& bname, int c_lo, int c_hi) {
    const HostTensor *w, *b = nullptr;
    int rc;
    if ((rc = needw(h, wname, w))) return rc;
    const int N = (int)w->shape[0], Kfull = (int)w->shape[1];
    if (c_hi < 0) c_hi = Kfull;
    L.N = N; L.K = c_hi - c_lo;
    std::vector<float> m((size_t)N * L.K);
    for (int n = 0; n < N; ++n)
        for (int k = 0; k < L.K; ++k) m[(size_t)n * L.K + k] = w->data[(size_t)n * Kfull + c_lo + k];
    if ((rc = dev_upload(h, &L.W, m))) return rc;
    if (!bname.empty() && ((rc = needw(h, bname, b)) || (rc = dev_upload(h, &L.bias, b->data)))) return rc;
    return SVHIP_OK;
}

int upload_f32(svhip_handle* h, const std::string& name, float** dst) {
    const HostTensor* t;
    int rc = needw(h, name, t);
    return rc ? rc : dev_upload(h, dst, t->data);
}

int upload_h16(svhip_handle* h, const std::vector<float>& m, void** dst) {
    std::vector<uint16_t> v(m.size());
    for (size_t i = 0; i < m.size(); ++i) v[i] = f32_to_bf16_rne(m[i]);
    uint16_t* d;
    int rc = dev_upload(h, &d, v);
    *dst = d;
    return rc;
}

// ---- the common workspace ----------------------------------------------------------------------------
int actbuf(svhip_handle* h, void** dst, size_t elems) {
    char* p = nullptr;
    int rc = dev_alloc(h, &p, elems * h->esz + 256);
    *dst = p;
    return rc;
}

int alloc_workspace(svhip_handle* h) {
    const svhip_config& c = h->cfg;
    const size_t B = c.max_batch, T = h->T;
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
    return SVHIP_OK;
}

}  // namespace svhip
