// seq_host.cpp — xh_seq_adjust_host and xh_xtc_host: DRY, the n-gram ban and XTC (xh_seq_ctl,
// include/xalm_hip.h) in plain C++, no device.  They restate sample_seq.h stage by stage with plain
// loops: the same match walk, the same f32 penalty loop (seq_dry_adjust), the same integer masses (by
// the host's expf), keys and tie rules.
#include <cstring>
#include <limits>
#include <unordered_set>

#include "seq_host.h"

using namespace xalm;

namespace {
uint32_t order_key(const float v) {
    uint32_t u;
    memcpy(&u, &v, 4);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
}  // namespace

extern "C" int xh_seq_adjust_host(const float* adjusted_in, int vocab, const xh_seq_ctl* q, const int* window, int n_window,
                                  float* out, int* rep_out, int* ng_out) {
    if (!adjusted_in || vocab <= 0 || n_window < 0 || (n_window > 0 && !window)) return XH_E_INVALID;
    if (seq_error(q, nullptr, vocab)) return XH_E_INVALID;
    const int n = std::min(std::min(q->seq_last_n, n_window), XH_CTL_MAX_WINDOW);
    const int* w = window + (n_window - n);
    for (int i = 0; i < n; i++)
        if (w[i] < 0 || w[i] >= vocab) return XH_E_INVALID;
    if (out && out != adjusted_in) std::copy(adjusted_in, adjusted_in + vocab, out);
    if (rep_out) std::fill(rep_out, rep_out + vocab, 0);
    if (ng_out) std::fill(ng_out, ng_out + vocab, 0);
    const bool dry = q->dry_multiplier > 0.f, ban = q->no_repeat_ngram >= 2;
    if ((!dry && !ban) || n < 2) return 0;
    const std::unordered_set<int> breakers(q->breaker_token, q->breaker_token + q->n_breakers);
    std::vector<int> rep((size_t)vocab, 0), ng((size_t)vocab, 0);
    std::vector<int> touched;
    for (int j = 0; j + 1 < n; j++) {
        if (w[j] != w[n - 1]) continue;
        const int lim = std::min(j + 1, XH_SEQ_MAX_MATCH);
        int raw = 0, dr = 0;
        bool clean = true;
        while (raw < lim && w[j - raw] == w[n - 1 - raw]) {
            clean = clean && !breakers.count(w[n - 1 - raw]);
            raw++;
            if (clean) dr = raw;
        }
        const int c = w[j + 1];
        if (!rep[(size_t)c] && !ng[(size_t)c]) touched.push_back(c);
        rep[(size_t)c] = std::max(rep[(size_t)c], dr);
        ng[(size_t)c] = std::max(ng[(size_t)c], raw);
    }
    for (const int c : touched) {
        if (rep_out) rep_out[c] = rep[(size_t)c];
        if (ng_out) ng_out[c] = ng[(size_t)c];
        if (!out) continue;
        if (dry && rep[(size_t)c] >= q->dry_allowed_length)
            out[c] = seq_dry_adjust(out[c], q->dry_multiplier, q->dry_base, rep[(size_t)c] - q->dry_allowed_length);
        if (ban && ng[(size_t)c] >= q->no_repeat_ngram - 1) out[c] = -std::numeric_limits<float>::infinity();
    }
    return 0;
}

extern "C" int xh_xtc_host(const float* logits, int vocab, float temperature, const xh_seq_ctl* q, uint64_t seed, uint64_t pos,
                           uint8_t* kept_io, int* n_kept_out, int* fired_out) {
    constexpr float NEG_INF = -std::numeric_limits<float>::infinity();
    if (!logits || !kept_io || vocab <= 0 || vocab > (1 << 17) || !(temperature > 0.f)) return XH_E_INVALID;
    if (seq_error(q, nullptr, vocab)) return XH_E_INVALID;
    const size_t V = (size_t)vocab;
    int n_c = 0;
    for (size_t i = 0; i < V; i++) n_c += kept_io[i] ? 1 : 0;
    if (n_kept_out) *n_kept_out = n_c;
    if (fired_out) *fired_out = 0;
    if (!(q->xtc_probability > 0.f)) return 0;
    uint32_t x[4];
    xh_philox4x32(seed, pos, x);
    const float u = (float)(x[1] >> 8) * 5.9604644775390625e-8f;  // 2^-24
    if (!(u < q->xtc_probability)) return 0;
    if (fired_out) *fired_out = 1;
    const float m = *std::max_element(logits, logits + V);
    if (!std::isfinite(m)) return 0;
    std::vector<uint64_t> M(V, 0);
    uint64_t S = 0;
    for (size_t i = 0; i < V; i++)
        if (kept_io[i] && logits[i] != NEG_INF) {
            M[i] = (uint64_t)(expf((logits[i] - m) / temperature) * 1099511627776.0f);
            S += M[i];
        }
    const uint64_t cut = (uint64_t)std::ceil((double)q->xtc_threshold * (double)S);
    int n_a = 0;
    uint32_t kmin = 0xffffffffu;
    for (size_t i = 0; i < V; i++)
        if (kept_io[i] && M[i] >= cut) {
            n_a++;
            kmin = std::min(kmin, order_key(logits[i]));
        }
    if (n_a < 2) return 0;
    size_t last = 0;
    for (size_t i = 0; i < V; i++)
        if (kept_io[i] && M[i] >= cut && order_key(logits[i]) == kmin) last = i;
    for (size_t i = 0; i < V; i++)
        if (kept_io[i] && M[i] >= cut && i != last) kept_io[i] = 0;
    if (n_kept_out) *n_kept_out = n_c - (n_a - 1);
    return 0;
}
