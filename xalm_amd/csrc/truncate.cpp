// truncate.cpp — xh_truncate_host: the kept set of the adaptive draw (xh_trunc_ctl, include/xalm_hip.h)
// in plain C++, no device.  It restates sample_adapt.h stage by stage with sorts in place of the
// radix selections: the same integer masses (by the host's expf), the same keys and tie rules.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <numeric>
#include <vector>

#include "truncate.h"

using namespace xalm;

namespace {
uint32_t order_key(const float v) {
    uint32_t u;
    memcpy(&u, &v, 4);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
}  // namespace

extern "C" int xh_truncate_host(const float* logits, int vocab, const xh_sampling* s, float min_p, const xh_trunc_ctl* t,
                                float mu, int token, uint8_t* kept_out, int* n_kept_out, float* thr_out, float* mu_out) {
    constexpr float NEG_INF = -std::numeric_limits<float>::infinity();
    if (!logits || vocab <= 0 || vocab > (1 << 17) || !s || !(s->temperature > 0.f) || s->top_k < 0 ||
        !(s->top_p > 0.f && s->top_p <= 1.f) || !(min_p >= 0.f && min_p <= 1.f) || token >= vocab)
        return XH_E_INVALID;
    if (trunc_error(t, s, min_p, mu)) return XH_E_INVALID;
    const size_t V = (size_t)vocab;
    const float temp = s->temperature;
    if (kept_out) std::fill(kept_out, kept_out + V, (uint8_t)0);
    if (n_kept_out) *n_kept_out = 0;
    if (thr_out) *thr_out = NEG_INF;
    if (mu_out) *mu_out = mu;
    const float m = *std::max_element(logits, logits + V);
    if (!std::isfinite(m)) return 0;
    std::vector<uint64_t> M(V);
    for (size_t i = 0; i < V; i++)
        M[i] = logits[i] == NEG_INF ? 0ull : (uint64_t)(expf((logits[i] - m) / temp) * 1099511627776.0f);
    // the order: logit descending by its f32 bits, then index ascending
    std::vector<int> order(V);
    std::iota(order.begin(), order.end(), 0);
    std::sort(order.begin(), order.end(), [&](const int a, const int b) {
        const uint32_t ka = order_key(logits[a]), kb = order_key(logits[b]);
        return ka != kb ? ka > kb : a < b;
    });
    size_t n = s->top_k > 0 && s->top_k < vocab ? (size_t)s->top_k : V;
    if (min_p > 0.f) {
        size_t n_minp = 0;
        for (size_t i = 0; i < V; i++) n_minp += logits[i] != NEG_INF && expf((logits[i] - m) / temp) >= min_p;
        if (n_minp >= 1 && n_minp < n) n = n_minp;
    }
    if (t->top_n_sigma > 0.f) {
        double sum = 0.0, sq = 0.0;
        size_t cnt = 0;
        for (size_t i = 0; i < V; i++)
            if (std::isfinite(logits[i])) { sum += (double)logits[i]; cnt++; }
        const double mean = sum / (double)cnt;
        for (size_t i = 0; i < V; i++)
            if (std::isfinite(logits[i])) { const double d = (double)logits[i] - mean; sq += d * d; }
        const float thr = (float)((double)m - (double)t->top_n_sigma * std::sqrt(sq / (double)cnt));
        size_t n_sigma = 0;
        for (size_t i = 0; i < V; i++) n_sigma += logits[i] >= thr;
        if (n_sigma >= 1 && n_sigma < n) n = n_sigma;
        if (thr_out) *thr_out = thr;
    }
    const bool miro = t->mirostat_tau > 0.f;
    if (miro) {
        uint64_t S = 0;
        for (size_t i = 0; i < V; i++) S += M[i];
        const uint64_t cut = (uint64_t)std::ceil((double)S * std::exp2(-(double)mu));
        size_t n_mu = 0;
        for (size_t i = 0; i < V; i++) n_mu += M[i] >= cut;
        n = std::max<size_t>(1, n_mu);
    }
    std::vector<uint8_t> kept(V, 0);
    if (t->typical_p < 1.f) {
        uint64_t S = 0;
        for (size_t j = 0; j < n; j++) S += M[(size_t)order[j]];
        const float Sf = (float)S;
        // d of the tokens of C that carry mass; the others are never kept
        std::vector<int> cand;
        std::vector<float> sv(V, 0.f);
        std::vector<int> in_c(order.begin(), order.begin() + (long)n);
        std::sort(in_c.begin(), in_c.end());
        float H = 0.f;
        for (const int i : in_c)
            if (M[(size_t)i]) {
                const float p = (float)M[(size_t)i] / Sf;
                sv[(size_t)i] = -logf(p);
                const float ps = p * sv[(size_t)i];
                H = H + ps;
                cand.push_back(i);
            }
        std::vector<uint32_t> dk(V, 0);
        for (const int i : cand) {
            const float d = std::fabs(sv[(size_t)i] - H);
            memcpy(&dk[(size_t)i], &d, 4);  // d >= 0: its bits order as its value
        }
        std::sort(cand.begin(), cand.end(), [&](const int a, const int b) {
            return dk[(size_t)a] != dk[(size_t)b] ? dk[(size_t)a] < dk[(size_t)b] : a < b;
        });
        const double want = std::ceil((double)t->typical_p * (double)S);
        uint64_t target = want >= (double)S ? S : (uint64_t)want;
        if (target < 1) target = 1;
        uint64_t cum = 0;
        for (const int i : cand) {
            kept[(size_t)i] = 1;
            cum += M[(size_t)i];
            if (cum >= target) break;
        }
    } else {
        for (size_t j = 0; j < n; j++) kept[(size_t)order[j]] = 1;
    }
    int n_kept = 0;
    uint64_t K = 0;
    for (size_t i = 0; i < V; i++)
        if (kept[i]) { n_kept++; K += M[i]; }
    if (kept_out) std::copy(kept.begin(), kept.end(), kept_out);
    if (n_kept_out) *n_kept_out = n_kept;
    if (miro && mu_out && token >= 0 && kept[(size_t)token] && M[(size_t)token])
        *mu_out = trunc_mu_next(mu, t->mirostat_eta, t->mirostat_tau, K, M[(size_t)token]);
    return 0;
}
