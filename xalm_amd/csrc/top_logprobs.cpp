// top_logprobs.cpp — the top-N log-probabilities on the host, plain C++ (no HIP, no device): the
// definition of include/xalm_hip.h (XH_TOP_MAX) restated directly, and its argument checks.
#include "top_logprobs_host.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <functional>
#include <vector>

namespace xalm {

const char* top_args_error(const float* logits, int vocab, int n_rows, int n_top, int min_top, const int* targets,
                           const int* ids_out, const float* lps_out, const float* target_lp_out,
                           const int* target_rank_out) {
    if (!logits) return "null logits";
    if (vocab <= 0 || vocab > TOP_MAX_VOCAB) return "vocab outside 1 .. 2^17";
    if (n_rows <= 0) return "n_rows must be positive";
    if (n_top < min_top || n_top > XH_TOP_MAX || n_top > vocab) return "n_top outside its range (at most min(XH_TOP_MAX, vocab))";
    if (n_top > 0 && (!ids_out || !lps_out)) return "null top list";
    const int given = (targets ? 1 : 0) + (target_lp_out ? 1 : 0) + (target_rank_out ? 1 : 0);
    if (given != 0 && given != 3) return "targets, target_lp_out and target_rank_out go together";
    if (targets)
        for (int r = 0; r < n_rows; r++)
            if (targets[r] < 0 || targets[r] >= vocab) return "target out of range";
    return nullptr;
}

namespace {
// the sampler's key (smp_key, sample.h): a larger logit = a larger key, +0 above -0
uint32_t key_of(const float v) {
    uint32_t u;
    std::memcpy(&u, &v, 4);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
}  // namespace
}  // namespace xalm

using namespace xalm;

extern "C" int xh_top_logprobs_host(const float* logits, int vocab, int n_rows, int n_top, const int* targets, int* ids_out,
                                    float* lps_out, float* target_lp_out, int* target_rank_out) {
    if (top_args_error(logits, vocab, n_rows, n_top, 1, targets, ids_out, lps_out, target_lp_out, target_rank_out))
        return XH_E_INVALID;
    std::vector<unsigned long long> ent((size_t)vocab);
    for (int r = 0; r < n_rows; r++) {
        const float* l = logits + (size_t)r * vocab;
        // (key << 32 | ~index) descending is the order: key descending, then index ascending
        for (int i = 0; i < vocab; i++) ent[(size_t)i] = ((unsigned long long)key_of(l[i]) << 32) | (uint32_t)~i;
        std::partial_sort(ent.begin(), ent.begin() + n_top, ent.end(), std::greater<unsigned long long>());
        const float M = l[(int)~(uint32_t)ent[0]];
        double sum = 0.0;  // the sum in double, as the host Sampler's
        for (int i = 0; i < vocab; i++) sum += (double)expf(l[i] - M);
        const float lse = logf((float)sum);
        const auto lp = [&](const float v) { return v == -INFINITY ? -INFINITY : (v - M) - lse; };
        for (int j = 0; j < n_top; j++) {
            const int id = (int)~(uint32_t)ent[(size_t)j];
            ids_out[(size_t)r * n_top + j] = id;
            lps_out[(size_t)r * n_top + j] = lp(l[id]);
        }
        if (targets) {
            const int t = targets[r];
            const uint32_t kt = key_of(l[t]);
            int rank = 0;
            for (int i = 0; i < vocab; i++) {
                const uint32_t k = key_of(l[i]);
                rank += (k > kt || (k == kt && i < t)) ? 1 : 0;
            }
            target_lp_out[r] = lp(l[t]);
            target_rank_out[r] = rank;
        }
    }
    return XH_OK;
}
