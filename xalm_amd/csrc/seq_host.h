// seq_host.h — what the device head of xh_decode_sample_seq (sample_seq.h) and its host mirror
// (seq_host.cpp, plain C++) share: the argument check of xh_seq_ctl and DRY's penalty loop.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "truncate.h"

namespace xalm {

// l' - p with p = multiplier * base^extra as `extra` separate f32 products: every operation rounded
// once (seq_host.cpp is built with contraction off, as ctl_adjust is here)
XH_HOST_DEVICE inline float seq_dry_adjust(const float l, const float multiplier, const float base, const int extra) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    float p = multiplier;
    for (int i = 0; i < extra; i++) p = p * base;
    return l - p;
}

// xh_seq_ctl as the header defines it (vocab <= 0: unknown, the breaker ids are only checked for
// sign), with what Mirostat requires of it.  nullptr = valid.
inline const char* seq_error(const xh_seq_ctl* q, const xh_trunc_ctl* t, const int vocab) {
    if (!q) return "null xh_seq_ctl";
    if (!(q->dry_multiplier >= 0.f) || !std::isfinite(q->dry_multiplier)) return "dry_multiplier must be >= 0 and finite";
    if (!(q->dry_base >= 1.f) || !std::isfinite(q->dry_base)) return "dry_base must be >= 1 and finite";
    if (q->dry_allowed_length < 1 || q->dry_allowed_length > XH_SEQ_MAX_MATCH) return "dry_allowed_length outside 1 .. XH_SEQ_MAX_MATCH";
    if (q->no_repeat_ngram != 0 && (q->no_repeat_ngram < 2 || q->no_repeat_ngram > XH_SEQ_MAX_MATCH))
        return "no_repeat_ngram must be 0 or 2 .. XH_SEQ_MAX_MATCH";
    if (q->seq_last_n < 0 || q->seq_last_n > XH_CTL_MAX_WINDOW) return "seq_last_n outside 0 .. XH_CTL_MAX_WINDOW";
    if (q->n_breakers < 0 || q->n_breakers > XH_SEQ_MAX_BREAKERS) return "n_breakers outside 0 .. XH_SEQ_MAX_BREAKERS";
    if (q->n_breakers > 0 && !q->breaker_token) return "null breaker array";
    if (!(q->xtc_probability >= 0.f && q->xtc_probability <= 1.f)) return "xtc_probability outside [0, 1]";
    if (!(q->xtc_threshold > 0.f && q->xtc_threshold <= 1.f)) return "xtc_threshold outside (0, 1]";
    std::vector<int32_t> ids(q->breaker_token, q->breaker_token + q->n_breakers);
    std::sort(ids.begin(), ids.end());
    for (int i = 0; i < q->n_breakers; i++) {
        if (ids[i] < 0 || (vocab > 0 && ids[i] >= vocab)) return "breaker id out of range";
        if (i && ids[i] == ids[i - 1]) return "duplicate breaker id";
    }
    if (t && t->mirostat_tau > 0.f && q->xtc_probability != 0.f) return "Mirostat takes xtc_probability 0";
    return nullptr;
}

}  // namespace xalm
