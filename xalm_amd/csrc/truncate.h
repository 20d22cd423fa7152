// truncate.h — what the device head of xh_decode_sample_adapt (sample_adapt.h) and its host mirror
// (truncate.cpp, plain C++) share: the argument check of xh_trunc_ctl and Mirostat's update.
#pragma once

#include <cmath>
#include <cstdint>

#include "../../include/xalm_hip.h"

#ifdef __HIPCC__
#define XH_HOST_DEVICE __host__ __device__
#else
#define XH_HOST_DEVICE
#endif

namespace xalm {

// mu' = mu - eta * (obs - tau), obs = log2(K / M_tok) from the kept mass and the token's mass: every
// f32 operation rounded once (truncate.cpp is built with contraction off, as ctl_adjust is here)
XH_HOST_DEVICE inline float trunc_mu_next(const float mu, const float eta, const float tau, const unsigned long long kept,
                                         const unsigned long long m_tok) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const float obs = (float)(log2((double)kept) - log2((double)m_tok));
    const float e = obs - tau;
    const float g = eta * e;
    return mu - g;
}

// xh_trunc_ctl as the header defines it, with what Mirostat requires of the other parameters
// (min_p: xh_logit_ctl's, 0 for a null ctl) and of mu.  nullptr = valid.
inline const char* trunc_error(const xh_trunc_ctl* t, const xh_sampling* s, const float min_p, const float mu) {
    if (!t) return "null xh_trunc_ctl";
    if (!(t->typical_p > 0.f && t->typical_p <= 1.f)) return "typical_p outside (0, 1]";
    if (!(t->top_n_sigma >= 0.f) || !std::isfinite(t->top_n_sigma)) return "top_n_sigma must be >= 0 and finite";
    if (!(t->mirostat_tau >= 0.f) || !std::isfinite(t->mirostat_tau)) return "mirostat_tau must be >= 0 and finite";
    if (t->mirostat_tau > 0.f) {
        if (!(t->mirostat_eta > 0.f) || !std::isfinite(t->mirostat_eta)) return "mirostat_eta must be > 0 and finite";
        if (!(mu >= 0.f) || !std::isfinite(mu)) return "mu must be >= 0 and finite";
        if (s && (s->top_k != 0 || s->top_p != 1.f)) return "Mirostat takes top_k 0 and top_p 1";
        if (min_p != 0.f || t->typical_p != 1.f || t->top_n_sigma != 0.f)
            return "Mirostat takes min_p 0, typical_p 1 and top_n_sigma 0";
    }
    return nullptr;
}

}  // namespace xalm
