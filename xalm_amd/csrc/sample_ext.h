// sample_ext.h — repetition penalties, logit bias, min-p and the log-probability in the sampling
// workgroup (the definition: include/xalm_hip.h, xh_logit_ctl).  Before the sampler of sample.h
// runs, ext_prepare
//   1. fetches the window, one token per thread, from the device ring the step head appends to,
//      and the bias table, into LDS;
//   2. copies the raw logits to `adj` and finds their maximum M (one pass);
//   3. fixes the entries the window and the biases touch: the adjustment is a pure function of
//      (l_t, c_t, b_t), so exactly one thread writes each: the lowest window slot holding the
//      token (it counts the occurrences and looks the bias up), or the bias entry's thread when
//      the token is not in the window;
//   4. sums expf(l - M) over the raw logits for the log-probability and, under min-p, finds the
//      maximum of l' (one pass over both buffers);
//   5. counts n_minp = #{ expf((l' - m) / T) >= min_p } (one pass, only with min_p and T > 0): a
//      prefix of the sampler's order, so min-p is an effective top-k.
// sample_token then runs on `adj` with that top-k.  The raw logits are never written.
#pragma once

#include "sample.h"

namespace xalm {

constexpr int EXT_RING = XH_CTL_MAX_WINDOW;  // ring slots: a power of two, the widest window
static_assert((EXT_RING & (EXT_RING - 1)) == 0 && EXT_RING <= SMP_THREADS, "one window token per thread");
static_assert(XH_CTL_MAX_BIAS <= SMP_THREADS, "one bias entry per thread");

// l' of one token: every operation rounded once (no contraction to fma), on both sides
__host__ __device__ inline float ctl_adjust(const float l, const int c, const bool biased, const float b,
                                            const float repeat, const float presence, const float frequency) {
#pragma clang fp contract(off)
    const float a = biased ? l + b : l;
    if (c == 0) return a;
    float r = a > 0.f ? a / repeat : a * repeat;
    const float f = (float)c * frequency;
    r = r - f;
    return r - presence;
}

struct ExtShared {
    int win[EXT_RING];
    int btok[XH_CTL_MAX_BIAS];
    float bval[XH_CTL_MAX_BIAS];
    uint32_t wkey[SMP_WAVES];
    float wsum[SMP_WAVES];
    unsigned wcnt[SMP_WAVES];
};

struct ExtPrep {
    float M;    // maximum raw logit
    float lse;  // logf(sum_j expf(l_j - M)) over the raw logits
    int top_k;  // the effective top-k: min(top_k or V, n_minp), 0 = off
};

// ext_prepare's hook between steps 3 and 4: every thread calls mask(adj, V) once l' is whole, and
// steps 4 and 5 see what it leaves (sample_dfa.h writes -inf over forbidden tokens there).  A thread
// may write only the entries tid, tid + SMP_THREADS, ...: step 4 reads them back with no barrier.
struct ExtNoMask {
    __device__ __forceinline__ void operator()(float*, int) const {}
};

// Every thread of the 1024-thread workgroup calls it and gets the same result.  `count` tokens have
// been appended to the ring so far (slot = index mod EXT_RING).
template <class Mask = ExtNoMask>
__device__ ExtPrep ext_prepare(ExtShared& es, const float* raw, float* adj, const int V, const ExtCtl c,
                               const int* ring, const int* btok, const float* bval, const Mask mask = Mask()) {
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int n_win = min(min(c.last_n, c.count), EXT_RING);
    const int n_bias = min(c.n_bias, XH_CTL_MAX_BIAS);
    if (tid < n_win) es.win[tid] = ring[(c.count - n_win + tid) & (EXT_RING - 1)];
    if (tid < n_bias) {
        es.btok[tid] = btok[tid];
        es.bval[tid] = bval[tid];
    }
    uint32_t kmax = 0;
    for (int i = tid; i < V; i += SMP_THREADS) {
        const float v = raw[i];
        adj[i] = v;
        const uint32_t k = smp_key(v);
        kmax = k > kmax ? k : kmax;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t other = __shfl_xor(kmax, o, 64);
        kmax = other > kmax ? other : kmax;
    }
    if (lane == 0) es.wkey[wid] = kmax;
    __syncthreads();  // the window, the biases and the copy are in place
    kmax = 0;
#pragma unroll
    for (int w = 0; w < SMP_WAVES; w++) kmax = es.wkey[w] > kmax ? es.wkey[w] : kmax;
    const float M = smp_key_value(kmax);

    if (tid < n_win) {
        const int t = es.win[tid];
        int cnt = 0;
        bool owner = true;
        for (int j = 0; j < n_win; j++) {
            const bool same = es.win[j] == t;
            cnt += same ? 1 : 0;
            owner = owner && !(same && j < tid);
        }
        if (owner && (unsigned)t < (unsigned)V) {
            bool biased = false;
            float b = 0.f;
            for (int j = 0; j < n_bias; j++)
                if (es.btok[j] == t) { biased = true; b = es.bval[j]; }
            adj[t] = ctl_adjust(raw[t], cnt, biased, b, c.repeat_penalty, c.presence_penalty, c.frequency_penalty);
        }
    }
    if (tid < n_bias) {
        const int t = es.btok[tid];
        bool in_win = false;
        for (int j = 0; j < n_win; j++) in_win = in_win || es.win[j] == t;
        if (!in_win && (unsigned)t < (unsigned)V)
            adj[t] = ctl_adjust(raw[t], 0, true, es.bval[tid], c.repeat_penalty, c.presence_penalty, c.frequency_penalty);
    }
    __syncthreads();  // adj holds l'; wkey is reused below
    mask(adj, V);

    const bool minp = c.min_p > 0.f && c.samp.temperature > 0.f;
    float s = 0.f;
    kmax = 0;
    for (int i = tid; i < V; i += SMP_THREADS) {
        s += expf(raw[i] - M);
        if (minp) {
            const uint32_t k = smp_key(adj[i]);
            kmax = k > kmax ? k : kmax;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s += __shfl_xor(s, o, 64);
        const uint32_t other = __shfl_xor(kmax, o, 64);
        kmax = other > kmax ? other : kmax;
    }
    if (lane == 0) { es.wsum[wid] = s; es.wkey[wid] = kmax; }
    __syncthreads();
    s = 0.f;
    kmax = 0;
#pragma unroll
    for (int w = 0; w < SMP_WAVES; w++) {
        s += es.wsum[w];
        kmax = es.wkey[w] > kmax ? es.wkey[w] : kmax;
    }
    ExtPrep out;
    out.M = M;
    out.lse = logf(s);
    out.top_k = c.samp.top_k;
    const float m = smp_key_value(kmax);
    if (minp && m > -INFINITY && m < INFINITY) {
        unsigned n = 0;
        for (int i = tid; i < V; i += SMP_THREADS) n += expf((adj[i] - m) / c.samp.temperature) >= c.min_p ? 1u : 0u;
        n = smp_wave_sum(n);
        if (lane == 0) es.wcnt[wid] = n;
        __syncthreads();
        n = 0;
#pragma unroll
        for (int w = 0; w < SMP_WAVES; w++) n += es.wcnt[w];
        if (n >= 1 && (int)n < V && (out.top_k <= 0 || (int)n < out.top_k)) out.top_k = (int)n;
    }
    return out;
}

}  // namespace xalm
