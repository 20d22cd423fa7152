// sample_dfa.h — the byte-DFA token mask in the sampling workgroup (the definition:
// include/xalm_hip.h, xh_byte_dfa).  It runs as ext_prepare's hook, once the adjusted logits l' are
// whole and before anything is computed from them:
//   1. the current state's row of `next` (the whole table when it has at most DFA_LDS_STATES
//      states) goes to LDS;
//   2. threads stride over the vocabulary, DFA_UNROLL tokens each at a time so their walks' loads
//      overlap: a token's piece is walked byte by byte from the current state, the first byte
//      through the LDS row; a forbidden token gets -inf in `adj`, an allowed one keeps its bits;
//   3. the allowed tokens are counted and their first maximum in the sampler's order is found (the
//      constrained greedy token: no FLT_MIN rule here, token 0 may be forbidden).
// min-p, top-k, top-p and the draw then see the masked logits.  State ids are unsigned throughout:
// uint16_t in the tables, uint32_t in registers.
#pragma once

#include "sample_ext.h"

namespace xalm {

constexpr int DFA_LDS_STATES = 8;  // tables up to this many states are walked from LDS alone
constexpr int DFA_UNROLL = 4;

struct DfaShared {
    uint16_t tab[DFA_LDS_STATES * 256];
    unsigned long long wbest[SMP_WAVES];
    unsigned wcnt[SMP_WAVES];
    unsigned long long best;  // argmax_key of the first allowed maximum, 0 = none
    unsigned n_allowed;
};

__device__ __forceinline__ int dfa_stuck_token(const DfaCtl& d) { return d.stop_a >= 0 ? d.stop_a : d.stop_b >= 0 ? d.stop_b : 0; }

// the successor of `state` under token t (one thread): an end token stays where the text may end
__device__ inline uint32_t dfa_advance(const DfaCtl& d, const uint32_t state, const int t) {
    if (state == XH_DFA_DEAD) return XH_DFA_DEAD;
    if (t == d.stop_a || t == d.stop_b) return d.accept[state] ? state : (uint32_t)XH_DFA_DEAD;
    const uint32_t lo = d.offsets[t], hi = d.offsets[t + 1];
    if (lo == hi) return XH_DFA_DEAD;
    uint32_t s = state;
    for (uint32_t i = lo; i < hi && s != XH_DFA_DEAD; i++) s = d.next[(size_t)s * 256 + d.bytes[i]];
    return s;
}

struct DfaMask {
    DfaShared* ds;
    DfaCtl d;

    __device__ void operator()(float* adj, const int V) const {
        const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
        const uint32_t s0 = d.state;
        if (s0 == XH_DFA_DEAD) return;  // stuck: nothing is masked, the head emits the stuck token
        const bool small = d.n_states <= DFA_LDS_STATES;
        const int n_tab = small ? d.n_states * 256 : 256;
        const uint16_t* src = small ? d.next : d.next + (size_t)s0 * 256;
        for (int i = tid; i < n_tab; i += SMP_THREADS) ds->tab[i] = src[i];
        __syncthreads();
        const uint16_t* row0 = ds->tab + (small ? s0 * 256 : 0u);
        const bool ends_ok = d.accept[s0] != 0;

        unsigned long long best = 0;
        unsigned cnt = 0;
        for (int base = tid; base < V; base += DFA_UNROLL * SMP_THREADS) {
            uint32_t at[DFA_UNROLL], end[DFA_UNROLL], st[DFA_UNROLL];
            bool is_end[DFA_UNROLL];
            uint32_t longest = 0;
#pragma unroll
            for (int j = 0; j < DFA_UNROLL; j++) {
                const int t = base + j * SMP_THREADS;
                at[j] = end[j] = 0;
                st[j] = XH_DFA_DEAD;
                is_end[j] = false;
                if (t < V) {
                    is_end[j] = t == d.stop_a || t == d.stop_b;
                    at[j] = d.offsets[t];
                    end[j] = d.offsets[t + 1];
                    if (is_end[j]) {
                        st[j] = ends_ok ? s0 : (uint32_t)XH_DFA_DEAD;
                        end[j] = at[j];
                    } else if (end[j] > at[j]) {
                        st[j] = row0[d.bytes[at[j]]];
                        at[j] += 1;
                    }
                    if (st[j] == XH_DFA_DEAD) end[j] = at[j];
                    longest = max(longest, end[j] - at[j]);
                }
            }
            for (uint32_t k = 0; k < longest; k++) {
                bool any = false;
#pragma unroll
                for (int j = 0; j < DFA_UNROLL; j++) {
                    if (at[j] < end[j]) {
                        const uint32_t b = d.bytes[at[j]];
                        const uint32_t s = small ? ds->tab[st[j] * 256 + b] : d.next[(size_t)st[j] * 256 + b];
                        st[j] = s;
                        at[j] = s == XH_DFA_DEAD ? end[j] : at[j] + 1;
                        any = any || at[j] < end[j];
                    }
                }
                if (!any) break;
            }
#pragma unroll
            for (int j = 0; j < DFA_UNROLL; j++) {
                const int t = base + j * SMP_THREADS;
                if (t < V) {
                    if (st[j] == XH_DFA_DEAD) {
                        adj[t] = -INFINITY;
                    } else {
                        cnt++;
                        const unsigned long long k = argmax_key(adj[t], t);
                        best = k > best ? k : best;
                    }
                }
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long other = __shfl_xor(best, o, 64);
            best = other > best ? other : best;
        }
        cnt = smp_wave_sum(cnt);
        if (lane == 0) { ds->wbest[wid] = best; ds->wcnt[wid] = cnt; }
        __syncthreads();
        if (tid == 0) {
            best = 0;
            cnt = 0;
            for (int w = 0; w < SMP_WAVES; w++) {
                best = ds->wbest[w] > best ? ds->wbest[w] : best;
                cnt += ds->wcnt[w];
            }
            ds->best = best;
            ds->n_allowed = cnt;
        }
        // the head reads best / n_allowed behind ext_prepare's later barriers
    }
};

// What one masked draw gives: the token, the size of the kept set (stuck: 0) and the successor
// state.  Every thread calls it after ext_prepare ran with DfaMask on `adj`; `pr` is its result.
struct DfaDraw {
    int token, n_kept;
    uint32_t state;
};
__device__ DfaDraw dfa_draw(SampleShared& sh, const DfaShared& ds, const float* adj, const int V, const ExtCtl& c,
                            const ExtPrep& pr, const DfaCtl& d, const uint32_t pos) {
    DfaDraw out;
    if (d.state == XH_DFA_DEAD || ds.n_allowed == 0) {
        out.token = dfa_stuck_token(d);
        out.n_kept = 0;
        out.state = XH_DFA_DEAD;
        return out;
    }
    if (c.samp.temperature == 0.f) {
        out.token = argmax_key_index(ds.best);
        out.n_kept = 1;
    } else {
        xh_sampling p = c.samp;
        p.top_k = pr.top_k;
        out.token = sample_token(sh, adj, V, p, pos, &out.n_kept);
    }
    out.state = dfa_advance(d, d.state, out.token);
    return out;
}

}  // namespace xalm
