// sample_adapt.h — top-n-sigma, locally typical and Mirostat v2 truncation in the sampling workgroup
// (the definition: include/xalm_hip.h, xh_trunc_ctl).  Between ext_prepare (with the DFA mask when
// constrained) and sample_token, adapt_prepare
//   1. finds the maximum m of l'' (one pass);
//   2. n-sigma: sums the finite l'' and then their squared deviations in double (two passes, a fixed
//      order: each thread its strided entries, the butterfly of a wave, the waves in turn), and
//      counts n_sigma = #{ l'' >= thr } (one pass): a prefix of the order, an effective top-k;
//   3. Mirostat: sums the masses, and counts and sums those at or above the cut (two passes):
//      again an effective top-k, and the kept mass K the update needs;
//   4. typical: selects the prefix C (smp_select<false>; where the k-th key's tokens are kept only
//      in part, adp_tie_limit gives the index below which they are), sums C's masses, then
//      H = sum p s in f32 in the fixed order, writes -|s - H| (-inf outside C and for massless
//      tokens) to `negd`, selects by mass over negd's keys (adp_select_mass, a sibling of
//      smp_select<true> whose keys and masses come from two buffers), resolves the last key's
//      tokens by index (adp_tie_limit: equal d need not mean equal mass) and writes -inf over the
//      dropped entries of `adj`.
// adapt_draw then runs sample_token on `adj` (top-k off after the typical stage) and Mirostat's
// update.  The kept sets are decided on integers: keys, indices and masses.
#pragma once

#include "sample_dfa.h"
#include "truncate.h"

namespace xalm {

struct AdaptShared {
    double wd[SMP_WAVES];
    unsigned long long wm[SMP_WAVES];
    float wf[SMP_WAVES];
    unsigned wc[SMP_WAVES];
    uint32_t wk[SMP_WAVES];
};

// Block sums in a fixed order; every thread calls them and gets the result.
__device__ __forceinline__ double adp_sum(AdaptShared& as, double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) as.wd[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < SMP_WAVES; w++) s += as.wd[w];
    __syncthreads();
    return s;
}
__device__ __forceinline__ float adp_sum(AdaptShared& as, float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) as.wf[threadIdx.x >> 6] = v;
    __syncthreads();
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < SMP_WAVES; w++) s += as.wf[w];
    __syncthreads();
    return s;
}
__device__ __forceinline__ unsigned long long adp_sum(AdaptShared& as, unsigned long long v) {
    v = smp_wave_sum(v);
    if ((threadIdx.x & 63) == 0) as.wm[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned long long s = 0;
#pragma unroll
    for (int w = 0; w < SMP_WAVES; w++) s += as.wm[w];
    __syncthreads();
    return s;
}
__device__ __forceinline__ unsigned adp_sum(AdaptShared& as, unsigned v) {
    v = smp_wave_sum(v);
    if ((threadIdx.x & 63) == 0) as.wc[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned s = 0;
#pragma unroll
    for (int w = 0; w < SMP_WAVES; w++) s += as.wc[w];
    __syncthreads();
    return s;
}

// the key of the maximum of v[0..V)
__device__ inline uint32_t adp_max_key(AdaptShared& as, const float* v, const int V) {
    uint32_t kmax = 0;
    for (int i = threadIdx.x; i < V; i += SMP_THREADS) {
        const uint32_t k = smp_key(v[i]);
        kmax = k > kmax ? k : kmax;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t other = __shfl_xor(kmax, o, 64);
        kmax = other > kmax ? other : kmax;
    }
    if ((threadIdx.x & 63) == 0) as.wk[threadIdx.x >> 6] = kmax;
    __syncthreads();
    kmax = 0;
#pragma unroll
    for (int w = 0; w < SMP_WAVES; w++) kmax = as.wk[w] > kmax ? as.wk[w] : kmax;
    __syncthreads();
    return kmax;
}

// n-sigma: the threshold and the number of logits at or above it (the maximum always is)
__device__ inline unsigned adp_n_sigma(AdaptShared& as, const float* adj, const int V, const float m, const float n_sigma,
                                       float* thr_out) {
    const int tid = threadIdx.x;
    double s = 0.0;
    unsigned n = 0;
    for (int i = tid; i < V; i += SMP_THREADS) {
        const float v = adj[i];
        if (v > -INFINITY && v < INFINITY) { s += (double)v; n++; }
    }
    s = adp_sum(as, s);
    n = adp_sum(as, n);
    const double mean = s / (double)n;  // n >= 1: m is finite
    double q = 0.0;
    for (int i = tid; i < V; i += SMP_THREADS) {
        const float v = adj[i];
        if (v > -INFINITY && v < INFINITY) {
            const double d = (double)v - mean;
            q += d * d;
        }
    }
    q = adp_sum(as, q);
    const double sigma = sqrt(q / (double)n);
    const float thr = (float)((double)m - (double)n_sigma * sigma);
    unsigned c = 0;
    for (int i = tid; i < V; i += SMP_THREADS) c += adj[i] >= thr ? 1u : 0u;
    c = adp_sum(as, c);
    *thr_out = thr;
    return c < 1u ? 1u : c;
}

// Mirostat: the number of tokens whose mass reaches the cut, at least 1, and their mass
__device__ inline unsigned adp_mirostat(AdaptShared& as, const float* adj, const int V, const float m, const float temp,
                                        const float mu, unsigned long long* kept_mass) {
    const int tid = threadIdx.x;
    unsigned long long S = 0;
    for (int i = tid; i < V; i += SMP_THREADS) S += smp_mass(adj[i], m, temp);
    S = adp_sum(as, S);
    const unsigned long long cut = (unsigned long long)ceil((double)S * exp2(-(double)mu));  // <= S < 2^57
    unsigned n = 0;
    unsigned long long K = 0;
    for (int i = tid; i < V; i += SMP_THREADS) {
        const unsigned long long q = smp_mass(adj[i], m, temp);
        if (q >= cut) { n++; K += q; }
    }
    n = adp_sum(as, n);
    K = adp_sum(as, K);
    if (n == 0) {  // the cut lies above every mass: the first maximum alone, expf(0) * 2^40
        n = 1;
        K = (unsigned long long)SMP_MASS_ONE;
    }
    *kept_mass = K;
    return n;
}

// Among the tokens whose key in kb equals t, in index order: the index limit e such that those
// below e are the shortest run weighing at least `need` (MASS: each its mass from `logits`, else 1
// each).  V when they never reach it.  Wave w owns a contiguous range, as in sample_token's draw.
template <bool MASS>
__device__ int adp_tie_limit(SampleShared& sh, const float* kb, const float* logits, const int V, const uint32_t t,
                             const unsigned long long need, const float m, const float temp) {
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int sub = ((V + SMP_WAVES - 1) / SMP_WAVES + 63) & ~63;
    const int w_lo = min(wid * sub, V), w_hi = min(w_lo + sub, V);
    unsigned long long acc = 0;
    for (int i = w_lo + lane; i < w_hi; i += 64)
        if (smp_key(kb[i]) == t) acc += MASS ? smp_mass(logits[i], m, temp) : 1ull;
    acc = smp_wave_sum(acc);
    if (lane == 0) sh.wmass[wid] = acc;
    if (tid == 0) sh.token = V;
    __syncthreads();
    int owner = -1;
    unsigned long long base = 0;
    for (int w = 0; w < SMP_WAVES && owner < 0; w++) {
        if (base + sh.wmass[w] >= need) owner = w;
        else base += sh.wmass[w];
    }
    if (wid == owner) {  // one wave walks its range, 64 tokens at a time
        for (int c0 = w_lo; c0 < w_hi; c0 += 64) {
            const int i = c0 + lane;
            unsigned long long incl = 0;
            if (i < w_hi && smp_key(kb[i]) == t) incl = MASS ? smp_mass(logits[i], m, temp) : 1ull;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned long long other = __shfl_up(incl, o, 64);
                if (lane >= o) incl += other;
            }
            const unsigned long long hit = __ballot(base + incl >= need);
            if (hit) {
                if (lane == 0) sh.token = c0 + __ffsll((long long)hit);
                break;
            }
            base += __shfl(incl, 63, 64);
        }
    }
    __syncthreads();
    const int e = sh.token;
    __syncthreads();  // token and wmass are reused
    return e;
}

// smp_select<true> over every token with the keys taken from `keys` and the masses from `logits`
// (a token whose key is that of -inf has none): the key at which the mass from the top reaches
// ceil(frac * total).  On return sh.prefix, sh.above_cnt, sh.above_mass, sh.bin_cnt and sh.target
// as smp_select leaves them.
__device__ void adp_select_mass(SampleShared& sh, const float* keys, const float* logits, const int V, const float m,
                                const float temp, const float frac) {
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid == 0) {
        sh.prefix = 0;
        sh.above_cnt = 0;
        sh.above_mass = 0;
        sh.target = 0;
    }
    for (int level = 3; level >= 0; level--) {
        const int shift = 8 * level;
        const uint32_t hmask = level == 3 ? 0u : 0xffffffffu << (shift + 8);
        for (int i = tid; i < 256 * SMP_REP; i += SMP_THREADS) {
            sh.cnt[i] = 0;
            sh.mass[i] = 0;
        }
        __syncthreads();  // zeroed, and the previous level's state is visible
        const uint32_t prefix = sh.prefix;
        for (int i = tid; i < V; i += SMP_THREADS) {
            const float kd = keys[i];
            const uint32_t k = smp_key(kd);
            if ((k & hmask) == (prefix & hmask)) {
                const int slot = (int)((k >> shift) & 255u) * SMP_REP + (lane & (SMP_REP - 1));
                atomicAdd(&sh.cnt[slot], 1u);
                if (kd != -INFINITY) atomicAdd(&sh.mass[slot], smp_mass(logits[i], m, temp));
            }
        }
        __syncthreads();
        if (tid < 256) {
            unsigned c = 0;
            unsigned long long ms = 0;
#pragma unroll
            for (int r = 0; r < SMP_REP; r++) {
                c += sh.cnt[tid * SMP_REP + r];
                ms += sh.mass[tid * SMP_REP + r];
            }
            sh.bcnt[tid] = c;
            sh.bmass[tid] = ms;
        }
        __syncthreads();
        if (tid < 64) {
            // lane L holds bins 255 - 4L ... 252 - 4L: a scan from the top bin down
            unsigned c[4], csum = 0;
            unsigned long long ms[4], msum = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                c[j] = sh.bcnt[255 - 4 * lane - j];
                ms[j] = sh.bmass[255 - 4 * lane - j];
                csum += c[j];
                msum += ms[j];
            }
            unsigned cincl = csum;
            unsigned long long mincl = msum;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned co = __shfl_up(cincl, o, 64);
                const unsigned long long mo = __shfl_up(mincl, o, 64);
                if (lane >= o) { cincl += co; mincl += mo; }
            }
            unsigned long long target = sh.target;
            if (level == 3) {
                const unsigned long long total = __shfl(mincl, 63, 64);
                const double want = ceil((double)frac * (double)total);
                target = want >= (double)total ? total : (unsigned long long)want;
                if (target < 1) target = 1;
            }
            unsigned crun = sh.above_cnt + (cincl - csum);
            unsigned long long mrun = sh.above_mass + (mincl - msum);
            bool found = false;
            int fbin = 0;
            unsigned fc = 0, fac = 0;
            unsigned long long fam = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                if (!found && (mrun + ms[j] >= target || (lane == 63 && j == 3))) {  // the last bin always closes the scan
                    found = true;
                    fbin = 255 - 4 * lane - j;
                    fc = c[j];
                    fac = crun;
                    fam = mrun;
                }
                crun += c[j];
                mrun += ms[j];
            }
            const unsigned long long who = __ballot(found);
            if (lane == __ffsll((long long)who) - 1) {
                sh.prefix = prefix | ((uint32_t)fbin << shift);
                sh.above_cnt = fac;
                sh.above_mass = fam;
                sh.bin_cnt = fc;
                sh.target = target;
            }
        }
        __syncthreads();
    }
}

// The first n_eff tokens of the order (0 or >= V: every token): the keys above t, and of key t the
// tokens below index e.
struct AdaptPrefix {
    bool all;
    uint32_t t;
    int e;
    __device__ __forceinline__ bool has(const float l, const int i) const {
        const uint32_t k = smp_key(l);
        return all || k > t || (k == t && i < e);
    }
};
__device__ AdaptPrefix adp_prefix(SampleShared& sh, const float* adj, const int V, const float m, const float temp,
                                  const int n_eff) {
    AdaptPrefix c;
    c.all = n_eff <= 0 || n_eff >= V;
    c.t = 0;
    c.e = V;
    if (c.all) return c;
    smp_select<false>(sh, adj, V, m, temp, true, 0u, 0u, (unsigned long long)n_eff, 1.f);
    c.t = sh.prefix;
    const unsigned r = (unsigned)n_eff - sh.above_cnt, in_bin = sh.bin_cnt;
    __syncthreads();
    if (r < in_bin) c.e = adp_tie_limit<false>(sh, adj, adj, V, c.t, (unsigned long long)r, m, temp);
    return c;
}

// The typical stage over the prefix c: writes -inf over the dropped entries of adj; returns the
// number of tokens kept.
__device__ unsigned adp_typical(SampleShared& sh, AdaptShared& as, float* adj, float* negd, const int V, const float m,
                                const float temp, const AdaptPrefix c, const float typical_p) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x;
    unsigned long long S = 0;
    for (int i = tid; i < V; i += SMP_THREADS) {
        const float l = adj[i];
        if (c.has(l, i)) S += smp_mass(l, m, temp);
    }
    S = adp_sum(as, S);
    const float Sf = (float)S;  // > 0: the maximum is in the prefix
    float h = 0.f;
    for (int i = tid; i < V; i += SMP_THREADS) {
        const float l = adj[i];
        const unsigned long long q = c.has(l, i) ? smp_mass(l, m, temp) : 0ull;
        if (q) {
            const float p = (float)q / Sf;
            const float s = -logf(p);
            const float ps = p * s;
            h = h + ps;
        }
    }
    const float H = adp_sum(as, h);
    for (int i = tid; i < V; i += SMP_THREADS) {
        const float l = adj[i];
        const unsigned long long q = c.has(l, i) ? smp_mass(l, m, temp) : 0ull;
        float nd = -INFINITY;
        if (q) {
            const float s = -logf((float)q / Sf);
            nd = -fabsf(s - H);
        }
        negd[i] = nd;
    }
    __syncthreads();  // negd is whole
    adp_select_mass(sh, negd, adj, V, m, temp, typical_p);
    const uint32_t t = sh.prefix;
    const unsigned long long need = sh.target - sh.above_mass;  // > 0: the cut lies in this key's tokens
    __syncthreads();
    const int e = adp_tie_limit<true>(sh, negd, adj, V, t, need, m, temp);
    unsigned n = 0;
    for (int i = tid; i < V; i += SMP_THREADS) {
        const uint32_t k = smp_key(negd[i]);
        if (k > t || (k == t && i < e)) n++;
        else adj[i] = -INFINITY;
    }
    return adp_sum(as, n);  // its barriers also make adj whole
}

// What adapt_prepare leaves for the draw.
struct AdaptPrep {
    int top_k;                  // the effective top-k of sample_token: 0 after the typical stage
    int n_typ;                  // tokens the typical stage kept, -1 = it did not run
    float thr;                  // the n-sigma threshold, -inf = off
    float m;                    // the maximum of l''
    unsigned long long K;       // Mirostat's kept mass, 0 = off
    int n_prefix;               // the prefix stage's effective top-k (0 = every token)
};

// Every thread calls it (temperature > 0, not stuck) after ext_prepare left l'' in adj; `pr` is its
// result.
__device__ AdaptPrep adapt_prepare(SampleShared& sh, AdaptShared& as, float* adj, float* negd, const int V,
                                   const ExtCtl& c, const AdaptCtl& a, const ExtPrep& pr) {
    AdaptPrep o;
    o.top_k = pr.top_k;
    o.n_typ = -1;
    o.thr = -INFINITY;
    o.m = -INFINITY;
    o.K = 0;
    o.n_prefix = pr.top_k > 0 && pr.top_k < V ? pr.top_k : 0;
    const bool sig = a.top_n_sigma > 0.f, typ = a.typical_p < 1.f, miro = a.tau > 0.f;
    if (!sig && !typ && !miro) return o;
    const float m = smp_key_value(adp_max_key(as, adj, V));
    o.m = m;
    if (!(m > -INFINITY) || m == INFINITY) return o;  // no finite logit: sample_token's rule
    const float temp = c.samp.temperature;
    int n_eff = o.n_prefix;
    if (sig) {
        const unsigned n = adp_n_sigma(as, adj, V, m, a.top_n_sigma, &o.thr);
        if ((int)n < V && (n_eff == 0 || (int)n < n_eff)) n_eff = (int)n;
    }
    if (miro) {
        const unsigned n = adp_mirostat(as, adj, V, m, temp, a.mu, &o.K);
        n_eff = (int)n < V ? (int)n : 0;
    }
    o.n_prefix = n_eff;
    o.top_k = n_eff;
    if (typ) {
        const AdaptPrefix cp = adp_prefix(sh, adj, V, m, temp, n_eff);
        o.n_typ = (int)adp_typical(sh, as, adj, negd, V, m, temp, cp, a.typical_p);
        o.top_k = 0;
    }
    return o;
}

// What one draw gives: the token, the size of the final kept set (stuck: 0), the successor state
// (unconstrained: the state as it was) and mu after the token.
struct AdaptDraw {
    int token, n_kept;
    uint32_t state;
    float mu;
};
__device__ AdaptDraw adapt_draw(SampleShared& sh, const DfaShared& ds, const float* adj, const int V, const ExtCtl& c,
                                const AdaptCtl& a, const AdaptPrep& ap, const DfaCtl& d, const uint32_t pos) {
    AdaptDraw out;
    out.mu = a.mu;
    out.state = d.state;
    if (a.constrain && (d.state == XH_DFA_DEAD || ds.n_allowed == 0)) {
        out.token = dfa_stuck_token(d);
        out.n_kept = 0;
        out.state = XH_DFA_DEAD;
        return out;
    }
    if (a.constrain && c.samp.temperature == 0.f) {
        out.token = argmax_key_index(ds.best);
        out.n_kept = 1;
    } else {
        xh_sampling p = c.samp;
        p.top_k = ap.top_k;
        out.token = sample_token(sh, adj, V, p, pos, &out.n_kept);
        if (p.temperature > 0.f) {
            if (ap.n_typ >= 0 && !(p.top_p < 1.f)) out.n_kept = ap.n_typ;
            if (ap.K) {
                const unsigned long long q = smp_mass(adj[out.token], ap.m, p.temperature);
                if (q) out.mu = trunc_mu_next(a.mu, a.eta, a.tau, ap.K, q);
            }
        }
    }
    if (a.constrain) out.state = dfa_advance(d, d.state, out.token);
    return out;
}

// the DFA mask when the block asks for it (the flag is uniform over the workgroup)
struct AdaptMask {
    bool on;
    DfaMask mask;
    __device__ void operator()(float* adj, const int V) const {
        if (on) mask(adj, V);
    }
};

// Adaptive sampled decode step head (xh_decode_sample_adapt): sample_dfa_embed_kernel's work with the
// truncation stages between the mask and the draw; mu and the DFA state live in their blocks.
__global__ __launch_bounds__(SMP_THREADS) void sample_adapt_embed_kernel(
    const float* logits, int vocab, ExtCtl* ctl, DfaCtl* dfa, AdaptCtl* actl, int* ring, const int* btok, const float* bval,
    float* adj, float* negd, StepParams* sp, int* tokens, float* logprobs, uint32_t* states, int cap, const void* emb,
    int dtype, int dim, float* x, const float* rope_freq, float* rope_cs, int half) {
    __shared__ SampleShared sh;
    __shared__ ExtShared es;
    __shared__ DfaShared ds;
    __shared__ AdaptShared as;
    __shared__ int pos_s;
    const int tid = threadIdx.x;
    const ExtCtl c = *ctl;
    const AdaptCtl a = *actl;
    const DfaCtl d = *dfa;  // unconstrained: never dereferenced
    const ExtPrep pr = ext_prepare(es, logits, adj, vocab, c, ring, btok, bval, AdaptMask{a.constrain != 0, DfaMask{&ds, d}});
    const bool stuck = a.constrain && (d.state == XH_DFA_DEAD || ds.n_allowed == 0);
    AdaptPrep ap;
    ap.top_k = pr.top_k;
    ap.n_typ = -1;
    ap.K = 0;
    if (c.samp.temperature > 0.f && !stuck) ap = adapt_prepare(sh, as, adj, negd, vocab, c, a, pr);
    const AdaptDraw dr = adapt_draw(sh, ds, adj, vocab, c, a, ap, d, (uint32_t)sp->pos_next);
    const int tok = dr.token;
    __syncthreads();  // every thread has read pos_next, the blocks and the ring
    if (tid == 0) {
        if (sp->step < cap) {
            tokens[sp->step] = tok;
            logprobs[sp->step] = (logits[tok] - pr.M) - pr.lse;
            states[sp->step] = dr.state;
        }
        if (a.constrain) dfa->state = dr.state;
        actl->mu = dr.mu;
        ring[c.count & (EXT_RING - 1)] = tok;
        ctl->count = c.count + 1;
        sp->step += 1;
        sp->token = tok;
        step_positions(sp, sp->pos_next);
        sp->pos_next += 1;
        pos_s = sp->pos;
    }
    __syncthreads();
    rope_table(rope_cs, rope_freq, half, pos_s, tid);
    for (int i = tid; i < dim; i += SMP_THREADS) x[i] = dec_row(dtype, emb, (size_t)tok, dim, i);
}

// xh_op_sample_adapt: one workgroup prepares the masked and truncated l'', the scalars of the draw
// and the 0/1 map of the set after the typical stage ...
struct AdaptOpPrep {
    ExtPrep ext;
    AdaptPrep ap;
    unsigned long long best;
    unsigned n_allowed;
};
__global__ __launch_bounds__(SMP_THREADS) void sample_adapt_prep_kernel(const float* logits, int vocab, const ExtCtl* ctl,
                                                                        const DfaCtl* dfa, const AdaptCtl* actl,
                                                                        const int* ring, const int* btok, const float* bval,
                                                                        float* adj, float* negd, uint8_t* kept,
                                                                        AdaptOpPrep* prep) {
    __shared__ SampleShared sh;
    __shared__ ExtShared es;
    __shared__ DfaShared ds;
    __shared__ AdaptShared as;
    const int tid = threadIdx.x;
    const ExtCtl c = *ctl;
    const AdaptCtl a = *actl;
    const DfaCtl d = *dfa;
    const ExtPrep pr = ext_prepare(es, logits, adj, vocab, c, ring, btok, bval, AdaptMask{a.constrain != 0, DfaMask{&ds, d}});
    const bool stuck = a.constrain && (d.state == XH_DFA_DEAD || ds.n_allowed == 0);
    AdaptPrep ap;
    ap.top_k = pr.top_k;
    ap.n_typ = -1;
    ap.thr = -INFINITY;
    ap.m = -INFINITY;
    ap.K = 0;
    ap.n_prefix = 0;
    const bool drawn = c.samp.temperature > 0.f && !stuck;
    if (drawn) ap = adapt_prepare(sh, as, adj, negd, vocab, c, a, pr);
    // the map: the survivors of the typical stage, else the prefix; all 0 when nothing is drawn from
    // a kept set (greedy, stuck, no finite logit)
    const float m = drawn ? smp_key_value(adp_max_key(as, adj, vocab)) : -INFINITY;
    if (m > -INFINITY && m < INFINITY && ap.n_typ < 0) {
        const AdaptPrefix cp = adp_prefix(sh, adj, vocab, m, c.samp.temperature, ap.n_prefix);
        for (int i = tid; i < vocab; i += SMP_THREADS) kept[i] = cp.has(adj[i], i) ? 1 : 0;
    } else {
        for (int i = tid; i < vocab; i += SMP_THREADS) kept[i] = ap.n_typ >= 0 && adj[i] > -INFINITY ? 1 : 0;
    }
    if (tid == 0) {
        prep->ext = pr;
        prep->ap = ap;
        prep->best = !a.constrain || d.state == XH_DFA_DEAD ? 0ull : ds.best;
        prep->n_allowed = !a.constrain || d.state == XH_DFA_DEAD ? 0u : ds.n_allowed;
    }
}
// ... and workgroup i draws at counter pos0 + i from it, every draw from the same state and mu
__global__ __launch_bounds__(SMP_THREADS) void sample_adapt_op_kernel(const float* adj, int vocab, const ExtCtl* ctl,
                                                                      const DfaCtl* dfa, const AdaptCtl* actl,
                                                                      const AdaptOpPrep* prep, uint32_t pos0, int* tokens,
                                                                      int* n_kept_out, uint32_t* states, float* mu_out) {
    __shared__ SampleShared sh;
    __shared__ DfaShared ds;
    const AdaptOpPrep pp = *prep;
    if (threadIdx.x == 0) {
        ds.best = pp.best;
        ds.n_allowed = pp.n_allowed;
    }
    __syncthreads();
    const AdaptDraw dr = adapt_draw(sh, ds, adj, vocab, *ctl, *actl, pp.ap, *dfa, pos0 + blockIdx.x);
    if (threadIdx.x == 0) {
        tokens[blockIdx.x] = dr.token;
        n_kept_out[blockIdx.x] = dr.n_kept;
        states[blockIdx.x] = dr.state;
        mu_out[blockIdx.x] = dr.mu;
    }
}

}  // namespace xalm
