// sample_seq.h — DRY, the no-repeat-n-gram ban and XTC in the sampling workgroup (the definition:
// include/xalm_hip.h, xh_seq_ctl).  Two stages around sample_adapt.h's:
//   sequence stage, in ext_prepare's hook in front of the DFA mask (seq_adjust):
//     1. the sequence window, one token per thread, from the ring the step head appends to, and the
//        sorted breaker list, into LDS; each thread's breaker flag by a binary search in it;
//     2. thread j with w[j] == w[n-1] walks back at most XH_SEQ_MAX_MATCH steps and leaves raw_j and
//        dry_j (the walk's length, and its length up to the first breaker of the suffix);
//     3. the lowest j of every distinct follower c = w[j+1] takes the maxima rep_c and ng_c over the
//        window (integers: the order does not matter) and writes l'_c: the f32 penalty loop
//        (seq_dry_adjust, shared with the host), then the ban;
//     4. a barrier: the writes are scattered, and the DFA mask and ext_prepare's later passes read
//        every entry.
//   XTC, between adapt_prepare and adapt_draw (seq_xtc): the coin from Philox word x1 at the draw's
//   counter; when it fires the exact integer sum S_C over C (the typical stage's survivors, else the
//   prefix through adp_prefix), the count and the lowest key of A = {M_i >= ceil(threshold * S_C)}
//   in one pass, the highest index of that key in C in another, and -inf over A minus that token and
//   over everything outside C in a last one.  sample_token then runs with top-k off.
// The sequence stage's arrays overlay SampleShared (a union in the kernels): nothing of the sampler
// runs before the hook returns, and the kernel's static LDS stays what sample_adapt_embed_kernel's is.
#pragma once

#include "sample_adapt.h"
#include "seq_host.h"

namespace xalm {

static_assert(XH_SEQ_MAX_BREAKERS <= SMP_THREADS, "one breaker per thread");
static_assert(XH_SEQ_MAX_MATCH < 256, "match lengths are packed in bytes");

struct SeqShared {
    int win[EXT_RING];
    int brk[XH_SEQ_MAX_BREAKERS];
    uint16_t mlen[EXT_RING];  // dry_j | raw_j << 8
    uint8_t isbrk[EXT_RING];
};
union SeqSampleShared {
    SampleShared sh;
    SeqShared sq;
};

// Every thread calls it once l' is whole (ext_prepare's hook).  `count` tokens are in the ring, `brk`
// holds the breakers in ascending order.  rep_out / ng_out (NULL in the step head): rep_c / ng_c of
// the followers, the other entries are left as they are.
__device__ void seq_adjust(SeqShared& sq, float* adj, const int V, const SeqCtl* ctl, const int count, const int* ring,
                           const int* brk, int* rep_out, int* ng_out) {
    const int tid = threadIdx.x;
    const SeqCtl q = *ctl;  // read here, not in the kernel's prologue: its scalars live for this stage only
    const bool dry = q.dry_multiplier > 0.f, ban = q.ngram >= 2;
    const int n = min(min(q.last_n, count), EXT_RING);
    if ((!dry && !ban) || n < 2) return;  // uniform over the workgroup
    const int nb = min(q.n_breakers, XH_SEQ_MAX_BREAKERS);
    if (tid < n) sq.win[tid] = ring[(count - n + tid) & (EXT_RING - 1)];
    if (tid < nb) sq.brk[tid] = brk[tid];
    __syncthreads();
    if (tid < n) {
        const int t = sq.win[tid];
        int lo = 0, hi = nb;  // the first entry >= t
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (sq.brk[mid] < t) lo = mid + 1;
            else hi = mid;
        }
        sq.isbrk[tid] = lo < nb && sq.brk[lo] == t ? 1 : 0;
    }
    __syncthreads();
    if (tid < n - 1) {
        int raw = 0, dr = 0;
        if (sq.win[tid] == sq.win[n - 1]) {
            const int lim = min(tid + 1, XH_SEQ_MAX_MATCH);
            bool clean = true;
            while (raw < lim && sq.win[tid - raw] == sq.win[n - 1 - raw]) {
                clean = clean && !sq.isbrk[n - 1 - raw];
                raw++;
                if (clean) dr = raw;
            }
        }
        sq.mlen[tid] = (uint16_t)(dr | (raw << 8));
    }
    __syncthreads();
    if (tid < n - 1) {
        const int c = sq.win[tid + 1];
        int rep = 0, ng = 0;
        bool owner = true;
        for (int j = 0; j < n - 1; j++) {
            if (sq.win[j + 1] == c) {
                owner = owner && j >= tid;
                const int ml = sq.mlen[j];
                rep = max(rep, ml & 255);
                ng = max(ng, ml >> 8);
            }
        }
        if (owner && (unsigned)c < (unsigned)V) {
            if (rep_out) rep_out[c] = rep;
            if (ng_out) ng_out[c] = ng;
            float v = adj[c];
            bool touched = false;
            if (dry && rep >= q.dry_allowed) {
                v = seq_dry_adjust(v, q.dry_multiplier, q.dry_base, rep - q.dry_allowed);
                touched = true;
            }
            if (ban && ng >= q.ngram - 1) {
                v = -INFINITY;
                touched = true;
            }
            if (touched) adj[c] = v;
        }
    }
    __syncthreads();  // the owners' writes are scattered: whole before the mask and ext_prepare's step 4
}

// the hook: the sequence stage, a copy of l' behind it when asked for (xh_op_sample_seq's
// adjusted_out), then the DFA mask
struct SeqMask {
    SeqShared* sq;
    const SeqCtl* q;
    int count;
    const int* ring;
    const int* brk;
    int* rep_out;
    int* ng_out;
    float* snap;
    AdaptMask dfa;
    __device__ void operator()(float* adj, const int V) const {
        seq_adjust(*sq, adj, V, q, count, ring, brk, rep_out, ng_out);
        if (snap)
            for (int i = threadIdx.x; i < V; i += SMP_THREADS) snap[i] = adj[i];
        dfa(adj, V);
    }
};

__device__ __forceinline__ uint32_t seq_max_u32(AdaptShared& as, uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t other = __shfl_xor(v, o, 64);
        v = other > v ? other : v;
    }
    if ((threadIdx.x & 63) == 0) as.wk[threadIdx.x >> 6] = v;
    __syncthreads();
    v = 0;
#pragma unroll
    for (int w = 0; w < SMP_WAVES; w++) v = as.wk[w] > v ? as.wk[w] : v;
    __syncthreads();
    return v;
}

// XTC for the draw at counter `pos`; every thread calls it (temperature > 0, not stuck,
// xtc_probability > 0) after adapt_prepare.  fired: the coin.  When tokens are removed, ap is what
// adapt_draw needs for the survivors (top-k off, their number in n_typ) and kept_out (may be NULL)
// their 0/1 map; otherwise ap is the caller's and kept_out is left as it is.
struct SeqXtc {
    AdaptPrep ap;
    bool fired;
};
__device__ __forceinline__ SeqXtc seq_xtc(SampleShared& sh, AdaptShared& as, float* adj, const int V, const ExtCtl& c,
                                          const float xtc_p, const float xtc_thr, const AdaptPrep& ap, const uint32_t pos,
                                          uint8_t* kept_out) {
    const int tid = threadIdx.x;
    SeqXtc out;
    out.ap = ap;
    out.fired = false;
    uint32_t x[4] = {pos, 0u, 0u, 0u};
    philox4x32_10((uint32_t)c.samp.seed, (uint32_t)(c.samp.seed >> 32), x);
    const float u = (float)(x[1] >> 8) * 5.9604644775390625e-8f;  // 2^-24: exact
    if (!(u < xtc_p)) return out;
    out.fired = true;
    const float temp = c.samp.temperature;
    const bool typ = ap.n_typ >= 0;
    const float m = typ ? ap.m : smp_key_value(adp_max_key(as, adj, V));
    if (!(m > -INFINITY) || m == INFINITY) return out;  // no finite logit: sample_token's rule
    AdaptPrefix cp;
    cp.all = true;
    cp.t = 0;
    cp.e = V;
    if (!typ) cp = adp_prefix(sh, adj, V, m, temp, ap.n_prefix);
    unsigned long long S = 0;
    for (int i = tid; i < V; i += SMP_THREADS) {
        const float l = adj[i];
        if (typ ? l != -INFINITY : cp.has(l, i)) S += smp_mass(l, m, temp);
    }
    S = adp_sum(as, S);
    const unsigned long long cut = (unsigned long long)ceil((double)xtc_thr * (double)S);  // <= S < 2^57
    unsigned n_a = 0;
    uint32_t kinv = 0;  // ~key of A's lowest key
    for (int i = tid; i < V; i += SMP_THREADS) {
        const float l = adj[i];
        if ((typ ? l != -INFINITY : cp.has(l, i)) && smp_mass(l, m, temp) >= cut) {
            n_a++;
            const uint32_t k = ~smp_key(l);
            kinv = k > kinv ? k : kinv;
        }
    }
    n_a = adp_sum(as, n_a);
    if (n_a < 2) return out;
    const uint32_t kmin = ~seq_max_u32(as, kinv);
    // A's last token: the highest index of its lowest key in C (equal keys carry equal masses)
    uint32_t last1 = 0;
    for (int i = tid; i < V; i += SMP_THREADS) {
        const float l = adj[i];
        if (smp_key(l) == kmin && (typ ? l != -INFINITY : cp.has(l, i))) last1 = (uint32_t)i + 1u;
    }
    const int last = (int)seq_max_u32(as, last1) - 1;
    const unsigned n_c = typ ? (unsigned)ap.n_typ : ap.n_prefix > 0 ? (unsigned)ap.n_prefix : (unsigned)V;
    for (int i = tid; i < V; i += SMP_THREADS) {
        const float l = adj[i];
        const bool in_c = typ ? l != -INFINITY : cp.has(l, i);
        const bool keep = in_c && (i == last || smp_mass(l, m, temp) < cut);
        if (!keep) adj[i] = -INFINITY;
        if (kept_out) kept_out[i] = keep ? 1 : 0;
    }
    __syncthreads();  // adj is whole for the sampler
    out.ap.top_k = 0;
    out.ap.n_typ = (int)(n_c - (n_a - 1u));
    return out;
}

// Sequence-aware sampled decode step head (xh_decode_sample_seq): sample_adapt_embed_kernel's work
// with the sequence stage in front of the mask and XTC in front of the draw.
__global__ __launch_bounds__(SMP_THREADS) void sample_seq_embed_kernel(
    const float* logits, int vocab, ExtCtl* ctl, DfaCtl* dfa, AdaptCtl* actl, const SeqCtl* sctl, int* ring, const int* btok,
    const float* bval, const int* brk, float* adj, float* negd, StepParams* sp, const SeqTail* tail) {
    __shared__ SeqSampleShared ss;
    __shared__ ExtShared es;
    __shared__ DfaShared ds;
    __shared__ AdaptShared as;
    __shared__ int pos_s;
    SampleShared& sh = ss.sh;
    const int tid = threadIdx.x;
    const ExtCtl c = *ctl;
    const bool constrain = actl->constrain != 0;
    const ExtPrep pr = ext_prepare(es, logits, adj, vocab, c, ring, btok, bval,
                                   SeqMask{&ss.sq, sctl, c.count, ring, brk, nullptr, nullptr, nullptr,
                                           AdaptMask{constrain, DfaMask{&ds, *dfa}}});
    const AdaptCtl a = *actl;  // likewise
    const DfaCtl d = *dfa;  // unconstrained: never dereferenced; read again behind the mask, not held across it
    const bool stuck = a.constrain && (d.state == XH_DFA_DEAD || ds.n_allowed == 0);
    const uint32_t pos = (uint32_t)sp->pos_next;
    AdaptPrep ap;
    ap.top_k = pr.top_k;
    ap.n_typ = -1;
    ap.K = 0;
    if (c.samp.temperature > 0.f && !stuck) {
        ap = adapt_prepare(sh, as, adj, negd, vocab, c, a, pr);
        const float xtc_p = sctl->xtc_p;
        if (xtc_p > 0.f) ap = seq_xtc(sh, as, adj, vocab, c, xtc_p, sctl->xtc_thr, ap, pos, nullptr).ap;
    }
    const AdaptDraw dr = adapt_draw(sh, ds, adj, vocab, c, a, ap, d, pos);
    const int tok = dr.token;
    __syncthreads();  // every thread has read pos_next, the blocks and the ring
    if (tid == 0) {  // the tail's fields are read where they are used: see SeqTail
        if (sp->step < tail->cap) {
            tail->tokens[sp->step] = tok;
            tail->logprobs[sp->step] = (logits[tok] - pr.M) - pr.lse;
            tail->states[sp->step] = dr.state;
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
    rope_table(tail->rope_cs, tail->rope_freq, tail->half, pos_s, tid);
    const int dim = tail->dim, dtype = tail->dtype;
    const void* emb = tail->emb;
    float* x = tail->x;
    for (int i = tid; i < dim; i += SMP_THREADS) x[i] = dec_row(dtype, emb, (size_t)tok, dim, i);
}

// xh_op_sample_seq: one workgroup prepares l'' (adjusted, sequence-adjusted, masked, truncated), the
// scalars of the draw and the 0/1 map of C ...
__global__ __launch_bounds__(SMP_THREADS) void sample_seq_prep_kernel(const float* logits, int vocab, const ExtCtl* ctl,
                                                                      const DfaCtl* dfa, const AdaptCtl* actl,
                                                                      const SeqCtl* sctl, const int* ring, const int* btok,
                                                                      const float* bval, const int* brk, float* adj,
                                                                      float* negd, float* snap, int* rep_out, int* ng_out,
                                                                      uint8_t* kept, AdaptOpPrep* prep) {
    __shared__ SeqSampleShared ss;
    __shared__ ExtShared es;
    __shared__ DfaShared ds;
    __shared__ AdaptShared as;
    SampleShared& sh = ss.sh;
    const int tid = threadIdx.x;
    const ExtCtl c = *ctl;
    const AdaptCtl a = *actl;
    const DfaCtl d = *dfa;
    const ExtPrep pr = ext_prepare(es, logits, adj, vocab, c, ring, btok, bval,
                                   SeqMask{&ss.sq, sctl, c.count, ring, brk, rep_out, ng_out, snap,
                                           AdaptMask{a.constrain != 0, DfaMask{&ds, d}}});
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
// ... and workgroup i copies them to rows of its own, runs XTC and draws at counter pos0 + i, every
// draw from the same state and mu
__global__ __launch_bounds__(SMP_THREADS) void sample_seq_op_kernel(const float* adj0, const uint8_t* kept0, float* adj_rows,
                                                                    uint8_t* kept_rows, int vocab, const ExtCtl* ctl,
                                                                    const DfaCtl* dfa, const AdaptCtl* actl,
                                                                    const SeqCtl* sctl, const AdaptOpPrep* prep,
                                                                    uint32_t pos0, int* tokens, int* n_kept_out,
                                                                    uint32_t* states, float* mu_out, int* fired_out) {
    __shared__ SampleShared sh;
    __shared__ DfaShared ds;
    __shared__ AdaptShared as;
    const int tid = threadIdx.x;
    const AdaptOpPrep pp = *prep;
    const ExtCtl c = *ctl;
    const AdaptCtl a = *actl;
    const SeqCtl q = *sctl;
    const DfaCtl d = *dfa;
    float* adj = adj_rows + (size_t)blockIdx.x * vocab;
    uint8_t* kept = kept_rows + (size_t)blockIdx.x * vocab;
    for (int i = tid; i < vocab; i += SMP_THREADS) {
        adj[i] = adj0[i];
        kept[i] = kept0[i];
    }
    if (tid == 0) {
        ds.best = pp.best;
        ds.n_allowed = pp.n_allowed;
    }
    __syncthreads();
    const bool stuck = a.constrain && (d.state == XH_DFA_DEAD || ds.n_allowed == 0);
    const uint32_t pos = pos0 + blockIdx.x;
    AdaptPrep ap = pp.ap;
    bool fired = false;
    if (c.samp.temperature > 0.f && !stuck && q.xtc_p > 0.f) {
        const SeqXtc xo = seq_xtc(sh, as, adj, vocab, c, q.xtc_p, q.xtc_thr, ap, pos, kept);
        ap = xo.ap;
        fired = xo.fired;
    }
    const AdaptDraw dr = adapt_draw(sh, ds, adj, vocab, c, a, ap, d, pos);
    if (tid == 0) {
        tokens[blockIdx.x] = dr.token;
        n_kept_out[blockIdx.x] = dr.n_kept;
        states[blockIdx.x] = dr.state;
        mu_out[blockIdx.x] = dr.mu;
        fired_out[blockIdx.x] = fired ? 1 : 0;
    }
}

}  // namespace xalm
