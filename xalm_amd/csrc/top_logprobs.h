// top_logprobs.h — the n_top most likely tokens of a logits row with their log-probabilities, and
// the log-probability and rank of a target token, in one 1024-thread workgroup per row (the
// definition: include/xalm_hip.h, XH_TOP_MAX).  What decides an id or a rank is an integer: the
// sampler's keys (smp_key, sample.h), counts of them, and indices.  Five passes over the row, each
// with consecutive lanes on consecutive indices:
//   A  the maximum key (M), the target's rank (keys above it, plus equal keys at a lower index),
//      and the count histogram of the top key digit
//   B  sum_j expf(l_j - M), in the fixed order of ext_prepare's sum (sample_ext.h), and the second
//      digit's histogram
//   C, D  the third and fourth digits: the n_top-th key t of the order is known, and how many keys
//      lie strictly above it (a < n_top)
//   E  the gather: each wave walks one contiguous range; a key above t takes the next of the first
//      a entry slots (an LDS counter: which slot does not matter, the entries are sorted after), a
//      key equal to t is numbered by ballot within the wave and kept while its number is below
//      r = n_top - a; the waves' lists are then joined in wave order, so the r lowest indices win
// and a rank sort of the at most 32 entries by (key << 32 | ~index), descending.
// LDS: 16 KB of count histograms (16 copies per bin, as the sampler's), 2 KB of per-wave tie lists,
// the entries and a few words of state; no mass histogram.  Integer LDS atomics only, one workgroup
// per row with nothing shared between workgroups.
#pragma once

#include "sample.h"

namespace xalm {

struct TopShared {
    unsigned cnt[256 * SMP_REP];
    unsigned bcnt[256];
    uint32_t wkey[SMP_WAVES];
    float wsum[SMP_WAVES];
    unsigned wcnt[SMP_WAVES];
    int wtie[SMP_WAVES][XH_TOP_MAX];
    unsigned long long ent[XH_TOP_MAX];
    // selection state, written by one lane between barriers
    unsigned prefix, above_cnt, n_above;
};

// One level of the radix selection from the histogram in sh.cnt: the bin in which the count from
// the top reaches `target`, appended to sh.prefix; sh.above_cnt = keys strictly above it so far.
// The count-only scan of smp_select<false>.  Ends with a barrier.
__device__ __forceinline__ void top_scan(TopShared& sh, const int shift, const unsigned target) {
    const int tid = threadIdx.x, lane = tid & 63;
    __syncthreads();  // the histogram is whole
    if (tid < 256) {
        unsigned c = 0;
#pragma unroll
        for (int r = 0; r < SMP_REP; r++) c += sh.cnt[tid * SMP_REP + r];
        sh.bcnt[tid] = c;
    }
    __syncthreads();
    if (tid < 64) {
        // lane L holds bins 255 - 4L ... 252 - 4L: a scan from the top bin down
        unsigned c[4], csum = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            c[j] = sh.bcnt[255 - 4 * lane - j];
            csum += c[j];
        }
        unsigned cincl = csum;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned co = __shfl_up(cincl, o, 64);
            if (lane >= o) cincl += co;
        }
        unsigned crun = sh.above_cnt + (cincl - csum);
        bool found = false;
        int fbin = 0;
        unsigned fac = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (!found && (crun + c[j] >= target || (lane == 63 && j == 3))) {  // the last bin closes the scan
                found = true;
                fbin = 255 - 4 * lane - j;
                fac = crun;
            }
            crun += c[j];
        }
        const unsigned long long who = __ballot(found);
        if (lane == __ffsll((long long)who) - 1) {
            sh.prefix |= (uint32_t)fbin << shift;
            sh.above_cnt = fac;
        }
    }
    // the next level's histogram; nothing reads sh.cnt between here and the barrier
    for (int i = tid; i < 256 * SMP_REP; i += SMP_THREADS) sh.cnt[i] = 0;
    __syncthreads();
}

// Row l[0..V): ids[0..n) / lps[0..n) = the first n tokens of the order (n = 0: none), and for
// 0 <= target < V its log-probability and rank.  Every thread of the 1024-thread workgroup calls
// it; 0 <= n <= min(XH_TOP_MAX, V), V <= SMP_MAX_VOCAB.
__device__ void top_row(TopShared& sh, const float* l, const int V, const int n, const int target, int* ids, float* lps,
                        float* target_lp, int* target_rank) {
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const bool has_t = (unsigned)target < (unsigned)V;
    const uint32_t kt = has_t ? smp_key(l[target]) : 0u;
    for (int i = tid; i < 256 * SMP_REP; i += SMP_THREADS) sh.cnt[i] = 0;
    if (tid == 0) {
        sh.prefix = 0;
        sh.above_cnt = 0;
        sh.n_above = 0;
    }
    __syncthreads();

    // pass A
    uint32_t kmax = 0;
    unsigned rank = 0;
    for (int i = tid; i < V; i += SMP_THREADS) {
        const uint32_t k = smp_key(l[i]);
        kmax = k > kmax ? k : kmax;
        rank += (k > kt || (k == kt && i < target)) ? 1u : 0u;
        if (n > 0) atomicAdd(&sh.cnt[(int)(k >> 24) * SMP_REP + (lane & (SMP_REP - 1))], 1u);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t other = __shfl_xor(kmax, o, 64);
        kmax = other > kmax ? other : kmax;
    }
    rank = smp_wave_sum(rank);
    if (lane == 0) {
        sh.wkey[wid] = kmax;
        sh.wcnt[wid] = rank;
    }
    if (n > 0) top_scan(sh, 24, (unsigned)n);
    else __syncthreads();
    kmax = 0;
    rank = 0;
#pragma unroll
    for (int w = 0; w < SMP_WAVES; w++) {
        kmax = sh.wkey[w] > kmax ? sh.wkey[w] : kmax;
        rank += sh.wcnt[w];
    }
    const float M = smp_key_value(kmax);

    // pass B
    float s = 0.f;
    {
        const uint32_t prefix = sh.prefix;
        for (int i = tid; i < V; i += SMP_THREADS) {
            const float v = l[i];
            s += expf(v - M);
            const uint32_t k = smp_key(v);
            if (n > 0 && (k & 0xff000000u) == prefix)
                atomicAdd(&sh.cnt[(int)((k >> 16) & 255u) * SMP_REP + (lane & (SMP_REP - 1))], 1u);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) sh.wsum[wid] = s;
    if (n > 0) top_scan(sh, 16, (unsigned)n);
    else __syncthreads();
    s = 0.f;
#pragma unroll
    for (int w = 0; w < SMP_WAVES; w++) s += sh.wsum[w];
    const float lse = logf(s);
    if (tid == 0 && has_t) {
        const float v = l[target];
        if (target_lp) *target_lp = v == -INFINITY ? -INFINITY : (v - M) - lse;
        if (target_rank) *target_rank = (int)rank;
    }
    if (n <= 0) return;

    // passes C and D
    for (int level = 1; level >= 0; level--) {
        const int shift = 8 * level;
        const uint32_t hmask = 0xffffffffu << (shift + 8), prefix = sh.prefix;
        for (int i = tid; i < V; i += SMP_THREADS) {
            const uint32_t k = smp_key(l[i]);
            if ((k & hmask) == prefix) atomicAdd(&sh.cnt[(int)((k >> shift) & 255u) * SMP_REP + (lane & (SMP_REP - 1))], 1u);
        }
        top_scan(sh, shift, (unsigned)n);
    }
    const uint32_t t = sh.prefix;
    const unsigned a = sh.above_cnt, r = (unsigned)n - a;  // a < n: the n-th key of the order is t

    // pass E
    {
        const int sub = ((V + SMP_WAVES - 1) / SMP_WAVES + 63) & ~63;
        const int w_lo = min(wid * sub, V), w_hi = min(w_lo + sub, V);
        unsigned ties = 0;
        for (int g = w_lo; g < w_hi; g += 64) {
            const int i = g + lane;
            const bool valid = i < w_hi;
            const uint32_t k = valid ? smp_key(l[i]) : 0u;
            if (valid && k > t) {
                const unsigned slot = atomicAdd(&sh.n_above, 1u);
                if (slot < (unsigned)XH_TOP_MAX) sh.ent[slot] = ((unsigned long long)k << 32) | (uint32_t)~i;
            }
            const bool tie = valid && k == t;
            const unsigned long long tb = __ballot(tie);
            const unsigned mine = ties + (unsigned)__popcll(tb & ((1ull << lane) - 1ull));
            if (tie && mine < r) sh.wtie[wid][mine] = i;
            ties += (unsigned)__popcll(tb);
        }
        if (lane == 0) sh.wcnt[wid] = ties < r ? ties : r;
    }
    __syncthreads();
    if ((unsigned)tid < r) {
        // tie number tid of the row, in index order: the waves' ranges ascend
        unsigned base = 0;
        int idx = 0;
        for (int w = 0; w < SMP_WAVES; w++) {
            const unsigned c = sh.wcnt[w];
            if ((unsigned)tid >= base && (unsigned)tid < base + c) idx = sh.wtie[w][(unsigned)tid - base];
            base += c;
        }
        sh.ent[a + (unsigned)tid] = ((unsigned long long)t << 32) | (uint32_t)~idx;
    }
    __syncthreads();
    if (tid < n) {
        const unsigned long long e = sh.ent[tid];
        int place = 0;
        for (int j = 0; j < n; j++) place += sh.ent[j] > e ? 1 : 0;  // the entries are distinct
        const float v = smp_key_value((uint32_t)(e >> 32));
        ids[place] = (int)~(uint32_t)e;
        lps[place] = v == -INFINITY ? -INFINITY : (v - M) - lse;
    }
}

// One workgroup per row.  sp == nullptr: workgroup b takes row b at logits + b * stride.  sp given
// (the decode loops, a grid of 1): the one row at `logits`, written as row sp->step - 1, the step
// the head ahead of this launch has just closed; its target is targets[that row], the token the
// head emitted.  The width is *n_top_dev when given (a device word: changing it needs no new
// capture), else n_top.  Row b writes ids / lps at b * out_stride, target_lp / target_rank at b;
// targets == nullptr: no target.
__global__ __launch_bounds__(SMP_THREADS) void top_logprobs_kernel(const float* logits, int vocab, size_t stride,
                                                                   const int* n_top_dev, int n_top, const StepParams* sp,
                                                                   int cap, const int* targets, int out_stride, int* ids,
                                                                   float* lps, float* target_lp, int* target_rank) {
    __shared__ TopShared sh;
    int row = (int)blockIdx.x;
    const float* l = logits + (size_t)blockIdx.x * stride;
    if (sp) {
        row = sp->step - 1;
        l = logits;
        if (row < 0 || row >= cap) return;
    }
    int n = n_top_dev ? *n_top_dev : n_top;
    n = max(0, min(n, min((int)XH_TOP_MAX, vocab)));
    if (!ids || !lps) n = 0;
    top_row(sh, l, vocab, n, targets ? targets[row] : -1, n ? ids + (size_t)row * out_stride : nullptr,
            n ? lps + (size_t)row * out_stride : nullptr, target_lp ? target_lp + row : nullptr,
            target_rank ? target_rank + row : nullptr);
}

}  // namespace xalm
