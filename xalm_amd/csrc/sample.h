// sample.h — seeded temperature / top-k / top-p sampling in one 1024-thread workgroup (the
// definition: include/xalm_hip.h, xh_sampling).  Everything that decides the token is an integer:
//   order    the logit's f32 bits mapped to an unsigned key (a larger logit = a larger key), ties
//            by index
//   top-k    radix selection of the k-th key, four 8-bit digits, from LDS histograms of counts
//   top-p    the same selection over masses: w_i * 2^40 truncated to u64 (w_i <= 1, V < 2^17, so a
//            sum stays below 2^57), the cut where the mass above reaches ceil(top_p * total)
//   draw     a search in index order for the first kept token whose cumulative mass exceeds
//            floor(u * total): per-wave sums of contiguous ranges, narrowed 16-fold per level
// Integer adds commute, so neither the LDS atomics nor the reductions depend on scheduling: the
// same logits bits, parameters and counter give the same token on every run.
// The logits are read from global memory in every pass (V = 128256 does not fit LDS next to the
// histograms; 501 KB stay in L2), each pass with consecutive lanes on consecutive indices.
#pragma once

#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdint>

#include "../../include/xalm_hip.h"
#include "common.h"

namespace xalm {

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): the one
// generator of the kernel and of xh_philox4x32.
__host__ __device__ inline void philox4x32_10(uint32_t k0, uint32_t k1, uint32_t c[4]) {
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
        c[0] = n0; c[1] = (uint32_t)p1; c[2] = n2; c[3] = (uint32_t)p0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}

constexpr int SMP_THREADS = 1024;
constexpr int SMP_WAVES = SMP_THREADS / 64;
// histogram copies per bin, chosen by lane & 15: at most 4 lanes of a wave meet on one LDS word
// however peaked the digit is (logits of one sign and exponent share the top digit)
constexpr int SMP_REP = 16;
constexpr float SMP_MASS_ONE = 1099511627776.0f;  // 2^40
constexpr int SMP_MAX_VOCAB = 1 << 17;             // the mass sums stay below 2^57

struct SampleShared {
    unsigned cnt[256 * SMP_REP];
    unsigned long long mass[256 * SMP_REP];
    unsigned bcnt[256];
    unsigned long long bmass[256];
    unsigned long long wmass[SMP_WAVES];
    unsigned wcnt[SMP_WAVES];
    // selection state, written by one lane between barriers
    unsigned prefix, above_cnt, bin_cnt;
    unsigned long long above_mass, target;
    int token;
};

__device__ __forceinline__ uint32_t smp_key(const float v) {
    const uint32_t u = __builtin_bit_cast(uint32_t, v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float smp_key_value(const uint32_t k) {
    return __builtin_bit_cast(float, (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}
// w = expf((l - m) / T) as a fixed-point mass; -inf has none
__device__ __forceinline__ unsigned long long smp_mass(const float l, const float m, const float temp) {
    if (l == -INFINITY) return 0ull;
    return (unsigned long long)(expf((l - m) / temp) * SMP_MASS_ONE);
}

__device__ __forceinline__ unsigned long long smp_wave_sum(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ unsigned smp_wave_sum(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// The kept set as the selections leave it: everything (all), or the keys above t and the first r
// tokens, by index, of key t.
struct SampleCut {
    bool all;
    uint32_t t;
    unsigned r;
    unsigned n_kept;
};

// Radix selection, most significant digit first.  Candidates: every token (all), or the keys
// above tk plus rk tokens of key tk (those are added per bin after the pass: equal keys share
// every digit, and which rk of them does not matter here).  MASS false: the key at which the
// count from the top reaches `target`; MASS true: the key at which the mass from the top reaches
// ceil(top_p * the candidates' mass).  On return sh.prefix = that key, sh.above_cnt /
// sh.above_mass = candidates strictly above it, sh.bin_cnt = candidates of that key.
template <bool MASS>
__device__ void smp_select(SampleShared& sh, const float* logits, const int V, const float m, const float temp,
                           const bool all, const uint32_t tk, const unsigned rk, const unsigned long long target_cnt,
                           const float top_p) {
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid == 0) {
        sh.prefix = 0;
        sh.above_cnt = 0;
        sh.above_mass = 0;
        sh.target = target_cnt;
    }
    const unsigned long long q_tk = MASS && !all ? smp_mass(smp_key_value(tk), m, temp) : 0ull;
    for (int level = 3; level >= 0; level--) {
        const int shift = 8 * level;
        const uint32_t hmask = level == 3 ? 0u : 0xffffffffu << (shift + 8);
        for (int i = tid; i < 256 * SMP_REP; i += SMP_THREADS) {
            sh.cnt[i] = 0;
            if (MASS) sh.mass[i] = 0;
        }
        __syncthreads();  // zeroed, and the previous level's state is visible
        const uint32_t prefix = sh.prefix;
        for (int i = tid; i < V; i += SMP_THREADS) {
            const float l = logits[i];
            const uint32_t k = smp_key(l);
            if ((all || !MASS || k > tk) && (k & hmask) == (prefix & hmask)) {
                const int slot = (int)((k >> shift) & 255u) * SMP_REP + (lane & (SMP_REP - 1));
                atomicAdd(&sh.cnt[slot], 1u);
                if (MASS) atomicAdd(&sh.mass[slot], smp_mass(l, m, temp));
            }
        }
        __syncthreads();
        if (tid < 256) {
            unsigned c = 0;
            unsigned long long ms = 0;
#pragma unroll
            for (int r = 0; r < SMP_REP; r++) {
                c += sh.cnt[tid * SMP_REP + r];
                if (MASS) ms += sh.mass[tid * SMP_REP + r];
            }
            if (MASS && !all && (tk & hmask) == (prefix & hmask) && (uint32_t)tid == ((tk >> shift) & 255u)) {
                c += rk;
                ms += (unsigned long long)rk * q_tk;
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
            if (MASS && level == 3) {
                // the candidates' mass is known now: the cut is where the mass reaches top_p of it
                const unsigned long long total = __shfl(mincl, 63, 64);
                const double want = ceil((double)top_p * (double)total);
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
                const bool reach = MASS ? mrun + ms[j] >= target : (unsigned long long)crun + c[j] >= target;
                if (!found && (reach || (lane == 63 && j == 3))) {  // the last bin always closes the scan
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

// The token at counter `pos` from logits[0..V) under `p` (the definition in include/xalm_hip.h);
// every thread of the 1024-thread workgroup calls it and gets the token; *n_kept as xh_op_sample
// reports it (greedy: 1; no finite logit: 0).
__device__ int sample_token(SampleShared& sh, const float* logits, const int V, const xh_sampling p, const uint32_t pos,
                            int* n_kept) {
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const bool greedy = p.temperature == 0.f;
    // the first maximum (greedy: among logits > FLT_MIN, Sampler::sample_argmax)
    unsigned long long best = 0;
    for (int i = tid; i < V; i += SMP_THREADS) {
        const float v = logits[i];
        if (!greedy || v > FLT_MIN) {
            const unsigned long long k = argmax_key(v, i);
            best = k > best ? k : best;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(best, o, 64);
        best = other > best ? other : best;
    }
    if (lane == 0) sh.wmass[wid] = best;
    __syncthreads();
    best = 0;
#pragma unroll
    for (int w = 0; w < SMP_WAVES; w++) best = sh.wmass[w] > best ? sh.wmass[w] : best;
    __syncthreads();  // wmass is reused below
    const int first_max = argmax_key_index(best);
    if (greedy) {
        *n_kept = 1;
        return first_max;
    }
    const float m = smp_key_value((uint32_t)(best >> 32));
    if (!(m > -INFINITY) || m == INFINITY) {  // no finite logit: token 0; +inf: the first of them
        *n_kept = m == INFINITY ? 1 : 0;
        return m == INFINITY ? first_max : 0;
    }
    const float temp = p.temperature;

    SampleCut cut;
    cut.all = p.top_k <= 0 || p.top_k >= V;
    cut.t = 0;
    cut.r = 0;
    cut.n_kept = (unsigned)V;
    if (!cut.all) {
        smp_select<false>(sh, logits, V, m, temp, true, 0u, 0u, (unsigned long long)p.top_k, 1.f);
        cut.t = sh.prefix;
        cut.r = (unsigned)p.top_k - sh.above_cnt;
        cut.n_kept = (unsigned)p.top_k;
        __syncthreads();
    }
    if (p.top_p < 1.f) {
        smp_select<true>(sh, logits, V, m, temp, cut.all, cut.t, cut.r, 0ull, p.top_p);
        const uint32_t t = sh.prefix;
        const unsigned long long q_t = smp_mass(smp_key_value(t), m, temp);
        const unsigned long long need = sh.target - sh.above_mass;  // > 0: the cut lies in this key's tokens
        unsigned long long r = q_t ? (need + q_t - 1) / q_t : 1ull;
        if (r < 1) r = 1;
        if (r > sh.bin_cnt) r = sh.bin_cnt;
        cut.all = false;
        cut.t = t;
        cut.r = (unsigned)r;
        cut.n_kept = sh.above_cnt + cut.r;
        __syncthreads();
    }
    *n_kept = (int)cut.n_kept;

    // the draw
    uint32_t c[4] = {pos, 0u, 0u, 0u};
    philox4x32_10((uint32_t)p.seed, (uint32_t)(p.seed >> 32), c);
    const unsigned long long u24 = c[0] >> 8;
    const unsigned long long q_t = cut.all ? 0ull : smp_mass(smp_key_value(cut.t), m, temp);
    unsigned long long thr = 0, base_mass = 0;
    unsigned base_ties = 0;
    int lo = 0, len = V;
    bool first = true;
    while (first || len > 64) {  // the first level also gives the kept total
        const int sub = ((len + SMP_WAVES - 1) / SMP_WAVES + 63) & ~63;
        const int w_lo = min(lo + wid * sub, lo + len), w_hi = min(w_lo + sub, lo + len);
        unsigned long long mg = 0;
        unsigned tc = 0;
        for (int i = w_lo + lane; i < w_hi; i += 64) {
            const float l = logits[i];
            const uint32_t k = smp_key(l);
            if (cut.all || k > cut.t) mg += smp_mass(l, m, temp);
            else if (k == cut.t) tc++;
        }
        mg = smp_wave_sum(mg);
        tc = smp_wave_sum(tc);
        if (lane == 0) { sh.wmass[wid] = mg; sh.wcnt[wid] = tc; }
        __syncthreads();
        if (first) {
            // the kept total, and floor(u * total): a cumulative integer mass exceeds u * total
            // exactly when it exceeds that floor
            unsigned long long total = (unsigned long long)cut.r * q_t;
            for (int w = 0; w < SMP_WAVES; w++) total += sh.wmass[w];
            thr = (__umul64hi(total, u24) << 40) | ((total * u24) >> 24);
            first = false;
        }
        int pick = -1;
        unsigned long long cum = base_mass;
        unsigned ties = base_ties;
        for (int w = 0; w < SMP_WAVES && pick < 0; w++) {
            const unsigned left = cut.r > ties ? cut.r - ties : 0u;
            const unsigned take = sh.wcnt[w] < left ? sh.wcnt[w] : left;
            const unsigned long long kept = sh.wmass[w] + (unsigned long long)take * q_t;
            if (cum + kept > thr) pick = w;
            else { cum += kept; ties += sh.wcnt[w]; }
        }
        __syncthreads();  // wmass / wcnt are rewritten by the next level
        if (pick < 0) return first_max;  // unreachable: thr < total
        base_mass = cum;
        base_ties = ties;
        const int n_lo = min(lo + pick * sub, lo + len), n_hi = min(n_lo + sub, lo + len);
        lo = n_lo;
        len = n_hi - n_lo;
    }
    if (tid < 64) {
        unsigned long long kept = 0;
        bool tie = false;
        if (lane < len) {
            const float l = logits[lo + lane];
            const uint32_t k = smp_key(l);
            if (cut.all || k > cut.t) kept = smp_mass(l, m, temp);
            else tie = k == cut.t;
        }
        const unsigned long long tb = __ballot(tie);
        if (tie && base_ties + (unsigned)__popcll(tb & ((1ull << lane) - 1ull)) < cut.r) kept = q_t;
        unsigned long long incl = kept;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long other = __shfl_up(incl, o, 64);
            if (lane >= o) incl += other;
        }
        const unsigned long long hit = __ballot(base_mass + incl > thr);
        if (lane == 0) sh.token = hit ? lo + __ffsll((long long)hit) - 1 : first_max;
    }
    __syncthreads();
    return sh.token;
}

}  // namespace xalm
