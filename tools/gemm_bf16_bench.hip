// gemm_bf16_bench.hip — the bf16-weight prompt GEMM (xalm_amd/csrc/gemm_bf16.h) on Mistral-7B shapes:
// correctness against a double-precision host sum on sampled outputs and device time per launch of
// its stage-count / MFMA-tile variants, beside gemm16.h's product instantiation on f16 weights of the
// same shape (tools/gemm_bench.hip's method: median of 5 rounds of 10 launches).
// Build: hipcc -O3 --offload-arch=gfx950 -std=c++17 -Xclang -target-feature -Xclang -packed-fp32-ops
//        -o tools/gemm_bf16_bench tools/gemm_bf16_bench.hip
// Run:   tools/gemm_bf16_bench [n_tokens ...]
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../xalm_amd/csrc/gemm_bf16.h"

using namespace xalm;  // gemm16.h's instantiation macros name its constants unqualified

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP %s @%d\n", hipGetErrorString(e), __LINE__); exit(1); } } while (0)

static uint16_t f2b(float f) { uint32_t u; memcpy(&u, &f, 4); return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16); }
static float b2f(uint16_t b) { const uint32_t u = (uint32_t)b << 16; float f; memcpy(&f, &u, 4); return f; }

template <class F>
static double time_us(hipEvent_t e0, hipEvent_t e1, const F& launch) {
    std::vector<float> rounds;
    for (int i = 0; i < 3; i++) launch();
    for (int rr = 0; rr < 5; rr++) {
        CK(hipEventRecord(e0, 0));
        for (int i = 0; i < 10; i++) launch();
        CK(hipEventRecord(e1, 0));
        CK(hipEventSynchronize(e1));
        float ms = 0;
        CK(hipEventElapsedTime(&ms, e0, e1));
        rounds.push_back(ms * 100.f);
    }
    std::sort(rounds.begin(), rounds.end());
    return rounds[2];
}

int main(int argc, char** argv) {
    setvbuf(stdout, nullptr, _IOLBF, 0);
    std::vector<int> ns;
    for (int i = 1; i < argc; i++) ns.push_back(atoi(argv[i]));
    if (ns.empty()) ns = {2048};
    struct Shape { const char* name; int rows, K; };
    const Shape shapes[] = {{"qkv", 6144, 4096}, {"wo", 4096, 4096}, {"w13", 28672, 4096}, {"w2", 4096, 14336}};
    const size_t wmax = (size_t)28672 * 4096, nmax = 2048, kmax = 14336, cap = (size_t)2 * 2048 * 28672;
    std::mt19937 rng(1);
    std::normal_distribution<float> nd(0.f, 1.f);
    std::vector<uint16_t> hw(wmax), hx(3 * nmax * kmax);
    for (auto& v : hw) v = f2b(0.02f * nd(rng));
    for (size_t i = 0; i < nmax * kmax; i++) {  // the three pieces of an N(0,1) value (as prefill_split_bf16_kernel)
        const float x = nd(rng);
        const uint16_t b0 = f2b(x), b1 = f2b(x - b2f(b0)), b2 = f2b(x - b2f(b0) - b2f(b1));
        hx[i] = b0; hx[nmax * kmax + i] = b1; hx[2 * nmax * kmax + i] = b2;
    }
    uint16_t *dw, *dx;
    float* dy;
    CK(hipMalloc(&dw, wmax * 2));
    CK(hipMalloc(&dx, 3 * nmax * kmax * 2));
    CK(hipMalloc(&dy, cap * 4));
    CK(hipMemcpy(dw, hw.data(), wmax * 2, hipMemcpyHostToDevice));
    struct Var { const char* name; void (*fn)(xalm::MbArgs); int ns; };
    const Var vars[] = {{"s3m16", xalm::mm_bf16_kernel_t<3, 16>, 3}, {"s2m16", xalm::mm_bf16_kernel_t<2, 16>, 2},
                        {"s3m32", xalm::mm_bf16_kernel_t<3, 32>, 3}, {"s2m32", xalm::mm_bf16_kernel_t<2, 32>, 2}};
    const int NV = sizeof vars / sizeof vars[0];
    for (const Var& v : vars)
        CK(hipFuncSetAttribute((const void*)v.fn, hipFuncAttributeMaxDynamicSharedMemorySize, xalm::mb_lds(v.ns)));
    CK(hipFuncSetAttribute((const void*)xalm::mm_f16_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, xalm::MM_LDS));
    CK(hipFuncSetAttribute((const void*)xalm::mm_f16_kernel_w4, hipFuncAttributeMaxDynamicSharedMemorySize, xalm::MM_LDS_W4));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    int bad = 0;
    for (int n : ns) {
        if (n < 1 || n > (int)nmax) continue;
        double tot[8] = {};
        for (const Shape& sh : shapes) {
            std::vector<uint16_t> xs(3 * (size_t)n * sh.K);  // planes [3][n][K]
            for (int p = 0; p < 3; p++)
                for (int t = 0; t < n; t++)
                    memcpy(&xs[((size_t)p * n + t) * sh.K], &hx[p * nmax * kmax + (size_t)t * kmax], (size_t)sh.K * 2);
            CK(hipMemcpy(dx, xs.data(), xs.size() * 2, hipMemcpyHostToDevice));
            const int ks = xalm::mm_pick_ks(sh.rows, sh.K, n, cap);
            const int n_rt = xalm::mm_row_tiles(sh.rows), n_tt = xalm::mm_tok_tiles(n), grid = n_rt * n_tt * ks;
            const double flop = 2.0 * sh.rows * sh.K * (double)n;
            // gemm16.h on the same bytes read as f16 (timing only: the values are not the bf16 ones)
            xalm::MmArgs m{};
            m.w = dw; m.xh = dx; m.xl = dx + (size_t)n * sh.K; m.out = dy;
            m.rows = sh.rows; m.K = sh.K; m.n = n; m.ks = ks; m.n_rt = n_rt; m.n_tt = n_tt;
            const bool w4 = grid >= xalm::MM_W4_PER_CU * 256;
            const double f16_us = time_us(e0, e1, [&]() {
                if (w4) hipLaunchKernelGGL(xalm::mm_f16_kernel_w4, dim3(grid), dim3(xalm::MM_THREADS_W4), xalm::MM_LDS_W4, 0, m);
                else hipLaunchKernelGGL(xalm::mm_f16_kernel, dim3(grid), dim3(xalm::MM_THREADS), xalm::MM_LDS, 0, m);
            });
            tot[NV] += f16_us;
            printf("n %5d %-4s rows %5d K %5d ks %d grid %4d | gemm16.h (f16, %s) %8.1f us = %6.1f TF/s\n", n, sh.name, sh.rows,
                   sh.K, ks, grid, w4 ? "w4" : "default", f16_us, flop / f16_us * 1e-6);
            xalm::MbArgs a{};
            a.w = dw; a.x = dx; a.out = dy;
            a.rows = sh.rows; a.K = sh.K; a.n = n; a.ks = ks; a.n_rt = n_rt; a.n_tt = n_tt;
            for (int v = 0; v < NV; v++) {
                auto launch = [&]() {
                    hipLaunchKernelGGL(vars[v].fn, dim3(grid), dim3(xalm::MB_THREADS), xalm::mb_lds(vars[v].ns), 0, a);
                };
                CK(hipMemset(dy, 0, (size_t)ks * n * sh.rows * 4));
                launch();
                CK(hipDeviceSynchronize());
                std::vector<float> y((size_t)ks * n * sh.rows);
                CK(hipMemcpy(y.data(), dy, y.size() * 4, hipMemcpyDeviceToHost));
                double maxrel = 0;
                std::mt19937 pr(n + sh.rows);
                for (int smp = 0; smp < 256; smp++) {
                    const int t = smp < 4 ? n - 1 : pr() % n, r = smp < 4 ? sh.rows - 1 : pr() % sh.rows;
                    double ref = 0, mag = 0, got = 0;
                    for (int k = 0; k < sh.K; k++) {
                        double xv = 0;
                        for (int p = 0; p < 3; p++) xv += b2f(xs[((size_t)p * n + t) * sh.K + k]);
                        const double wv = b2f(hw[(size_t)r * sh.K + k]);
                        ref += wv * xv;
                        mag += fabs(wv * xv);
                    }
                    for (int s = 0; s < ks; s++) got += y[((size_t)s * n + t) * sh.rows + r];
                    maxrel = fmax(maxrel, fabs(got - ref) / mag);
                }
                const double us = time_us(e0, e1, launch);
                tot[v] += us;
                const bool ok = maxrel < 2e-6;
                bad += !ok;
                printf("    %-6s %8.1f us = %6.1f TF/s (MFMA %6.1f) x %.2f of gemm16.h, err %.2e %s\n", vars[v].name, us,
                       flop / us * 1e-6, 3 * flop / us * 1e-6, us / f16_us, maxrel, ok ? "ok" : "BAD");
            }
        }
        printf("n %5d layer: gemm16.h %8.1f us\n", n, tot[NV]);
        for (int v = 0; v < NV; v++) printf("    %-6s %8.1f us, x %.2f\n", vars[v].name, tot[v], tot[v] / tot[NV]);
    }
    CK(hipEventDestroy(e0));
    CK(hipEventDestroy(e1));
    CK(hipFree(dy));
    CK(hipFree(dx));
    CK(hipFree(dw));
    printf("done: %d bad\n", bad);
    return bad ? 1 : 0;
}
