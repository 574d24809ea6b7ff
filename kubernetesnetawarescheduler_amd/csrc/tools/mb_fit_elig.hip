// mb_fit_elig.hip -- microbenchmark of the constrained resource-fit filter
// (k_fit.hip, nas::Elig: node selectors and taints) at the C3 shape (10k nodes
// x 100k pods) against the unconstrained kernel in the same run, for three
// word patterns:
//   allfit   every pod has require = 0, no node is tainted
//   nolabel  every pod requires a label no node carries (every word is 0)
//   mix      3 of 8 label bits per node, 0-2 required per pod, about half the
//            nodes tainted and half the pods tolerating
// Rounds alternate the four launches, so drift hits them alike.  A sample of
// every pattern's words is checked against the host's rule.
//   build: hipcc -O3 -std=c++17 --offload-arch=gfx950 -I/opt/rocm/include tools/mb_fit_elig.hip -o tools/mb_fit_elig
//   run:   tools/mb_fit_elig [rounds]
#include "../k_fit.hip"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CK(x)                                                                       \
    do {                                                                            \
        hipError_t e_ = (x);                                                        \
        if (e_ != hipSuccess) {                                                     \
            fprintf(stderr, "%s: %s (line %d)\n", #x, hipGetErrorString(e_), __LINE__); \
            exit(1);                                                                \
        }                                                                           \
    } while (0)

using namespace nas;
typedef unsigned long long u64w;

int main(int argc, char **argv) {
    const int rounds = argc > 1 ? atoi(argv[1]) : 30;
    const int N = 10000, P = 100000, Pp = 100096, Mp = 10240, n_chunks = Mp / 64;
    std::vector<int> cap(3 * N), req(3 * (size_t)Pp);
    srand(7);
    for (int n = 0; n < N; ++n) {  // (mb_fit.hip's cluster)
        const int big = rand() & 1;
        cap[n] = (big ? 8000 : 4000) - rand() % 600;
        cap[N + n] = (big ? 8 : 4) * 1048576 - rand() % 400000;
        cap[2 * N + n] = 110 - rand() % 12;
    }
    for (int p = 0; p < Pp; ++p) {
        req[p] = 1 + rand() % 540;
        req[Pp + p] = 7464 + rand() % 300000;
        req[2 * (size_t)Pp + p] = 1;
    }
    // the three patterns' words: node [labels N | taints N], pod [require Pp | tolerate Pp]
    const char *names[3] = {"allfit", "nolabel", "mix"};
    std::vector<u64w> nw[3], pw[3];
    for (int k = 0; k < 3; ++k) {
        nw[k].assign(2 * (size_t)N, 0);
        pw[k].assign(2 * (size_t)Pp, 0);
    }
    for (int n = 0; n < N; ++n) {
        u64w l = 0;
        while (__builtin_popcountll(l) < 3) l |= 1ull << (rand() % 8);
        nw[0][n] = nw[1][n] = nw[2][n] = l;
        nw[2][N + n] = (rand() & 1) ? 1ull << 40 : 0;
    }
    for (int p = 0; p < P; ++p) {
        pw[1][p] = 1ull << 63;
        u64w r = 0;
        for (int j = rand() % 3; j > 0; --j) r |= 1ull << (rand() % 8);
        pw[2][p] = r;
        pw[2][Pp + p] = (rand() & 1) ? 1ull << 40 : 0;
    }
    int *dcap, *dreq;
    u64w *mask, *dn[3], *dp[3];
    CK(hipMalloc(&dcap, cap.size() * 4));
    CK(hipMalloc(&dreq, req.size() * 4));
    CK(hipMalloc(&mask, (size_t)n_chunks * Pp * 8));
    CK(hipMemcpy(dcap, cap.data(), cap.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(dreq, req.data(), req.size() * 4, hipMemcpyHostToDevice));
    Elig el[3];
    for (int k = 0; k < 3; ++k) {
        CK(hipMalloc(&dn[k], nw[k].size() * 8));
        CK(hipMalloc(&dp[k], pw[k].size() * 8));
        CK(hipMemcpy(dn[k], nw[k].data(), nw[k].size() * 8, hipMemcpyHostToDevice));
        CK(hipMemcpy(dp[k], pw[k].data(), pw[k].size() * 8, hipMemcpyHostToDevice));
        el[k].labels = reinterpret_cast<uint64_t *>(dn[k]);
        el[k].taints = reinterpret_cast<uint64_t *>(dn[k]) + N;
        el[k].require = reinterpret_cast<uint64_t *>(dp[k]);
        el[k].tolerate = reinterpret_cast<uint64_t *>(dp[k]) + Pp;
    }
    hipEvent_t a, b;
    CK(hipEventCreate(&a));
    CK(hipEventCreate(&b));
    std::vector<float> t[4];  // 0: unconstrained, 1..3: the patterns
    FitArgs fa;
    fa.cap = dcap;
    fa.N = fa.nloc = N;
    fa.Mp = Mp;
    fa.req = dreq;
    fa.Pp = Pp;
    fa.np = P;
    fa.mask = (uint64_t *)mask;
    for (int r = -3; r < rounds; ++r)  // (three warm-up rounds)
        for (int v = 0; v < 4; ++v) {
            float ms = 0;
            fa.el = v ? &el[v - 1] : nullptr;
            CK(hipEventRecord(a));
            CK(launch_fit(0, fa));
            CK(hipEventRecord(b));
            CK(hipEventSynchronize(b));
            CK(hipEventElapsedTime(&ms, a, b));
            if (r >= 0) t[v].push_back(ms);
        }
    for (int v = 0; v < 4; ++v) std::sort(t[v].begin(), t[v].end());
    const double bytes = (double)P * n_chunks * 8;
    const float base = t[0][rounds / 2];
    for (int v = 0; v < 4; ++v)
        printf("%-13s median %.2f us  min %.2f us  mask write %.2f TB/s  x%.3f of unconstrained\n",
               v ? names[v - 1] : "unconstrained", t[v][rounds / 2] * 1e3, t[v][0] * 1e3,
               bytes / (t[v][rounds / 2] * 1e-3) / 1e12, t[v][rounds / 2] / base);
    // every 97th pod's words of every pattern against the rule on the host
    std::vector<u64w> h((size_t)n_chunks * Pp);
    for (int k = 0; k < 3; ++k) {
        fa.el = &el[k];
        CK(launch_fit(0, fa));
        CK(hipMemcpy(h.data(), mask, h.size() * 8, hipMemcpyDeviceToHost));
        size_t bad = 0, set = 0;
        for (int p = 0; p < P; p += 97)
            for (int c = 0; c < n_chunks; ++c) {
                u64w w = 0;
                for (int j = 0; j < 64 && c * 64 + j < N; ++j) {
                    const int n = c * 64 + j;
                    const bool ok = req[p] <= cap[n] && req[Pp + p] <= cap[N + n] &&
                                    req[2 * (size_t)Pp + p] <= cap[2 * N + n] &&
                                    (nw[k][n] & pw[k][p]) == pw[k][p] &&
                                    (nw[k][N + n] & ~pw[k][Pp + p]) == 0;
                    w |= (u64w)ok << j;
                }
                bad += w != h[(size_t)c * Pp + p];
                set += __builtin_popcountll(w);
            }
        printf("%-13s sampled words: %zu mismatches, %zu bits set\n", names[k], bad, set);
        if (bad) return 1;
    }
    return 0;
}
