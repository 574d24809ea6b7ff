// Traffic ingestion (csrc/traffic_ingest.h) under ASan + UBSan, without a GPU
// or the HIP runtime.  The reference is a dense restatement written here with
// plain loops: an int64 / double matrix [P][n] accumulated peer by peer.
//  a. literal pins: sums at the int8 and int32 limits, cancelling pairs,
//     skipped peers, duplicates, empty rows, the fp32 "double sum, rounded
//     once" case, and every argument-check failure with its code and message;
//  b. over random small cases: triplets scattered into a zero plane and joined
//     with the lists reproduce the dense reference, the lists' invariants, and
//     split_row + carry_offsets over the dense rows give the same plane and
//     lists as the CSR path;
//  c. ovf_window_max against a brute-force maximum over its windows.
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "traffic_ingest.h"

using namespace nas;

static long n_checked = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                    \
        }                                                                    \
        ++n_checked;                                                         \
    } while (0)

typedef std::vector<int32_t> I32s;

struct Peer {
    int32_t node;
    int64_t w;  // fp32 cases: wf instead
    float wf;
};

// rows of peers -> the three CSR arrays (weights in every dtype at once)
struct Csr {
    I32s rp{0}, pn, w32;
    std::vector<int8_t> w8;
    std::vector<float> wf;
    int32_t P() const { return (int32_t)rp.size() - 1; }
    int64_t nnz() const { return (int64_t)pn.size(); }
    void row(const std::vector<Peer> &peers) {
        for (const Peer &q : peers) {
            pn.push_back(q.node);
            w32.push_back((int32_t)q.w);
            w8.push_back((int8_t)q.w);
            wf.push_back(q.wf);
        }
        rp.push_back((int32_t)pn.size());
    }
    const void *weights(int dtype) const {
        return dtype == NAS_DT_I8 ? (const void *)w8.data() : (const void *)w32.data();
    }
};
static Peer pi(int32_t node, int64_t w) { return {node, w, 0.f}; }
static Peer pf(int32_t node, float w) { return {node, 0, w}; }

// ---- the dense restatement: D[p][m] += w, peer by peer
template <typename Acc, typename W>
static std::vector<Acc> dense_ref(const Csr &c, const W *w, int n, std::vector<char> *seen = nullptr) {
    std::vector<Acc> D((size_t)c.P() * n, 0);
    if (seen) seen->assign(D.size(), 0);
    for (int p = 0; p < c.P(); ++p)
        for (int x = c.rp[p]; x < c.rp[p + 1]; ++x) {
            const int m = c.pn[x];
            if (m < 0 || m >= n) continue;
            D[(size_t)p * n + m] += (Acc)w[x];
            if (seen) (*seen)[(size_t)p * n + m] = 1;
        }
    return D;
}
static std::vector<int64_t> dense_int(const Csr &c, int dtype, int n) {
    return dtype == NAS_DT_I8 ? dense_ref<int64_t>(c, c.w8.data(), n)
                              : dense_ref<int64_t>(c, c.w32.data(), n);
}

struct IntResult {
    int rc;
    std::string msg;
    Triplets<signed char> t;
    OvfLists ovf;
};
static IntResult ingest(const Csr &c, int dtype, int n, int Pp) {
    IntResult r;
    r.rc = check_csr_arrays(c.rp.data(), c.pn.data(), c.weights(dtype), dtype, c.nnz(), r.msg);
    CHECK(r.rc == NAS_OK);
    r.rc = check_csr_rows(c.rp.data(), c.P(), c.nnz(), r.msg);
    CHECK(r.rc == NAS_OK);
    r.rc = ingest_csr_int(c.rp.data(), c.pn.data(), c.weights(dtype), dtype, c.P(), Pp, n, r.t, r.ovf,
                          r.msg);
    return r;
}

// the properties every accepted integer ingestion has, against the dense
// reference D; returns the plane [P][n] the triplets give
static std::vector<signed char> check_int(const IntResult &r, const std::vector<int64_t> &D, int P,
                                          int Pp, int n) {
    const Triplets<signed char> &t = r.t;
    const OvfLists &o = r.ovf;
    CHECK(r.rc == NAS_OK && r.msg.empty());
    CHECK(t.pod.size() == t.node.size() && t.pod.size() == t.val.size());
    CHECK(o.m.size() == o.e.size());
    // ptr: monotone, the padding rows carry the last offset, the end is the entry count
    CHECK(o.ptr.size() == (size_t)Pp + 1 && o.ptr[0] == 0);
    for (int r2 = 0; r2 < Pp; ++r2) CHECK(o.ptr[r2] <= o.ptr[r2 + 1]);
    for (int r2 = P; r2 <= Pp; ++r2) CHECK(o.ptr[r2] == o.ptr[P]);
    CHECK(o.ptr[Pp] == (int32_t)o.m.size());
    // triplets: pods ascending, nodes ascending within a pod, never a zero
    std::vector<signed char> plane((size_t)P * n, 0);
    for (size_t i = 0; i < t.pod.size(); ++i) {
        CHECK(t.pod[i] >= 0 && t.pod[i] < P && t.node[i] >= 0 && t.node[i] < n);
        if (i) CHECK(t.pod[i] > t.pod[i - 1] || (t.pod[i] == t.pod[i - 1] && t.node[i] > t.node[i - 1]));
        CHECK(t.val[i] != 0);
        plane[(size_t)t.pod[i] * n + t.node[i]] = t.val[i];
    }
    // entries: nodes ascending within a row, excess non-zero, plane saturated
    for (int p = 0; p < P; ++p)
        for (int j = o.ptr[p]; j < o.ptr[p + 1]; ++j) {
            CHECK(o.m[j] >= 0 && o.m[j] < n);
            if (j > o.ptr[p]) CHECK(o.m[j] > o.m[j - 1]);
            CHECK(o.e[j] != 0);
            const signed char v = plane[(size_t)p * n + o.m[j]];
            CHECK(v == -128 || v == 127);
            CHECK((o.e[j] > 0) == (v == 127));
        }
    // plane + lists = the dense reference, exactly
    std::vector<int32_t> out((size_t)P * n + 1, -777);
    join_rows(plane.data(), P, n, o.ptr.data(), o.m.data(), o.e.data(), out.data());
    for (size_t i = 0; i < D.size(); ++i) CHECK(out[i] == D[i]);
    CHECK(out[D.size()] == -777);
    // the dense path over the same traffic: split_row per row + the fix-up
    std::vector<signed char> plane2((size_t)P * n, 77);
    OvfLists d;
    d.ptr.assign((size_t)Pp + 1, 0);
    for (int p = 0; p < P; ++p) {
        split_row(D.data() + (size_t)p * n, n, plane2.data() + (size_t)p * n, d.m, d.e);
        d.ptr[p + 1] = (int32_t)d.m.size();
    }
    carry_offsets(d.ptr);
    CHECK(plane2 == plane && d.ptr == o.ptr && d.m == o.m && d.e == o.e);
    return plane;
}

static void expect_lists(const IntResult &r, const I32s &pod, const I32s &node,
                         const std::vector<signed char> &val, const I32s &ptr, const I32s &m,
                         const I32s &e) {
    CHECK(r.t.pod == pod && r.t.node == node && r.t.val == val);
    CHECK(r.ovf.ptr == ptr && r.ovf.m == m && r.ovf.e == e);
}

static void pins_int() {
    const int n = 6;
    {  // sums of exactly 127, 128, -128 and -129; Pp > P
        Csr c;
        c.row({pi(0, 100), pi(1, 127), pi(0, 27), pi(1, 1), pi(2, -100), pi(3, -100), pi(2, -28),
               pi(3, -29)});
        const IntResult r = ingest(c, NAS_DT_I32, n, 4);
        check_int(r, dense_int(c, NAS_DT_I32, n), 1, 4, n);
        expect_lists(r, {0, 0, 0, 0}, {0, 1, 2, 3}, {127, 127, -128, -128}, {0, 2, 2, 2, 2}, {1, 3},
                     {1, -1});
        // the same weights fit int8
        const IntResult r8 = ingest(c, NAS_DT_I8, n, 4);
        check_int(r8, dense_int(c, NAS_DT_I8, n), 1, 4, n);
        expect_lists(r8, {0, 0, 0, 0}, {0, 1, 2, 3}, {127, 127, -128, -128}, {0, 2, 2, 2, 2}, {1, 3},
                     {1, -1});
    }
    {  // exactly INT32_MAX and exactly INT32_MIN are accepted
        Csr c;
        c.row({pi(4, INT32_MAX - 5), pi(4, 5)});
        c.row({});
        c.row({pi(2, INT32_MIN + 5), pi(5, 1), pi(2, -5)});
        const IntResult r = ingest(c, NAS_DT_I32, n, 3);
        check_int(r, dense_int(c, NAS_DT_I32, n), 3, 3, n);
        expect_lists(r, {0, 2, 2}, {4, 2, 5}, {127, -128, 1}, {0, 1, 1, 2}, {4, 2},
                     {INT32_MAX - 127, INT32_MIN + 128});
    }
    {  // one beyond either end is refused, naming the pod and the node
        Csr c;
        c.row({pi(1, 7)});
        c.row({});
        c.row({pi(0, 3), pi(4, INT32_MAX), pi(4, 1)});
        IntResult r = ingest(c, NAS_DT_I32, n, 3);
        CHECK(r.rc == NAS_ERR_UNSUPPORTED);
        CHECK(r.msg == "traffic of pod 2 to node 4 exceeds int32");
        Csr d;
        d.row({pi(3, -1), pi(5, 9), pi(3, INT32_MIN)});
        r = ingest(d, NAS_DT_I32, n, 1);
        CHECK(r.rc == NAS_ERR_UNSUPPORTED);
        CHECK(r.msg == "traffic of pod 0 to node 3 exceeds int32");
    }
    {  // int8 weights whose sum leaves int8
        Csr c;
        c.row({pi(2, 127), pi(2, 127), pi(2, 127), pi(0, -128), pi(0, -128)});
        const IntResult r = ingest(c, NAS_DT_I8, n, 2);
        check_int(r, dense_int(c, NAS_DT_I8, n), 1, 2, n);
        expect_lists(r, {0, 0}, {0, 2}, {-128, 127}, {0, 2, 2}, {0, 2}, {-128, 254});
    }
    {  // a pair that cancels: no triplet and no entry; its neighbours stay
        Csr c;
        c.row({pi(1, 50), pi(3, 9), pi(1, -50)});
        c.row({pi(2, 300), pi(2, -300)});
        const IntResult r = ingest(c, NAS_DT_I32, n, 2);
        check_int(r, dense_int(c, NAS_DT_I32, n), 2, 2, n);
        expect_lists(r, {0}, {3}, {9}, {0, 0, 0}, {}, {});
    }
    {  // peers -1 and n are skipped, node n - 1 next to them is not
        Csr c;
        c.row({pi(-1, 1000), pi(n, 1000), pi(n - 1, 200), pi(INT32_MIN, 5), pi(INT32_MAX, 5)});
        const IntResult r = ingest(c, NAS_DT_I32, n, 1);
        check_int(r, dense_int(c, NAS_DT_I32, n), 1, 1, n);
        expect_lists(r, {0}, {n - 1}, {127}, {0, 1}, {n - 1}, {73});
    }
    {  // non-adjacent duplicates of one node
        Csr c;
        c.row({pi(3, 100), pi(1, 5), pi(3, 100), pi(0, -7), pi(3, 100)});
        const IntResult r = ingest(c, NAS_DT_I32, n, 1);
        check_int(r, dense_int(c, NAS_DT_I32, n), 1, 1, n);
        expect_lists(r, {0, 0, 0}, {0, 1, 3}, {-7, 5, 127}, {0, 1}, {3}, {173});
    }
    {  // an empty CSR (no arrays behind nnz = 0) and P = 1
        const int32_t rp[3] = {0, 0, 0};
        for (int P = 1; P <= 2; ++P) {
            std::string msg;
            CHECK(check_csr_arrays(rp, nullptr, nullptr, NAS_DT_I32, 0, msg) == NAS_OK);
            CHECK(check_csr_rows(rp, P, 0, msg) == NAS_OK);
            Triplets<signed char> t;
            OvfLists o;
            CHECK(ingest_csr_int(rp, nullptr, nullptr, NAS_DT_I32, P, 4, n, t, o, msg) == NAS_OK);
            CHECK(t.pod.empty() && t.node.empty() && t.val.empty() && o.m.empty() && o.e.empty());
            CHECK(o.ptr == I32s(5, 0) && msg.empty());
            Triplets<float> tf;
            ingest_csr_f32(rp, nullptr, nullptr, P, n, tf);
            CHECK(tf.pod.empty() && tf.node.empty() && tf.val.empty());
        }
    }
}

static bool same_bits(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

static void pins_f32() {
    const int n = 5;
    Csr c;
    // sequential float summation gives 0: the sum is taken in double, rounded once
    c.row({pf(2, 1e8f), pf(2, 1.0f), pf(2, -1e8f)});
    // a cancelling pair still emits its 0.0; skipped peers; non-adjacent duplicates
    c.row({pf(4, 2.5f), pf(-1, 9.f), pf(0, 0.1f), pf(4, -2.5f), pf(n, 9.f), pf(0, 0.2f)});
    c.row({});
    Triplets<float> t;
    ingest_csr_f32(c.rp.data(), c.pn.data(), c.wf.data(), c.P(), n, t);
    CHECK(t.pod == I32s({0, 1, 1}) && t.node == I32s({2, 0, 4}));
    CHECK(t.val.size() == 3 && same_bits(t.val[0], 1.0f) && same_bits(t.val[2], 0.0f));
    CHECK(same_bits(t.val[1], (float)((double)0.1f + (double)0.2f)));
}

static void pins_checks() {
    const int32_t rp[4] = {0, 2, 2, 3}, pn[3] = {0, 1, 2}, w[3] = {1, 2, 3};
    std::string msg;
    const auto arrays = [&](const int32_t *r, const int32_t *p, const void *wt, int dt, int64_t nnz,
                            const char *want) {
        msg.clear();
        const int rc = check_csr_arrays(r, p, wt, dt, nnz, msg);
        CHECK(rc == (want ? NAS_ERR_ARG : NAS_OK) && msg == (want ? want : ""));
    };
    arrays(rp, pn, w, NAS_DT_I32, 3, nullptr);
    arrays(nullptr, pn, w, NAS_DT_I32, 3, "csr arrays");
    arrays(rp, pn, w, NAS_DT_I32, -1, "csr arrays");
    arrays(rp, nullptr, w, NAS_DT_I32, 3, "csr arrays");
    arrays(rp, pn, nullptr, NAS_DT_I32, 3, "csr arrays");
    arrays(nullptr, pn, w, 99, 3, "csr arrays");  // the arrays are looked at first
    for (int dt : {NAS_DT_I8, NAS_DT_BF16, NAS_DT_I32, NAS_DT_F32}) arrays(rp, pn, w, dt, 3, nullptr);
    for (int dt : {0, -1, 5, 99}) arrays(rp, pn, w, dt, 3, "csr weight dtype");
    const auto rows = [&](const int32_t *r, int P, int64_t nnz, const char *want) {
        msg.clear();
        const int rc = check_csr_rows(r, P, nnz, msg);
        CHECK(rc == (want ? NAS_ERR_ARG : NAS_OK) && msg == (want ? want : ""));
    };
    rows(rp, 3, 3, nullptr);
    rows(rp, 0, 0, "row_ptr bounds");
    rows(rp, -2, 3, "row_ptr bounds");
    rows(rp, 3, 4, "row_ptr bounds");   // row_ptr[P] != nnz
    rows(rp, 2, 3, "row_ptr bounds");
    const int32_t off[4] = {1, 2, 2, 3};
    rows(off, 3, 3, "row_ptr bounds");  // row_ptr[0] != 0
    const int32_t dip[4] = {0, 2, 1, 3};
    rows(dip, 3, 3, "row_ptr not monotone");
    const int32_t neg[4] = {0, -1, 2, 3};
    rows(neg, 3, 3, "row_ptr not monotone");
}

// P <= 40, n <= 12, degrees 0..20, about 10 % of the peers out of range;
// weights over int8 and over the whole int32 range
static long random_cases(int count) {
    std::mt19937_64 rng(0x4E4153);
    const auto below = [&](int k) { return (int)(rng() % (uint64_t)k); };
    long refused = 0;
    for (int it = 0; it < count; ++it) {
        const int P = 1 + below(40), n = 1 + below(12), Pp = P + below(9), kind = below(4);
        Csr c;
        for (int p = 0; p < P; ++p) {
            std::vector<Peer> peers(below(21));
            for (Peer &q : peers) {
                const int o = below(20);
                q.node = o == 0 ? -1 - below(3) : o == 1 ? n + below(3) : below(n);
                const int64_t full = (int64_t)(rng() >> 32) + INT32_MIN;  // all of int32
                // int8; a few hundred; one peer in eight anywhere in int32 (mostly
                // accepted); every peer anywhere in int32 (mostly refused)
                q.w = kind == 0 ? below(256) - 128 : kind == 1 || (kind == 2 && below(8)) ? below(801) - 400
                                                                                            : full;
                q.wf = (float)(below(2001) - 1000) * 0.125f;
            }
            c.row(peers);
        }
        const int dtype = kind == 0 ? NAS_DT_I8 : NAS_DT_I32;
        const std::vector<int64_t> D = dense_int(c, dtype, n);
        const IntResult r = ingest(c, dtype, n, Pp);
        // refused exactly when a dense sum leaves int32, naming the first such (pod, node)
        size_t bad = 0;
        while (bad < D.size() && D[bad] >= INT32_MIN && D[bad] <= INT32_MAX) ++bad;
        if (bad < D.size()) {
            ++refused;
            CHECK(r.rc == NAS_ERR_UNSUPPORTED);
            CHECK(r.msg == "traffic of pod " + std::to_string(bad / n) + " to node " +
                               std::to_string(bad % n) + " exceeds int32");
        } else {
            check_int(r, D, P, Pp, n);
        }
        // fp32: the double sums rounded once, for every (pod, node) with a peer
        // (the weights are multiples of 1/8 below 2^10: every sum is exact)
        std::vector<char> seen;
        const std::vector<double> F = dense_ref<double>(c, c.wf.data(), n, &seen);
        Triplets<float> t;
        ingest_csr_f32(c.rp.data(), c.pn.data(), c.wf.data(), P, n, t);
        size_t k = 0;
        for (size_t i = 0; i < F.size(); ++i) {
            if (!seen[i]) continue;
            CHECK(k < t.pod.size() && t.pod[k] == (int32_t)(i / n) && t.node[k] == (int32_t)(i % n));
            CHECK(same_bits(t.val[k], (float)F[i]));
            ++k;
        }
        CHECK(k == t.pod.size() && k == t.node.size() && k == t.val.size());
    }
    return refused;
}

// the brute-force maximum over all 384-row windows starting at multiples of 128
static void window_max() {
    std::mt19937_64 rng(7);
    for (int rows : {1, 100, 128, 256, 383, 384, 385, 512, 768, 1000, 1280})
        for (int rep = 0; rep < 6; ++rep) {
            I32s ptr((size_t)rows + 1, 0);
            for (int r = 0; r < rows; ++r) {
                // rep 0: no entries; else sparse rows with a few heavy ones
                const int k = rep == 0 ? 0 : rng() % 50 == 0 ? (int)(rng() % 400) : (int)(rng() % 3);
                ptr[r + 1] = ptr[r] + k;
            }
            int32_t want = 0;
            for (int s = 0; s < rows; s += 128) {
                int32_t cnt = 0;
                for (int r = s; r < s + 384 && r < rows; ++r) cnt += ptr[r + 1] - ptr[r];
                want = std::max(want, cnt);
            }
            CHECK(ovf_window_max(ptr.data(), rows) == want);
        }
    static_assert(OVF_WINDOW_ROWS == 384 && OVF_WINDOW_STEP == 128, "the wide cost tile's windows");
}

int main() {
    pins_int();
    pins_f32();
    pins_checks();
    const int cases = 4000;
    const long refused = random_cases(cases);
    CHECK(refused > cases / 20 && refused < cases / 2);  // both outcomes, the accepted one mostly
    window_max();
    std::printf("TRAFFIC INGEST OK %ld checks (%d random cases, %ld refused)\n", n_checked, cases,
                refused);
    return 0;
}
