// traffic_ingest.h -- uploaded traffic into what the device holds: the int8
// plane, the overflow lists (nas::Ovf, nas_internal.h) and the triplets the
// scatter kernels take.  Host code with no HIP dependence (it compiles alone,
// e.g. into a sanitizer driver).
//
// Exact integer traffic WA = plane + E: the plane holds every entry clamped to
// [-128, 127], E the entries outside it as per-row lists -- row r of the pod
// array owns entries [ptr[r], ptr[r + 1]) of (node m, excess e = WA - plane).
// split_value is that rule and join_rows its inverse.  CSR traffic is
// aggregated per (pod, node) a row at a time: int64 sums that must fit int32,
// or fp64 sums rounded to fp32 once.  Nothing here allocates O(P n).
#pragma once

#include <stdint.h>

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "../../include/nas.h"

namespace nas {

// (pod, node, value) entries of the dense traffic rows, pods ascending and
// nodes ascending within a pod
template <typename T>
struct Triplets {
    std::vector<int32_t> pod, node;
    std::vector<T> val;
};

// overflow lists of the padded pod rows: ptr[rows + 1] absolute offsets
struct OvfLists {
    std::vector<int32_t> ptr, m, e;
};

// exact value (within int32) at `node` -> its plane value; what the plane
// cannot hold is appended to the row's overflow entries
inline signed char split_value(int64_t x, int32_t node, std::vector<int32_t> &m,
                               std::vector<int32_t> &e) {
    const int64_t c = x < -128 ? -128 : x > 127 ? 127 : x;
    if (x != c) {
        m.push_back(node);
        e.push_back((int32_t)(x - c));
    }
    return (signed char)c;
}

// exact traffic row (n values, each within int32) -> the int8 plane row and
// the row's overflow entries (node, excess)
inline void split_row(const int64_t *v, int n, signed char *plane, std::vector<int32_t> &m,
                      std::vector<int32_t> &e) {
    for (int j = 0; j < n; ++j) plane[j] = split_value(v[j], j, m, e);
}

// ptr with ptr[r + 1] set for the rows that were split and 0 elsewhere:
// padding rows carry the running offset
inline void carry_offsets(std::vector<int32_t> &ptr) {
    for (size_t r = 1; r < ptr.size(); ++r) ptr[r] = std::max(ptr[r], ptr[r - 1]);
}

// plane rows [rows][n] and their lists -> the exact int32 rows.  ptr[rows + 1]
// holds absolute offsets, m / e the entries from ptr[0] on.
inline void join_rows(const signed char *plane, int64_t rows, int n, const int32_t *ptr,
                      const int32_t *m, const int32_t *e, int32_t *out) {
    for (int64_t i = 0; i < rows * n; ++i) out[i] = plane[i];
    for (int64_t r = 0; r < rows; ++r)
        for (int32_t j = ptr[r]; j < ptr[r + 1]; ++j) out[r * n + m[j - ptr[0]]] += e[j - ptr[0]];
}

// The wide cost tile covers OVF_WINDOW_ROWS pod rows and starts at multiples
// of OVF_WINDOW_STEP (k_cost.hip asserts both against its tiles): the most
// entries of any such window of ptr[0 .. rows] (Ovf::tile_max)
constexpr int OVF_WINDOW_ROWS = 384;
constexpr int OVF_WINDOW_STEP = 128;
inline int32_t ovf_window_max(const int32_t *ptr, int64_t rows) {
    int32_t mx = 0;
    for (int64_t s = 0; s < rows; s += OVF_WINDOW_STEP)
        mx = std::max(mx, ptr[std::min<int64_t>(s + OVF_WINDOW_ROWS, rows)] - ptr[s]);
    return mx;
}

// ---- CSR traffic: pod p's peers are entries [row_ptr[p], row_ptr[p + 1]) of
// (peer_node, weight)

// NAS_OK or NAS_ERR_ARG with msg set: the arrays and the weight dtype ...
inline int check_csr_arrays(const int32_t *row_ptr, const int32_t *peer_node, const void *weight,
                            int32_t dtype, int64_t nnz, std::string &msg) {
    if (!row_ptr || nnz < 0 || (nnz > 0 && (!peer_node || !weight))) {
        msg = "csr arrays";
        return NAS_ERR_ARG;
    }
    if (dtype != NAS_DT_I8 && dtype != NAS_DT_I32 && dtype != NAS_DT_BF16 && dtype != NAS_DT_F32) {
        msg = "csr weight dtype";
        return NAS_ERR_ARG;
    }
    return NAS_OK;
}
// ... and the row offsets of the P pods
inline int check_csr_rows(const int32_t *row_ptr, int32_t P, int64_t nnz, std::string &msg) {
    if (P <= 0 || row_ptr[0] != 0 || row_ptr[P] != nnz) {
        msg = "row_ptr bounds";
        return NAS_ERR_ARG;
    }
    for (int p = 0; p < P; ++p)
        if (row_ptr[p + 1] < row_ptr[p]) {
            msg = "row_ptr not monotone";
            return NAS_ERR_ARG;
        }
    return NAS_OK;
}

// Pod p's peers on nodes [0, n) (an unbound or off-cluster peer is skipped),
// summed per node in Acc: emit(node, sum) per node with a peer, nodes
// ascending; a result other than NAS_OK ends the row and is returned.
// weight_at(x) reads entry x's weight; agg is scratch the caller reuses.
template <typename Acc, typename WeightAt, typename Emit>
inline int aggregate_row(const int32_t *row_ptr, const int32_t *peer_node, int32_t p, int32_t n,
                         std::vector<std::pair<int32_t, Acc>> &agg, WeightAt weight_at, Emit emit) {
    agg.clear();
    for (int64_t x = row_ptr[p]; x < row_ptr[p + 1]; ++x)
        if (peer_node[x] >= 0 && peer_node[x] < n) agg.push_back({peer_node[x], (Acc)weight_at(x)});
    std::sort(agg.begin(), agg.end(), [](const auto &a, const auto &b) { return a.first < b.first; });
    for (size_t i = 0; i < agg.size();) {
        const int32_t m = agg[i].first;
        Acc v = 0;
        for (; i < agg.size() && agg[i].first == m; ++i) v += agg[i].second;
        const int rc = emit(m, v);
        if (rc != NAS_OK) return rc;
    }
    return NAS_OK;
}

// int8 / int32 weights (dtype NAS_DT_I8 / NAS_DT_I32): exact int64 sums.  A
// non-zero sum gives a plane triplet and, beyond int8, an overflow entry;
// ovf.ptr covers the Pp >= P padded rows.  A sum outside int32:
// NAS_ERR_UNSUPPORTED with msg set (the outputs are then unspecified).
inline int ingest_csr_int(const int32_t *row_ptr, const int32_t *peer_node, const void *weight,
                          int32_t dtype, int32_t P, int32_t Pp, int32_t n,
                          Triplets<signed char> &t, OvfLists &ovf, std::string &msg) {
    ovf.ptr.assign((size_t)Pp + 1, 0);
    std::vector<std::pair<int32_t, int64_t>> agg;
    const auto weight_at = [&](int64_t x) {
        return dtype == NAS_DT_I8 ? (int64_t) static_cast<const int8_t *>(weight)[x]
                                  : (int64_t) static_cast<const int32_t *>(weight)[x];
    };
    for (int32_t p = 0; p < P; ++p) {
        const int rc = aggregate_row<int64_t>(row_ptr, peer_node, p, n, agg, weight_at,
                                              [&](int32_t m, int64_t v) {
            if (v < INT32_MIN || v > INT32_MAX) {
                msg = "traffic of pod " + std::to_string(p) + " to node " + std::to_string(m) +
                      " exceeds int32";
                return NAS_ERR_UNSUPPORTED;
            }
            if (v == 0) return NAS_OK;
            t.pod.push_back(p);
            t.node.push_back(m);
            t.val.push_back(split_value(v, m, ovf.m, ovf.e));
            return NAS_OK;
        });
        if (rc != NAS_OK) return rc;
        ovf.ptr[(size_t)p + 1] = (int32_t)ovf.m.size();
    }
    carry_offsets(ovf.ptr);
    return NAS_OK;
}

// fp32 weights: per-node sums in fp64, rounded to fp32 once; every (pod, node)
// with a peer gives a triplet, a sum of 0.0 too
inline void ingest_csr_f32(const int32_t *row_ptr, const int32_t *peer_node, const float *weight,
                           int32_t P, int32_t n, Triplets<float> &t) {
    std::vector<std::pair<int32_t, double>> agg;
    for (int32_t p = 0; p < P; ++p)
        (void)aggregate_row<double>(row_ptr, peer_node, p, n, agg,
                                    [&](int64_t x) { return weight[x]; },
                                    [&](int32_t m, double v) {
            t.pod.push_back(p);
            t.node.push_back(m);
            t.val.push_back((float)v);
            return NAS_OK;
        });
}

}  // namespace nas
