// bound_index.h -- the per-node index of the running ("bound") pods that
// nas_upload_bound builds for k_preempt.hip.  Host code with no HIP dependence
// (it compiles alone, e.g. into a sanitizer driver).
//
// The bound pods in a stable order by (node ascending, priority descending, b
// ascending), as eight arrays of B ints (nas::BT_*) plus row offsets: node n's
// pods are entries [row[n], row[n + 1]).  The suffix arrays hold, per entry,
// the node's requests summed from that entry to the end of its row -- what
// evicting everything from there on gives back -- so the sum over the pods
// below a priority is one lookup at the first such entry.  Every per-node sum
// fits int32: a larger one is rejected here.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <numeric>
#include <string>
#include <vector>

#include "../../include/nas.h"

namespace nas {

// rows of BoundIndex::tab ([BT_ROWS][B])
enum { BT_PRIO, BT_REQ, BT_SUF = BT_REQ + 3, BT_ORIG = BT_SUF + 3, BT_ROWS };

struct BoundIndex {
    std::vector<int32_t> row;  // [N + 1]
    std::vector<int32_t> tab;  // [BT_ROWS][B]
};

// NAS_OK, or NAS_ERR_ARG / NAS_ERR_UNSUPPORTED with msg set (out is then unspecified)
inline int build_bound_index(const int32_t *node, const int32_t *priority, const int32_t *rc,
                             const int32_t *rm, const int32_t *rp, int32_t B, int32_t N,
                             BoundIndex &out, std::string &msg) {
    if (B < 0 || N <= 0) {
        msg = "nas_upload_bound: B = " + std::to_string(B) + ", n = " + std::to_string(N);
        return NAS_ERR_ARG;
    }
    if (B > 0 && (!node || !priority || !rc || !rm || !rp)) {
        msg = "nas_upload_bound: a NULL array with B > 0";
        return NAS_ERR_ARG;
    }
    const int32_t *req[3] = {rc, rm, rp};
    for (int32_t b = 0; b < B; ++b) {
        if (node[b] < 0 || node[b] >= N) {
            msg = "nas_upload_bound: node[" + std::to_string(b) + "] = " + std::to_string(node[b]) +
                  " is not one of the " + std::to_string(N) + " nodes";
            return NAS_ERR_ARG;
        }
        for (int r = 0; r < 3; ++r)
            if (req[r][b] < 0) {
                msg = "nas_upload_bound: bound pod " + std::to_string(b) + " has a negative request";
                return NAS_ERR_ARG;
            }
    }
    std::vector<int32_t> order((size_t)B);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) {
        return node[x] != node[y] ? node[x] < node[y] : priority[x] > priority[y];
    });
    out.row.assign((size_t)N + 1, 0);
    for (int32_t b = 0; b < B; ++b) ++out.row[(size_t)node[b] + 1];
    for (int32_t n = 0; n < N; ++n) out.row[(size_t)n + 1] += out.row[n];
    out.tab.assign((size_t)BT_ROWS * B, 0);
    int32_t *t = out.tab.data();
    const size_t s = (size_t)B;
    int64_t sum[3] = {0, 0, 0};
    for (int32_t e = B - 1; e >= 0; --e) {
        const int32_t b = order[e];
        if (e == B - 1 || node[order[e + 1]] != node[b]) sum[0] = sum[1] = sum[2] = 0;
        t[BT_PRIO * s + e] = priority[b];
        t[BT_ORIG * s + e] = b;
        for (int r = 0; r < 3; ++r) {
            sum[r] += req[r][b];
            if (sum[r] > INT32_MAX) {
                msg = "nas_upload_bound: the bound requests of node " + std::to_string(node[b]) +
                      " sum above INT32_MAX";
                return NAS_ERR_UNSUPPORTED;
            }
            t[(BT_REQ + r) * s + e] = req[r][b];
            t[(BT_SUF + r) * s + e] = (int32_t)sum[r];
        }
    }
    return NAS_OK;
}

}  // namespace nas
