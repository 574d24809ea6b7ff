// k_preempt.hip -- preemption: for each listed pod the node to take and the
// lower-priority bound pods to evict there (nas_preempt, include/nas.h), over
// the listed pods x all nodes.
//
// One node's answer for one pod (walk_node): the node's bound pods lie in
// priority-descending order (bound_index.h), so the pods below the asking
// priority are a suffix of its row.  A binary search finds where it starts, the
// suffix sums there give what evicting all of them frees, and if the pod fits
// into that the row is walked once from there: a pod that the rest still fits
// beside stays (reprieve), the others are the victims.  A pod that fits the
// free capacity as it is has no victims (requests are >= 0, so every step of
// the walk would reprieve) and skips the row.  All integer, 64-bit where free +
// freed can pass int32, so the answer is exact.
//
// k_preempt_scan, layout as k_explain: lane-per-NODE, a wave keeps PR_CHUNKS
// 64-node chunks (fit_wave.h's FitChunk, and the nodes' row bounds) in
// registers, a block one slab of PR_SLAB nodes.  The block walks 64-entry
// groups of the list (lane i loads entry i); each entry is broadcast
// (v_readlane: its operands are wave-uniform) and every lane answers it for its
// nodes, keeps the smallest key of them, and the wave reduces the 64 keys with
// shuffles.  The key orders (victimless first, top victim priority, priority
// sum, victim count, node) lexicographically in three 64-bit words
// (nas::PreemptPart); the node is its last component, so no two keys are equal
// and the order of reduction cannot matter.  Lane i keeps entry i's key and
// candidate count, the block's waves meet in LDS and wave 0 stores one partial
// per (slab, entry).  Grid: entry groups (x, striding) x node slabs (y).
//
// k_preempt_pick, a thread per entry: the smallest key over the slabs, the sum
// of their candidate counts, and the winner's row walked again to write the
// record and the victims' original indices.
#include "bound_index.h"
#include "fit_wave.h"

namespace nas {
namespace {

constexpr int PR_THREADS = 256;
constexpr int PR_WAVES = PR_THREADS / 64;
constexpr int PR_CHUNKS = 2;  // 64-node chunks resident per wave
constexpr int PR_SLAB = PR_WAVES * PR_CHUNKS * 64;  // nodes per block
constexpr u64 PR_NONE = ~0ull;

struct Key {
    u64 k0, k1, k2;
};
__device__ __forceinline__ bool key_less(const Key &a, const Key &b) {
    return a.k0 != b.k0 ? a.k0 < b.k0 : a.k1 != b.k1 ? a.k1 < b.k1 : a.k2 < b.k2;
}

struct Walk {
    bool cand;  // the pod fits the node once every lower-priority pod is gone
    int nv;     // victims
    int top;    // the first (= highest-priority) victim's priority
    u64 psum;   // sum of the victims' priority + 2^31
};

// Node with free capacity f and row [beg, end) of the table, for a pod with
// requests (a, b, d) and priority pi.  `elig`: the node may be a candidate at
// all.  W: the victims' original indices go to vout[0 .. min(nv, maxv)).
template <bool W>
__device__ __forceinline__ Walk walk_node(const BoundTab &t, int beg, int end, const int *f, int a,
                                          int b, int d, int pi, bool elig, int *vout, int maxv) {
    const size_t s = (size_t)t.B;
    const int *prio = t.tab + BT_PRIO * s, *req = t.tab + BT_REQ * s, *suf = t.tab + BT_SUF * s;
    Walk w{false, 0, 0, 0};
    if (elig && a <= f[0] && b <= f[1] && d <= f[2]) {
        // fits as it is: the walk would let every lower-priority pod stay
        w.cand = true;
        return w;
    }
    // the first entry with a priority below pi
    int lo = elig ? beg : end, hi = end;
    while (lo < hi) {
        const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
        if (prio[mid] >= pi) lo = mid + 1;
        else hi = mid;
    }
    long long av[3] = {f[0], f[1], f[2]};
    if (lo < end) {
#pragma unroll
        for (int r = 0; r < 3; ++r) av[r] += suf[r * s + lo];
    }
    w.cand = elig && a <= av[0] && b <= av[1] && d <= av[2];
    if (!w.cand) return w;
    for (int j = lo; j < end; ++j) {
        const int q0 = req[j], q1 = req[s + j], q2 = req[2 * s + j];
        if (av[0] - q0 >= a && av[1] - q1 >= b && av[2] - q2 >= d) {
            av[0] -= q0;
            av[1] -= q1;
            av[2] -= q2;
        } else {
            const int pj = prio[j];
            if (w.nv == 0) w.top = pj;
            w.psum += (unsigned)pj ^ 0x80000000u;
            if constexpr (W) {
                if (w.nv < maxv) vout[w.nv] = t.tab[BT_ORIG * s + j];
            }
            ++w.nv;
        }
    }
    return w;
}

template <bool C>
__global__ void __launch_bounds__(PR_THREADS)
k_preempt_scan(const int *cap, int N, const int *__restrict__ req, int rs,
               const int *__restrict__ pods, int first, const int *__restrict__ prio, int n,
               const BoundTab t, const Elig el, PreemptPart *__restrict__ part) {
    __shared__ u64 sk[PR_WAVES][3][64];
    __shared__ int sc[PR_WAVES][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int node0 = ((int)blockIdx.y * PR_WAVES + w) * PR_CHUNKS * 64 + lane;
    // (a wave whose nodes are all past N holds no candidate; every wave of the
    // block meets the barriers below)
    FitChunk<C> ch[PR_CHUNKS];
    int beg[PR_CHUNKS], end[PR_CHUNKS];
#pragma unroll
    for (int k = 0; k < PR_CHUNKS; ++k) {
        const bool real = node0 + 64 * k < N;
        ch[k].load(cap, N, node0 + 64 * k, real);
        beg[k] = real ? t.row[node0 + 64 * k] : 0;
        end[k] = real ? t.row[node0 + 64 * k + 1] : 0;
    }
#pragma unroll
    for (int k = 0; k < PR_CHUNKS; ++k) {
        const bool real = node0 + 64 * k < N;
        ch[k].reduce(real);
        if constexpr (C) ch[k].constrain(el, node0 + 64 * k, real);
    }
    for (long long pb = (long long)blockIdx.x * 64; pb < n; pb += (long long)gridDim.x * 64) {
        const int cnt = (int)min(64LL, n - pb);
        const bool in = lane < cnt;
        const int q = in ? (pods ? pods[pb + lane] : first + (int)pb + lane) : 0;
        const int ra = req[q], rb = req[rs + q], rd = req[2 * (size_t)rs + q];
        const int rp = in ? prio[pb + lane] : 0;
        u64 rq = 0, rt = 0;
        if constexpr (C) {
            rq = el.require[q];
            rt = el.tolerate[q];
        }
        Key mine{PR_NONE, PR_NONE, PR_NONE};
        int mc = 0;
        for (int i = 0; i < cnt; ++i) {
            const int a = __builtin_amdgcn_readlane(ra, i), b = __builtin_amdgcn_readlane(rb, i);
            const int d = __builtin_amdgcn_readlane(rd, i), pi = __builtin_amdgcn_readlane(rp, i);
            const u64 qi = C ? readlane64(rq, i) : 0, ti = C ? readlane64(rt, i) : 0;
            Key best{PR_NONE, PR_NONE, PR_NONE};
            int c = 0;
#pragma unroll
            for (int k = 0; k < PR_CHUNKS; ++k) {
                const FitChunk<C> &h = ch[k];
                bool e = node0 + 64 * k < N;
                if constexpr (C) e = e && (h.lb & qi) == qi && (h.tn & ~ti) == 0;
                const Walk r = walk_node<false>(t, beg[k], end[k], h.f, a, b, d, pi, e, nullptr, 0);
                c += __builtin_popcountll(__builtin_amdgcn_ballot_w64(r.cand));
                if (r.cand) {
                    const Key x{r.nv ? (u64)((unsigned)r.top ^ 0x80000000u) + 1 : 0, r.psum,
                                ((u64)(unsigned)r.nv << 32) | (unsigned)(node0 + 64 * k)};
                    if (key_less(x, best)) best = x;
                }
            }
#pragma unroll
            for (int o = 32; o; o >>= 1) {
                const Key y{__shfl_xor(best.k0, o), __shfl_xor(best.k1, o), __shfl_xor(best.k2, o)};
                if (key_less(y, best)) best = y;
            }
            if (lane == i) {
                mine = best;
                mc = c;
            }
        }
        sk[w][0][lane] = mine.k0;
        sk[w][1][lane] = mine.k1;
        sk[w][2][lane] = mine.k2;
        sc[w][lane] = mc;
        __syncthreads();
        if (w == 0 && in) {
#pragma unroll
            for (int v = 1; v < PR_WAVES; ++v) {
                const Key y{sk[v][0][lane], sk[v][1][lane], sk[v][2][lane]};
                if (key_less(y, mine)) mine = y;
                mc += sc[v][lane];
            }
            part[(size_t)blockIdx.y * n + pb + lane] = PreemptPart{mine.k0, mine.k1, mine.k2, mc, 0};
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(PR_THREADS)
k_preempt_pick(const PreemptPart *__restrict__ part, int slabs, const int *__restrict__ cap, int N,
               const int *__restrict__ req, int rs, const int *__restrict__ pods, int first,
               const int *__restrict__ prio, int n, const BoundTab t,
               nas_preemption *__restrict__ out, int *__restrict__ vict, int maxv) {
    const long long i = (long long)blockIdx.x * PR_THREADS + threadIdx.x;
    if (i >= n) return;
    Key best{PR_NONE, PR_NONE, PR_NONE};
    int cand = 0;
    for (int sl = 0; sl < slabs; ++sl) {
        const PreemptPart p = part[(size_t)sl * n + i];
        const Key y{p.k0, p.k1, p.k2};
        if (key_less(y, best)) best = y;
        cand += p.candidates;
    }
    nas_preemption r{NAS_EMPTY, 0, 0, cand, 0};
    if (best.k0 != PR_NONE) {
        const int node = (int)(unsigned)best.k2;
        const int q = pods ? pods[i] : first + (int)i;
        const int f[3] = {cap[node], cap[(size_t)N + node], cap[2 * (size_t)N + node]};
        const Walk wk = walk_node<true>(t, t.row[node], t.row[node + 1], f, req[q], req[rs + q],
                                        req[2 * (size_t)rs + q], prio[i], true,
                                        vict ? vict + (size_t)i * maxv : nullptr, vict ? maxv : 0);
        r.node = node;
        r.n_victims = wk.nv;
        r.top_priority = wk.top;
        r.priority_sum = (long long)wk.psum;
    }
    out[i] = r;
}

}  // namespace

int preempt_slabs(int N) { return (int)(((long long)N + PR_SLAB - 1) / PR_SLAB); }

hipError_t launch_preempt(hipStream_t st, const PreemptArgs &a) {
    if (a.n <= 0) return hipSuccess;
    if (a.N <= 0 || !a.cap || !a.req || !a.prio || !a.part || !a.out || !a.tab.row ||
        (a.tab.B > 0 && !a.tab.tab) || a.maxv < 0 || (a.maxv > 0 && !a.vict))
        return hipErrorInvalidValue;
    const Elig *el = a.el;
    if (el && (!el->labels || !el->taints || !el->require || !el->tolerate))
        return hipErrorInvalidValue;
    const int slabs = preempt_slabs(a.N);
    if (slabs > 65535) return hipErrorInvalidValue;
    // entry groups: every group its own block until the device is full (8
    // blocks of 4 waves per CU); beyond that the blocks stride over the groups
    // and keep their chunks
    const long long groups = ((long long)a.n + 63) / 64;
    const long long room = std::max(1LL, 8LL * std::max(a.n_cu, 1) / slabs);
    dim3 grid((unsigned)std::min(groups, room), (unsigned)slabs);
    if (el)
        k_preempt_scan<true><<<grid, PR_THREADS, 0, st>>>(a.cap, a.N, a.req, a.rs, a.pods, a.first,
                                                          a.prio, a.n, a.tab, *el, a.part);
    else
        k_preempt_scan<false><<<grid, PR_THREADS, 0, st>>>(a.cap, a.N, a.req, a.rs, a.pods, a.first,
                                                           a.prio, a.n, a.tab, Elig{}, a.part);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    k_preempt_pick<<<(unsigned)(((long long)a.n + PR_THREADS - 1) / PR_THREADS), PR_THREADS, 0, st>>>(
        a.part, slabs, a.cap, a.N, a.req, a.rs, a.pods, a.first, a.prio, a.n, a.tab, a.out, a.vict,
        a.maxv);
    return hipGetLastError();
}

}  // namespace nas
