// k_explain.hip -- why a pod does not fit: per-reason node counts over the
// listed pods x all nodes (nas_explain, include/nas.h NAS_WHY_*).
//
// A node is owned by the first filter that rejects it, in Kubernetes' plugin
// order: an untolerated taint, else a missing required label, else short
// resources (req > free; the node then counts once under RESOURCES and under
// each of CPU / MEM / PODS that is short), else it fits.  So for every pod
// TAINT + SELECTOR + RESOURCES + FIT == N.
//
// Layout: lane-per-NODE, as k_fit.  A wave keeps EX_CHUNKS 64-node chunks
// (fit_wave.h's FitChunk: capacities, label / taint words, their extremes) in
// registers; the four waves of a block hold consecutive node ranges, a block
// one slab of EX_SLAB nodes.  The block walks 64-pod groups of the list (lane
// i loads list entry i's requests and words); each pod is broadcast
// (v_readlane, so its operands are wave-uniform) and classified against the
// wave's chunks: five compares, ballots masked with the chunk's valid nodes,
// six popcounts (FIT is what the three owners leave of the valid nodes).  The
// loop body is branch-free scalar code, and the CU's one scalar unit bounds
// the kernel.  Wave-uniform shortcuts from the chunk's extremes ("fits every
// valid node", "a taint of AND(taints) is not tolerated") were measured and
// dropped: the pods one asks about fit nowhere, and where neither decides (the
// mixed words of tools/explain_pass.py) their tests and branches doubled the
// scalar work per chunk.  Lane i keeps pod i's seven counts; the
// block adds its waves' counts in LDS and wave 0 adds the non-zero sums into
// the zeroed record with integer atomics (order-independent, so the output is
// deterministic).  Slot NAS_WHY_NODES is stored by node slab 0 alone.
// Grid: pod slabs (x, striding over the groups) x node slabs (y).
#include "fit_wave.h"

namespace nas {
namespace {

constexpr int EX_THREADS = 256;
constexpr int EX_WAVES = EX_THREADS / 64;
constexpr int EX_CHUNKS = 4;  // 64-node chunks resident per wave
constexpr int EX_SLAB = EX_WAVES * EX_CHUNKS * 64;  // nodes per block
constexpr int EX_SUMS = NAS_WHY_NODES;  // the seven counted slots

__device__ __forceinline__ int popc(u64 m) { return __builtin_popcountll(m); }

template <bool C>
__global__ void __launch_bounds__(EX_THREADS)
k_explain(const int *cap, int N, const int *__restrict__ req, int rs,
          const int *__restrict__ pods, int n_pods, int *__restrict__ out, const Elig el) {
    __shared__ int acc[EX_SUMS][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int node0 = ((int)blockIdx.y * EX_WAVES + w) * EX_CHUNKS * 64 + lane;
    // (a wave whose nodes are all past N keeps empty chunks and counts nothing:
    // every wave of the block meets the barriers below)
    FitChunk<C> ch[EX_CHUNKS];
    int nv = 0;  // the wave's valid nodes
#pragma unroll
    for (int k = 0; k < EX_CHUNKS; ++k) ch[k].load(cap, N, node0 + 64 * k, node0 + 64 * k < N);
#pragma unroll
    for (int k = 0; k < EX_CHUNKS; ++k) {
        const bool real = node0 + 64 * k < N;
        ch[k].reduce(real);
        if constexpr (C) ch[k].constrain(el, node0 + 64 * k, real);
        nv += popc(ch[k].valid);
    }
    for (long long pb = (long long)blockIdx.x * 64; pb < n_pods; pb += (long long)gridDim.x * 64) {
        const int cnt = (int)min(64LL, n_pods - pb);
        const bool in = lane < cnt;
        const int q = in ? (pods ? pods[pb + lane] : (int)pb + lane) : 0;
        const int ra = req[q], rb = req[rs + q], rd = req[2 * (size_t)rs + q];
        u64 rq = 0, rt = 0;
        if constexpr (C) {
            rq = el.require[q];
            rt = el.tolerate[q];
        }
        int c[EX_SUMS];
#pragma unroll
        for (int j = 0; j < EX_SUMS; ++j) c[j] = 0;
        for (int i = 0; i < cnt; ++i) {
            const int a = __builtin_amdgcn_readlane(ra, i), b = __builtin_amdgcn_readlane(rb, i);
            const int d = __builtin_amdgcn_readlane(rd, i);
            const u64 qi = C ? readlane64(rq, i) : 0, ti = C ? readlane64(rt, i) : 0;
            // class ballots of the wave's chunks.  Padding lanes hold zero
            // words and capacity -1: never tainted, masked out of the rest by
            // `valid`.  FIT is what the three owners leave of the valid nodes
            int s[NAS_WHY_FIT];
#pragma unroll
            for (int j = 0; j < NAS_WHY_FIT; ++j) s[j] = 0;
#pragma unroll
            for (int k = 0; k < EX_CHUNKS; ++k) {
                const FitChunk<C> &h = ch[k];
                u64 E = h.valid;
                if constexpr (C) {
                    const u64 T = __builtin_amdgcn_ballot_w64((h.tn & ~ti) != 0);
                    const u64 S = __builtin_amdgcn_ballot_w64((h.lb & qi) != qi) & E & ~T;
                    E ^= T | S;
                    s[NAS_WHY_TAINT] += popc(T);
                    s[NAS_WHY_SELECTOR] += popc(S);
                }
                const u64 Rc = __builtin_amdgcn_ballot_w64(a > h.f[0]) & E;
                const u64 Rm = __builtin_amdgcn_ballot_w64(b > h.f[1]) & E;
                const u64 Rp = __builtin_amdgcn_ballot_w64(d > h.f[2]) & E;
                s[NAS_WHY_RESOURCES] += popc(Rc | Rm | Rp);
                s[NAS_WHY_CPU] += popc(Rc);
                s[NAS_WHY_MEM] += popc(Rm);
                s[NAS_WHY_PODS] += popc(Rp);
            }
            if (lane == i) {
#pragma unroll
                for (int j = 0; j < NAS_WHY_FIT; ++j) c[j] = s[j];
                c[NAS_WHY_FIT] = nv - s[NAS_WHY_TAINT] - s[NAS_WHY_SELECTOR] - s[NAS_WHY_RESOURCES];
            }
        }
        // the block's sums of the group's pods: wave 0 stores, the others add
        if (w == 0) {
#pragma unroll
            for (int j = 0; j < EX_SUMS; ++j) acc[j][lane] = c[j];
        }
        __syncthreads();
        if (w != 0) {
#pragma unroll
            for (int j = 0; j < EX_SUMS; ++j)
                if (c[j]) atomicAdd(&acc[j][lane], c[j]);
        }
        __syncthreads();
        // (wave 0 alone reads acc here and stores it next round, in program
        // order; the other waves add again only behind the next barrier)
        if (w == 0 && in) {
            int *rec = out + (size_t)(pb + lane) * NAS_WHY_COUNT;
#pragma unroll
            for (int j = 0; j < EX_SUMS; ++j) {
                const int v = acc[j][lane];
                if (v) atomicAdd(rec + j, v);
            }
            if (blockIdx.y == 0) rec[NAS_WHY_NODES] = N;
        }
    }
}

}  // namespace

hipError_t launch_explain(hipStream_t st, const int32_t *cap, int N, const int32_t *req, int rs,
                          const int32_t *pods, int n_pods, int32_t *out, const Elig *el, int n_cu) {
    if (n_pods <= 0) return hipSuccess;
    if (N <= 0 || !cap || !req || !out) return hipErrorInvalidValue;
    if (el && (!el->labels || !el->taints || !el->require || !el->tolerate))
        return hipErrorInvalidValue;
    const long long slabs = ((long long)N + EX_SLAB - 1) / EX_SLAB;
    if (slabs > 65535) return hipErrorInvalidValue;
    // pod slabs: every group its own block until the device is full (8 blocks
    // of 4 waves per CU); beyond that the blocks stride over the groups and
    // keep their chunks
    const long long groups = ((long long)n_pods + 63) / 64;
    const long long room = std::max(1LL, 8LL * std::max(n_cu, 1) / slabs);
    dim3 grid((unsigned)std::min(groups, room), (unsigned)slabs);
    if (el)
        k_explain<true><<<grid, EX_THREADS, 0, st>>>(cap, N, req, rs, pods, n_pods, out, *el);
    else
        k_explain<false><<<grid, EX_THREADS, 0, st>>>(cap, N, req, rs, pods, n_pods, out, Elig{});
    return hipGetLastError();
}

}  // namespace nas
