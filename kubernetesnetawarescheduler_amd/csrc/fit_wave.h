// fit_wave.h -- the wave-level fit decision (device only), written once for
// k_fit.hip, the fused fit of k_cost.hip and tools/mb_fit.hip.
//
// Pod p fits node n iff req[r][p] <= free[r][n] for the three resources and,
// in the constrained form (C = true, nas::Elig), n is eligible for p:
// (labels[n] & require[p]) == require[p] and (taints[n] & ~tolerate[p]) == 0.
//
// A wave owns one 64-node chunk (lane j = the chunk's node j):
//   * FitChunk::load reads the lane's node's free capacities, FitChunk::reduce
//     makes the chunk's valid-node mask, minima and maxima, FitChunk::constrain
//     (C) reads the node's label and taint words and makes the AND / OR of
//     each -- all wave-uniform;
//   * fit_decide takes one pod per lane and returns the lane's pod's fit word
//     (bit j <=> the pod fits node j of the chunk): the pods that fit EVERY
//     valid node (requests <= the minima, require within AND(labels), every
//     taint of OR(taints) tolerated: word = the valid mask) and the pods that
//     fit NONE (a request above its maximum, a required label outside
//     OR(labels), a taint of AND(taints) not tolerated: word = 0) are decided
//     for all lanes at once; each remaining pod is broadcast (v_readlane) and
//     compared against the 64 lanes' nodes, three (five) ballots ANDed.
#pragma once

#include "nas_internal.h"

namespace nas {

typedef unsigned long long u64;

// the chunk's AND / OR of a per-node word, wave-uniform
__device__ __forceinline__ u64 wave_and(u64 v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v &= __shfl_xor(v, o);
    return ((u64)(unsigned)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32) |
           (unsigned)__builtin_amdgcn_readfirstlane((int)v);
}
__device__ __forceinline__ u64 wave_or(u64 v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v |= __shfl_xor(v, o);
    return ((u64)(unsigned)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32) |
           (unsigned)__builtin_amdgcn_readfirstlane((int)v);
}
// lane i's 64-bit word, wave-uniform
__device__ __forceinline__ u64 readlane64(u64 v, int i) {
    return ((u64)(unsigned)__builtin_amdgcn_readlane((int)(v >> 32), i) << 32) |
           (unsigned)__builtin_amdgcn_readlane((int)v, i);
}

// One wave's 64-node chunk.  `real`: the lane's node exists (padding lanes
// hold capacity -1 and fit nothing).  load and reduce are separate steps so
// that a caller can put work between the loads' issue and their first use.
template <bool C>
struct FitChunk {
    int f[3];          // the lane's node's free capacities
    u64 valid;         // the chunk's real nodes (wave-uniform, as all below)
    int mn[3], mx[3];  // smallest / largest capacity over the real nodes
    u64 lb, tn;        // (C) the lane's node's label / taint words
    u64 l_and, l_or, t_and, t_or;  // (C) their AND / OR over the real nodes

    // cap: [3][N] free capacity, node: the lane's index into it.  Relaxed
    // atomic loads: nas_place filters against the working capacity while the
    // commit stream publishes into it.
    __device__ __forceinline__ void load(const int *cap, int N, int node, bool real) {
        f[0] = f[1] = f[2] = -1;
        if (!real) return;
        int *cp = const_cast<int *>(cap) + node;
#pragma unroll
        for (int r = 0; r < 3; ++r, cp += N)
            f[r] = __hip_atomic_load(cp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __device__ __forceinline__ void reduce(bool real) {
        valid = __builtin_amdgcn_ballot_w64(real);
        int a[3], x[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            a[r] = real ? f[r] : 0x7fffffff;
            x[r] = real ? f[r] : (int)0x80000000;
        }
        // (the six reductions step together: one shuffle address per step)
#pragma unroll
        for (int o = 32; o; o >>= 1)
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                a[r] = min(a[r], __shfl_xor(a[r], o));
                x[r] = max(x[r], __shfl_xor(x[r], o));
            }
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            mn[r] = __builtin_amdgcn_readfirstlane(a[r]);
            mx[r] = __builtin_amdgcn_readfirstlane(x[r]);
        }
    }
    // (C) the node's constraint words and their AND / OR, a step of its own
    // after reduce(): loaded beside the capacities, the words and the padding
    // lanes' neutral values stay live through the minima / maxima (k_fit_c
    // took 6 more registers)
    __device__ __forceinline__ void constrain(const Elig &el, int node, bool real) {
        lb = tn = 0;
        if (real) {
            lb = el.labels[node];
            tn = el.taints[node];
        }
        l_and = wave_and(real ? lb : ~0ull);
        l_or = wave_or(lb);
        t_and = wave_and(real ? tn : ~0ull);
        t_or = wave_or(tn);
    }
};

// The fit word of the lane's pod: requests (a, b, d) and, under C, its
// require / tolerate words (rq, rt).  NP = distinct pods per wave: lanes l,
// l + NP, ... hold the same pod.  `in`: the lane's pod is in range (the word
// of a lane out of range is 0).  Every lane of the wave calls it: the ballots
// and broadcasts run over all 64.
template <int NP, bool C>
__device__ __forceinline__ u64 fit_decide(const FitChunk<C> &ch, int lane, int a, int b, int d,
                                          bool in, u64 rq = 0, u64 rt = 0) {
    // eligible on every valid node / on none (the words are read under C only)
    const bool e_all = !C || ((rq & ~ch.l_and) == 0 && (ch.t_or & ~rt) == 0);
    const bool e_none = C && ((rq & ~ch.l_or) != 0 || (ch.t_and & ~rt) != 0);
    const bool all = in && a <= ch.mn[0] && b <= ch.mn[1] && d <= ch.mn[2] && e_all;
    const bool none = a > ch.mx[0] || b > ch.mx[1] || d > ch.mx[2] || e_none;
    u64 word = all ? ch.valid : 0ull;
    u64 rest = __builtin_amdgcn_ballot_w64(in && !all && !none);
    if constexpr (NP < 64) rest &= (1ull << NP) - 1;
    while (rest) {
        const int i = (int)__builtin_ctzll(rest);
        rest &= rest - 1;
        const int ba = __builtin_amdgcn_readlane(a, i), bb = __builtin_amdgcn_readlane(b, i);
        const int bd = __builtin_amdgcn_readlane(d, i);
        u64 m = __builtin_amdgcn_ballot_w64(ba <= ch.f[0]) &
                __builtin_amdgcn_ballot_w64(bb <= ch.f[1]) &
                __builtin_amdgcn_ballot_w64(bd <= ch.f[2]);
        if constexpr (C) {
            const u64 qi = readlane64(rq, i), ti = readlane64(rt, i);
            m &= __builtin_amdgcn_ballot_w64((ch.lb & qi) == qi) &
                 __builtin_amdgcn_ballot_w64((ch.tn & ~ti) == 0);
        }
        if ((lane & (NP - 1)) == i) word = m;
    }
    return word;
}

}  // namespace nas
