"""Reference for node selectors and taints (include/nas.h): eligibility from
the four uint64 word arrays, the sequential greedy placement over `fits =
eligible and the three resources fit` as a plain Python loop, and the seeded
word patterns the CPU and GPU tests share."""
import numpy as np

import oracle


def eligible(labels, taints, require, tolerate):
    """(P, N) bool: (labels[n] & require[p]) == require[p] and
    (taints[n] & ~tolerate[p]) == 0."""
    lab = np.asarray(labels, np.uint64)[None, :]
    tnt = np.asarray(taints, np.uint64)[None, :]
    rq = np.asarray(require, np.uint64)[:, None]
    tl = np.asarray(tolerate, np.uint64)[:, None]
    return ((lab & rq) == rq) & ((tnt & ~tl) == 0)


def place(WA, L, req, free, elig, dtype="i8"):
    """Sequential greedy: pod p takes the smallest (cost, node) among the nodes
    with elig[p] and req[p] <= free in all three resources at its own turn.
    -> (node [P] (-1: none), cost [P] (0 for none), free_after (N, 3))."""
    cost = oracle.cost(WA, L, dtype)
    free = np.asarray(free, np.int64).copy()
    req = np.asarray(req, np.int64)
    P = req.shape[0]
    node = np.full(P, -1, np.int32)
    score = np.zeros(P, cost.dtype)
    for p in range(P):
        ok = np.flatnonzero(elig[p] & (req[p] <= free).all(1))
        if len(ok):
            n = ok[np.argmin(cost[p, ok])]  # the first minimum: the smallest node among ties
            node[p], score[p] = n, cost[p, n]
            free[n] -= req[p]
    return node, score, free.astype(np.int32)


def words32(bits):
    """(P, N) bool -> uint32 (P, ceil(N/32)), bit j of word w = node 32w + j
    (oracle.fit_mask's layout)."""
    P, N = bits.shape
    W = (N + 31) // 32
    pad = np.zeros((P, W * 32), np.uint8)
    pad[:, :N] = bits
    return np.packbits(pad, axis=1, bitorder="little").view("<u4").reshape(P, W)


def words64(w32):
    """uint32 (P, W) -> Engine.filter()'s layout: uint64 [ceil(N/64)][P]."""
    P, W = w32.shape
    pad = np.zeros((P, (W + 1) // 2 * 2), np.uint32)
    pad[:, :W] = w32
    lo, hi = pad[:, 0::2].astype(np.uint64), pad[:, 1::2].astype(np.uint64)
    return np.ascontiguousarray((lo | (hi << np.uint64(32))).T)


def fits32(req, free, elig):
    """oracle.fit_mask's resource words ANDed with the eligibility words."""
    return oracle.fit_mask(req, free) & words32(elig)


def pattern(name, rng, P, N):
    """-> (labels [N], taints [N], require [P], tolerate [P]) uint64.
    "allfit": nodes carry random labels, every pod has require = 0 and no node
    is tainted (eligibility never excludes: the all-fit fast path);
    "nolabel": every pod requires a label no node carries (the fit-none fast
    path); "mix": each node carries 3 of 8 label bits, each pod requires 0 to
    2 of the 8, about half the nodes carry taint bit 40 and about half the
    pods tolerate it."""
    lab = np.zeros(N, np.uint64)
    tnt = np.zeros(N, np.uint64)
    rq = np.zeros(P, np.uint64)
    tl = np.zeros(P, np.uint64)
    if name == "allfit":
        lab[:] = rng.integers(0, 256, N).astype(np.uint64)
    elif name == "nolabel":
        lab[:] = rng.integers(0, 256, N).astype(np.uint64)
        rq[:] = np.uint64(1) << np.uint64(63)
    elif name == "mix":
        for n in range(N):
            for b in rng.choice(8, 3, replace=False):
                lab[n] |= np.uint64(1) << np.uint64(b)
        k = rng.integers(0, 3, P)
        for p in range(P):
            for b in rng.choice(8, k[p], replace=False):
                rq[p] |= np.uint64(1) << np.uint64(b)
        tnt[rng.random(N) < 0.5] = np.uint64(1) << np.uint64(40)
        tl[rng.random(P) < 0.5] = np.uint64(1) << np.uint64(40)
    else:
        raise ValueError(name)
    return lab, tnt, rq, tl
