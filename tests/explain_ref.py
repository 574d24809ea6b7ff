"""Reference for nas_explain (include/nas.h NAS_WHY_*): per-reason node counts
of every pod by numpy broadcasting over (P, N), and the seeded generator the
CPU and GPU tests share.

A node is owned by the first filter that rejects it: an untolerated taint,
else a missing required label, else short resources (req > free; the node then
counts once under RESOURCES and under each short resource), else it fits."""
import numpy as np

import constraint_ref as cref
from util import cluster

TAINT, SELECTOR, RESOURCES, CPU, MEM, PODS, FIT, NODES, COUNT = range(9)


def explain(req, free, labels=None, taints=None, require=None, tolerate=None):
    """req (P, 3), free (N, 3), uint64 words ([N], [N], [P], [P]; None: all
    zero) -> int32 (P, 8)."""
    req = np.asarray(req, np.int64).reshape(-1, 3)
    free = np.asarray(free, np.int64).reshape(-1, 3)
    P, N = req.shape[0], free.shape[0]

    def w(a, n):
        return np.zeros(n, np.uint64) if a is None else np.asarray(a, np.uint64).reshape(n)

    lab, tnt = w(labels, N)[None, :], w(taints, N)[None, :]
    rq, tl = w(require, P)[:, None], w(tolerate, P)[:, None]
    taint = (tnt & ~tl) != 0
    sel = ~taint & ((lab & rq) != rq)
    elig = ~taint & ~sel
    short = req[:, None, :] > free[None, :, :]  # (P, N, 3)
    res = elig & short.any(2)
    out = np.zeros((P, COUNT), np.int32)
    out[:, TAINT] = taint.sum(1)
    out[:, SELECTOR] = sel.sum(1)
    out[:, RESOURCES] = res.sum(1)
    for r, slot in enumerate((CPU, MEM, PODS)):
        out[:, slot] = (elig & short[:, :, r]).sum(1)
    out[:, FIT] = (elig & ~short.any(2)).sum(1)
    out[:, NODES] = N
    return out


def case(P, N, cap_scale=0.07, pat="mix"):
    """The shared test instance of shape (P, N): util.cluster, pod slots and
    pod-slot requests in 0..2 (so PODS is short somewhere and two resources are
    short together), constraint_ref's word pattern.
    -> (WA, L, free, req, (labels, taints, require, tolerate))."""
    rng = np.random.default_rng(P * 7 + N)
    WA, L, free, req = cluster(rng, P, N, cap_scale=cap_scale)
    free[:, 2] = rng.integers(0, 3, N)
    req[:, 2] = rng.integers(0, 3, P)
    return WA, L, free, req, cref.pattern(pat, rng, P, N)


def message(c):
    """The FailedScheduling line of one record (nas_host_explain_message)."""
    parts = [f"{c[s]}{t}" for s, t in ((TAINT, " node(s) had untolerated taint"),
                                        (SELECTOR, " node(s) didn't match Pod's node selector"),
                                        (CPU, " Insufficient cpu"), (MEM, " Insufficient memory"),
                                        (PODS, " Too many pods")) if c[s]]
    head = f"{c[FIT]}/{c[NODES]} nodes are available"
    return head + (": " + ", ".join(parts) if parts else "") + "."
