"""Reference for nas_preempt (include/nas.h): the steps of the header's text as
plain Python loops over Python ints, and the seeded generator the CPU and GPU
tests share.

For list entry (pod requests r, priority pi) and node n with free capacity f:
n must be eligible; `lower` is n's bound pods with priority < pi in index order
(priority descending, then bound index ascending); avail = f + sum of lower's
requests must hold r; walking lower, a pod that avail - req still holds r
without stays (avail -= req), the others are victims.  The node's key is
(top victim priority, priority sum, victim count, n), a node without victims
before every node with some; the smallest key wins."""
import numpy as np

import constraint_ref as cref
from util import cluster

EMPTY = -1
DTYPE = np.dtype([("node", "<i4"), ("n_victims", "<i4"), ("top_priority", "<i4"),
                  ("candidates", "<i4"), ("priority_sum", "<i8")])
BIAS = 2**31
I32_MIN = -2**31


def node_lists(N, bound):
    """bound = (node [B], priority [B], req (B, 3)) or None -> per node the
    bound indices in walk order."""
    lists = [[] for _ in range(N)]
    if bound is not None:
        node, prio = [np.asarray(a).reshape(-1).tolist() for a in bound[:2]]
        for b in sorted(range(len(node)), key=lambda b: (node[b], -prio[b], b)):
            lists[node[b]].append(b)
    return lists


def answer_node(r, pi, f, lst, bprio, breq):
    """One node for one pod -> None (not a candidate) or (key, victims):
    key = (0, 0, 0) without victims, else (1 + top + 2^31, sum, count)."""
    lower = [b for b in lst if bprio[b] < pi]
    avail = [f[k] + sum(breq[b][k] for b in lower) for k in range(3)]
    if any(r[k] > avail[k] for k in range(3)):
        return None
    victims = []
    for b in lower:
        if all(avail[k] - breq[b][k] >= r[k] for k in range(3)):
            avail = [avail[k] - breq[b][k] for k in range(3)]
        else:
            victims.append(b)
    if not victims:
        return (0, 0, 0), victims
    top = max(bprio[b] for b in victims)
    return (1 + top + BIAS, sum(bprio[b] + BIAS for b in victims), len(victims)), victims


def preempt(req, prio, free, bound=None, elig=None, max_victims=0, detail=False):
    """req (n, 3) and prio [n] of the listed pods, free (N, 3), bound as in
    node_lists, elig (n, N) bool or None -> (records [n] of DTYPE, victims
    (n, max_victims) int32, -1 past the victims).  detail=True also returns per
    entry the sorted (key, node, victims) of every candidate node."""
    req = np.asarray(req, np.int64).reshape(-1, 3).tolist()
    prio = np.asarray(prio, np.int64).reshape(-1).tolist()
    free = np.asarray(free, np.int64).reshape(-1, 3).tolist()
    N = len(free)
    lists = node_lists(N, bound)
    bprio = [] if bound is None else np.asarray(bound[1], np.int64).reshape(-1).tolist()
    breq = [] if bound is None else np.asarray(bound[2], np.int64).reshape(-1, 3).tolist()
    rec = np.zeros(len(req), DTYPE)
    vict = np.full((len(req), max_victims), -1, np.int32)
    details = []
    for i, (r, pi) in enumerate(zip(req, prio)):
        cands = []
        for n in range(N):
            if elig is not None and not elig[i][n]:
                continue
            a = answer_node(r, pi, free[n], lists[n], bprio, breq)
            if a is not None:
                cands.append((a[0], n, a[1]))
        cands.sort(key=lambda c: (c[0], c[1]))
        details.append(cands)
        if not cands:
            rec[i] = (EMPTY, 0, 0, 0, 0)
            continue
        (k0, psum, nv), n, victims = cands[0]
        rec[i] = (n, nv, k0 - 1 - BIAS if nv else 0, len(cands), psum)
        m = min(nv, max_victims)
        vict[i, :m] = victims[:m]
    return (rec, vict, details) if detail else (rec, vict)


# ---- the ladder of step 5, shared by the CPU and GPU tests
def ladder_cases():
    """name -> (bound on two nodes, the winner's record fields without the node
    and candidates): node A is better than node B at exactly one level."""
    u = (100, 0, 0)
    return {
        # top priority: A evicts {5}, B evicts {6}
        "top": (([5], [u]), ([6], [u]), (1, 5, 5 + BIAS)),
        # sum: A evicts {5, 1}, B evicts {5, 2}
        "sum": (([5, 1], [u, u]), ([5, 2], [u, u]), (2, 5, 6 + 2 * BIAS)),
        # count: A evicts {5}, B evicts {5, INT32_MIN}: equal top, equal sum
        "count": (([5], [(200, 0, 0)]), ([5, I32_MIN], [u, u]), (1, 5, 5 + BIAS)),
        # index: the same victims on both
        "index": (([5], [u]), ([5], [u]), (1, 5, 5 + BIAS)),
    }


def ladder_bound(A, B, swap):
    """A's pods on node `swap`, B's on the other; A = (priorities, requests)."""
    na, nb = (1, 0) if swap else (0, 1)
    node = [na] * len(A[0]) + [nb] * len(B[0])
    return node, list(A[0]) + list(B[0]), list(A[1]) + list(B[1])



PROFILES = ("tight", "roomy")
LONG_ROW = 70  # one node's bound pods: longer than a wave


def case(P, N, profile="tight", pat=None):
    """The shared instance of shape (P, N), seeded by default_rng(P * 7 + N):
    -> dict with WA, L (int8, for the uploads), free (N, 3), req (P, 3), prio
    [P], bound = (node, priority, req) shuffled, and words (constraint_ref's
    pattern `pat`) or None."""
    if profile not in PROFILES:
        raise ValueError(profile)
    rng = np.random.default_rng(P * 7 + N)
    tight = profile == "tight"
    unit = np.array([100, 1000, 1])
    # (this order of draws reaches every feature test_preempt_cpu.py pins)
    per = rng.integers(0, 7, N)
    per[N - 1] = LONG_ROW
    bnode = np.repeat(np.arange(N), per).astype(np.int32)
    B = len(bnode)
    bprio = rng.integers(-3, 40, B) if tight else rng.choice([-5, 0, 0, 10, 10, 100, 1000], B)
    breq = np.stack([rng.integers(1, 4, B), rng.integers(1, 4, B), rng.integers(0, 2, B)], 1)
    order = rng.permutation(B)
    bound = (bnode[order], bprio[order].astype(np.int32), (breq * unit)[order].astype(np.int32))
    if tight:
        req = np.stack([rng.integers(2, 9, P), rng.integers(1, 9, P), rng.integers(0, 3, P)], 1)
        prio = rng.choice([-3, 5, 20, 50], P)
        free = np.stack([rng.integers(0, 2, N), rng.integers(0, 4, N), rng.integers(0, 2, N)], 1)
    else:
        req = np.stack([rng.integers(1, 8, P), rng.integers(1, 8, P), rng.integers(0, 3, P)], 1)
        prio = rng.choice([-5, 0, 10, 100, 2000], P)
        free = np.stack([rng.integers(0, 4, N), rng.integers(0, 4, N), rng.integers(0, 3, N)], 1)
    WA, L, _, _ = cluster(rng, P, N)
    words = None if pat is None else cref.pattern(pat, rng, P, N)
    return dict(WA=WA, L=L, free=(free * unit).astype(np.int32), req=(req * unit).astype(np.int32),
                prio=prio.astype(np.int32), bound=bound, words=words)


def elig_of(words):
    return None if words is None else cref.eligible(*words)
