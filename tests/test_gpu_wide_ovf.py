"""Exact int32 traffic on the wide cost tile (k_cost.hip seed_ovf_staged): a
256 x 384 tile stages its pods' overflow entries -- (m, e) records and the
256-byte segments of their latency rows -- through LDS behind the first K
stage when no 384-pod tile of the upload holds more than OVF_STAGE_ENTRIES
of them; traffic with a fuller tile keeps the walk through global memory.
Every case must equal the oracle exactly: placements, integer scores and
remaining capacity through nas_place, or every checked pod's first candidate
and its cost through nas_score (one launch, tiles 384-aligned from pod 0)."""
import os
import re

import numpy as np
import pytest

import oracle
from kubernetesnetawarescheduler_amd import Engine
from util import cluster

pytestmark = pytest.mark.gpu

TILE = 384
_HDR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                    "kubernetesnetawarescheduler_amd", "csrc", "nas_internal.h")
with open(_HDR) as _f:
    CAP = int(re.search(r"constexpr\s+int\s+OVF_STAGE_ENTRIES\s*=\s*(\d+)\s*;", _f.read()).group(1))


def upload(e, WA, L, free, req):
    e.upload_latency(L, "i8")
    e.upload_capacity(free)
    e.upload_pods(req)
    e.upload_traffic(WA, "i8")  # int32: the host split builds plane + lists


def excess(rng, n):
    """n values outside the int8 plane, of either sign."""
    v = rng.integers(128, 100000, n)
    return np.where(rng.random(n) < 0.5, v, -v - 1).astype(np.int32)


def put(rng, WA, pod, k, nodes=None):
    """k entries on distinct nodes of one pod."""
    N = WA.shape[1]
    m = rng.choice(N if nodes is None else nodes, k, replace=False)
    WA[pod, m] = excess(rng, k)


def sparse(rng, WA, shares=(0.25, 0.04, 0.005), pods=None):
    """C3-like lists: `shares` of the pods hold 1, 2, 3 entries."""
    P = WA.shape[0]
    u = rng.random(P)
    lo = 0.0
    for k, sh in enumerate(shares, 1):
        sel = np.nonzero((u >= lo) & (u < lo + sh))[0]
        for p in sel if pods is None else np.intersect1d(sel, pods):
            put(rng, WA, p, k)
        lo += sh


def check_place(WA, L, free, req):
    with Engine(0) as e:
        upload(e, WA, L, free, req)
        node, _, ci = e.place()
        cap = e.get_capacity()
    want, wcost, wfree = oracle.place(WA, L, req, free, "i8")
    assert node.tolist() == want.tolist()
    assert ci.tolist() == wcost.tolist()
    assert (cap == wfree).all()


def check_first_candidates(keys, pods, WA, L, free, req):
    """keys[p, 0] is pod p's (cost, node)-smallest fitting node, with its cost."""
    cost = oracle.cost(WA[pods], L, "i8")
    fits = (req[pods][:, None, :].astype(np.int64) <= free[None, :, :].astype(np.int64)).all(2)
    assert fits.any(1).all()
    cost = np.where(fits, cost, np.iinfo(np.int64).max)
    best = cost.argmin(1)
    k0 = keys[pods, 0]
    got_node = (k0 & np.uint64(0xFFFFFFFF)).astype(np.int64)
    got_cost = (k0 >> np.uint64(32)).astype(np.int64) ^ 0x80000000
    got_cost = np.where(got_cost >= 2**31, got_cost - 2**32, got_cost)
    bad = np.nonzero((got_node != best) | (got_cost != cost[np.arange(len(pods)), best]))[0]
    assert len(bad) == 0, (len(bad), pods[bad[:8]].tolist())


def test_sparse_lists_every_tile_staged():
    """25% of the pods with one entry, 4% two, 0.5% three (~130 per tile),
    excess and latency of both signs."""
    P, N = 33100, 300
    rng = np.random.default_rng(21)
    WA8, L, free, req = cluster(rng, P, N, lo=-20, hi=60, cap_scale=0.6)
    WA = WA8.astype(np.int32)
    sparse(rng, WA)
    assert (L < 0).any()
    check_place(WA, L, free, req)


@pytest.mark.parametrize("fullest", ["cap", "3cap"])
def test_tiles_at_the_cap(fullest):
    """Tiles of 0, 1, CAP - 1, CAP (spread, and all on one pod) entries with
    empty tiles between them: the staged kernel up to its last slot; with
    tiles of CAP + 1, 3 CAP, CAP + 5 on one pod and one entry on every pod
    added, the same upload on the global walk."""
    P, N = 33000, 320
    assert CAP + 5 <= N and CAP <= TILE
    rng = np.random.default_rng(22)
    WA8, L, free, req = cluster(rng, P, N, lo=-20, hi=60, cap_scale=0.8)
    WA = WA8.astype(np.int32)

    def spread(t, k):  # k entries over tile t's pods, one pod after the other
        per = np.bincount(np.arange(k) % TILE, minlength=TILE)
        for i in np.nonzero(per)[0]:
            put(rng, WA, t * TILE + i, per[i])

    plan = {2: 1, 4: CAP - 1, 6: CAP}
    one_pod = {8: CAP}
    if fullest == "3cap":
        plan.update({10: CAP + 1, 12: 3 * CAP, 16: TILE})
        one_pod[14] = CAP + 5
    for t, k in plan.items():
        spread(t, k)
    for t, k in one_pod.items():
        put(rng, WA, t * TILE + 200, k)
    cnt = ((WA > 127) | (WA < -128)).sum(1)
    tiles = np.concatenate([cnt, np.zeros(-P % TILE, np.int64)]).reshape(-1, TILE).sum(1)
    for t, k in {**plan, **one_pod}.items():
        assert tiles[t] == k
    assert tiles.sum() == sum(plan.values()) + sum(one_pod.values())
    with Engine(0) as e:
        upload(e, WA, L, free, req)
        e.score()
        keys, _ = e.candidate_keys()
    pods = np.arange(0, 18 * TILE)
    check_first_candidates(keys, pods, WA, L, free, req)


@pytest.mark.parametrize("P", [33100, 33500])
def test_partial_last_tile(P):
    """The last tile is partial (its rows past the padded pod count, 128 or
    256 of them, belong to nobody); heavy lists on the last 10 real pods."""
    N = 300
    assert P % TILE and (-(-P // 256) * 256) % TILE in (128, 256)
    rng = np.random.default_rng(P)
    WA8, L, free, req = cluster(rng, P, N, lo=-20, hi=60, cap_scale=0.8)
    WA = WA8.astype(np.int32)
    sparse(rng, WA)
    for p in range(P - 10, P):
        put(rng, WA, p, 12)
    with Engine(0) as e:
        upload(e, WA, L, free, req)
        e.score()
        keys, _ = e.candidate_keys()
    check_first_candidates(keys, np.arange(P - 500, P), WA, L, free, req)


def test_entry_nodes_in_first_and_last_node_tile():
    """N = 600 is three node tiles, the last with 88 real nodes: the same
    entry node seeds a different row segment in each."""
    P, N = 33100, 600
    rng = np.random.default_rng(24)
    WA8, L, free, req = cluster(rng, P, N, lo=-20, hi=60, cap_scale=0.4)
    WA = WA8.astype(np.int32)
    edge = np.concatenate([np.arange(0, 10), np.arange(N - 10, N)])
    for p in np.nonzero(rng.random(P) < 0.3)[0]:
        put(rng, WA, p, int(rng.integers(1, 4)), nodes=edge)
    check_place(WA, L, free, req)


def test_batch_of_two_clusters():
    """B = 2: the wide tile scores each cluster's first 4,608 pods; cluster
    1's lists, latency and traffic differ from cluster 0's."""
    B, P, N = 2, 4700, 300
    rng = np.random.default_rng(25)
    cs = []
    for b in range(B):
        WA8, L, free, req = cluster(rng, P, N, lo=-20, hi=60, cap_scale=0.2)
        WA = WA8.astype(np.int32)
        sparse(rng, WA, shares=(0.25, 0.04, 0.005) if b == 0 else (0.1, 0.2, 0.02))
        cs.append((WA, L, free, req))
    with Engine(0) as e:
        e.set_batch(B)
        e.upload_latency(np.stack([c[1] for c in cs]), "i8")
        e.upload_capacity(np.stack([c[2] for c in cs]))
        e.upload_pods(np.stack([c[3] for c in cs]))
        e.upload_traffic(np.stack([c[0] for c in cs]), "i8")
        node, _, score = e.place()
        cap = e.get_capacity()
    for b, (WA, L, free, req) in enumerate(cs):
        want, wcost, wfree = oracle.place(WA, L, req, free, "i8")
        assert node[b].tolist() == want.tolist(), b
        assert score[b].tolist() == wcost.tolist(), b
        assert (cap[b] == wfree).all(), b


def test_repeat_pass_identical():
    """Two passes on one engine: nothing of a pass's LDS scratch or lists
    leaks into the next."""
    P, N = 33100, 257
    rng = np.random.default_rng(26)
    WA8, L, free, req = cluster(rng, P, N, lo=-20, hi=60, cap_scale=0.7)
    WA = WA8.astype(np.int32)
    sparse(rng, WA)
    with Engine(0) as e:
        upload(e, WA, L, free, req)
        n1, _, c1 = e.place()
        cap1 = e.get_capacity()
        e.reset_capacity()
        n2, _, c2 = e.place()
        cap2 = e.get_capacity()
    assert n1.tolist() == n2.tolist() and c1.tolist() == c2.tolist()
    assert (cap1 == cap2).all()
    want, wcost, wfree = oracle.place(WA, L, req, free, "i8")
    assert n1.tolist() == want.tolist() and c1.tolist() == wcost.tolist()
    assert (cap1 == wfree).all()
