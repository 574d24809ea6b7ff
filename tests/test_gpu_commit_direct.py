"""The commit kernels (k_commit.hip) on crafted candidate lists, kernel by
kernel: nas_set_candidate_keys + nas_commit feed each of launch_commit's five
variants the lists commit_cases.py builds -- herds wider than a window,
requests of every size class on shared nodes, roomy nodes past the bound,
halts and resumes at unaligned pods, exhausted zero-traffic lists -- at the
node and pod counts on both sides of every boundary, and compare placements,
scores, the stop pod and the capacity exactly with util.commit_ref (pinned to
the oracle by test_commit_ref_cpu.py).  Nothing is scored: L is all zero and
only its size matters, the traffic only tells zero-traffic pods (an empty
row) from ordinary ones (one peer)."""
import numpy as np
import pytest

import commit_cases as cc
from kubernetesnetawarescheduler_amd import Engine
from util import KEY_INVALID, commit_ref

pytestmark = pytest.mark.gpu

SENT_NODE, SENT_SCORE = -77, -(2**40)  # what the commit must leave outside [p_begin, stop)


@pytest.fixture(scope="module")
def engine_for():
    """One context of this module's own with an all-zero latency matrix of N
    nodes, uploaded again only when N changes (the shapes below keep equal N
    together)."""
    have = [None]
    with Engine(0) as e:
        def get(N):
            if have[0] != N:
                e.upload_latency(np.zeros((N, N), np.int8), "i8")
                have[0] = N
            return e

        yield get


def upload(e, case, N):
    zero = case["zero"]
    row_ptr = np.concatenate([[0], np.cumsum(~zero)]).astype(np.int32)
    nnz = int(row_ptr[-1])
    e.upload_capacity(case["free"])
    e.upload_pods(case["req"])
    e.upload_traffic_csr(row_ptr, np.zeros(nnz, np.int32), np.ones(nnz, np.int8), "i8", N)


def run_case(e, case, N):
    """Walk the whole case: commit, compare with commit_ref, and at every
    halt write the pod's fresh list and resume from it.  A halt is accepted
    at the pods the case names, and -- the one exception -- at a zero-traffic
    pod whose first fitting node lies further than ZSCAN_LDS above its
    bound's node; anything else the reference does not do is a failure.
    Returns (halts, of them early ones, [(p_begin, stop, rounds)])."""
    upload(e, case, N)
    keys, bounds = case["keys"].copy(), case["bounds"].copy()
    req, zero = case["req"], case["zero"]
    P = len(bounds)
    e.set_candidate_keys(0, keys, bounds)
    gk, gb = e.candidate_keys_range(0, P)
    assert gk.tobytes() == keys.tobytes() and gb.tobytes() == bounds.tobytes()
    gk, gb = e.candidate_keys_range(P - 3, 3)
    assert gk.tobytes() == keys[P - 3:].tobytes() and gb.tobytes() == bounds[P - 3:].tobytes()
    node = np.full(P, SENT_NODE, np.int32)
    score = np.full(P, SENT_SCORE, np.int64)
    p, cur, halts, early, walks = 0, case["free"].astype(np.int64), [], [], []
    while True:
        rnode, rscore, rfree, rstop, rdist = commit_ref(keys, bounds, req, cur, zero, p, True)
        done_node, done_score = node[:p].copy(), score[:p].copy()
        stop = e.commit(p, node, score)
        walks.append((p, stop, e.timings()["commit_rounds"]))
        fresh = case["fixups"].get(stop)
        if stop != rstop:
            assert p <= stop < rstop and rdist[stop] > cc.ZSCAN_LDS, (p, stop, rstop)
            early.append(stop)
            took = rnode[p:stop] >= 0
            rfree = cur.copy()
            np.subtract.at(rfree, rnode[p:stop][took], req[p:stop][took].astype(np.int64))
            fresh = (np.full(cc.KC, KEY_INVALID, np.uint64), KEY_INVALID)
            fresh[0][0] = cc.zkey(rnode[stop])  # the placement the reference gives
        assert node[p:stop].tolist() == rnode[p:stop].tolist(), (p, stop)
        assert score[p:stop].tolist() == rscore[p:stop].tolist(), (p, stop)
        assert (node[:p] == done_node).all() and (score[:p] == done_score).all()
        assert (node[stop:] == SENT_NODE).all() and (score[stop:] == SENT_SCORE).all()
        assert (e.get_capacity() == rfree).all(), (p, stop)
        if stop == P:
            break
        assert fresh is not None, ("halt at a pod that must not halt", stop)
        halts.append(stop)
        keys[stop], bounds[stop] = fresh
        e.set_candidate_keys(stop, keys[stop:stop + 1], bounds[stop:stop + 1])
        lo = max(0, stop - 1)  # the write touched that pod's list alone
        gk, gb = e.candidate_keys_range(lo, min(3, P - lo))
        assert gk.tobytes() == keys[lo:lo + 3].tobytes() and gb.tobytes() == bounds[lo:lo + 3].tobytes()
        p, cur = stop, rfree
    # nothing left to walk: P comes back and nothing is written
    node[:], score[:] = SENT_NODE, SENT_SCORE
    assert e.commit(P, node, score) == P
    assert (node == SENT_NODE).all() and (score == SENT_SCORE).all()
    assert (e.get_capacity() == rfree).all()
    return halts, early, walks


@pytest.mark.parametrize("N,P", sorted(cc.SHAPES))
def test_commit_direct(engine_for, N, P):
    """Generators (a) herd, (b) mixed requests, (c) stops and resumes on the
    kernel launch_commit picks for (N, P): (300, 1500) and (8656, 700)
    k_commit_w<true,true>; (8657, 700) and (11541, 700) k_commit_w<true,false>;
    (11542, 700) k_commit_w<false>; (300, 16384) the last one-wave pod count;
    (300, 16385) k_commit<true>; (11542, 16385) k_commit<false>."""
    e = engine_for(N)
    W = cc.window(P)
    for name in ("herd", "mixed", "stops"):
        case = cc.make(name, N, P)
        halts, early, walks = run_case(e, case, N)
        assert halts == sorted(case["fixups"]) and not early, name
        if name == "herd":
            # conflicts really happened: a window without one takes one round
            p0, stop, rounds = walks[0]
            print(f"{cc.variant(N, P)} herd: {rounds} rounds over {stop // W + 1} windows")
            assert p0 == 0 and stop < P and rounds > stop // W + 1
        if name == "stops":
            assert halts == cc.halting_pods(P)


@pytest.mark.parametrize("N,P", sorted(cc.ZSCAN_SHAPES))
def test_zero_traffic_scan(engine_for, N, P):
    """Exhausted zero-traffic lists (commit_cases.zscan): placed 1..16 nodes
    above the bound's node, -1 when nothing fits up to N - 1, ordinary pods
    with the same lists halt, contenders move on to the next fitting node.
    Only a first fit further than 1,024 nodes above may halt instead
    (run_case); with the capacity in LDS a fit up to 1,024 above must place."""
    case = cc.make("zscan", N, P)
    rows = cc.zscan_rows(case)
    lds = N <= cc.LDS_CAP_MAX_NODES
    assert rows["near"] >= 8 and rows["none_near_end"] >= 4 and rows["bound_is_last"] == 2
    assert rows["last_node"] == 1 and rows["ordinary_halts"] == 3 and rows["contended"] == 4
    assert rows["mid"] == (2 if lds else 0) and rows["far"] == (2 if N >= 8657 else 0)
    assert rows["at_lds_limit"] == (1 if lds and N >= 8657 else 0)
    halts, early, _ = run_case(engine_for(N), case, N)
    print(f"{cc.variant(N, P)} zscan: halts {halts}, of them beyond the scan limit {early}")
    assert sorted(set(halts) - set(early)) == sorted(case["fixups"])
    assert len(early) <= rows["far"]
