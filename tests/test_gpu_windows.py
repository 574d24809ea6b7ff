"""Host-driven scoring windows (nas_score_range) list by list against the
reference of window_cases.py, through Engine only.

Every context first runs one real pass (score_range + commit, rescoring at the
stops), so that the working capacity differs from the uploaded one; it must
then equal the oracle's remaining capacity.  Every window [lo, hi) after that
follows one procedure (run_window): read the working capacity, write a
distinct sentinel list into every pod's slot, score the window, read all P
lists back, and judge them with window_cases.check_window against the
reference built from the capacity read -- sentinels untouched outside, and
inside the rules of csrc/klist.h per pod -- and the working capacity must be
what it was.  Once per context a commit starts right after a window [lo, P)
with sentinels below lo and must equal util.commit_ref on the lists read back.

tests/test_window_cases_cpu.py pins the reference to the oracle, holds the
cases to the list classes they must show and to the boundaries of the launch
forms, and shows that check_window catches each fault."""
import numpy as np
import pytest

import window_cases as wc
from kubernetesnetawarescheduler_amd import Engine, LocalGroup, local_ranks
from util import KEY_INVALID, commit_ref, merge_lists

pytestmark = pytest.mark.gpu

RESCORE_PODS = 1024


@pytest.fixture(scope="module")
def own_engine():
    """An Engine of this module's own (constraints are context state)."""
    with Engine(0) as e:
        yield e


@pytest.fixture
def eng(own_engine):
    own_engine.clear_constraints()
    yield own_engine
    own_engine.clear_constraints()


def upload(e, c):
    e.upload_latency(c["L"], c["dtype"])
    e.upload_capacity(c["free"])
    e.upload_pods(c["req"])
    e.upload_traffic(c["WA"], c["dtype"])  # (int32 traffic: the exact path of int8 scoring)
    if c["words"] is not None:
        lab, tnt, rq, tl = c["words"]
        e.upload_node_constraints(lab, tnt)
        e.upload_pod_constraints(rq, tl)


def first_pass(engines, c):
    """The loop of include/nas.h over the first `prefix` pods (the others get
    empty complete lists: unplaced), lists merged on the host between shards.
    Every context must end on the oracle's remaining capacity, which differs
    from the uploaded one.  -> the number of stops."""
    P, K = c["P"], c["prefix"]
    if K < P:
        for e in engines:
            e.set_candidate_keys(0, np.full((P, wc.KC), KEY_INVALID), np.full(P, KEY_INVALID))
    node = [np.full(P, -9, np.int32) for _ in engines]

    def sync(lo, hi):
        parts = []
        for e in engines:
            e.score_range(lo, hi)
            parts.append(e.candidate_keys_range(lo, hi - lo))
        if len(engines) > 1:
            mk, mb = merge_lists(parts)
            for e in engines:
                e.set_candidate_keys(lo, mk, mb)

    sync(0, K)
    stop, stops = 0, 0
    while True:
        at = {e.commit(stop, nd) for e, nd in zip(engines, node)}
        assert len(at) == 1, at
        stop = at.pop()
        if stop >= P:
            break
        assert stop < K
        stops += 1
        sync(stop, min(K, stop + RESCORE_PODS))
    left = wc.remaining(c)
    assert (left != c["free"]).any()
    for e in engines:
        assert (e.get_capacity() == left).all()
    return stops


def run_window(e, c, lo, hi, sk, sb, n0=0, n1=None):
    """One window by the procedure above.  -> (keys, bounds) of all P pods."""
    cap = e.get_capacity()
    e.set_candidate_keys(0, sk, sb)
    e.score_range(lo, hi)
    keys, bounds = e.candidate_keys()
    ref = wc.window_ref(c, lo, hi, cap, n0, n1)
    try:
        wc.check_window(keys, bounds, sk, sb, lo, hi, ref)
    except AssertionError as ex:
        raise AssertionError(f"{c['name']} window ({lo}, {hi}) columns [{n0}, {n1}): {ex}") from None
    assert (e.get_capacity() == cap).all(), "a window changed the working capacity"
    return keys, bounds


def commit_from_window(e, c, lo, sk, sb, n0=0, n1=None):
    """Window [lo, P) over sentinels, then commit(lo): equals commit_ref on
    the lists read back (the sentinels below lo are not the commit's to read)."""
    P = c["P"]
    cap = e.get_capacity()
    keys, bounds = run_window(e, c, lo, P, sk, sb, n0, n1)
    node = np.full(P, -3, np.int32)
    score = np.zeros(P, np.int64)
    stop = e.commit(lo, node, score)
    wnode, wscore, wfree, wstop = commit_ref(keys, bounds, c["req"], cap, wc.zero_rows(c), lo)
    assert stop == wstop, (c["name"], stop, wstop)
    assert node[lo:stop].tolist() == wnode[lo:stop].tolist()
    assert (node[:lo] == -3).all() and (node[stop:] == -3).all()
    if c["dtype"] == "i8":
        assert score[lo:stop].tolist() == wscore[lo:stop].tolist()
    assert (e.get_capacity() == wfree).all()
    assert (node[lo:stop] >= 0).any()


# ------------------------------------------- A. fused 256 x 256 tile, world 1
@pytest.mark.parametrize("name", wc.A_NAMES)
def test_fused_tile_windows(eng, name):
    c = wc.make(name)
    upload(eng, c)
    first_pass([eng], c)
    sk, sb = wc.sentinels(c["P"], c["N"])
    for lo, hi in c["windows"]:
        assert wc.launch_form(c["P"], lo, hi)[0] is False
        run_window(eng, c, lo, hi, sk, sb)
    commit_from_window(eng, c, 511, sk, sb)


# ------------------------------------------------------ B. wide tile, world 1
@pytest.mark.parametrize("name", wc.B_NAMES)
def test_wide_tile_windows(eng, name):
    """32,600 pods (32,768 padded): every window runs the 256 x 384 tile, from
    each start class modulo 384 and with each overshoot past the window's
    rounded end -- into the next pods' rows or the padding behind the traffic
    (with exact traffic: entries on those rows, staged through LDS in B-i32,
    walked in global memory in B-i32g)."""
    c = wc.make(name)
    upload(eng, c)
    first_pass([eng], c)
    sk, sb = wc.sentinels(c["P"], c["N"])
    for lo, hi in c["windows"]:
        assert wc.launch_form(c["P"], lo, hi)[0] is True
        run_window(eng, c, lo, hi, sk, sb)
    commit_from_window(eng, c, 32200, sk, sb)


# ------------------------------------- C. node shards without a communicator
def shard_contexts(c, G, windows, commit_lo):
    """G set_shard contexts on c's inputs: the pass with a host merge, every
    window on every rank against the reference of its own columns, the ranks'
    window lists merged against the unsharded reference, and a commit from a
    window on every rank's own lists."""
    P, N = c["P"], c["N"]
    engines = [Engine(0) for _ in range(G)]
    try:
        for r, e in enumerate(engines):
            e.set_shard(r, G)
            upload(e, c)
        first_pass(engines, c)
        sk, sb = wc.sentinels(P, N)
        for lo, hi in windows:
            parts = []
            for r, e in enumerate(engines):
                keys, bounds = run_window(e, c, lo, hi, sk, sb, *wc.shard_cols(N, r, G))
                parts.append((keys[lo:hi], bounds[lo:hi]))
            keys, bounds = sk.copy(), sb.copy()
            keys[lo:hi], bounds[lo:hi] = merge_lists(parts)
            wc.check_window(keys, bounds, sk, sb, lo, hi,
                            wc.window_ref(c, lo, hi, engines[0].get_capacity()))
        for r, e in enumerate(engines):
            commit_from_window(e, c, commit_lo, sk, sb, *wc.shard_cols(N, r, G))
    finally:
        for e in engines:
            e.close()


@pytest.mark.parametrize("G", wc.SHARD_WORLDS)
@pytest.mark.parametrize("name", wc.C_NAMES)
def test_shard_windows(name, G):
    """The wide tile at a small size (any set_shard context runs it): lists
    hold local nodes only."""
    c = wc.make(name)
    assert all(wc.launch_form(c["P"], lo, hi, shard=True)[0] for lo, hi in c["windows"])
    shard_contexts(c, G, c["windows"], 640)


# ------------------------------------------------------------- D. constrained
@pytest.mark.parametrize("name", wc.D_NAMES)
def test_constrained_windows(eng, name):
    """k_fit2_c (even p_lo) and k_fit_c (odd p_lo) write the mask, the
    mask-reading 256 x 256 tile follows either."""
    c = wc.make(name)
    assert not wc.zero_rows(c).any()
    upload(eng, c)
    first_pass([eng], c)
    sk, sb = wc.sentinels(c["P"], c["N"])
    for lo, hi in c["windows"]:
        run_window(eng, c, lo, hi, sk, sb)
    commit_from_window(eng, c, 1025, sk, sb)


@pytest.mark.parametrize("name", wc.D_NAMES)
def test_constrained_shard_windows(name):
    """Constraints on node shards: the mask path instead of the wide tile,
    from an odd and an even p_lo."""
    c = wc.make(name)
    shard_contexts(c, wc.D_SHARD_WORLD, wc.D_SHARD_WINDOWS, 1025)


# ------------------------------------------------ E. one in-process local group
@pytest.mark.parametrize("name", wc.C_NAMES)
def test_local_group_windows(name):
    """Two exchanging ranks of one process, each on its own thread: the
    window's lists travel in a send buffer indexed from the rounded-down start
    (0 for the window (255, 513), 256 for (300, 513)) and the cross-rank merge
    writes them back at an offset.  Both ranks' lists
    must be the merged (whole-cluster) reference, the sentinels intact."""
    c = wc.make(name)
    P, N = c["P"], c["N"]
    sk, sb = wc.sentinels(P, N)
    wc.remaining(c)  # (cached before the threads start)
    group = LocalGroup(2)
    engines = [Engine(0) for _ in range(2)]
    try:
        def run(r, e):
            e.set_option("COMM_TIMEOUT_MS", 60000)
            e.comm_init_local(group, r)
            upload(e, c)
            first_pass([e], c)
            for lo, hi in wc.E_WINDOWS:
                run_window(e, c, lo, hi, sk, sb)
            commit_from_window(e, c, 300, sk, sb)
            return True
        assert local_ranks(engines, run) == [True, True]
    finally:
        for e in engines:
            e.close()
        group.close()
