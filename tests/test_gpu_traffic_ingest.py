"""Traffic ingestion through the C ABI: what csrc/traffic_ingest.h promises
(tests/sanitize/traffic_ingest_driver.cpp pins it on the CPU) as the library
delivers it.  Uploaded CSR / dense integer traffic reads back as the exact
dense sums and places like the oracle on the unclipped traffic; fp32 CSR
traffic reads back as float32(float64 sum) bit for bit; what is refused is
refused with its code.

P = 700, N = 130: P % 256 != 0, so padding rows exist behind the pods, and the
768 padded rows hold more than one 384-row window of overflow entries.
"""
import functools

import numpy as np
import pytest

import oracle
from kubernetesnetawarescheduler_amd import Engine, NasError, _lib
from util import cluster

pytestmark = pytest.mark.gpu

P, N = 700, 130
I32_MAX, I32_MIN = 2**31 - 1, -2**31

# (node, weight) peers of the first pods: sums at the edges of the int8 plane ...
PLANTED = [
    [(0, 100), (1, 127), (0, 27), (1, 1), (2, -100), (3, -100), (2, -28), (3, -29)],  # 127 128 -128 -129
    [(7, 127), (7, 127), (7, 127), (9, -128), (9, -128)],  # int8 weights whose sums leave int8
    [(4, 50), (6, 9), (4, -50)],                           # a pair that cancels to 0
    [(-1, 90), (N, 90), (N - 1, 120), (N - 1, 80)],        # skipped peers beside node N - 1
    [(5, 100), (1, 5), (5, 100), (0, -7), (5, 100)],       # non-adjacent duplicates of one node
    [],                                                    # an empty row
]
# ... and of int32 itself (int32 weights only; no latency but zero can score them)
LIMITS = [
    [(8, I32_MAX - 5), (3, 11), (8, 5)],
    [(2, I32_MIN + 5), (2, -5)],
]


def csr_of(rows, wdtype=np.int64):
    deg = [len(r) for r in rows]
    row_ptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    peer = np.array([m for r in rows for m, _ in r], np.int32)
    w = np.array([x for r in rows for _, x in r], wdtype)
    return row_ptr, peer, w


def random_rows(rng, count, draw):
    """Pods with 0..12 peers on a few nodes (several peers per node), about one
    peer in ten unbound or off the cluster."""
    rows = []
    for p in range(count):
        home = int(rng.integers(0, N - 6))
        r = []
        for _ in range(int(rng.integers(0, 13))):
            u = rng.random()
            m = -1 if u < 0.05 else N + int(rng.integers(0, 3)) if u < 0.1 else home + int(rng.integers(0, 6))
            r.append((m, draw(p)))
        rows.append(r)
    return rows


def dense_sum(row_ptr, peer, w, dtype):
    """The dense reference: every in-range peer's weight added to its (pod, node)."""
    D = np.zeros((len(row_ptr) - 1, N), dtype)
    pod = np.repeat(np.arange(len(row_ptr) - 1), np.diff(row_ptr))
    ok = (peer >= 0) & (peer < N)
    np.add.at(D, (pod[ok], peer[ok]), w[ok].astype(dtype))
    return D, pod[ok], peer[ok]


@functools.lru_cache(maxsize=None)
def int_case(kind, limits):
    """-> (row_ptr, peer, weights, dense int64 reference) of one integer case."""
    rng = np.random.default_rng(700130)
    if kind == "i8":
        def draw(p):
            return int(rng.integers(-128, 128))
        wt = np.int8
    else:
        def draw(p):  # the later pods' peers are mostly beyond int8: the windows differ
            big = rng.random() < (0.6 if p >= 384 else 0.1)
            return int(rng.integers(-50000, 50001)) if big else int(rng.integers(-300, 301))
        wt = np.int32
    planted = PLANTED + (LIMITS if limits else [])
    row_ptr, peer, w = csr_of(planted + random_rows(rng, P - len(planted), draw))
    D, _, _ = dense_sum(row_ptr, peer, w, np.int64)
    assert D.min() >= I32_MIN and D.max() <= I32_MAX
    assert (np.abs(D) > 127).sum() > (300 if kind != "i8" else 30)  # overflow entries in number
    w = w.astype(wt)
    for a in (row_ptr, peer, w, D):
        a.setflags(write=False)
    return row_ptr, peer, w, D


@functools.lru_cache(maxsize=None)
def instance():
    _, L, free, req = cluster(np.random.default_rng(130700), P, N, lo=-60, hi=100, cap_scale=0.1)
    return L, free, req


CASES = ["csr_i8", "csr_i32", "dense_i32"]


def upload_int(e, case, limits, L):
    row_ptr, peer, w, D = int_case("i8" if case == "csr_i8" else "i32", limits)
    _, free, req = instance()
    e.upload_latency(L, "i8")
    e.upload_capacity(free)
    e.upload_pods(req)
    if case == "dense_i32":
        e.upload_traffic(D.astype(np.int32), "i8")
    else:
        e.upload_traffic_csr(row_ptr, peer, w, "i8", N)
    return D


@pytest.mark.parametrize("case", CASES)
def test_integer_traffic_reads_back_and_places_exactly(engine, case):
    L, free, req = instance()
    D = upload_int(engine, case, False, L)
    rows, _, _, _ = engine.read_inputs(0, P, want_L=False)
    assert rows.dtype == np.int32 and (rows == D).all()
    assert D[0, :4].tolist() == [127, 128, -128, -129] and D[1, 7] == 381 and D[2, 4] == 0
    node, _, ci = engine.place()
    want, wcost, wfree = oracle.place(D, L, req, free, "i8")
    assert node.tolist() == want.tolist()
    assert ci.tolist() == wcost.tolist()
    assert (engine.get_capacity() == wfree).all()
    assert (want >= 0).sum() > P // 4 and (want < 0).any()  # the pass fills the cluster


@pytest.mark.parametrize("case", CASES[1:])
def test_int32_limits_read_back(engine, case):
    """Sums of exactly INT32_MAX and INT32_MIN are taken and read back.  (Under
    an all-zero latency: against any other, costs of such traffic leave int32
    and the engine refuses the inputs, test_gpu_exact_traffic.py.)"""
    D = upload_int(engine, case, True, np.zeros((N, N), np.int8))
    assert D[len(PLANTED), 8] == I32_MAX and D[len(PLANTED) + 1, 2] == I32_MIN
    rows, _, _, _ = engine.read_inputs(0, P, want_L=False)
    assert (rows == D).all()
    # a window of rows away from row 0: the lists' base offset
    rows, _, _, _ = engine.read_inputs(389, 300, want_L=False)
    assert (rows == D[389:689]).all()


def test_csr_f32_is_the_double_sum_rounded_once(engine):
    rng = np.random.default_rng(4)
    planted = [
        [(3, 1e8), (3, 1.0), (3, -1e8)],              # sequential float summation gives 0
        [(4, 2.5), (-1, 9.0), (4, -2.5), (N, 9.0)],   # a cancelling pair: 0.0
        [],
    ]
    # multiples of 1/8 below 2^17: every float64 sum is exact, in any order
    row_ptr, peer, w = csr_of(planted + random_rows(
        rng, P - len(planted), lambda p: float(rng.integers(-2**20, 2**20)) / 8), np.float32)
    D, _, _ = dense_sum(row_ptr, peer, w, np.float64)
    want = D.astype(np.float32)
    assert want[0, 3] == 1.0 and want[1, 4] == 0.0
    u = rng.uniform(50.0, 500.0, (N, N))
    L = (np.triu(u, 1) + np.triu(u, 1).T).astype(np.float32)
    _, free, req = instance()
    engine.upload_latency(L, "f32")
    engine.upload_capacity(free)
    engine.upload_pods(req)
    engine.upload_traffic_csr(row_ptr, peer, w, "f32", N)
    rows, _, _, _ = engine.read_inputs(0, P, want_L=False)
    assert rows.dtype == np.float32
    assert (rows.view(np.uint32) == want.view(np.uint32)).all()


def error_of(call):
    with pytest.raises(NasError) as ei:
        call()
    return ei.value


def code_of(call):
    return error_of(call).code


def test_refused_uploads(engine):
    L, free, req = instance()
    row_ptr, peer, w, _ = int_case("i32", False)
    # an aggregate beyond int32: refused, and the context is left without traffic
    for pair in ([I32_MAX, 1], [I32_MIN, -1]):
        upload_int(engine, "csr_i32", False, L)
        rp, pn, ww = csr_of([[(9, 3)], [(5, pair[0]), (4, 7), (5, pair[1])]] + [[]] * (P - 2), np.int32)
        err = error_of(lambda: engine.upload_traffic_csr(rp, pn, ww, "i8", N))
        assert err.code == _lib.NAS_ERR_UNSUPPORTED and "pod 1 to node 5 exceeds int32" in str(err)
        assert code_of(engine.place) == _lib.NAS_ERR_STATE
    # row offsets that do not describe the arrays
    dip = row_ptr.copy()
    dip[300] = dip[301] + 1
    assert code_of(lambda: engine.upload_traffic_csr(dip, peer, w, "i8", N)) == _lib.NAS_ERR_ARG
    short = row_ptr.copy()
    short[P] -= 1
    assert code_of(lambda: engine.upload_traffic_csr(short, peer, w, "i8", N)) == _lib.NAS_ERR_ARG
    with Engine(0) as e:  # CSR traffic on a cluster batch
        e.set_batch(2)
        assert code_of(lambda: e.upload_traffic_csr(row_ptr, peer, w, "i8", N)) == _lib.NAS_ERR_UNSUPPORTED
