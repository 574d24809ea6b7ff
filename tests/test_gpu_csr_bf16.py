"""k_csr_bf16 (k_misc.hip): bf16 CSR traffic aggregated on the device -- per
(pod, node) the peers' weights summed in fp32, rounded once to bf16 (nearest
even), peers that are unbound (-1) or off the cluster (>= N) skipped.  The
case of float_cases.csr_bf16_case makes every fp32 sum exact, so the rows read
back must equal the reference bit for bit: planted ties in both directions and
a carry, non-adjacent duplicates, cancelling pairs, a whole row that cancels,
one pod with ~300 peers, node N - 1 next to the skipped N.  Then the placement
on those rows against the oracle on the dense reference, and an empty CSR
(bf16 and fp32), which must place first-fit with every cost 0."""
import numpy as np
import pytest

import float_cases as fc
import oracle
from util import bf16_bits_to_f64, cluster, f32_to_bf16_bits

pytestmark = pytest.mark.gpu
P, N = 777, 130


@pytest.fixture(scope="module")
def case():
    rng = np.random.default_rng(2)
    row_ptr, peer, w, planted = fc.csr_bf16_case(rng, P, N)
    ref = fc.csr_bf16_reference(row_ptr, peer, w, N)
    _, _, free, req = cluster(rng, P, N, cap_scale=0.06)
    # integer-valued latency of both signs: with traffic in multiples of 2^-8
    # below 2^10 every product and partial sum is exact in fp32
    L = f32_to_bf16_bits(rng.integers(-20, 21, (N, N)).astype(np.float32))
    assert (np.abs(bf16_bits_to_f64(ref)) @ np.abs(bf16_bits_to_f64(L))).max() < 2 ** 16
    return row_ptr, peer, w, planted, ref, L, free, req


def test_csr_bf16_rows_bit_exact(engine, case):
    row_ptr, peer, w, planted, ref, L, free, req = case
    engine.upload_latency(L, "bf16")
    engine.upload_capacity(free)
    engine.upload_pods(req)
    engine.upload_traffic_csr(row_ptr, peer, w, "bf16", N)
    rows, _, _, _ = engine.read_inputs(0, P, want_L=False)
    assert rows.dtype == np.uint16 and rows.shape == (P, N)
    for (p, m), v in planted.items():  # first, so a failure names the case
        assert bf16_bits_to_f64(rows[p, m]) == v, (p, m, bf16_bits_to_f64(rows[p, m]), v)
    assert not rows[2].any(), "the cancelled row must be +0 bits"
    bad = np.argwhere(rows != ref)
    assert len(bad) == 0, (len(bad), bad[:8].tolist())
    assert np.array_equal(rows, ref)


def test_csr_bf16_place_equals_oracle_on_dense_rows(engine, case):
    row_ptr, peer, w, _, ref, L, free, req = case
    engine.upload_latency(L, "bf16")
    engine.upload_capacity(free)
    engine.upload_pods(req)
    engine.upload_traffic_csr(row_ptr, peer, w, "bf16", N)
    node, cf, _ = engine.place()
    want, wcost, wfree = oracle.place(ref, L, req, free, "bf16")
    assert (want < 0).any() and (want >= 0).any() and (wcost < 0).any()
    assert node.tolist() == want.tolist()
    assert np.array_equal(cf.astype(np.float64), wcost)
    assert (engine.get_capacity() == wfree).all()


def first_fit(req, free):
    free = free.astype(np.int64).copy()
    node = np.full(len(req), -1, np.int64)
    for p, r in enumerate(req.astype(np.int64)):
        fits = np.flatnonzero((free >= r).all(1))
        if len(fits):
            node[p] = fits[0]
            free[fits[0]] -= r
    return node, free


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_empty_csr_places_first_fit(engine, dtype):
    """row_ptr all zero, no peers, no weights: every cost is 0 and every pod
    takes the lowest-numbered node that fits."""
    rng = np.random.default_rng(4)
    _, _, free, req = cluster(rng, P, N, cap_scale=0.03)
    L = rng.integers(-20, 21, (N, N)).astype(np.float32)
    engine.upload_latency(f32_to_bf16_bits(L) if dtype == "bf16" else L, dtype)
    engine.upload_capacity(free)
    engine.upload_pods(req)
    wdt = np.uint16 if dtype == "bf16" else np.float32
    engine.upload_traffic_csr(np.zeros(P + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, wdt),
                              dtype, N)
    rows, _, _, _ = engine.read_inputs(0, P, want_L=False)
    assert not rows.any()
    node, cf, _ = engine.place()
    want, wfree = first_fit(req, free)
    assert (want < 0).any()
    assert node.tolist() == want.tolist()
    assert (cf == 0).all()
    assert (engine.get_capacity() == wfree).all()
