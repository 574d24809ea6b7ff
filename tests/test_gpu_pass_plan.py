"""The library runs the plan the CPU test pins (csrc/pass_plan.h,
tests/sanitize/pass_plan_driver.cpp): after a one-cluster place(),
timings()["cost_launches"] is the number of planned chunks -- every chunk's
scoring books one cost launch, a gathered rescore slot books none.  Four
shapes whose chunk counts tell their plans apart, each placed twice with
identical results."""
import pytest

from kubernetesnetawarescheduler_amd import Engine

pytestmark = pytest.mark.gpu

SEED = 0x4E4153


@pytest.fixture(scope="module")
def own_engine():
    """An Engine of this module's own: the plan reads what earlier passes of
    the context left (slot hints, the auto herd shape)."""
    with Engine(0) as e:
        yield e


@pytest.mark.parametrize("N,P,herd,chunks", [
    (4097, 8193, 0, 2),    # 17 node tiles -> 32-tile chunks: the fewest pods with two of them
    (4097, 20000, 0, 3),   # ... and a tail chunk behind the commit stream
    (300, 33000, 0, 4),    # the wide tile's balanced plan with its half-length second chunk
    (600, 3000, 1, 6),     # the herd plan's one-wave chunks
])
def test_cost_launches_are_the_planned_chunks(own_engine, N, P, herd, chunks):
    e = own_engine
    e.set_option("HERD_PLAN", herd)
    try:
        e.synth_cluster(SEED, N, P, "i8", peers=8)
        runs = []
        for _ in range(2):
            e.reset_capacity()
            node, _, score = e.place()
            assert e.timings()["cost_launches"] == chunks, e.timings()
            runs.append((node.copy(), score.copy()))
        assert (runs[0][0] == runs[1][0]).all() and (runs[0][1] == runs[1][1]).all()
        assert (runs[0][0] >= -1).all() and (runs[0][0] < N).all()
    finally:
        e.set_option("HERD_PLAN", 2)
