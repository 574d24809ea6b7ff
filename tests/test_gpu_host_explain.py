"""The opt-in unschedulable message of the host mirror (include/nas_host.h
nas_host_set_explain): one nas_explain call behind nas_place, each unplaced
pod reported with the FailedScheduling line of its record.  The scenario is
the 6-node one of test_gpu_host_constraints.py."""
import numpy as np
import pytest

import explain_ref as xref
from kubernetesnetawarescheduler_amd import Engine
from kubernetesnetawarescheduler_amd import hostlib as H

pytestmark = pytest.mark.gpu

OLD_REASON = "no node fits the pod's requests"
NEW_REASON = "no node matches the pod's node selector and tolerations"
N = 6
NODES = [f"node{i}" for i in range(N)]
WANT = {"ns/p0": "node1", "ns/p1": "node3", "ns/p2": "node0", "ns/p3": "node1", "ns/p4": None,
        "ns/p5": None, "ns/p6": "node3", "ns/p7": "node4", "ns/p8": None, "ns/p9": "node2"}
# the scenario's strings as bits: labels disk=ssd 1, gpu=mi355x 2, zone=b 4; taint dedicated=infra 1
LABELS = np.array([0, 0, 0, 1 | 4, 1, 0], np.uint64)
TAINTS = np.array([1, 0, 0, 0, 0, 0], np.uint64)
REQUIRE = np.array([0, 1, 0, 0, 2, 0, 1 | 4, 1, 1 | 4, 0], np.uint64)
TOLERATE = np.array([0, 0, 1, 0, 0, 0, 0, 0, 0, 0], np.uint64)
REQ = np.array([(9000 if p == 5 else 100, 1000, 1) for p in range(10)], np.int32)


def run(e, explain):
    """The scenario through place_pending -> (outcomes, capacity left)."""
    cl = H.FakeCluster(nodes=NODES, capacity={nd: (4000, 4_000_000, 2) for nd in NODES})
    s = H.HostScheduler(e, cl)
    s.set_latency(NODES, np.zeros((N, N), np.int8))
    if explain is not None:
        s.set_explain(explain)
    s.set_node_constraints("node0", taints=["dedicated=infra:NoSchedule"])
    s.set_node_constraints("node3", labels=["disk=ssd", "zone=b"])
    s.set_node_constraints("node4", labels=["disk=ssd"])
    s.set_node_constraints("node5", labels=["rack=9"])
    s.set_pod_constraints("ns/p1", node_selector=["disk=ssd"])
    s.set_pod_constraints("ns/p2", tolerations=["dedicated=infra:NoSchedule"])
    s.set_pod_constraints("ns/p4", node_selector=["gpu=mi355x"])
    s.set_pod_constraints("ns/p6", node_selector=["disk=ssd", "zone=b"])
    s.set_pod_constraints("ns/p7", node_selector=["disk=ssd"],
                          tolerations=["other=thing:NoSchedule"])
    s.set_pod_constraints("ns/p8", node_selector=["disk=ssd", "zone=b"])
    for p in range(10):
        s.enqueue("ns", f"p{p}", cpu_milli=int(REQ[p, 0]), mem_kib=int(REQ[p, 1]))
    out = s.place_pending()
    e.n_nodes, e.n_pods = N, 10  # the host loop uploaded through the C ABI: the Engine's shape
    left = e.get_capacity()
    s.close()
    return out, left, cl


def check_placements(out, cl):
    assert len(out) == 10
    for kind, pod, node, _ in out:
        if WANT[pod] is None:
            assert (kind, node) == ("UNSCHEDULABLE", ""), pod
        else:
            assert (kind, node) == ("BOUND", WANT[pod]), pod
    assert [b[2] for b in cl.bindings] == [WANT[f"ns/p{p}"] for p in range(10)
                                           if WANT[f"ns/p{p}"]]


def test_opt_in_message_explains_each_unplaced_pod():
    with Engine(0) as e:
        out, left, cl = run(e, True)
        check_placements(out, cl)  # placements are unchanged
        reason = {pod: msg for kind, pod, _, msg in out if kind == "UNSCHEDULABLE"}
        assert sorted(reason) == ["ns/p4", "ns/p5", "ns/p8"]
        assert reason["ns/p4"] == ("0/6 nodes are available: 1 node(s) had untolerated taint, "
                                   "5 node(s) didn't match Pod's node selector.")
        # the other two from the reference on the capacity the pass left
        want = xref.explain(REQ, left, LABELS, TAINTS, REQUIRE, TOLERATE)
        assert want[:, xref.NODES].tolist() == [N] * 10
        for p in (4, 5, 8):
            assert want[p, xref.FIT] == 0
            assert reason[f"ns/p{p}"] == xref.message(want[p]) == H.explain_message(want[p]), p
        assert reason["ns/p5"] == ("0/6 nodes are available: 1 node(s) had untolerated taint, "
                                   "5 Insufficient cpu, 2 Too many pods.")  # nodes 1 and 3 are full
        assert reason["ns/p8"] == ("0/6 nodes are available: 1 node(s) had untolerated taint, "
                                   "4 node(s) didn't match Pod's node selector, 1 Too many pods.")
        # the engine's own records for the same pods agree
        assert (e.explain([4, 5, 8]) == want[[4, 5, 8]]).all()
        # switching it off again brings the fixed strings back
        out, _, cl = run(e, False)
        check_placements(out, cl)
        reason = {pod: msg for kind, pod, _, msg in out if kind == "UNSCHEDULABLE"}
        assert reason == {"ns/p4": NEW_REASON, "ns/p5": OLD_REASON, "ns/p8": OLD_REASON}


def test_default_keeps_the_two_fixed_messages():
    with Engine(0) as e:
        out, _, cl = run(e, None)
    check_placements(out, cl)
    reason = {pod: msg for kind, pod, _, msg in out if kind == "UNSCHEDULABLE"}
    assert reason == {"ns/p4": NEW_REASON, "ns/p5": OLD_REASON, "ns/p8": OLD_REASON}
