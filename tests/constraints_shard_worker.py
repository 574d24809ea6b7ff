"""Child process of test_gpu_constraints.py::test_local_group_node_shards:
node selectors and taints on node shards.  G ranks of an in-process group
(nas_comm_init_local), every rank uploading the same full-length word arrays,
must place like one context on the whole cluster and like the reference loop
(constraint_ref.place): placements, integer scores, remaining capacity on
every rank, and timings.unschedulable.  Usage: constraints_shard_worker.py G"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import constraint_ref as cref  # noqa: E402
from kubernetesnetawarescheduler_amd import Engine, LocalGroup, local_ranks  # noqa: E402
from util import cluster  # noqa: E402


def upload(e, WA, L, free, req, words):
    e.upload_latency(L, "i8")
    e.upload_capacity(free)
    e.upload_pods(req)
    e.upload_traffic(WA, "i8")
    e.upload_node_constraints(words[0], words[1])
    e.upload_pod_constraints(words[2], words[3])


def main(G):
    P, N = 1200, 333
    rng = np.random.default_rng(90 + G)
    WA, L, free, req = cluster(rng, P, N, lo=0, hi=60, cap_scale=0.05)
    # test_place_i8_exact's locality boost: many pods want the same few nodes
    WA[:, : N // 10] = np.minimum(WA[:, : N // 10].astype(np.int32) + 60, 127).astype(np.int8)
    words = cref.pattern("mix", rng, P, N)
    elig = cref.eligible(*words)
    want, wcost, wfree = cref.place(WA, L, req, free, elig)
    assert (want < 0).any() and (want >= 0).any()
    with Engine(0) as e:
        upload(e, WA, L, free, req, words)
        node1, _, ci1 = e.place()
        cap1 = e.get_capacity()
    assert node1.tolist() == want.tolist() and ci1.tolist() == wcost.tolist()
    assert (cap1 == wfree).all()
    group = LocalGroup(G)
    engines = [Engine(0) for _ in range(G)]
    try:
        def run(r, e):
            e.set_option("COMM_TIMEOUT_MS", 60000)
            e.comm_init_local(group, r)
            upload(e, WA, L, free, req, words)  # every rank: the same full-length arrays
            node, _, ci = e.place()
            return node, ci, e.get_capacity(), e.timings()
        res = local_ranks(engines, run)
    finally:
        for e in engines:
            e.close()
        group.close()
    for r, (node, ci, cap, t) in enumerate(res):
        assert node.tolist() == node1.tolist(), (G, r)
        assert ci.tolist() == ci1.tolist(), (G, r)
        assert (cap == wfree).all(), (G, r)
        assert t["unschedulable"] == int((want < 0).sum()), (G, r, t)
    print(f"G={G} ok")


if __name__ == "__main__":
    main(int(sys.argv[1]))
