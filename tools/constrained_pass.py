#!/usr/bin/env python3
"""Price of a constrained pass: reset_capacity + place at the C3 shape
(nas_synth_cluster, 10k nodes x 100k pods, int8), unconstrained and with node
selectors / taints uploaded (3 of 8 label bits per node, 0-2 required per pod,
about half the nodes tainted and half the pods tolerating).  A constrained
pass runs k_fit + the 256 x 256 cost tile instead of the fused fit in the wide
tile, without the cost-row cache and the commit's zero-traffic scan.

Prints one JSON line: the median of --reps passes of each kind (host wall
time around the two calls; place() synchronises) and the pass's own timings.

    python tools/constrained_pass.py [--nodes 10000 --pods 100000 --reps 20]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kubernetesnetawarescheduler_amd import Engine  # noqa: E402


def words(rng, P, N):
    bit = lambda idx: np.uint64(1) << idx.astype(np.uint64)  # noqa: E731
    lab = np.zeros(N, np.uint64)
    order = np.argsort(rng.random((N, 8)), axis=1)[:, :3]  # 3 distinct bits per node
    for j in range(3):
        lab |= bit(order[:, j])
    rq = np.zeros(P, np.uint64)
    k = rng.integers(0, 3, P)
    pick = np.argsort(rng.random((P, 8)), axis=1)[:, :2]
    for j in range(2):
        rq |= np.where(k > j, bit(pick[:, j]), np.uint64(0))
    tnt = np.where(rng.random(N) < 0.5, np.uint64(1) << np.uint64(40), np.uint64(0))
    tl = np.where(rng.random(P) < 0.5, np.uint64(1) << np.uint64(40), np.uint64(0))
    return lab, tnt, rq, tl


def timed(e, reps, warmup):
    out = (np.empty(e.n_pods, np.int32), np.empty(e.n_pods, np.float32),
           np.empty(e.n_pods, np.int64))
    ms = []
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        e.reset_capacity()
        e.place(out=out)
        if i >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    t = e.timings()
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4),
            "max_ms": round(max(ms), 4), "unschedulable": t["unschedulable"],
            "rescore_rounds": t["rescore_rounds"], "cost_launches": t["cost_launches"],
            "fit_ms": round(t["fit_ms"], 4), "cost_ms": round(t["cost_ms"], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=10000)
    ap.add_argument("--pods", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=lambda s: int(s, 0), default=0x4E4153)
    a = ap.parse_args()
    res = {"nodes": a.nodes, "pods": a.pods, "reps": a.reps}
    with Engine(0) as e:
        e.synth_cluster(a.seed, a.nodes, a.pods, "i8", peers=8)
        res["unconstrained"] = timed(e, a.reps, a.warmup)
        lab, tnt, rq, tl = words(np.random.default_rng(a.seed), a.pods, a.nodes)
        e.upload_node_constraints(lab, tnt)
        e.upload_pod_constraints(rq, tl)
        res["constrained"] = timed(e, a.reps, a.warmup)
        e.clear_constraints()
        res["cleared"] = timed(e, a.reps, a.warmup)
    res["ratio"] = round(res["constrained"]["median_ms"] / res["unconstrained"]["median_ms"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
