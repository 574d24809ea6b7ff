#!/usr/bin/env python3
"""Time of nas_explain at the C3 shape (nas_synth_cluster, 10k nodes x 100k
pods, int8) with node selectors / taints uploaded (tools/constrained_pass.py's
words: 3 of 8 label bits per node, 0-2 required per pod, about half the nodes
tainted and half the pods tolerating), after one place(): the median of --reps
blocking Engine.explain calls (host wall time, list upload and record copy
included) for
  (a) the pass's unschedulable pods (pods 0..1023 if there are none),
  (b) 1,024 listed pods,
  (c) all pods,
and, for scale, the same context's filter(want_mask=False) fit_ms.  A sample of
the records is compared with a numpy count first.  Prints one JSON line.

    python tools/explain_pass.py [--nodes 10000 --pods 100000 --reps 20]
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
from tools.constrained_pass import words  # noqa: E402


def count(req, free, lab, tnt, rq, tl):
    """The records of include/nas.h NAS_WHY_* by broadcasting over (P, N)."""
    taint = (tnt[None, :] & ~tl[:, None]) != 0
    sel = ~taint & ((lab[None, :] & rq[:, None]) != rq[:, None])
    elig = ~taint & ~sel
    short = req.astype(np.int64)[:, None, :] > free.astype(np.int64)[None, :, :]
    cols = [taint, sel, elig & short.any(2)] + [elig & short[:, :, r] for r in range(3)]
    cols.append(elig & ~short.any(2))
    out = np.stack([c.sum(1) for c in cols] + [np.full(len(req), len(free))], 1)
    return out.astype(np.int32)


def timed(e, pods, reps, warmup):
    ms = []
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        e.explain(pods)
        if i >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return {"pods": e.n_pods if pods is None else len(pods),
            "median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4),
            "max_ms": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=10000)
    ap.add_argument("--pods", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=lambda s: int(s, 0), default=0x4E4153)
    a = ap.parse_args()
    res = {"nodes": a.nodes, "pods": a.pods, "reps": a.reps}
    rng = np.random.default_rng(a.seed)
    with Engine(0) as e:
        e.synth_cluster(a.seed, a.nodes, a.pods, "i8", peers=8)
        lab, tnt, rq, tl = words(rng, a.pods, a.nodes)
        e.upload_node_constraints(lab, tnt)
        e.upload_pod_constraints(rq, tl)
        e.reset_capacity()
        node, _, _ = e.place()
        none = np.flatnonzero(node < 0).astype(np.int32)
        res["unschedulable"] = int(len(none))
        # a sample of the records against numpy, on the capacity the pass left
        _, _, _, req = e.read_inputs(0, 0, want_L=False)
        left = e.get_capacity()
        sample = np.unique(np.concatenate([none[:128], rng.integers(0, a.pods, 128)])).astype(np.int32)
        got = e.explain(sample)
        want = count(req[sample], left, lab, tnt, rq[sample], tl[sample])
        if not (got == want).all():
            raise SystemExit(f"explain differs from numpy at pods "
                             f"{sample[(got != want).any(1)][:8].tolist()}")
        if len(none) and got[np.isin(sample, none), 6].any():
            raise SystemExit("an unschedulable pod still fits a node")
        res["checked_pods"] = int(len(sample))
        listed = np.sort(rng.choice(a.pods, min(1024, a.pods), replace=False)).astype(np.int32)
        res["unschedulable_pods"] = timed(e, none if len(none) else np.arange(
            min(1024, a.pods), dtype=np.int32), a.reps, a.warmup)
        res["listed_1024"] = timed(e, listed, a.reps, a.warmup)
        res["all_pods"] = timed(e, None, a.reps, a.warmup)
        fit = []
        for _ in range(a.warmup + a.reps):
            e.filter(want_mask=False)
            fit.append(e.timings()["fit_ms"])
        res["filter_fit_ms"] = round(statistics.median(fit[a.warmup:]), 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
