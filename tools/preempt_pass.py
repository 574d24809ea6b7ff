#!/usr/bin/env python3
"""Time of nas_preempt at the C3 shape (nas_synth_cluster, 10k nodes x 100k
pods, int8) after one place(), on a full cluster: every node has less free
than the smallest request (--left: the capacity the pass left instead) and a
seeded table of running pods, about 30 per node (20..40, 300k in all),
priorities uniform in 0..999, requests drawn from the pending pods' own.  The
listed pods ask with priorities from {0, 100, 500, 1000}.  Reports the median
of --reps blocking Engine.preempt calls (host wall time, list upload and record
copy included) for
  (a) 1,024 listed pods (the pass's unschedulable pods first, filled up with
      random ones), without and with 8 victim slots,
  (b) all pods, once,
and, for scale in the same run, Engine.explain for list (a) and one place()
pass (reset_capacity + place, host wall time).  --words uploads node selectors
/ taints first (tools/constrained_pass.py's words).  A sample of the records is
compared with a numpy reference first.  Prints one JSON line.

    python tools/preempt_pass.py [--nodes 10000 --pods 100000 --reps 20 --words --left]
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

BIAS = 2**31


def padded(N, node, prio, breq):
    """The bound pods as per-node rows in walk order (priority descending,
    index ascending), padded to the longest row: prio, req, index, valid."""
    order = np.lexsort((np.arange(len(node)), -prio.astype(np.int64), node))
    cnt = np.bincount(node, minlength=N)
    col = np.arange(len(node)) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    shape = (N, int(cnt.max()))
    P, R, I, V = (np.zeros(shape, np.int64), np.zeros(shape + (3,), np.int64),
                  np.full(shape, -1, np.int64), np.zeros(shape, bool))
    at = (node[order], col)
    P[at], R[at], I[at], V[at] = prio[order], breq[order], order, True
    return P, R, I, V


def reference(r, pi, free, elig, rows, max_victims):
    """include/nas.h's steps for one pod, vectorised over the nodes."""
    P, R, I, V = rows
    lower = V & (P < pi)
    avail = free.astype(np.int64) + (R * lower[:, :, None]).sum(1)
    cand = elig & (r[None, :] <= avail).all(1)
    nv = np.zeros(len(free), np.int64)
    top = np.zeros(len(free), np.int64)
    psum = np.zeros(len(free), np.int64)
    vict = np.full((len(free), max_victims), -1, np.int64)
    for j in range(P.shape[1]):
        act = lower[:, j] & cand
        stay = act & (avail - R[:, j] >= r[None, :]).all(1)
        avail = np.where(stay[:, None], avail - R[:, j], avail)
        out = act & ~stay
        top = np.where(out & (nv == 0), P[:, j], top)
        psum += np.where(out, P[:, j] + BIAS, 0)
        for s in range(max_victims):
            vict[:, s] = np.where(out & (nv == s), I[:, j], vict[:, s])
        nv += out
    if not cand.any():
        return (-1, 0, 0, 0, 0), [-1] * max_victims
    k0 = np.where(nv > 0, top + BIAS + 1, 0)
    n = np.lexsort((np.arange(len(free)), nv, psum, np.where(cand, k0, 2**40)))[0]
    return (int(n), int(nv[n]), int(top[n]), int(cand.sum()), int(psum[n])), vict[n].tolist()


def timed(fn, reps, warmup):
    ms = []
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        fn()
        if i >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4),
            "max_ms": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=10000)
    ap.add_argument("--pods", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--check", type=int, default=48, help="records compared with numpy")
    ap.add_argument("--words", action="store_true")
    ap.add_argument("--left", action="store_true",
                    help="ask against the capacity the pass left, not a full cluster")
    ap.add_argument("--seed", type=lambda s: int(s, 0), default=0x4E4153)
    a = ap.parse_args()
    res = {"nodes": a.nodes, "pods": a.pods, "reps": a.reps, "words": a.words, "left": a.left}
    rng = np.random.default_rng(a.seed)
    with Engine(0) as e:
        e.synth_cluster(a.seed, a.nodes, a.pods, "i8", peers=8)
        w = None
        if a.words:
            w = words(rng, a.pods, a.nodes)
            e.upload_node_constraints(w[0], w[1])
            e.upload_pod_constraints(w[2], w[3])

        def one_pass():
            e.reset_capacity()
            return e.place()[0]

        res["place_pass"] = timed(one_pass, max(3, a.reps // 4), 2)
        node = one_pass()
        none = np.flatnonzero(node < 0).astype(np.int32)
        res["unschedulable"] = int(len(none))
        _, _, _, req = e.read_inputs(0, 0, want_L=False)
        if not a.left:
            # a full cluster: less free than the smallest request in every
            # resource, so no pod fits anywhere as it is
            e.upload_capacity(np.stack([rng.integers(0, max(1, int(req[:, r].min())), a.nodes)
                                        for r in range(3)], 1).astype(np.int32))
        left = e.get_capacity()
        # the running pods
        per = rng.integers(20, 41, a.nodes)
        bnode = np.repeat(np.arange(a.nodes), per).astype(np.int32)
        B = len(bnode)
        shuffle = rng.permutation(B)
        bnode = bnode[shuffle]
        bprio = rng.integers(0, 1000, B).astype(np.int32)
        breq = req[rng.integers(0, a.pods, B)]
        t0 = time.perf_counter()
        e.upload_bound(bnode, bprio, breq)
        res["bound_pods"] = B
        res["upload_bound_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        prio = rng.choice([0, 100, 500, 1000], a.pods).astype(np.int32)
        n_list = min(1024, a.pods)
        fill = rng.permutation(a.pods)[:n_list].astype(np.int32)
        fill = fill[~np.isin(fill, none[:n_list])]
        listed = np.sort(np.concatenate([none[:n_list], fill])[:n_list]).astype(np.int32)
        # a sample of the records against numpy, on the capacity the pass left
        rows = padded(a.nodes, bnode, bprio, breq)
        sample = listed[rng.permutation(len(listed))[:a.check]]
        got, vict = e.preempt(prio[sample], sample, max_victims=8)
        for i, p in enumerate(sample):
            el = np.ones(a.nodes, bool) if w is None else \
                ((w[0] & w[2][p]) == w[2][p]) & ((w[1] & ~w[3][p]) == 0)
            want = reference(req[p].astype(np.int64), int(prio[p]), left, el, rows, 8)
            if (got[i].tolist(), vict[i].tolist()) != want:
                raise SystemExit(f"preempt differs from numpy at pod {p}: "
                                 f"{got[i].tolist()} {vict[i].tolist()} != {want}")
        res["checked_pods"] = int(len(sample))
        got, _ = e.preempt(prio[listed], listed)
        res["listed_answers"] = {
            "empty": int((got["node"] < 0).sum()), "victimless": int(
                ((got["node"] >= 0) & (got["n_victims"] == 0)).sum()),
            "with_victims": int((got["n_victims"] > 0).sum()),
            "mean_candidates": round(float(got["candidates"].mean()), 1),
            "max_victims": int(got["n_victims"].max())}
        res["listed_1024"] = timed(lambda: e.preempt(prio[listed], listed), a.reps, a.warmup)
        res["listed_1024_8_victims"] = timed(
            lambda: e.preempt(prio[listed], listed, max_victims=8), a.reps, a.warmup)
        res["explain_listed_1024"] = timed(lambda: e.explain(listed), a.reps, a.warmup)
        e.preempt(prio)  # (sizes the buffers)
        res["all_pods"] = timed(lambda: e.preempt(prio), 1, 0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
