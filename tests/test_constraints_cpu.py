"""CPU side of node selectors and taints: the Python reference loop of the GPU
tests pinned to the project's oracle, the new libnas entries on a null context,
nas_host_intern_bits, and header / binding agreement on the new names."""
import ctypes
import os
import re

import numpy as np
import pytest

import constraint_ref as cref
import oracle
from kubernetesnetawarescheduler_amd import _lib, hostlib
from util import cluster

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_NAS = ["nas_upload_node_constraints", "nas_upload_pod_constraints", "nas_clear_constraints"]
NEW_HOST = ["nas_host_set_node_constraints", "nas_host_set_pod_constraints",
            "nas_host_intern_bits"]


@pytest.mark.parametrize("P,N", [(500, 200), (1200, 333)])
def test_reference_loop_equals_oracle_without_constraints(P, N):
    """All-zero words: the loop is oracle.place (placements, scores, capacity)."""
    rng = np.random.default_rng(P + N)
    WA, L, free, req = cluster(rng, P, N, lo=0, hi=60, cap_scale=0.05)
    z = np.zeros
    elig = cref.eligible(z(N, np.uint64), z(N, np.uint64), z(P, np.uint64), z(P, np.uint64))
    assert elig.all()
    node, score, left = cref.place(WA, L, req, free, elig)
    want, wcost, wfree = oracle.place(WA, L, req, free, "i8")
    assert node.tolist() == want.tolist()
    assert score.tolist() == wcost.tolist()
    assert (left == wfree).all()
    assert (want < 0).any() and (want >= 0).any()


def test_eligibility_rule_and_word_layouts():
    lab = np.array([0b011, 0b001, 0b111, 0], np.uint64)
    tnt = np.array([0, 0b10, 0b10, 0b01], np.uint64)
    rq = np.array([0, 0b001, 0b110], np.uint64)
    tl = np.array([0, 0b10, 0b11], np.uint64)
    e = cref.eligible(lab, tnt, rq, tl)
    assert e.tolist() == [[True, False, False, False], [True, True, True, False],
                          [False, False, True, False]]
    w = cref.words32(e)
    assert w[:, 0].tolist() == [0b0001, 0b0111, 0b0100]
    assert cref.words64(w).tolist() == [[0b0001, 0b0111, 0b0100]]
    # bit 33 lands in the second 32-bit word / the high half of the 64-bit one
    wide = np.zeros((1, 70), bool)
    wide[0, [33, 65]] = True
    assert cref.words32(wide).tolist() == [[0, 2, 2]]
    assert cref.words64(cref.words32(wide)).tolist() == [[2 << 32], [2]]


def test_new_entries_reject_a_null_context():
    L = _lib.lib()
    assert L.nas_upload_node_constraints(None, None, None, 4) == _lib.NAS_ERR_ARG
    assert L.nas_upload_pod_constraints(None, None, None, 4) == _lib.NAS_ERR_ARG
    assert L.nas_clear_constraints(None) == _lib.NAS_ERR_ARG


def test_intern_bits():
    uni = ["zone=a", "zone=b", "disk=ssd", "gpu=mi355x"]
    assert hostlib.intern_bits(uni, ["disk=ssd", "zone=a"]) == 0b0101       # a subset
    assert hostlib.intern_bits(uni, []) == 0                                # the empty set
    assert hostlib.intern_bits(uni, ["zone=b", "rack=7"]) == 0b0010         # outside: ignored
    assert hostlib.intern_bits(uni, ["zone=bb", "zone"]) == 0               # exact match only
    assert hostlib.intern_bits([], ["zone=a"]) == 0
    u64 = [f"k{i}=v" for i in range(64)]
    assert hostlib.intern_bits(u64, ["k63=v", "k0=v"]) == (1 << 63) | 1
    with pytest.raises(_lib.NasError) as ex:
        hostlib.intern_bits([f"k{i}=v" for i in range(65)], ["k1=v"])
    assert ex.value.code == _lib.NAS_ERR_ARG
    bits = ctypes.c_uint64(7)
    assert hostlib.hostlib().nas_host_intern_bits(None, 0, None, 0, None) == _lib.NAS_ERR_ARG
    assert hostlib.hostlib().nas_host_intern_bits(None, 0, None, 0, ctypes.byref(bits)) == 0
    assert bits.value == 0


def _declared(header, prefix):
    with open(os.path.join(ROOT, "include", header)) as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return set(re.findall(r"\b(" + prefix + r"[a-z0-9_]+)\s*\(", src))


def test_header_and_bindings_agree_on_the_new_names():
    nas, host = _declared("nas.h", "nas_"), _declared("nas_host.h", "nas_host_")
    for n in NEW_NAS:
        assert n in nas and n in _lib.SIGNATURES and hasattr(_lib.lib(), n), n
    for n in NEW_HOST:
        assert n in host and n in hostlib.SIGNATURES and hasattr(hostlib.hostlib(), n), n
    with open(os.path.join(ROOT, "scheduler", "nas.go")) as f:
        go = f.read()
    assert {"nas_upload_node_constraints", "nas_upload_pod_constraints"} <= set(
        re.findall(r"\bC\.(nas_[a-z0-9_]+)\(", go))
    # no layout change: the ABI version and the structs the host fills stay
    assert _lib.lib().nas_version() == 2
    assert ctypes.sizeof(hostlib.HostPod) == 5 * 8 + 3 * 4 + 4 + 2 * 8


def test_snapshot_files_carry_constraints(tmp_path):
    from kubernetesnetawarescheduler_amd import snapshot
    rng = np.random.default_rng(3)
    WA, L, free, req = cluster(rng, 20, 9)
    lab, tnt, rq, tl = cref.pattern("mix", rng, 20, 9)
    old, new = str(tmp_path / "old.npz"), str(tmp_path / "new.npz")
    snapshot.save_place(old, L, free, req, WA)
    snapshot.save_place(new, L, free, req, WA,
                        constraints={"labels": lab, "taints": tnt, "require": rq, "tolerate": tl})
    assert not any(k in snapshot.load(old) for k in snapshot.CONSTRAINT_KEYS)
    f = snapshot.load(new)
    for k, v in zip(snapshot.CONSTRAINT_KEYS, (lab, tnt, rq, tl)):
        assert f[k].dtype == np.uint64 and (f[k] == v).all()
    with pytest.raises(ValueError):
        snapshot.save_place(new, L, free, req, WA, constraints={"affinity": lab})

    class Rec:  # records what replay_place uploads
        def __init__(self):
            self.calls = []

        def __getattr__(self, name):
            return lambda *a, **k: self.calls.append((name, a)) or (None, None, None)

    for path, want in ((old, []), (new, ["upload_node_constraints", "upload_pod_constraints"])):
        r = Rec()
        snapshot.replay_place(r, path)
        names = [c[0] for c in r.calls]
        assert names[-1] == "place" and "clear_constraints" in names
        assert [n for n in names if n.startswith("upload_") and "constraints" in n] == want
