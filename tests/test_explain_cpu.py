"""CPU side of nas_explain: the numpy reference of the GPU tests on a hand
case, what the shared generator covers, nas_host_explain_message, and header /
binding agreement on the new names."""
import os
import re

import numpy as np
import pytest

import constraint_ref as cref
import explain_ref as xref
from kubernetesnetawarescheduler_amd import _lib, hostlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# N = 4; pod A requires label 1 and tolerates nothing, pod B tolerates taint 2
FREE = [(1000, 1000, 1), (500, 2000, 1), (1000, 1000, 0), (100, 100, 1)]
LABELS, TAINTS = [1, 1, 0, 1], [0, 2, 0, 2]
REQ = [(600, 1500, 1), (100, 100, 1)]
REQUIRE, TOLERATE = [1, 0], [0, 2]
REC_A = [2, 1, 1, 0, 1, 0, 0, 4]
REC_B = [0, 0, 1, 0, 0, 1, 3, 4]  # node 3 fits by equality
MSG_A = ("0/4 nodes are available: 2 node(s) had untolerated taint, "
         "1 node(s) didn't match Pod's node selector, 1 Insufficient memory.")
MSG_B = "3/4 nodes are available: 1 Too many pods."


def test_reference_on_the_hand_case():
    got = xref.explain(REQ, FREE, LABELS, TAINTS, REQUIRE, TOLERATE)
    assert got.dtype == np.int32 and got.tolist() == [REC_A, REC_B]
    # without words: resources alone (pod A: cpu short on nodes 1 and 3,
    # memory on 0, 2 and 3, pod slots on 2)
    assert xref.explain(REQ, FREE).tolist() == [[0, 0, 4, 2, 3, 1, 0, 4], [0, 0, 1, 0, 0, 1, 3, 4]]


@pytest.mark.parametrize("P,N", [(65, 63), (64, 64), (130, 65), (257, 129), (700, 1100)])
def test_generator_reaches_every_slot(P, N):
    """From 65 x 63 up some pod has each of the seven counts non-zero, pairs
    that fail both taint and selector exist (the ownership rule decides them)
    and so do pairs short in two resources; the four classes partition N."""
    _, _, free, req, (lab, tnt, rq, tl) = xref.case(P, N)
    c = xref.explain(req, free, lab, tnt, rq, tl)
    assert (c[:, :xref.NODES] > 0).any(0).all()
    assert (c[:, [xref.TAINT, xref.SELECTOR, xref.RESOURCES, xref.FIT]].sum(1) == N).all()
    assert (c[:, xref.NODES] == N).all()
    both = ((tnt[None, :] & ~tl[:, None]) != 0) & ((lab[None, :] & rq[:, None]) != rq[:, None])
    assert both.sum() >= 100
    short = req.astype(np.int64)[:, None, :] > free.astype(np.int64)[None, :, :]
    assert ((short.sum(2) >= 2) & cref.eligible(lab, tnt, rq, tl)).any()
    assert (c[:, [xref.CPU, xref.MEM, xref.PODS]].sum(1) > c[:, xref.RESOURCES]).any()
    assert (c[:, xref.FIT] == (cref.eligible(lab, tnt, rq, tl)
                               & ~short.any(2)).sum(1)).all()


def test_explain_message():
    assert hostlib.explain_message(REC_A) == MSG_A == xref.message(REC_A)
    assert hostlib.explain_message(REC_B) == MSG_B == xref.message(REC_B)
    assert hostlib.explain_message([0, 0, 0, 0, 0, 0, 4, 4]) == "4/4 nodes are available."
    every = [7, 6, 5, 4, 3, 2, 1, 19]
    assert hostlib.explain_message(every) == (
        "1/19 nodes are available: 7 node(s) had untolerated taint, 6 node(s) didn't match "
        "Pod's node selector, 4 Insufficient cpu, 3 Insufficient memory, 2 Too many pods.")
    assert hostlib.explain_message(every) == xref.message(every)


def test_explain_message_never_truncates():
    import ctypes
    with pytest.raises(_lib.NasError) as ex:
        hostlib.explain_message(REC_A, cap=10)
    assert ex.value.code == _lib.NAS_ERR_ARG
    L = hostlib.hostlib()
    c = (ctypes.c_int32 * 8)(*REC_B)
    buf = ctypes.create_string_buffer(b"x" * 63, 64)
    n = len(MSG_B)
    assert L.nas_host_explain_message(c, buf, n) == _lib.NAS_ERR_ARG  # no room for the NUL
    assert buf.raw[:63] == b"x" * 63                                   # left untouched
    assert L.nas_host_explain_message(c, buf, n + 1) == 0
    assert buf.value.decode() == MSG_B
    assert L.nas_host_explain_message(None, buf, 64) == _lib.NAS_ERR_ARG
    assert L.nas_host_explain_message(c, None, 64) == _lib.NAS_ERR_ARG
    assert L.nas_host_set_explain(None, 1) == _lib.NAS_ERR_ARG


def test_null_context_is_rejected():
    assert _lib.lib().nas_explain(None, None, 0, None) == _lib.NAS_ERR_ARG


def _declared(header, prefix):
    with open(os.path.join(ROOT, "include", header)) as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return set(re.findall(r"\b(" + prefix + r"[a-z0-9_]+)\s*\(", src)), src


def test_header_and_bindings_agree_on_the_new_names():
    (nas, hdr), (host, _) = _declared("nas.h", "nas_"), _declared("nas_host.h", "nas_host_")
    assert "nas_explain" in nas and "nas_explain" in _lib.SIGNATURES
    assert hasattr(_lib.lib(), "nas_explain")
    for n in ("nas_host_explain_message", "nas_host_set_explain"):
        assert n in host and n in hostlib.SIGNATURES and hasattr(hostlib.hostlib(), n), n
    # the slot names: header, _lib and the reference agree
    slots = dict(re.findall(r"#define\s+NAS_WHY_([A-Z]+)\s+(\d+)", hdr))
    assert len(slots) == 9
    for name, v in slots.items():
        assert getattr(_lib, "NAS_WHY_" + name) == int(v) == getattr(xref, name), name
    with open(os.path.join(ROOT, "scheduler", "nas.go")) as f:
        go = f.read()
    assert "nas_explain" in set(re.findall(r"\bC\.(nas_[a-z0-9_]+)\(", go))
    assert re.search(r"func \(e \*nasEngine\) Explain\(pods \[\]int32\) \(\[\]\[8\]int32, error\)", go)
    assert _lib.lib().nas_version() == 2  # additive: no layout change
