"""GPU: the QP kernel with the problem flags at compile time and without diagnostics in that instantiation
(DESIGN §3.3 "Non-arithmetic instructions") against goldens recorded with the build before the change
(tests/golden/qp_insn_steps.npz, written by tests/golden/make_qp_insn_goldens.py on an MI355X).

No floating-point expression of a live lane changed, so every output is asserted equal bit for bit: np.array_equal on
obj, status, iters and the collision slack of every step and on X, U (nu) of the last step, and the SHA-256 of the raw
bytes of X, U (nu) of every step (the golden file keeps the earlier steps' big arrays as digests only).

Each case is a Jacobi loop of one cold and two warm steps of 8 agents (4 for n = 12), at K = 50 and at a small runtime
K, for every instantiation the library has: flag- and K-specialised, K-specialised with runtime flags
(SCVX_QP_GENERIC_FLAGS=1), fully generic (SCVX_QP_GENERIC_K=1).  Which one a solve takes is read back from the library
(scvx_qp_instantiation, the launch's own selection function), so a case cannot pass on another kernel than it names.
The mismatch cases change one field of the C3 template each: the host must fall back to runtime flags."""
import ctypes
import os

import numpy as np
import pytest

import qp_insn_cases as ic

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "qp_insn_steps.npz")
GENERIC, KSPEC, KFLAGS = 0, 1, 2


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as d:
        g = {k: d[k] for k in d.files}
    # the parent's two instantiations agreed everywhere, so one golden serves every instantiation
    assert g["generic_equals_parent"].all() and len(g["generic_equals_parent"]) == len(ic.all_cases())
    return g


def _instantiation(name, K, inst):
    """what the library would launch for the case's template under the instantiation's environment"""
    from scvx_hip import _lib
    tpl = ic.build(name, K)[2].to_c()
    before = {e: os.environ.get(e) for e in (ic.ENV_K, ic.ENV_F)}
    try:
        for e in before:
            os.environ.pop(e, None)
        if inst == "generic":
            os.environ[ic.ENV_K] = "1"
        elif inst == "kspec":
            os.environ[ic.ENV_F] = "1"
        return int(_lib.lib().scvx_qp_instantiation(ctypes.byref(tpl)))
    finally:
        for e, v in before.items():
            if v is None:
                os.environ.pop(e, None)
            else:
                os.environ[e] = v


def _check(golden, name, K, steps):
    assert len(steps) == ic.STEPS
    assert any((s["status"] == 0).any() for s in steps)
    for s, got in enumerate(steps):
        for k in ic.keys_of(name):
            key = ic.golden_key(name, K, "parent", s, k)
            v = got[k].astype(np.float64) if got[k].dtype.kind == "f" else got[k]
            if key in golden:
                eq = np.array_equal(v, golden[key])
                dmax = float(np.abs(v.astype(np.float64) - golden[key]).max()) if not eq else 0.0
                print(f"{name} K={K} step {s} {k}: equal {eq}, max |d| {dmax:.3e}")
                assert eq, (name, K, s, k, dmax)
            if k in ic.BIG:
                assert np.array_equal(ic.digest(v), golden[key + ".sha256"]), (name, K, s, k, "bytes differ")
        print(f"{name} K={K} step {s}: iters {got['iters'].tolist()}, status {got['status'].tolist()}")


@pytest.mark.parametrize("inst", ic.INSTS)
@pytest.mark.parametrize("name", ic.CLASSES)
def test_k50_steps_equal_parent(cuda, golden, name, inst):
    spec_k = name != "quad_vc"   # the n = 12 classes have runtime-K instantiations only
    want = {"flags": KFLAGS if spec_k else GENERIC, "kspec": KSPEC if spec_k else GENERIC, "generic": GENERIC}[inst]
    assert _instantiation(name, 50, inst) == want
    _check(golden, name, 50, ic.run(cuda, name, 50, inst))


@pytest.mark.parametrize("name", ic.CLASSES)
def test_runtime_k_steps_equal_parent(cuda, golden, name):
    """a K without a compiled instantiation: every setting runs the generic kernel (checked), so it is run once"""
    K = ic.small_k(name)
    assert [_instantiation(name, K, i) for i in ic.INSTS] == [GENERIC] * 3
    _check(golden, name, K, ic.run(cuda, name, K, "flags"))


@pytest.mark.parametrize("name", ic.MISMATCH)
def test_flag_mismatch_takes_runtime_flags(cuda, golden, name):
    assert _instantiation("c3", 50, "flags") == KFLAGS
    assert _instantiation(name, 50, "flags") == KSPEC
    _check(golden, name, 50, ic.run(cuda, name, 50, "flags"))
