"""CPU, no GPU: which qp_ipm_kernel instantiation the host picks for a template (csrc/qp_inst.hpp qp_select, read
through scvx_qp_instantiation, which calls the function the launch calls): 2 = K and the problem flags at compile time,
1 = K at compile time, 0 = everything at run time.

The flag-specialised instantiations read none of the fields they fix, so the selection must compare every one of them:
each is changed alone here and must leave the flag-specialised kernel, while every field that stays run-time data
(bounds, weights, obstacle geometry, u_max, tolerances, the collision rows per node) must not."""
import ctypes
import os

import pytest

ENV_K, ENV_F = "SCVX_QP_GENERIC_K", "SCVX_QP_GENERIC_FLAGS"
BOX = [(0, -12.0, 12.0), (1, -12.0, 12.0)]
OBS8 = [((float(i), 1.0, -2.0), 0.5 + 0.1 * i) for i in range(8)]


def _spec(name, **kw):
    import scvx_hip
    base = dict(model="di", K=50, box=BOX, obs=[], w_obs=1e6, u_max=None, tol=1e-8, max_iter=60)
    if name == "c3":
        base.update(obs=OBS8, u_max=1.0)
    elif name == "c4":
        base.update(j_max=8, w_coll=1e4)
    base.update(kw)
    return scvx_hip.QPSpec(**base)


def _inst(spec, edit=None):
    from scvx_hip import _lib
    t = spec.to_c()
    if edit:
        edit(t)
    return int(_lib.lib().scvx_qp_instantiation(ctypes.byref(t)))


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    monkeypatch.delenv(ENV_K, raising=False)
    monkeypatch.delenv(ENV_F, raising=False)


@pytest.mark.parametrize("name", ("c2", "c3", "c4"))
def test_bench_templates_take_the_flag_specialised_kernel(name):
    assert _inst(_spec(name)) == 2


@pytest.mark.parametrize("name", ("c2", "c3", "c4"))
def test_every_fixed_field_is_compared(name):
    changes = {
        "has_final": dict(has_final=False),
        "fix_last_input": dict(fix_last_input=False),
        "ineq_last": dict(ineq_last=True),
        "has_soc": dict(u_max=None if name == "c3" else 1.0),
        "n_box": dict(box=BOX[:1]),
        "box_idx[0]": dict(box=[(2, -12.0, 12.0), (1, -12.0, 12.0)]),
        "box_idx[1]": dict(box=[(0, -12.0, 12.0), (2, -12.0, 12.0)]),
        "box order": dict(box=[BOX[1], BOX[0]]),
        "soft terminal": dict(has_final=False, w_final=100.0),
        "w_prox": dict(w_prox=10.0),
    }
    if name == "c3":
        changes["n_obs 7"] = dict(obs=OBS8[:7])
        changes["n_obs 3"] = dict(obs=OBS8[:3])
    for what, kw in changes.items():
        assert _inst(_spec(name, **kw)) == 1, (name, what)
    # fields of the struct no QPSpec produces: any non-zero flag value is true, as in the kernel
    assert _inst(_spec(name), lambda t: setattr(t, "has_final", 2)) == 2
    assert _inst(_spec(name), lambda t: setattr(t, "ineq_last", 7)) == 1


def test_row_counts_that_change_the_class():
    # one obstacle / one collision row on the C2 template: the 8-obstacle / 8-row class, whose flags do not match
    assert _inst(_spec("c2", obs=OBS8[:1])) == 1
    assert _inst(_spec("c4", obs=OBS8[:1])) == 0       # <6,3,2,8,8,0> has no K = 50 instantiation
    assert _inst(_spec("c3", j_max=8)) == 0
    assert _inst(_spec("c3", w_nu=1e4)) == 0           # the virtual-control class
    assert _inst(_spec("c4", j_max=16)) == 0


@pytest.mark.parametrize("name", ("c2", "c3", "c4"))
def test_runtime_data_keeps_the_flag_specialised_kernel(name):
    kws = [dict(box=[(0, -3.0, 5.0), (1, -1.0, 2.0)]), dict(w_obs=10.0), dict(tol=1e-6), dict(max_iter=7),
           dict(w_last=0.5), dict(w_coll=3.0), dict(pos_dim=2)]
    if name == "c3":
        kws += [dict(u_max=2.5), dict(obs=[((9.0, 9.0, 9.0), 1.0)] * 8)]
    if name == "c4":
        kws += [dict(j_max=5), dict(j_max=1)]    # rows per node stay run-time data; only j_max > 0 is a flag
    for kw in kws:
        assert _inst(_spec(name, **kw)) == 2, (name, kw)


def test_k_and_other_models():
    import scvx_hip
    assert _inst(_spec("c3", K=49)) == 0 and _inst(_spec("c3", K=12)) == 0
    quad = scvx_hip.QPSpec(model="quad", K=50, box=[], obs=[], tol=1e-8, max_iter=60)
    assert _inst(quad) == 0
    bad = _spec("c3", K=65)
    assert _inst(bad) < 0


def test_environment_overrides(monkeypatch):
    s = _spec("c3")
    monkeypatch.setenv(ENV_F, "1")
    assert _inst(s) == 1
    monkeypatch.setenv(ENV_F, "0")
    assert _inst(s) == 2
    monkeypatch.setenv(ENV_F, "")
    assert _inst(s) == 2
    monkeypatch.setenv(ENV_K, "1")
    assert _inst(s) == 0
    monkeypatch.setenv(ENV_F, "1")
    assert _inst(s) == 0


def test_trace_takes_the_kernel_with_diagnostics():
    """the flag-specialised instantiation carries no region timers or iteration trace: while a trace buffer is set the
    solve runs the runtime-flag one (host state only here: nothing is launched, the pointer is never used)"""
    from scvx_hip import _lib
    L = _lib.lib()
    s = _spec("c3")
    assert _inst(s) == 2
    L.scvx_qp_set_trace(ctypes.c_void_p(4096), 0, 1)
    try:
        assert _inst(s) == 1
    finally:
        L.scvx_qp_set_trace(None, 0, 0)
    assert _inst(s) == 2
