"""CPU, no GPU: the split QP launch's host side -- the argument checks of the two entry points
(scvx_qp_dispatch_select, scvx_qp_solve_batched_split: rejected before anything touches a device) and the driver's
choice between the single launch, the ordered launch and the split launch (JacobiSCvx: dispatch_order, the
SCVX_QP_SPLIT switch, the agent count against the GPU's compute units), with a stub solver that records how it is
called."""
import ctypes

import pytest
import torch

from scvx_hip import QPSpec, _lib
from scvx_hip.scvx import JacobiSCvx

ENV = ("SCVX_QP_SPLIT", "SCVX_QP_SPLIT_THR", "SCVX_QP_SPLIT_T", "SCVX_QP_SPLIT_RESERVE")


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


def test_entry_points_are_declared_and_check_their_arguments():
    L = _lib.lib()
    for name in ("scvx_qp_dispatch_select", "scvx_qp_solve_batched_split"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    hdr = open(__file__.replace("tests/test_qp_split_cpu.py", "include/scvx_hip.h")).read()
    assert "#define SCVX_QP_ORDER_SKIP (-2147483647 - 1)" in hdr and _lib.SCVX_QP_ORDER_SKIP == -2 ** 31
    assert "#define SCVX_QP_RESERVE_WHOLE 1" in hdr and "#define SCVX_QP_RESERVE_HALF 2" in hdr
    assert _lib.SCVX_QP_RESERVE == {"whole": 1, "half": 2}
    t = QPSpec(model="di", K=50).to_c()
    one = ctypes.c_void_p(8)   # a non-null address that is never followed: every call below fails its checks first

    def split(N=4, order_bulk=one, order_tail=one, T=2, reserve=1, tpl=t):
        return L.scvx_qp_solve_batched_split(ctypes.byref(tpl), N, *([None] * 17), order_bulk, order_tail, T, reserve,
                                             None, 0, None)
    assert split(order_bulk=None) == -1 and b"order list" in L.scvx_last_error()
    assert split(order_tail=None) == -1
    assert split(T=0) == -1 and b"T" in L.scvx_last_error()
    assert split(T=5) == -1                      # T > N
    assert split(reserve=0) == -1 and b"reserve" in L.scvx_last_error()
    assert split(reserve=3) == -1
    assert split() == -1 and b"null buffer" in L.scvx_last_error()     # the lists pass, the solve's own checks follow
    bad = QPSpec(model="di", K=50).to_c()
    bad.K = 100
    assert split(tpl=bad) == -2                  # the template's checks are those of the single launch
    # the selection: no launch on bad arguments
    assert L.scvx_qp_dispatch_select(-1, one, 8, 0, 0, 60, one, one, None) == -1
    assert L.scvx_qp_dispatch_select(4, one, 8, 5, 0, 60, one, one, None) == -1        # T > N
    assert L.scvx_qp_dispatch_select(4, one, 8, 2, -1, 60, one, one, None) == -1       # short_per_tail < 0
    assert L.scvx_qp_dispatch_select(4, one, 8, 2, 0, 0, one, one, None) == -1         # max_iter < 1
    assert L.scvx_qp_dispatch_select(4, None, 8, 2, 0, 60, one, one, None) == -1       # no counts
    assert L.scvx_qp_dispatch_select(4, one, 8, 2, 0, 60, None, one, None) == -1       # T > 0 needs the tail list
    assert L.scvx_qp_dispatch_select(4, one, 8, 2, 0, 60, one, None, None) == -1
    assert L.scvx_qp_dispatch_select(8192, one, 8, 2, 0, 200, one, one, None) == -2    # count table: 128 x 201 > 12288
    assert L.scvx_qp_dispatch_select(4, one, 8, 2, 0, 1024, one, one, None) == -2      # more keys than threads
    assert L.scvx_qp_dispatch_select(0, None, 8, 0, 0, 60, None, None, None) == 0      # no agents: nothing to do


class _StubQP:
    """Records every solve's dispatch arguments; dispatch_lists restates the selection with torch."""
    supports_order = supports_split = True

    def __init__(self, N, iters):
        self.N, self.iters, self.calls, self.selects = N, iters, [], []

    def solve(self, disc, sigma, Xref, Uref, x_init, x_final, tr, rows=None, count=None, n=None, warm=None,
              order=None, order_tail=None, reserve=None):
        self.calls.append(dict(order=order, order_tail=order_tail, reserve=reserve))
        N = Xref.shape[0]
        return {"X": Xref + 1.0, "U": Uref * 0.5, "slack_coll": torch.zeros(N, Xref.shape[1], dtype=torch.float64),
                "obj": torch.zeros(N, dtype=torch.float64), "status": torch.zeros(N, dtype=torch.int32),
                "iters": self.iters}

    def dispatch_lists(self, thr, T, short_per_tail=0):
        self.selects.append((thr, T, short_per_tail))
        order = torch.argsort(self.iters, descending=True, stable=True).to(torch.int32)
        nq = int((self.iters >= thr).sum())
        nt = min(T, nq, (self.N - nq) // short_per_tail) if short_per_tail else min(T, nq)
        skip = torch.full((self.N,), _lib.SCVX_QP_ORDER_SKIP, dtype=torch.int32)
        tail = torch.cat([order[:nt], skip[:T - nt]]) if T else None
        return tail, torch.cat([order[nt:], skip[:nt]])


class _StubBackend:
    def __init__(self, iters):
        self.iters = iters

    def foh(self, model, X, U, sigma, nsub, out):
        return torch.zeros(X.shape[0], X.shape[1] - 1, 90, dtype=torch.float64)

    def qp_solver(self, spec, N, device):
        self.solver = _StubQP(N, self.iters)
        return self.solver


def _drive(monkeypatch, N, cus, steps=3, **kw):
    monkeypatch.setattr(JacobiSCvx, "_cu_count", lambda self: cus)
    iters = (torch.arange(N, dtype=torch.int32) % 5) + 5          # counts 5..9
    be = _StubBackend(iters)
    K = 5
    kw.setdefault("tr_rule", "global")
    drv = JacobiSCvx(QPSpec(model="di", K=K, max_iter=60), torch.zeros(N, 6), torch.zeros(N, 6), torch.ones(N), 0.25,
                     backend=be, **kw)
    X, U = torch.zeros(N, K, 6, dtype=torch.float64), torch.ones(N, K, 3, dtype=torch.float64)
    for _ in range(steps):
        X, U, _ = drv.step(X, U)
    return drv, be.solver


def test_split_engages_when_agents_share_compute_units(monkeypatch):
    drv, s = _drive(monkeypatch, N=8, cus=2, split_T=3, split_thr=8)      # 8 agents, 2 CUs, 8 resident waves
    assert s.selects == [(8, 3, 3)] * 3        # whole CU: a tail workgroup displaces three
    assert s.calls[0] == dict(order=None, order_tail=None, reserve=None)  # the first solve has no counts yet
    for c in s.calls[1:]:
        assert c["reserve"] == "whole"
        assert c["order_tail"].tolist() == [4, 3, _lib.SCVX_QP_ORDER_SKIP]    # counts 9 and 8 (six are below 8); T = 3
        assert c["order"].tolist() == [2, 7, 1, 6, 0, 5] + [_lib.SCVX_QP_ORDER_SKIP] * 2   # 7 7 6 6 5 5, ties by index
    # the settings from the environment
    monkeypatch.setenv("SCVX_QP_SPLIT_THR", "9")
    monkeypatch.setenv("SCVX_QP_SPLIT_T", "2")
    monkeypatch.setenv("SCVX_QP_SPLIT_RESERVE", "half")
    drv, s = _drive(monkeypatch, N=8, cus=2)
    assert s.selects[0] == (9, 2, 1) and s.calls[-1]["reserve"] == "half"
    assert s.calls[-1]["order_tail"].tolist() == [4, _lib.SCVX_QP_ORDER_SKIP]


@pytest.mark.parametrize("how", ["env", "none", "few_agents", "no_gpu", "runtime_model", "per_agent_rule"])
def test_unsplit_paths_keep_the_single_launch(monkeypatch, how):
    kw, N, cus = {}, 8, 2
    if how == "env":
        monkeypatch.setenv("SCVX_QP_SPLIT", "0")
    elif how == "none":
        kw["dispatch_order"] = "none"
    elif how == "few_agents":
        N = 2                                  # one compute unit each: nothing to reserve
    elif how == "no_gpu":
        cus = 0
    elif how == "per_agent_rule":
        kw["tr_rule"] = "per_agent"            # its steady state has no tail: the split is for the global rule
    if how == "runtime_model":
        monkeypatch.setattr("scvx_hip.scvx.default_nsub", lambda *a, **k: 1)
        monkeypatch.setattr("scvx_hip.scvx.model_dims", lambda m: (6, 3))
        drv, s = _drive_runtime(monkeypatch, N, cus)
    else:
        drv, s = _drive(monkeypatch, N, cus, **kw)
    assert not s.selects
    assert all(c == dict(order=None, order_tail=None, reserve=None) for c in s.calls) and len(s.calls) == 3


def _drive_runtime(monkeypatch, N, cus):
    """a model that is not one of the built-in names (the runtime-compiled classes keep the single launch)"""
    monkeypatch.setattr(JacobiSCvx, "_cu_count", lambda self: cus)
    be = _StubBackend(torch.full((N,), 9, dtype=torch.int32))
    K = 5
    spec = QPSpec(model="di", K=K, max_iter=60)
    spec.model = object()
    drv = JacobiSCvx(spec, torch.zeros(N, 6), torch.zeros(N, 6), torch.ones(N), 0.25, backend=be, nsub=1,
                     tr_rule="global")
    X, U = torch.zeros(N, K, 6, dtype=torch.float64), torch.ones(N, K, 3, dtype=torch.float64)
    for _ in range(3):
        X, U, _ = drv.step(X, U)
    return drv, be.solver


def test_more_agents_than_resident_waves_orders_only(monkeypatch):
    drv, s = _drive(monkeypatch, N=12, cus=2)                              # 12 agents > 8 resident waves
    assert s.selects == [(61, 0, 0)] * 3                                      # thr above max_iter, no tail list
    assert s.calls[0]["order"] is None
    for c in s.calls[1:]:
        assert c["order_tail"] is None and c["reserve"] is None
        assert c["order"].tolist() == torch.argsort(s.iters, descending=True, stable=True).tolist()


def test_switch_2_engages_under_the_per_agent_rule_and_with_few_agents(monkeypatch):
    monkeypatch.setenv("SCVX_QP_SPLIT", "2")
    drv, s = _drive(monkeypatch, N=2, cus=2, tr_rule="per_agent", split_T=1, split_thr=6, split_short_per_tail=0)
    assert s.selects == [(6, 1, 0)] * 3 and s.calls[-1]["order_tail"].tolist() == [1]


def test_split_settings_are_checked(monkeypatch):
    with pytest.raises(ValueError):
        _drive(monkeypatch, N=8, cus=2, split_reserve="third")
