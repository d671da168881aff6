"""GPU: the split QP launch (scvx_qp_solve_batched_split, include/scvx_hip.h; QPSolver.solve(order_tail=...);
JacobiSCvx(dispatch_order="lpt") with every agent resident).  The same kernel runs the tail list's agents and the bulk
list's agents in two launches: a scheduling change, so every output must be bit-identical to the single launch --
through cold and warm-started Jacobi steps, under both trust-region rules, for the flag-specialised K = 50 class and
the runtime-K class; an order entry SCVX_QP_ORDER_SKIP must leave its workgroup without any effect."""
import numpy as np
import pytest

import scvx_hip
from scvx_hip import _lib

pytestmark = pytest.mark.gpu
SKIP = _lib.SCVX_QP_ORDER_SKIP
N, T = 16, 4
ENV = ("SCVX_QP_SPLIT", "SCVX_QP_SPLIT_THR", "SCVX_QP_SPLIT_T", "SCVX_QP_SPLIT_RESERVE")


def _c3(cuda, K):
    """bench.py's c3 construction (seed 1, 8 obstacles, input cone) for N agents at horizon K"""
    import bench
    import torch
    from scvx_hip import workloads
    sc = workloads.synthetic_di(N, K=K, seed=1, sigma=bench.SIGMA, obstacles=bench.N_OBS)
    w = {k: torch.tensor(sc[k], device=cuda) for k in ("X", "U", "x_init", "x_final", "sigma")}
    spec = scvx_hip.QPSpec(model="di", K=K, box=bench.BOX, obs=sc["obs"], w_obs=1e6, u_max=bench.U_MAX, tol=1e-8,
                           max_iter=60)
    return spec, w


def _run(monkeypatch, spec, w, rule, split, thr=1, reserve="whole", coupling=None, steps=3):
    """`steps` Jacobi steps (the first cold, the others warm); every step's X, U, tr, obj, status, iters and the entry
    point its solve went through"""
    import bench
    from scvx_hip.scvx import JacobiSCvx
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    # 2: also under the per-agent rule and where the agents do not outnumber the CUs
    monkeypatch.setenv("SCVX_QP_SPLIT", "2" if split else "0")
    drv = JacobiSCvx(spec, w["x_init"], w["x_final"], w["sigma"], bench.TR0, tr_rule=rule, warm_max_status=1,
                     coupling=coupling, split_thr=thr, split_T=T, split_reserve=reserve, split_short_per_tail=0)
    X, U = w["X"].clone(), w["U"].clone()
    hist = []
    for _ in range(steps):
        X, U, out = drv.step(X, U)
        hist.append(dict(X=X.clone(), U=U.clone(), tr=drv.tr.clone(), obj=out["obj"].clone(),
                         status=out["status"].clone(), iters=out["iters"].clone(), entry=drv.solver.last_entry))
    return drv, hist


def _same(a, b):
    import torch
    assert len(a) == len(b)
    for sa, sb in zip(a, b):
        for k in ("X", "U", "tr", "obj", "status", "iters"):
            assert torch.equal(sa[k], sb[k]), k


@pytest.mark.parametrize("rule", ["global", "per_agent"])
@pytest.mark.parametrize("K,inst", [(50, 2), (12, 0)], ids=["K50_flags", "K12_runtime"])
def test_split_jacobi_steps_are_bit_identical(cuda, monkeypatch, rule, K, inst):
    spec, w = _c3(cuda, K)
    import ctypes
    assert _lib.lib().scvx_qp_instantiation(ctypes.byref(spec.to_c())) == inst   # the class this case is about
    _, ref = _run(monkeypatch, spec, w, rule, split=False)
    assert all(s["entry"] == "scvx_qp_solve_batched_ordered" for s in ref)
    assert (ref[-1]["status"] != 2).all()
    for reserve in ("whole", "half"):
        drv, got = _run(monkeypatch, spec, w, rule, split=True, reserve=reserve)
        assert [s["entry"] for s in got] == ["scvx_qp_solve_batched_ordered"] + ["scvx_qp_solve_batched_split"] * 2
        # thr = 1 and no short-solve limit: every agent qualifies, the T longest of each step form its tail
        order = np.argsort(-got[-1]["iters"].cpu().numpy(), kind="stable")
        assert np.array_equal(drv.order_tail.cpu().numpy(), order[:T])
        assert np.array_equal(drv.order.cpu().numpy(), np.concatenate([order[T:], np.full(T, SKIP)]))
        _same(got, ref)


def test_threshold_above_every_count_is_the_single_launch(cuda, monkeypatch):
    spec, w = _c3(cuda, 50)
    _, ref = _run(monkeypatch, spec, w, "global", split=False)
    drv, got = _run(monkeypatch, spec, w, "global", split=True, thr=spec.max_iter + 1)
    assert (drv.order_tail.cpu().numpy() == SKIP).all()
    bulk = drv.order.cpu().numpy()
    assert np.array_equal(np.sort(bulk), np.arange(N))       # the bulk list holds everyone
    _same(got, ref)


def test_native_ordering_c4_template(cuda, monkeypatch):
    """The c4 template (collision rows) at N = 16 with the agents-outnumber-waves mode forced: the order of the native
    sort is torch's stable descending argsort, and the run is the agent-order run."""
    import bench
    import torch
    from scvx_hip import workloads
    from scvx_hip.scvx import CouplingSpec, JacobiSCvx
    sc = workloads.synthetic_lattice(side=4, K=bench.K, seed=2, sigma=bench.SIGMA)
    w = bench.shard_tensors(sc, np.arange(N), cuda)
    spec = scvx_hip.QPSpec(model="di", K=bench.K, box=[(0, -50.0, 50.0), (1, -50.0, 50.0)], obs=[], w_obs=1e6, j_max=8,
                           w_coll=1e4, tol=1e-8, max_iter=60)
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    runs = []
    for lpt in (False, True):
        drv = JacobiSCvx(spec, w["x_init"], w["x_final"], w["sigma"], bench.TR0, coupling=CouplingSpec(R=2.3),
                         tr_rule="global", warm_max_status=1, dispatch_order="lpt" if lpt else "none")
        drv._lpt, drv._split = lpt, False
        X, U = w["X"].clone(), w["U"].clone()
        hist = []
        for _ in range(3):
            X, U, out = drv.step(X, U)
            hist.append(dict(X=X.clone(), U=U.clone(), tr=drv.tr.clone(), obj=out["obj"].clone(),
                             status=out["status"].clone(), iters=out["iters"].clone()))
            if lpt:
                want = torch.argsort(out["iters"], descending=True, stable=True).to(torch.int32)
                assert torch.equal(drv.order, want) and drv.order_tail is None
        runs.append(hist)
    _same(runs[1], runs[0])


def test_skip_entries_leave_outputs_untouched(cuda):
    import torch
    spec, w = _c3(cuda, 50)
    disc = scvx_hip.foh_batched("di", w["X"], w["U"], w["sigma"])
    tr = torch.full((N,), 0.25, dtype=torch.float64, device=cuda)
    args = (disc, w["sigma"], w["X"], w["U"], w["x_init"], w["x_final"], tr)
    ref = {k: v.clone() for k, v in scvx_hip.QPSolver(spec, N, device=cuda).solve(*args).items()}
    live = np.arange(12)                       # agents 12..15 appear in no list
    pad = np.full(4, SKIP)

    def i32(x):
        return torch.tensor(np.asarray(x, dtype=np.int64), dtype=torch.int32, device=cuda)
    cases = {"ordered": dict(order=i32(np.concatenate([live[::-1], pad]))),
             "split": dict(order=i32(np.concatenate([live[live != 3], pad, [SKIP]])), order_tail=i32([3, SKIP, SKIP, SKIP]))}
    for name, kw in cases.items():
        s = scvx_hip.QPSolver(spec, N, device=cuda)
        for buf in (s.X, s.U, s.slack, s.obj):
            buf.fill_(-777.25)
        s.status.fill_(-7)
        s.iters.fill_(-7)
        per = s.workspace.numel() // N             # agent i's share of the workspace: [i * per, (i + 1) * per)
        s.workspace.fill_(-777.25)
        out = s.solve(*args, **kw)
        for k in ("X", "U", "slack_coll", "obj", "status", "iters"):
            assert torch.equal(out[k][:12], ref[k][:12]), (name, k)
            sentinel = -7 if k in ("status", "iters") else -777.25
            assert (out[k][12:] == sentinel).all(), (name, k)
        assert (s.workspace[12 * per:] == -777.25).all(), name
