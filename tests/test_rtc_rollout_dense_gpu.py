"""The dense roll-out of runtime-compiled user models on the GPU (scvx_rtc_rollout_dense, csrc/foh_rtc.hip; the
body is csrc/foh_body.hpp's rollout_dense_body) against its numpy restatement (tests/rtc_rollout_ref.py), against
the built-in kernels on the same dynamics, and through everything built on it: the fleet scans, the analysis
drop-ins, the row records and the Jacobi driver with the continuous-time rows on.

Shapes: N = 5, K = 4 (15 lanes, one partial block of 64) and N = 70, K = 2 (one segment per agent, a second block
with 6 live lanes); (S, nsub) = (1, 1), (3, 7), (16, 16).  1e-12 is the project's figure for a kernel against the
CPU restatement of the same RK4 (tests/test_separation_gpu.py::test_rollout_dense_matches_the_helper)."""
import functools

import numpy as np
import pytest

import custom_models as cm
import intersample_rows_ref as ir
import obstacle_rows_ref as orf
import rtc_rollout_ref as rr
import separation_ref as sr

pytestmark = pytest.mark.gpu
TOL = 1e-12


def _t(a, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype or torch.float64, device="cuda:0")


def _roll(dm, X, U, sig, **kw):
    return tuple(t.cpu().numpy() for t in dm.rollout_dense(_t(X), _t(U), _t(sig), **kw))


def _errors(P, L, Pr, Lr):
    """The error measures of test_rollout_dense_matches_the_helper: P against the position scale, L relative."""
    return np.abs(P - Pr).max() / np.abs(Pr).max(), (np.abs(L - Lr) / Lr).max()


@pytest.mark.parametrize("S,nsub", rr.S_NSUB)
@pytest.mark.parametrize("N,K", rr.SHAPES)
@pytest.mark.parametrize("name,pd", rr.CASES)
def test_samples_match_the_restatement(cuda, name, pd, N, K, S, nsub):
    X, U, sig = rr.inputs(name, N, K)
    Pr, Lr = rr.reference(name, N, K, S, nsub, pd)
    # the relative measure of L: a few ulp of the position scale (1e-15) are below 1e-12 of a length above 1e-3
    assert Lr.min() > 1e-3
    P, L = _roll(rr.device_model(name), X, U, sig, S=S, nsub=nsub, pos_dim=pd)
    assert P.shape == (N, K - 1, S + 1, 3) and L.shape == (N, K - 1)
    eP, eL = _errors(P, L, Pr, Lr)
    print(f"{name} pos_dim={pd} N={N} K={K} S={S} nsub={nsub}: P {eP:.2e} of the position scale, L {eL:.2e} relative")
    assert eP <= TOL and eL <= TOL
    assert np.array_equal(P[:, :, 0, :pd], X[:, :-1, :pd])          # sample 0 is the node, exactly
    assert not P[..., pd:].any()                                      # zeros past pos_dim


def test_launch_parameters_reach_the_kernel(cuda):
    N, K, S, nsub = rr.SHAPES[0] + rr.S_NSUB[1]
    X, U, sig = rr.inputs("car", N, K)
    car = rr.device_model("car")
    P1, L1 = _roll(car, X, U, sig, S=S, nsub=nsub, pos_dim=2, params=[1.0])
    Pr, Lr = rr.dense_rk4_f(rr.car_f(1.0), X, U, sig, S, -(-nsub // S), 2)
    eP, eL = _errors(P1, L1, Pr, Lr)
    print(f"car at L = 1.0: P {eP:.2e}, L {eL:.2e}")
    assert eP <= TOL and eL <= TOL
    P25, _ = _roll(car, X, U, sig, S=S, nsub=nsub, pos_dim=2)          # the model's own L = 2.5
    assert np.abs(P25 - rr.reference("car", N, K, S, nsub, 2)[0]).max() <= TOL * np.abs(P25).max()
    assert np.abs(P1 - P25).max() > 1e-3


@pytest.mark.parametrize("model", ["di", "unicycle"])
def test_same_integrator_as_the_built_in_kernels(cuda, model):
    """The drop-in model re-traced through hipRTC against the library's own kernel for it, default substeps (1 and
    16): the same body on the same dynamics, whose expressions differ only in how sympy printed them."""
    import scvx_hip
    X, U, sig = sr.random_fleet(model, 70, 5, 1)
    pd = 2 if model == "unicycle" else 3
    dm = rr.retraced(model)
    nsub = scvx_hip.DEFAULT_NSUB[model]
    for S in (3, 8, 16):
        Pb, Lb = (t.cpu().numpy() for t in scvx_hip.rollout_dense(model, _t(X), _t(U), _t(sig), S=S, pos_dim=pd))
        P, L = _roll(dm, X, U, sig, S=S, nsub=nsub, pos_dim=pd)
        eP, eL = np.abs(P - Pb).max() / np.abs(Pb).max(), np.abs(L - Lb).max() / np.abs(Pb).max()
        print(f"{model} S={S}: P {eP:.2e}, L {eL:.2e} of the position scale")
        assert eP <= TOL and eL <= TOL
        assert np.array_equal(P[:, :, 0], Pb[:, :, 0])


def test_outputs_do_not_depend_on_the_launch_geometry(cuda):
    (N, K), (S, nsub) = rr.SHAPES[1], rr.S_NSUB[1]
    for name, pd in (("car", 2), ("tiny1", 1)):
        X, U, sig = rr.inputs(name, N, K)
        dm = rr.device_model(name)
        P, L = _roll(dm, X, U, sig, S=S, nsub=nsub, pos_dim=pd)
        Ps, Ls = _roll(dm, X[3:8], U[3:8], sig[3:8], S=S, nsub=nsub, pos_dim=pd)
        assert np.array_equal(Ps, P[3:8]) and np.array_equal(Ls, L[3:8])


def _car_fleet(N=12, K=5, seed=9):
    """Cars on a grid of pitch 3 with random headings, speeds and inputs."""
    rng = np.random.default_rng(seed)
    X = np.zeros((N, K, 4))
    X[:, :, 0] = 3.0 * (np.arange(N) % 4)[:, None] + rng.uniform(-0.3, 0.3, (N, K))
    X[:, :, 1] = 3.0 * (np.arange(N) // 4)[:, None] + rng.uniform(-0.3, 0.3, (N, K))
    X[:, :, 2] = rng.uniform(-np.pi, np.pi, (N, K))
    X[:, :, 3] = rng.uniform(0.5, 1.5, (N, K))
    U = np.stack([rng.uniform(-0.5, 0.5, (N, K)), rng.uniform(-0.4, 0.4, (N, K))], 2)
    return X, U, rng.uniform(1.0, 2.0, N)


OBSTACLES = [((1.5, 1.5), 0.4), ((7.0, 4.0), 0.6)]


def test_fleet_functions_are_the_roll_out_and_the_scans(cuda):
    import torch
    import scvx_hip
    car = rr.device_model("car")
    X, U, sig = (_t(a) for a in _car_fleet())
    N = X.shape[0]
    P, L = car.rollout_dense(X, U, sig, S=8, pos_dim=2)
    fs = scvx_hip.fleet_separation(car, X, U, sig, pos_dim=2)
    assert torch.equal(fs["P"], P) and torch.equal(fs["L"], L)
    scan = scvx_hip.separation_scan(P, L, 0, N)
    for key in ("sep", "j", "s", "alpha"):
        assert torch.equal(fs[key], scan[key]), key
    assert fs["min"] == float(scan["sep"].min().item()) and 0.0 < fs["min"] < 3.5
    fo = scvx_hip.fleet_obstacle_clearance(car, X, U, sig, OBSTACLES, robot_radius=0.1, pos_dim=2)
    assert torch.equal(fo["P"], P) and torch.equal(fo["L"], L)
    sc = scvx_hip.obstacle_scan(P, OBSTACLES)
    total = torch.as_tensor([0.4 + 0.1, 0.6 + 0.1], dtype=torch.float64, device=X.device)
    assert torch.equal(fo["clear"], sc["dist"] - total) and torch.equal(fo["tau"], sc["alpha"])
    assert fo["clear"].shape == (N, X.shape[1] - 1, 2) and fo["min"] == float(fo["clear"].min().item())


def test_analysis_drop_ins_take_a_user_model(cuda):
    import scvx_hip
    from SCvx.discretization.first_order_hold import FirstOrderHold
    from SCvx.utils.analysis import (compute_intersample_clearance, min_agent_obstacle_clearance_continuous,
                                     min_inter_agent_separation_continuous)
    X, U, sig = _car_fleet()
    K = X.shape[1]
    foh = FirstOrderHold(cm.KinematicCar(), K)
    dm = foh._name
    assert not isinstance(dm, str) and dm.dims == (4, 2)
    X_list, U_list = [x.T for x in X], [u.T for u in U]
    ref = scvx_hip.fleet_separation(dm, _t(X), _t(U), _t(sig), S=8, nsub=16, pos_dim=2)
    for how in (foh, cm.KinematicCar(), dm):
        d_min, d_seg, info = min_inter_agent_separation_continuous(X_list, U_list, how, sig, S=8, pos_dim=2)
        assert d_min == ref["min"] and info["argmin"] == ref["argmin"]
        assert np.array_equal(d_seg, ref["sep"].cpu().numpy()) and np.array_equal(info["j"], ref["j"].cpu().numpy())
    refo = scvx_hip.fleet_obstacle_clearance(dm, _t(X), _t(U), _t(sig), OBSTACLES, 0.1, S=8, nsub=16, pos_dim=2)
    o_min, o_mat = min_agent_obstacle_clearance_continuous(X_list, U_list, foh, sig, OBSTACLES, 0.1, S=8, pos_dim=2)
    assert o_min == refo["min"] and np.array_equal(o_mat, refo["D"].cpu().numpy())
    with pytest.raises(ValueError, match="pos_dim"):
        min_inter_agent_separation_continuous(X_list, U_list, foh, sig, S=8)
    with pytest.raises(ValueError, match="pos_dim"):
        min_agent_obstacle_clearance_continuous(X_list, U_list, foh, sig, OBSTACLES, 0.1, S=8)
    # resolution 20 = one chunk of 16 samples and one of 4
    res, center, total = 20, np.array([1.0, 0.5]), 1.0 + 0.25 + 0.05
    Xa, Ua = X[0].T.copy(), U[0].T.copy()
    tau_c, h_c, tau_d, h_d = compute_intersample_clearance(Xa, Ua, foh, center, 1.0, 0.25, 0.05, resolution=res)
    href = rr.clearance_rollout_f(rr.car_f(2.5), Xa, Ua, foh.dt, foh.rollout_nsub(1.0), center, total, res)
    e = np.abs(h_c - href).max() / np.abs(href).max()
    print(f"car: h_cont {e:.2e} relative")
    assert tau_c.shape == h_c.shape == (res * (K - 1),) and e <= TOL
    assert np.array_equal(h_d, np.linalg.norm(Xa[:2].T - center, axis=1) - total)
    assert np.array_equal(h_c[::res], h_d[:-1])                      # t = 0 of every segment is the node


@functools.lru_cache(maxsize=None)
def _head_on_iterate():
    X, U, sig, _, _ = ir.run_head_on(_t, None, True)
    return X, U, sig


def test_row_records_match_the_built_in_model(cuda):
    """The backend's two record hooks on the final iterate of the head-on fixture (built-in run), with the re-traced
    double integrator against "di".  The iterate keeps the margins of tests/test_rtc_rollout_dense_cpu.py, so the
    two roll-outs (equal to 1e-12) select the same records."""
    from scvx_hip.scvx import HipBackend
    X, U, sig = _head_on_iterate()
    n_pair, n_obs = rr.row_margins(X, U, sig)
    r = rr.ROWS
    scale = max(1.0, np.abs(X[:, :, :3]).max())
    be = HipBackend()
    got = {}
    for key, model in (("di", "di"), ("rtc", rr.retraced("di"))):
        pr = be.intersample_pair_rows(model, _t(X), _t(U), _t(sig), r["S"], 1, 3, r["R"], r["pair_cull"], r["J"])
        ob = be.obstacle_rows(model, _t(X), _t(U), _t(sig), r["S"], 1, 3, r["obstacles"], r["obs_cull"], r["J"])
        got[key] = [t.cpu().numpy() for t in pr + ob]
    for (rec_b, cnt_b), (rec, cnt), n_ref, what in ((got["di"][:2], got["rtc"][:2], n_pair, "pair"),
                                                     (got["di"][2:], got["rtc"][2:], n_obs, "obstacle")):
        e = np.abs(rec - rec_b).max() / scale
        print(f"{what} records: {int(cnt.sum())}, largest difference {e:.2e} of the scale")
        assert np.array_equal(cnt, cnt_b) and np.array_equal(cnt_b, n_ref) and cnt.sum() > 0
        assert e <= TOL


def test_head_on_fixture_end_to_end_with_a_device_model(cuda):
    """test_head_on_fixture_end_to_end (tests/test_intersample_rows_gpu.py) with the re-traced double integrator as
    QPSpec.model: FOH, QP class and dense roll-out all compiled at run time.  Then the obstacle rows on the fixture
    of DESIGN §3.8 at the same QP class (the obstacle comes through the option).  That fixture starts at rest with
    U = 0, so the roll-outs of its warm start do not move and the first step has no record, whatever the model; the
    second step's records come from the first solve's iterate (count_seg 1 in segment 3 with the built-in model on the
    CPU restatement as well)."""
    import scvx_hip
    from scvx_hip.scvx import CouplingSpec, JacobiSCvx, ObstacleRowsSpec
    h = ir.HEAD_ON
    dm = rr.retraced("di")
    R2 = 2 * h["R"]

    def spec():
        return scvx_hip.QPSpec(model=dm, K=h["K"], box=h["box"], j_max=h["j_max"], w_coll=h["w_coll"], tol=h["tol"],
                               max_iter=80)

    def run(on):
        X0, U0, sig = ir.head_on()
        cpl = CouplingSpec(R=h["R"], check=False, intersample_S=h["S"] if on else 0, intersample_J=h["J"])
        drv = JacobiSCvx(spec(), _t(X0[:, 0]), _t(X0[:, -1]), _t(sig), h["tr0"], coupling=cpl, tr_rule="global")
        X, U = _t(X0), _t(U0)
        for _ in range(h["iters"]):
            Xn, Un, out = drv.step(X, U)
            X, U = Xn.clone(), Un.clone()
        return X.cpu().numpy(), U.cpu().numpy(), sig, {k: v.cpu().numpy() for k, v in out.items()}, drv

    X, U, sig, out, _ = run(False)
    cont, node, bound, st, slack = ir.head_on_figures(X, U, sig, out)
    print(f"off: continuous minimum {cont:.4f}, node minimum {node:.4f}, status {st}, slack {slack:.1e}")
    assert cont < 0.5 * R2
    X, U, sig, out, drv = run(True)
    cont, node, bound, st, slack = ir.head_on_figures(X, U, sig, out)
    print(f"on: continuous minimum {cont:.6f} (bound {bound:.2e}), node minimum {node:.6f}, status {st}, "
          f"slack {slack:.1e}")
    assert cont >= R2 - bound - 1e-6
    assert st == 0
    assert slack < 1e-6
    assert int(drv._is["overflow"].item()) == 0
    sep = drv.separation(_t(X), _t(U), S=h["S"])                       # the driver's own check, same model
    assert abs(sep["min"] - cont) <= bound + 1e-9

    X0, U0, sig = orf.fixture()
    drv = JacobiSCvx(spec(), _t(X0[:, 0]), _t(X0[:, -1]), _t(sig), orf.FIXTURE["tr0"], tr_rule="global",
                     obstacle_rows=ObstacleRowsSpec(S=8, J=1, obstacles=orf.FIXTURE["obs"]))
    X, U = _t(X0), _t(U0)
    for it in range(2):
        Xn, Un, out = drv.step(X, U)
        X, U = Xn.clone(), Un.clone()
        assert int(out["status"].max().item()) == 0 and int(drv._ob["overflow"].item()) == 0
        assert drv._ob["count_seg"].cpu().numpy().tolist() == [[0, 0, 0, it, 0, 0, 0]]
    oc = drv.obstacle_clearance(X, U)                                   # the driver's own check, same model
    ref = scvx_hip.fleet_obstacle_clearance(dm, X, U, _t(sig), orf.FIXTURE["obs"], 0.0, S=8, nsub=drv.nsub, pos_dim=3)
    assert oc["min"] == ref["min"] and oc["argmin"] == ref["argmin"] and oc["argmin"][2] == 3
