"""The dense roll-out of runtime-compiled user models without a device: the C-ABI symbol, the generated kernel,
hipRTC compiles down to n_x = 1 (hipRTC runs on the host), argument rejection before any GPU call, the wrappers'
and the driver's checks, and the margins of the GPU row-record test's fixture (tests/rtc_rollout_ref.py) on the
numpy restatement alone."""
import ctypes
import functools
import os
import re

import pytest
import torch

import intersample_rows_ref as ir
import obstacle_rows_ref as orf
import rtc_rollout_ref as rr
from test_obstacle_rows_cpu import CpuBackend, _T

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
NAME = "scvx_rtc_rollout_dense_batched"


def test_symbol_is_exported_and_the_revision_stays():
    from scvx_hip import _lib
    hdr = open(os.path.join(REPO, "include", "scvx_hip.h")).read()
    assert int(re.search(r"#define SCVX_HIP_VERSION (\d+)", hdr).group(1)) == 7
    assert re.search(r"int\s+" + NAME + r"\(const scvx_rtc_model\* model", hdr)
    L = _lib.lib()
    assert _lib.SCVX_HIP_VERSION == 7 == L.scvx_version()
    assert NAME in _lib.EXPORTS and hasattr(L, NAME)
    assert len(getattr(L, NAME).argtypes) == 14


def test_generated_source_names_the_kernel():
    src = rr.device_model("car").source
    assert 'extern "C" __global__ __launch_bounds__(64) void scvx_rtc_rollout_dense(' in src
    assert "scvx::rollout_dense_body<UserModel>(" in src
    assert "scvx_rtc_foh" in src and "scvx_rtc_nonlinear" in src          # next to the other two, not instead


@pytest.mark.parametrize("n", [1, 2, 3, 9, 16])
def test_models_of_every_state_dimension_compile(n):
    """The roll-out's samples are the first pos_dim <= min(3, n_x) states: the body must not index x[1], x[2] of a
    model that has none (hipRTC compiles on the host, so this needs no device)."""
    from scvx_hip.rtc import DeviceModel
    f = [f"u[0] - p[0]*x[{(i + 1) % n}]" for i in range(n)]
    A = [["-p[0]" if j == (i + 1) % n else "0" for j in range(n)] for i in range(n)]
    dm = DeviceModel(n, 1, f, A=A, B=["1"] * n, params=[0.5], name=f"ring{n}")
    assert dm.dims == (n, 1) and "scvx_rtc_rollout_dense" in dm.source
    assert callable(dm.rollout_dense)


def test_bad_arguments_are_rejected_without_a_device():
    from scvx_hip import _lib
    L = _lib.lib()
    fn = getattr(L, NAME)
    buf = (ctypes.c_double * 8)()   # a non-null address; a rejected call never reads it
    p = ctypes.cast(buf, ctypes.c_void_p)
    par = (ctypes.c_double * 17)(*([0.5] * 17))
    good = dict(model=rr.device_model("car")._h.ptr, params=par, n_params=1, K=5, N=4, X=p, U=p, sigma=p, S=8, sub=1,
                pos_dim=2, P=p, L=p)

    def call(**kw):
        a = dict(good, **kw)
        return fn(a["model"], a["params"], a["n_params"], a["K"], a["N"], a["X"], a["U"], a["sigma"], a["S"], a["sub"],
                  a["pos_dim"], a["P"], a["L"], None)

    tiny2 = rr.device_model("tiny2")._h.ptr
    for kw in (dict(S=0), dict(S=17), dict(sub=0), dict(pos_dim=0), dict(pos_dim=4), dict(model=tiny2, pos_dim=3),
               dict(K=1), dict(X=None), dict(U=None), dict(sigma=None), dict(P=None), dict(L=None), dict(model=None),
               dict(n_params=17)):
        L.scvx_last_error()
        assert call(**kw) == -1, kw
        assert L.scvx_last_error(), kw
    assert call(N=0) == 0 and call(N=0, pos_dim=3) == 0 and call(model=tiny2, N=0, pos_dim=2) == 0
    assert call(N=-1) == -1
    # the built-in entry point keeps answering "unsupported" for the run-time model id
    roll = L.scvx_rollout_dense_batched
    assert roll(_lib.SCVX_MODEL_RUNTIME, None, 5, 4, p, p, p, 8, 1, 3, p, p, None) == -2
    assert roll(0, None, 5, 4, p, p, p, 8, 1, 4, p, p, None) == -1 and roll(2, None, 5, 0, p, p, p, 8, 1, 3, p, p, None) == 0


def test_wrappers_validate_before_the_device():
    import scvx_hip
    car = rr.device_model("car")
    X, U, sig = (torch.zeros(4, 5, 4, dtype=torch.float64), torch.zeros(4, 5, 2, dtype=torch.float64),
                 torch.ones(4, dtype=torch.float64))
    for fn in (car.rollout_dense, functools.partial(scvx_hip.rollout_dense, car)):
        with pytest.raises(ValueError):
            fn(X, U, sig, S=17, pos_dim=2)
        with pytest.raises(ValueError):
            fn(X, U, sig, pos_dim=5)
        with pytest.raises(ValueError):
            fn(X, U, sig, pos_dim=0)
        with pytest.raises(ValueError, match="pos_dim"):
            fn(X, U, sig)                                          # no default for a user model
        with pytest.raises(ValueError):
            fn(X, U[:, :, :1], sig, pos_dim=2)
        with pytest.raises(ValueError):
            fn(X, U, sig, pos_dim=2, nsub=0)
        with pytest.raises(scvx_hip.ScvxError):                    # host tensors: no CPU fallback
            fn(X, U, sig, pos_dim=2)
    with pytest.raises(ValueError):
        rr.device_model("tiny2").rollout_dense(X[:, :, :2].contiguous(), U[:, :, :1].contiguous(), sig, pos_dim=3)
    with pytest.raises(ValueError, match="pos_dim"):
        scvx_hip.fleet_separation(car, X, U, sig)
    with pytest.raises(ValueError, match="pos_dim"):
        scvx_hip.fleet_obstacle_clearance(car, X, U, sig, [((0.0, 0.0), 1.0)])
    # an empty batch needs no device
    P, L = car.rollout_dense(X[:0], U[:0], sig[:0], S=3, pos_dim=2)
    assert P.shape == (0, 4, 4, 3) and L.shape == (0, 4)
    # built-in defaults are unchanged: the unicycle's 2, else 3 (checked against the state dimension before the device)
    with pytest.raises(ValueError):
        scvx_hip.rollout_dense("si", X, U, sig)
    with pytest.raises(NotImplementedError):
        scvx_hip.rollout_dense(type("Stub", (), {"dims": (4, 2), "nsub": 4})(), X, U, sig, pos_dim=2)


class _NoSolver:
    """A backend for constructing a driver only."""

    def qp_solver(self, spec, N, device):
        return None


def test_driver_accepts_a_device_model_for_the_obstacle_rows():
    import scvx_hip
    from scvx_hip.scvx import JacobiSCvx, ObstacleRowsSpec
    X, U, sig = orf.fixture()
    obs = orf.FIXTURE["obs"]
    dm = rr.retraced("di")

    def mk(model):
        return JacobiSCvx(scvx_hip.QPSpec(model=model, K=8, j_max=4, obs=obs), _T(X[:, 0]), _T(X[:, -1]), _T(sig), 4.0,
                          backend=_NoSolver(), obstacle_rows=ObstacleRowsSpec())

    drv = mk(dm)
    assert drv._ob is not None and drv._ob["S"] == 8 and drv._ob["j_node"] == 0 and drv._ob["obstacles"] == list(obs)
    assert drv.rows.shape == (1, 8, 4, 4)

    class UserModel:   # a model object without a dense roll-out
        dims, nsub = (6, 3), 4

    with pytest.raises(NotImplementedError, match="built-in"):
        mk(UserModel())


@functools.lru_cache(maxsize=None)
def _head_on_iterate():
    X, U, sig, _, _ = ir.run_head_on(_T, CpuBackend(), True)
    return X, U, sig


def test_row_record_fixture_has_margins():
    """The GPU row-record test compares counts exactly and records to 1e-12 between two roll-outs that differ by
    rounding: on the restatement, at the fixture's final iterate, no decision of either selection is within 1e-9 of
    turning over (rtc_rollout_ref.row_margins), and both selections keep something and drop something."""
    X, U, sig = _head_on_iterate()
    n_pair, n_obs = rr.row_margins(X, U, sig)
    print(f"pair records per (agent, segment):\n{n_pair}\nobstacle records:\n{n_obs}")
    assert n_pair.shape == n_obs.shape == (2, ir.HEAD_ON["K"] - 1)
    assert n_pair.any() and not n_pair.all() and n_obs.any() and not n_obs.all()
