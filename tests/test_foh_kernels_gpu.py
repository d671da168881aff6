"""GPU: foh_kernel, nonlinear_kernel (built-in and hipRTC) and rollout_dense_kernel through scvx_hip against the
derivative-free extended-precision reference (tests/foh_ref.py: f alone, complex-step derivatives of the RK4 map) at
the edges of their launches (tests/foh_cases.py, proven on the reference alone by tests/test_foh_ref_cpu.py): one
interval, partial and exactly full last blocks, block edges inside intervals and between agents, both block sizes of
the roll-out, a different sigma per agent, large headings, and a quadrotor whose parameters are not the defaults
(Jx != Jy, so the gyroscopic row of f / Av / fab is not multiplied by zero).

Every agent, interval and element is compared: 1e-12 of max(1, max |ref|), per block (A, B, C, S, z) for the FOH --
the project's figure for the GPU against the same algorithm on the CPU.  Outputs that take `out=` are
the middle of a buffer with one agent's worth of sentinel on either side: the guards keep it, no interior element
does.  The worst error per (kernel, model) is printed."""
import numpy as np
import pytest

import foh_cases as fc
import foh_ref as fr
import scvx_hip
from scvx_hip import workloads

pytestmark = pytest.mark.gpu

TOL = 1e-12
SENTINEL = -7.25e300
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    for (kernel, model), e in sorted(WORST.items()):
        print(f"worst error vs reference, {kernel} {model}: {e:.1e}")


def _note(kernel, model, err):
    WORST[kernel, model] = max(WORST.get((kernel, model), 0.0), err)
    print(f"{kernel} {model}: {err:.2e}")
    return err


def _t(x, cuda):
    import torch
    return torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device=cuda)


def _guarded(cuda, N, tail):
    """(buffer of N + 2 agents filled with the sentinel, its middle N agents)"""
    import torch
    buf = torch.full((N + 2,) + tuple(tail), SENTINEL, dtype=torch.float64, device=cuda)
    return buf, buf[1:N + 1]


def _interior(buf):
    """The middle of a guarded buffer after the launch, once the guards are seen intact and the middle overwritten."""
    b = buf.cpu().numpy()
    assert (b[0] == SENTINEL).all() and (b[-1] == SENTINEL).all(), "a store outside the output"
    assert (b[1:-1] != SENTINEL).all(), "an output element was never stored"
    return b[1:-1]


@pytest.fixture(scope="module")
def cartpole():
    import rollout_bitwise_cases as rbc
    return rbc.device_model()


def _foh(cuda, c, dm=None, guarded=True):
    X, U, sigma = (_t(a, cuda) for a in fc.case_inputs(c))
    buf, out = _guarded(cuda, c.N, (c.K - 1, fr.disc_stride(c.model))) if guarded else (None, None)
    if dm is not None:
        got = dm.foh(X, U, sigma, nsub=c.nsub, out=out)
    else:
        got = scvx_hip.foh_batched(c.model, X, U, sigma, nsub=c.nsub, params=c.params, out=out)
    if not guarded:
        return got.cpu().numpy()
    assert got.data_ptr() == out.data_ptr()
    return _interior(buf)


def _nl(cuda, c, dm=None):
    X, U, sigma = (_t(a, cuda) for a in fc.case_inputs(c))
    buf, out = _guarded(cuda, c.N, (c.K, fr.DIMS[c.model][0]))
    if dm is not None:
        dm.integrate_nonlinear(X, U, sigma, c.piecewise, nsub=c.nsub, out=out)
    else:
        scvx_hip.integrate_nonlinear(c.model, X, U, sigma, c.piecewise, nsub=c.nsub, params=c.params, out=out)
    return _interior(buf)


def _assert_foh(c, got, kernel="foh"):
    ref = fc.reference(c)
    assert got.shape == ref.shape
    err = fr.rel_blocks(c.model, got, ref)
    _note(kernel, c.model, max(err))
    for b, e in zip("ABCSz", err):
        assert e <= TOL, (c.name, b, e)


def _assert_nl(c, got, kernel):
    ref = fc.reference(c)
    assert got.shape == ref.shape
    assert (got[:, 0] == fc.case_inputs(c)[0][:, 0]).all()
    assert _note(kernel, c.model, fr.rel(got, ref)) <= TOL, c.name


@pytest.mark.parametrize("name", list(fc.FOH_CASES))
def test_foh_matches_reference(cuda, name):
    c = fc.FOH_CASES[name]
    _assert_foh(c, _foh(cuda, c))


@pytest.mark.parametrize("model", fc.BUILTIN)
def test_foh_allocates_the_same_result(cuda, model):
    c = fc.FOH_CASES[f"foh/{model}/N7K5/nsub3"]
    assert (_foh(cuda, c, guarded=False) == _foh(cuda, c)).all()


@pytest.mark.parametrize("name", list(fc.NL_CASES))
def test_integrate_nonlinear_matches_reference(cuda, name):
    c = fc.NL_CASES[name]
    _assert_nl(c, _nl(cuda, c), "nonlinear/" + ("piecewise" if c.piecewise else "full"))


@pytest.mark.parametrize("name", list(fc.DENSE_CASES))
def test_rollout_dense_matches_reference(cuda, name):
    c = fc.DENSE_CASES[name]
    Xn, Un, sn = fc.case_inputs(c)
    P, L = scvx_hip.rollout_dense(c.model, _t(Xn, cuda), _t(Un, cuda), _t(sn, cuda), S=c.S, nsub=c.nsub,
                                  pos_dim=c.pos_dim, params=c.params)
    P, L = P.cpu().numpy(), L.cpu().numpy()
    Pr, Lr = fc.reference(c)
    assert P.shape == Pr.shape == (c.N, c.K - 1, c.S + 1, 3) and L.shape == Lr.shape == (c.N, c.K - 1)
    assert np.isfinite(P).all() and np.isfinite(L).all()
    assert (P[:, :, 0, :c.pos_dim] == Xn[:, :-1, :c.pos_dim]).all()
    assert (P[..., c.pos_dim:] == 0).all()
    assert _note("rollout_dense/P", c.model, fr.rel(P, Pr)) <= TOL, name
    assert _note("rollout_dense/L", c.model, fr.rel(L, Lr)) <= TOL, name


@pytest.mark.parametrize("name", list(fc.RTC_CASES))
def test_cartpole_through_hiprtc_matches_reference(cuda, cartpole, name):
    c = fc.RTC_CASES[name]
    if c.kind == "foh":
        _assert_foh(c, _foh(cuda, c, cartpole), "rtc foh")
    else:
        _assert_nl(c, _nl(cuda, c, cartpole), "rtc nonlinear/piecewise")


def _identity(cuda, model, sc, nsub, params):
    """max over every agent and interval of |A x_k + B u_k + C u_k+1 + sigma S + z - piecewise roll-out[k+1]| over the
    state scale: the FOH's own linearisation evaluated at its expansion point is the nonlinear step"""
    X, U, sigma = (_t(sc[k], cuda) for k in ("X", "U", "sigma"))
    disc = scvx_hip.foh_batched(model, X, U, sigma, nsub=nsub, params=params).cpu().numpy()
    nl = scvx_hip.integrate_nonlinear(model, X, U, sigma, True, nsub=nsub, params=params).cpu().numpy()
    A, B, C, S, z = fr.blocks(model, disc)
    Xn, Un, sn = sc["X"], sc["U"], sc["sigma"]
    pred = (np.einsum("akij,akj->aki", A, Xn[:, :-1]) + np.einsum("akij,akj->aki", B, Un[:, :-1])
            + np.einsum("akij,akj->aki", C, Un[:, 1:]) + sn[:, None, None] * S + z)
    assert np.isfinite(pred).all()
    return float(np.abs(pred - nl[:, 1:]).max() / max(1.0, np.abs(nl).max()))


def test_identity_with_the_rollout_at_the_bench_size_di(cuda):
    sc = workloads.synthetic_di(1024, K=50, seed=1, sigma=30.0)
    assert _note("foh = nonlinear identity", "di", _identity(cuda, "di", sc, 1, None)) <= TOL


def test_identity_with_the_rollout_quad(cuda):
    mass, g = fc.QUAD_CUSTOM[:2]
    sc = workloads.synthetic_quad(64, K=50, mass=mass, g=g)
    assert _note("foh = nonlinear identity", "quad", _identity(cuda, "quad", sc, 10, fc.QUAD_CUSTOM)) <= TOL


# ---- argument checks: through the wrappers, an exception and never a launch ---------------------------------------

def _entry_points(cartpole):
    return {
        "foh": (lambda X, U, s, **kw: scvx_hip.foh_batched("di", X, U, s, **kw), 6, 3),
        "nl": (lambda X, U, s, **kw: scvx_hip.integrate_nonlinear("di", X, U, s, True, **kw), 6, 3),
        "dense": (lambda X, U, s, **kw: scvx_hip.rollout_dense("di", X, U, s, **kw), 6, 3),
        "rtc_foh": (lambda X, U, s, **kw: cartpole.foh(X, U, s, **kw), 4, 1),
        "rtc_nl": (lambda X, U, s, **kw: cartpole.integrate_nonlinear(X, U, s, True, **kw), 4, 1),
    }


@pytest.mark.parametrize("entry", ["foh", "nl", "dense", "rtc_foh", "rtc_nl"])
def test_argument_checks(cuda, cartpole, entry):
    import torch
    fn, n, m = _entry_points(cartpole)[entry]
    z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=cuda)  # noqa: E731
    sig = torch.ones(2, dtype=torch.float64, device=cuda)
    bad = (ValueError, scvx_hip.ScvxError)
    with pytest.raises(bad):
        fn(z(2, 1, n), z(2, 1, m), sig)                                  # K = 1
    with pytest.raises(bad):
        fn(z(2, 4, n), z(2, 4, m), sig, nsub=0)
    with pytest.raises(bad):
        fn(z(2, 4, n), z(2, 4, m), sig, nsub=-1)
    with pytest.raises(ValueError):
        fn(z(2, 4, n), z(2, 4, m + 1), sig)                              # U of the wrong m
    with pytest.raises(ValueError):
        fn(z(2, n, 4).transpose(1, 2), z(2, 4, m), sig)                  # X (2, 4, n), not contiguous
    out = fn(z(0, 4, n), z(0, 4, m), sig[:0])                            # N = 0: empty, no launch
    if entry == "dense":
        assert tuple(out[0].shape) == (0, 3, 9, 3) and tuple(out[1].shape) == (0, 3)
    elif entry.endswith("foh"):
        assert tuple(out.shape) == (0, 3, n * (n + 2 * m + 2))
    else:
        assert tuple(out.shape) == (0, 4, n)
    torch.cuda.synchronize()
