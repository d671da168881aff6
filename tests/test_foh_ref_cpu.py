"""CPU: the derivative-free reference of the discretization stage (tests/foh_ref.py) and the fixtures of
tests/test_foh_kernels_gpu.py (tests/foh_cases.py), proven without a GPU.

  * the reference against the restatements of the kernels' algorithm, oracle/foh_ref.c (built-in models) and
    oracle/foh_generic.py (CartPole with custom_models.CartPole's lambdified f, A, B), on every fixture, to 1e-13 of
    max(1, max |ref|) per block: the complex-step derivative of the RK4 map and the RK4 of the sensitivity system are
    the same numbers;
  * the hand-written f against the models it restates;
  * the fixture conditions: finite, scale <= 1e3, the quadrotor away from the Euler singularity at every RK4 stage,
    the gyroscopic coefficients and the Jacobian entries they feed well away from zero, the lane counts;
  * closed forms of the two linear models."""
import numpy as np
import pytest

import custom_models as cm
import foh_cases as fc
import foh_ref as fr
from oracle import foh_generic, foh_oracle, models_np

ORACLE_TOL = 1e-13
BLOCKS = ("A", "B", "C", "S", "z")


@pytest.fixture(scope="module")
def cartpole():
    return cm.CartPole()


def _oracle_disc(c, nsub, cartpole):
    X, U, sigma = fc.case_inputs(c)
    if c.model != "cartpole":
        return np.stack([foh_oracle.foh_disc(c.model, X[a], U[a], sigma[a], nsub, c.params) for a in range(c.N)])
    f, A, B = cartpole.get_equations()
    n, m = fr.DIMS[c.model]
    out = np.zeros((c.N, c.K - 1, fr.disc_stride(c.model)))
    for a in range(c.N):
        parts = foh_generic.foh(f, A, B, n, m, X[a].T, U[a].T, sigma[a], nsub)
        out[a] = np.concatenate([p.T for p in parts], axis=1)
    return out


def _oracle_nl(c, cartpole):
    X, U, sigma = fc.case_inputs(c)
    if c.model != "cartpole":
        return np.stack([foh_oracle.integrate_nonlinear(c.model, X[a].T, U[a].T, sigma[a], c.piecewise, c.nsub,
                                                        c.params).T for a in range(c.N)])
    f = cartpole.get_equations()[0]
    return np.stack([foh_generic.integrate_nonlinear(f, 4, X[a].T, U[a].T, sigma[a], c.piecewise, c.nsub).T
                     for a in range(c.N)])


@pytest.mark.parametrize("model", fc.MODELS)
def test_foh_reference_matches_the_oracle(model, cartpole):
    cases = [c for c in list(fc.FOH_CASES.values()) + list(fc.RTC_CASES.values()) if c.kind == "foh" and c.model == model]
    assert cases
    if model == "quad":
        assert {c.params for c in cases} == {fc.QUAD_CUSTOM, None}
    worst = dict.fromkeys(BLOCKS, 0.0)
    for c in cases:
        err = fr.rel_blocks(model, _oracle_disc(c, fc.resolved_nsub(c), cartpole), fc.reference(c))
        for b, e in zip(BLOCKS, err):
            worst[b] = max(worst[b], e)
            assert e <= ORACLE_TOL, (c.name, b, e)
    print(f"foh reference vs oracle, {model}: " + ", ".join(f"{b} {e:.1e}" for b, e in worst.items()))


@pytest.mark.parametrize("model", fc.MODELS)
def test_rollout_reference_matches_the_oracle(model, cartpole):
    cases = [c for c in list(fc.NL_CASES.values()) + list(fc.RTC_CASES.values()) if c.kind == "nl" and c.model == model]
    assert cases
    worst = 0.0
    for c in cases:
        e = fr.rel(_oracle_nl(c, cartpole), fc.reference(c))
        worst = max(worst, e)
        assert e <= ORACLE_TOL, (c.name, e)
    print(f"roll-out reference vs oracle, {model}: {worst:.1e}")


def test_dense_reference_is_the_piecewise_rollout_at_the_nodes():
    """sample S of rollout_dense after S sub steps is integrate_nonlinear(piecewise) with nsub = S sub; sample 0 is the
    node; nothing past pos_dim"""
    for c in fc.DENSE_CASES.values():
        X, U, sigma = fc.case_inputs(c)
        P, L = fc.reference(c)
        sub = -(-c.nsub // c.S)
        nl = fr.integrate_nonlinear(c.model, X, U, sigma, True, c.S * sub, c.params)
        assert fr.rel(P[:, :, c.S, :c.pos_dim], nl[:, 1:, :c.pos_dim]) <= 1e-17, c.name
        assert (P[:, :, 0, :c.pos_dim] == X[:, :-1, :c.pos_dim]).all()
        assert (P[..., c.pos_dim:] == 0).all()
        chord = np.sqrt(((P[:, :, -1] - P[:, :, 0]) ** 2).sum(axis=-1))
        assert (L >= chord * (1 - 1e-15)).all()
    assert sorted({-(-c.nsub // c.S) for c in fc.DENSE_CASES.values()}) == [1, 2]
    assert any(c.nsub < c.S for c in fc.DENSE_CASES.values())
    assert any(c.nsub > c.S and c.nsub % c.S for c in fc.DENSE_CASES.values())


def test_handwritten_f_matches_the_models(cartpole):
    rng = np.random.default_rng(fc.SEED)
    f_cart = cartpole.get_equations()[0]
    for params in (fc.QUAD_CUSTOM, fr.QUAD_DEFAULT):
        f_quad = models_np.quad_equations(*params)[0]
        for _ in range(50):
            x, u = rng.normal(0.0, 0.5, 12), rng.normal(0.0, 1.0, 4) + np.array([8.0, 0, 0, 0])
            want = f_quad(x, u)
            got = fr.f("quad", x.astype(fr.LD), u.astype(fr.LD), params)
            assert np.abs(got - want).max() <= 1e-15 * max(1.0, np.abs(want).max())
    for _ in range(50):
        x, u = rng.normal(0.0, 1.0, 4), rng.normal(0.0, 1.0, 1)
        want = np.asarray(f_cart(x, u), float).reshape(4)
        got = fr.f("cartpole", x.astype(fr.LD), u.astype(fr.LD))
        assert np.abs(got - want).max() <= 1e-15 * max(1.0, np.abs(want).max())
    assert tuple(cartpole.params.values()) == fr.CARTPOLE_DEFAULT
    assert tuple(models_np.QUAD_DEFAULT.values()) == fr.QUAD_DEFAULT


@pytest.mark.parametrize("name", list(fc.CASES))
def test_fixture_is_finite_and_tame(name):
    c = fc.CASES[name]
    ref = fc.reference(c)
    for a in (ref if isinstance(ref, tuple) else (ref,)):
        assert np.isfinite(a).all()
        assert np.abs(a).max() <= 1e3
    if c.model == "quad":
        assert fc.min_abs_cos_theta(c) >= 0.3


def test_quadrotor_fixtures_excite_the_gyroscopic_terms():
    mass, g, Jx, Jy, Jz = fc.QUAD_CUSTOM
    assert min(abs((Jx - Jy) / Jz), abs((Jy - Jz) / Jx), abs((Jz - Jx) / Jy)) >= 0.1
    assert fc.QUAD_CUSTOM != fr.QUAD_DEFAULT and mass != 1.0 and g != 9.81
    for c in fc.FOH_CASES.values():
        if c.model == "quad" and c.params is not None:
            A = fr.blocks("quad", fc.reference(c))[0]
            assert np.abs(A[..., 11, 9]).max() >= 1e-3 and np.abs(A[..., 11, 10]).max() >= 1e-3, c.name
    X = np.concatenate([fc.case_inputs(c)[0][:, :, 2].ravel() for c in fc.FOH_CASES.values() if c.model == "unicycle"])
    assert X.min() < -15 and X.max() > 15 and np.abs(X).max() <= 20


def test_sigma_differs_per_agent():
    for c in fc.CASES.values():
        sigma = fc.case_inputs(c)[2]
        assert np.unique(sigma).size == c.N
        T = sigma / (c.K - 1)
        if c.model == "quad":
            assert 0.05 <= T.min() and T.max() <= 0.4
        elif c.model != "cartpole":
            assert 0.1 <= sigma.min() and sigma.max() <= 30.0


def test_lane_counts():
    for mdl in fc.BUILTIN:
        by_shape = {(c.N, c.K): fc.lanes(c) for c in fc.FOH_CASES.values() if c.model == mdl}
        assert by_shape[1, 2] == fc.NCOL[mdl] < 256
        assert by_shape[7, 5] % 256 != 0
        assert any(v % 256 != 0 and v > 256 for v in by_shape.values()), mdl     # a partial last block of several
        assert by_shape[16, 17] % 256 == 0 and by_shape[16, 17] // 256 == fc.NCOL[mdl]
    assert fc.NCOL == {"di": 14, "unicycle": 9, "si": 11, "quad": 22, "cartpole": 8}
    for c in fc.RTC_CASES.values():
        if c.kind == "foh" and c.N == 16:
            assert fc.lanes(c) % 256 == 0
    nl = {(c.N, c.K, c.piecewise): (fc.lanes(c), fc.block(c)) for c in fc.NL_CASES.values()}
    assert nl[7, 38, True] == (259, 256) and nl[65, 4, False] == (65, 64)
    assert nl[1, 2, True] == (1, 256) and nl[1, 2, False] == (1, 64)
    dense = {(c.N, c.K): (fc.lanes(c), fc.block(c)) for c in fc.DENSE_CASES.values()}
    assert dense == {(1, 2): (1, 64), (13, 6): (65, 64)}


def test_nsub_coverage():
    import scvx_hip
    for mdl in fc.BUILTIN:
        ns = {c.nsub for c in fc.FOH_CASES.values() if c.model == mdl}
        assert {1, 3, None} <= ns
        for c in fc.FOH_CASES.values():
            if c.model == mdl and c.nsub is None:
                assert fc.resolved_nsub(c) >= scvx_hip.DEFAULT_NSUB[mdl]
    assert 16 in {c.nsub for c in fc.FOH_CASES.values() if c.model == "unicycle"}
    assert 10 in {c.nsub for c in fc.FOH_CASES.values() if c.model == "quad"}


@pytest.mark.parametrize("model", ["di", "si"])
def test_closed_forms(model):
    """di: A = [[I, hI], [0, I]], B + C = [h^2/2 I; h I], C = [h^2/6 I; h/2 I]; si: A = I, B = C = h/2 I;
    sigma S + z = 0 for both (f is linear and homogeneous in (x, u)); h = sigma / (K - 1)"""
    I3, Z3 = np.eye(3, dtype=fr.LD), np.zeros((3, 3), dtype=fr.LD)
    for c in fc.FOH_CASES.values():
        if c.model != model:
            continue
        sigma = fc.case_inputs(c)[2].astype(fr.LD)
        A, B, C, S, z = fr.blocks(model, fc.reference(c))
        h = np.broadcast_to((sigma / fr.LD(c.K - 1))[:, None, None, None], A.shape[:2] + (1, 1))
        if model == "di":
            wantA = np.block([[I3 + 0 * h, h * I3], [Z3 + 0 * h, I3 + 0 * h]])
            wantBC = np.concatenate([h * h / 2 * I3, h * I3], axis=-2)
            wantC = np.concatenate([h * h / 6 * I3, h / 2 * I3], axis=-2)
        else:
            wantA, wantBC, wantC = I3 + 0 * h, h * I3, h / 2 * I3
        for got, want in ((A, wantA), (B + C, wantBC), (C, wantC)):
            assert np.abs(got - want).max() <= 1e-15 * max(1, np.abs(want).max()), c.name
        resid = sigma[:, None, None] * S + z
        assert np.abs(resid).max() <= 1e-15 * max(1, np.abs(z).max()), c.name
