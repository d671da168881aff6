"""Derivative-free extended-precision reference of the discretization stage: foh_kernel, nonlinear_kernel (csrc/foh.hip,
csrc/foh_rtc.hip; bodies in csrc/foh_body.hpp) and rollout_dense_kernel (csrc/separation.hip).

The kernels integrate the forward-sensitivity system with hand-written Jacobian products (Av, Bw, fab of
csrc/models.hpp), and so do the oracles they are compared with elsewhere (oracle/foh_ref.c, oracle/foh_generic.py).
This file needs only f.  RK4 applied to the sensitivity system is the exact derivative of the RK4 step map, so with
    g(x_k, u_k, u_k+1, sigma) = the state after nsub classical RK4 steps of x' = sigma f(x, u_k + (t/dt)(u_k+1 - u_k))
                                on [0, dt], dt = 1/(K-1)
the kernel's outputs are, exactly,
    A_k = dg/dx_k,  B_k = dg/du_k,  C_k = dg/du_k+1,  S_k = dg/dsigma,
    z_k = g - A_k x_k - B_k u_k - C_k u_k+1 - sigma S_k
(the last line: e = Phi x_k + P_B u_k + P_C u_k+1 + sigma P_S + P_z - x(t) of foh_body.hpp's columns obeys
e' = sigma A e, e(0) = 0 through every RK4 stage).  g is evaluated in np.clongdouble and each derivative is one complex
step of 1e-40, imag(g(. + 1e-40j .)) / 1e-40: every f here is analytic (sin, cos, +, *, /) and the step's truncation
error, 1e-80 relative, is far below the 64-bit mantissa.

Plain numpy, np.longdouble / np.clongdouble throughout, vectorised over a leading batch axis; imports neither the
package's kernels nor oracle/."""
import numpy as np

LD, CLD = np.longdouble, np.clongdouble
STEP = LD("1e-40")
DIMS = {"di": (6, 3), "unicycle": (3, 2), "si": (3, 3), "quad": (12, 4), "cartpole": (4, 1)}
QUAD_DEFAULT = (1.0, 9.81, 0.02, 0.02, 0.04)          # mass, g, Jx, Jy, Jz (csrc/models.hpp model_params)
CARTPOLE_DEFAULT = (1.0, 0.2, 0.5, 9.81)              # mc, mp, l, g (tests/custom_models.CartPole.params)


def disc_stride(model):
    n, m = DIMS[model]
    return n * (n + 2 * m + 2)


def _params(model, params):
    if params is None:
        params = {"quad": QUAD_DEFAULT, "cartpole": CARTPOLE_DEFAULT}.get(model, ())
    return [LD(float(p)) for p in params]


def f(model, x, u, params=None):
    """x (..., n), u (..., m), real or complex extended precision -> dx/dt (..., n) of the same type."""
    x, u = np.asarray(x), np.asarray(u)
    o = np.zeros(x.shape, dtype=np.result_type(x.dtype, u.dtype, LD))
    if model == "di":
        o[..., 0:3] = x[..., 3:6]
        o[..., 3:6] = u
    elif model == "si":
        o[...] = u
    elif model == "unicycle":
        o[..., 0] = u[..., 0] * np.cos(x[..., 2])
        o[..., 1] = u[..., 0] * np.sin(x[..., 2])
        o[..., 2] = u[..., 1]
    elif model == "quad":
        mass, g, Jx, Jy, Jz = _params(model, params)
        phi, th, psi = x[..., 6], x[..., 7], x[..., 8]
        p, q, r = x[..., 9], x[..., 10], x[..., 11]
        acc = u[..., 0] / mass
        o[..., 0:3] = x[..., 3:6]
        o[..., 3] = acc * (np.cos(phi) * np.sin(th) * np.cos(psi) + np.sin(phi) * np.sin(psi))
        o[..., 4] = acc * (np.cos(phi) * np.sin(th) * np.sin(psi) - np.sin(phi) * np.cos(psi))
        o[..., 5] = acc * np.cos(phi) * np.cos(th) - g
        o[..., 6] = p + (q * np.sin(phi) + r * np.cos(phi)) * np.sin(th) / np.cos(th)
        o[..., 7] = q * np.cos(phi) - r * np.sin(phi)
        o[..., 8] = (q * np.sin(phi) + r * np.cos(phi)) / np.cos(th)
        o[..., 9] = (u[..., 1] + (Jy - Jz) * q * r) / Jx
        o[..., 10] = (u[..., 2] + (Jz - Jx) * p * r) / Jy
        o[..., 11] = (u[..., 3] + (Jx - Jy) * p * q) / Jz
    elif model == "cartpole":
        mc, mp, ell, g = _params(model, params)
        s, c, w, F = np.sin(x[..., 1]), np.cos(x[..., 1]), x[..., 3], u[..., 0]
        den = mc + mp * s * s
        o[..., 0] = x[..., 2]
        o[..., 1] = w
        o[..., 2] = (F + mp * s * (ell * w * w + g * c)) / den
        o[..., 3] = (-F * c - mp * ell * w * w * c * s - (mc + mp) * g * s) / (ell * den)
    else:
        raise KeyError(model)
    return o


def _rk4(fn, x, t, h, watch=None):
    """One classical RK4 step of x' = fn(t, x) from t; watch(x_stage) sees the state of each of the four stages."""
    half = LD(0.5)
    k1 = fn(t, x)
    x2 = x + half * h * k1
    k2 = fn(t + half * h, x2)
    x3 = x + half * h * k2
    k3 = fn(t + half * h, x3)
    x4 = x + h * k3
    k4 = fn(t + h, x4)
    if watch is not None:
        for xs in (x, x2, x3, x4):
            watch(xs)
    return x + h / LD(6) * (k1 + LD(2) * k2 + LD(2) * k3 + k4)


def step_map(model, x0, u0, u1, sigma, K, nsub, params=None, watch=None):
    """g of the module docstring for a batch: x0 (B, n), u0, u1 (B, m), sigma (B,) -> (B, n)."""
    dt = LD(1) / LD(K - 1)
    h = dt / LD(nsub)
    sg = np.asarray(sigma)[..., None]
    du = u1 - u0
    fn = lambda t, x: sg * f(model, x, u0 + (t / dt) * du, params)  # noqa: E731
    x = x0
    for s in range(nsub):
        x = _rk4(fn, x, LD(s) * h, h, watch)
    return x


def _ld(a):
    return np.asarray(a, dtype=np.float64).astype(LD)


def foh_disc(model, X, U, sigma, nsub, params=None, watch=None):
    """X (N,K,n), U (N,K,m), sigma (N,) -> (N, K-1, n(n+2m+2)) np.longdouble in include/scvx_hip.h's layout, per
    (agent, interval) vec_F(A) | vec_F(B) | vec_F(C) | S | z.  watch: see _rk4 (the unperturbed evaluation only)."""
    n, m = DIMS[model]
    X, U, sigma = _ld(X), _ld(U), _ld(sigma)
    N, K = X.shape[:2]
    B = N * (K - 1)
    x0 = X[:, :-1].reshape(B, n)
    u0, u1 = U[:, :-1].reshape(B, m), U[:, 1:].reshape(B, m)
    sg = np.repeat(sigma, K - 1)
    g = step_map(model, x0, u0, u1, sg, K, nsub, params, watch)
    D = n + 2 * m + 1
    # direction d perturbs x_k[d] | u_k[d - n] | u_k+1[d - n - m] | sigma: one batch of D * B complex evaluations
    xc = np.broadcast_to(x0.astype(CLD), (D, B, n)).copy()
    u0c = np.broadcast_to(u0.astype(CLD), (D, B, m)).copy()
    u1c = np.broadcast_to(u1.astype(CLD), (D, B, m)).copy()
    sc = np.broadcast_to(sg.astype(CLD), (D, B)).copy()
    ih = CLD(1j) * STEP
    for d in range(n):
        xc[d, :, d] += ih
    for j in range(m):
        u0c[n + j, :, j] += ih
        u1c[n + m + j, :, j] += ih
    sc[n + 2 * m] += ih
    gc = step_map(model, xc, u0c, u1c, sc, K, nsub, params)
    J = gc.imag / STEP                                    # (D, B, n): J[d, b, i] = d g_i / d direction d
    A, Bm, Cm, S = J[:n], J[n:n + m], J[n + m:n + 2 * m], J[n + 2 * m]
    z = (g - np.einsum("dbi,bd->bi", A, x0) - np.einsum("dbi,bd->bi", Bm, u0) - np.einsum("dbi,bd->bi", Cm, u1)
         - sg[:, None] * S)
    cols = np.concatenate([J[:n + 2 * m], S[None], z[None]], axis=0)      # (ncol, B, n)
    return np.ascontiguousarray(cols.transpose(1, 0, 2)).reshape(N, K - 1, (D + 1) * n)


def blocks(model, disc):
    """disc (..., n(n+2m+2)) -> (A (..., n, n), B (..., n, m), C (..., n, m), S (..., n), z (..., n)) as matrices."""
    n, m = DIMS[model]
    c = np.asarray(disc).reshape(disc.shape[:-1] + (n + 2 * m + 2, n))
    mat = lambda a: np.swapaxes(a, -1, -2)  # noqa: E731
    return (mat(c[..., :n, :]), mat(c[..., n:n + m, :]), mat(c[..., n + m:n + 2 * m, :]), c[..., n + 2 * m, :],
            c[..., n + 2 * m + 1, :])


def integrate_nonlinear(model, X, U, sigma, piecewise, nsub, params=None, watch=None):
    """FirstOrderHold.integrate_nonlinear_piecewise (restart at X[:, k]) / _full (chained): physical time, interval
    T = sigma/(K-1), input interpolated by t/T, nsub RK4 steps per interval -> (N, K, n) np.longdouble."""
    X, U, sigma = _ld(X), _ld(U), _ld(sigma)
    N, K = X.shape[:2]
    T = (sigma / LD(K - 1))[:, None]
    h = T / LD(nsub)
    out = np.zeros(X.shape, dtype=LD)
    out[:, 0] = X[:, 0]
    for k in range(K - 1):
        x = X[:, k] if piecewise else out[:, k]
        u0, du = U[:, k], U[:, k + 1] - U[:, k]
        fn = lambda t, xs: f(model, xs, u0 + (t / T) * du, params)  # noqa: E731
        for s in range(nsub):
            x = _rk4(fn, x, LD(s) * h, h, watch)
        out[:, k + 1] = x
    return out


def rollout_dense(model, X, U, sigma, S, nsub, pos_dim, params=None, watch=None):
    """scvx_hip.rollout_dense: every segment restarted at X[:, k] and sampled at s/S of the interval, sub = ceil(nsub/S)
    RK4 steps of h = T / (S sub) between samples -> P (N, K-1, S+1, 3), the first pos_dim states (zeros past them),
    and L (N, K-1), the polyline length of the samples."""
    n, m = DIMS[model]
    X, U, sigma = _ld(X), _ld(U), _ld(sigma)
    N, K = X.shape[:2]
    sub = -(-int(nsub) // int(S))
    T = np.repeat(sigma / LD(K - 1), K - 1)[:, None]
    h = T / LD(S * sub)
    x = X[:, :-1].reshape(-1, n)
    u0 = U[:, :-1].reshape(-1, m)
    du = U[:, 1:].reshape(-1, m) - u0
    fn = lambda t, xs: f(model, xs, u0 + (t / T) * du, params)  # noqa: E731
    P = np.zeros((x.shape[0], S + 1, 3), dtype=LD)
    P[:, 0, :pos_dim] = x[:, :pos_dim]
    for s in range(1, S + 1):
        for i in range(sub):
            x = _rk4(fn, x, LD((s - 1) * sub + i) * h, h, watch)
        P[:, s, :pos_dim] = x[:, :pos_dim]
    L = np.sqrt((np.diff(P, axis=1) ** 2).sum(axis=2)).sum(axis=1)
    return P.reshape(N, K - 1, S + 1, 3), L.reshape(N, K - 1)


class MinAbsCos:
    """A `watch` that records the smallest |cos x[component]| over every RK4 stage it sees (the quadrotor's Euler
    kinematics divide by cos theta, component 7)."""

    def __init__(self, component=7):
        self.component, self.value = component, np.inf

    def __call__(self, x):
        self.value = min(self.value, float(np.abs(np.cos(x[..., self.component].real)).min()))


def rel_blocks(model, got, ref):
    """max |got - ref| / max(1, max |ref|) per block (A, B, C, S, z) over everything in front of the last axis."""
    out = []
    for g, r in zip(blocks(model, np.asarray(got).astype(LD)), blocks(model, ref)):
        out.append(float(np.abs(g - r).max() / max(LD(1), np.abs(r).max())))
    return out


def rel(got, ref):
    ref = np.asarray(ref)
    return float(np.abs(np.asarray(got).astype(LD) - ref).max() / max(LD(1), np.abs(ref).max()))
