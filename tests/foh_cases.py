"""Fixtures of the discretization-stage reference tests (tests/test_foh_kernels_gpu.py), shared with the CPU test that
proves their conditions on the reference alone (tests/test_foh_ref_cpu.py).

Every shape is the smallest that reaches one mechanism of the launch.  foh_kernel has one lane per
(agent, interval, column) in 256-lane blocks, ncol = n + 2m + 2 columns per interval (NCOL):
    (1, 2)     one interval: ncol live lanes, the rest of the block dead (the clamp tidc = total - 1)
    (7, 5)     28 ncol lanes: a partial last block, block edges inside intervals and between agents; two or three
               blocks for di / si / quad.  The unicycle's 252 lanes fit one block, so it also runs (8, 5): 288
    (16, 17)   256 ncol lanes: the last block exactly full, `lim` of the LDS-staged store exactly 256 n
nonlinear_kernel: (7, 38) piecewise is 259 lanes of a 256-block, (65, 4) full 65 lanes of a 64-block;
rollout_dense_kernel: (13, 6) is 65 lanes of a 64-block.  CartPole through hipRTC has ncol = 8: every block of
(16, 17) is exactly full.

Inputs.  A different sigma per agent, 0.1 .. 30 for di / si / unicycle.  Unicycle headings in +-20 rad (the range
reduction of sincos).  The quadrotor runs with parameters that are not the defaults and Jx != Jy != Jz (QUAD_CUSTOM;
with the default Jx == Jy the gyroscopic coefficient (Jx - Jy) / Jz is exactly 0), intervals sigma/(K-1) of
0.05 .. 0.4, attitudes uniform in +-0.6 rad, body rates N(0, 0.2), thrust mass g + N(0, 0.5), torques N(0, 0.004):
the reference stays at scale ~10 and far from the Euler singularity.  One more quadrotor case runs the defaults."""
import functools
from collections import namedtuple

import numpy as np

import foh_ref as fr

SEED = 9318      # one at which the single-interval quadrotor fixture has both body rates p, q well away from zero
QUAD_CUSTOM = (0.8, 3.71, 0.015, 0.03, 0.05)      # mass, g, Jx, Jy, Jz
BUILTIN = ("di", "unicycle", "si", "quad")
MODELS = BUILTIN + ("cartpole",)
NCOL = {mdl: n + 2 * m + 2 for mdl, (n, m) in fr.DIMS.items()}
FOH_SHAPES = ((1, 2), (7, 5), (16, 17))
FOH_EXTRA_SHAPES = {"unicycle": ((8, 5),)}
FOH_NSUB = (1, 3)
FOH_MODEL_NSUB = {"unicycle": 16, "quad": 10}    # at (7, 5)
NL_SHAPES = ((1, 2, True), (1, 2, False), (7, 38, True), (65, 4, False))   # (N, K, piecewise)
NL_NSUB = (1, 3, 16)
DENSE_SHAPES = ((1, 2), (13, 6))
DENSE_STEPS = ((1, 1), (5, 7), (16, 16), (16, 3))                          # (S, nsub): sub = 1, 2, 1, 1
DENSE_MODELS = (("di", 1), ("di", 2), ("di", 3), ("unicycle", 2), ("quad", 3))   # (model, pos_dim)
RTC_SHAPES = ((1, 2), (16, 17))
RTC_NSUB = 3

# kind: "foh" | "nl" | "dense"; nsub None: the wrapper's default; params: None (the model's defaults) or a tuple;
# piecewise for "nl"; S, pos_dim for "dense"
Case = namedtuple("Case", "name kind model N K nsub params piecewise S pos_dim", defaults=(None, None, None))


def model_params(model, default=False):
    return QUAD_CUSTOM if model == "quad" and not default else None


@functools.lru_cache(maxsize=None)
def inputs(model, N, K, default_params=False):
    """X (N,K,n), U (N,K,m), sigma (N,), read-only float64"""
    n, m = fr.DIMS[model]
    rng = np.random.default_rng([SEED, MODELS.index(model), N, K, int(default_params)])
    X = rng.normal(0.0, 0.5, (N, K, n))
    U = rng.normal(0.0, 0.4, (N, K, m))
    sigma = np.exp(rng.uniform(np.log(0.1), np.log(30.0), N))
    if model == "unicycle":
        X[:, :, 2] = rng.uniform(-20.0, 20.0, (N, K))
    elif model == "quad":
        mass, g = (fr.QUAD_DEFAULT if default_params else QUAD_CUSTOM)[:2]
        X[:, :, 0:3] = rng.normal(0.0, 2.0, (N, K, 3))
        X[:, :, 6:9] = rng.uniform(-0.6, 0.6, (N, K, 3))
        X[:, :, 9:12] = rng.normal(0.0, 0.2, (N, K, 3))
        U[:, :, 0] = mass * g + rng.normal(0.0, 0.5, (N, K))
        U[:, :, 1:] = rng.normal(0.0, 0.004, (N, K, 3))
        sigma = (K - 1) * rng.uniform(0.05, 0.4, N)
    elif model == "cartpole":
        X[:, :, 1] = rng.uniform(-1.0, 1.0, (N, K))
        sigma = rng.uniform(0.3, 1.5, N)
    for a in (X, U, sigma):
        a.setflags(write=False)
    return X, U, sigma


def case_inputs(c):
    return inputs(c.model, c.N, c.K, c.model == "quad" and c.params is None)


def _tag(nsub, params, model):
    return f"nsub{'_default' if nsub is None else nsub}" + ("/default_params" if model == "quad" and params is None
                                                            else "")


def foh_cases():
    out = []
    for mdl in BUILTIN:
        p = model_params(mdl)
        for N, K in FOH_SHAPES + FOH_EXTRA_SHAPES.get(mdl, ()):
            out += [Case(f"foh/{mdl}/N{N}K{K}/{_tag(ns, p, mdl)}", "foh", mdl, N, K, ns, p) for ns in FOH_NSUB]
        extra = ((FOH_MODEL_NSUB[mdl],) if mdl in FOH_MODEL_NSUB else ()) + (None,)
        out += [Case(f"foh/{mdl}/N7K5/{_tag(ns, p, mdl)}", "foh", mdl, 7, 5, ns, p) for ns in extra]
    out.append(Case(f"foh/quad/N7K5/{_tag(3, None, 'quad')}", "foh", "quad", 7, 5, 3, None))
    return out


def nl_cases():
    return [Case(f"nl/{mdl}/N{N}K{K}/{'pw' if pw else 'full'}/nsub{ns}", "nl", mdl, N, K, ns, model_params(mdl), pw)
            for mdl in BUILTIN for N, K, pw in NL_SHAPES for ns in NL_NSUB]


def dense_cases():
    return [Case(f"dense/{mdl}/pd{pd}/N{N}K{K}/S{S}nsub{ns}", "dense", mdl, N, K, ns, model_params(mdl), None, S, pd)
            for mdl, pd in DENSE_MODELS for N, K in DENSE_SHAPES for S, ns in DENSE_STEPS]


def rtc_cases():
    out = []
    for N, K in RTC_SHAPES:
        out.append(Case(f"foh/cartpole/N{N}K{K}/nsub{RTC_NSUB}", "foh", "cartpole", N, K, RTC_NSUB, None))
        out.append(Case(f"nl/cartpole/N{N}K{K}/pw/nsub{RTC_NSUB}", "nl", "cartpole", N, K, RTC_NSUB, None, True))
    return out


FOH_CASES = {c.name: c for c in foh_cases()}
NL_CASES = {c.name: c for c in nl_cases()}
DENSE_CASES = {c.name: c for c in dense_cases()}
RTC_CASES = {c.name: c for c in rtc_cases()}
CASES = {**FOH_CASES, **NL_CASES, **DENSE_CASES, **RTC_CASES}


def lanes(c):
    """Live lanes of the case's launch."""
    if c.kind == "foh":
        return c.N * (c.K - 1) * NCOL[c.model]
    return c.N if c.kind == "nl" and not c.piecewise else c.N * (c.K - 1)


def block(c):
    """Lanes per block of the case's launch (csrc/foh.hip launch_foh / launch_nl, csrc/separation.hip)."""
    return 256 if c.kind == "foh" or (c.kind == "nl" and c.piecewise) else 64


def resolved_nsub(c):
    """The substeps the wrapper runs: the case's, or the package's default for the batch's longest interval."""
    if c.nsub is not None:
        return c.nsub
    import scvx_hip
    return scvx_hip.default_nsub(c.model, float(case_inputs(c)[2].max()), c.K)


@functools.lru_cache(maxsize=None)
def _reference(name):
    c = CASES[name]
    X, U, sigma = case_inputs(c)
    watch = fr.MinAbsCos() if c.model == "quad" else None
    if c.kind == "foh":
        ref = fr.foh_disc(c.model, X, U, sigma, resolved_nsub(c), c.params, watch)
    elif c.kind == "nl":
        ref = fr.integrate_nonlinear(c.model, X, U, sigma, c.piecewise, c.nsub, c.params, watch)
    else:
        ref = fr.rollout_dense(c.model, X, U, sigma, c.S, c.nsub, c.pos_dim, c.params, watch)
    for a in (ref if isinstance(ref, tuple) else (ref,)):
        a.setflags(write=False)
    return ref, (watch.value if watch else None)


def reference(c):
    """The case's reference (foh: disc; nl: Xout; dense: (P, L)), np.longdouble, computed once per session."""
    return _reference(c.name)[0]


def min_abs_cos_theta(c):
    """Smallest |cos theta| over every RK4 stage of a quadrotor case's reference."""
    return _reference(c.name)[1]
