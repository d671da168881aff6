"""GPU: the kernels that advance a state by the FOH-input RK4 step -- integrate_nonlinear (nonlinear_body),
rollout_dense (rollout_dense_kernel) and intersample_batched (intersample_body's h) -- after their three copies of
the step became one function (csrc/foh_body.hpp rk4_step), against goldens recorded with the build before that
change (tests/golden/rollout_parent.npz, written by tests/golden/make_rollout_parent_goldens.py on an MI355X).

The step's expressions are the copies' own, term for term, so every output is required to be equal bit for bit
(np.array_equal): the four built-in models and a runtime-compiled user model (CartPole), 5 agents x 3 segments and
a single segment.  foh_batched, whose augmented RK4 is a different system and was not touched, is a guard.  The
fixtures and what is recorded of them: tests/rollout_bitwise_cases.py."""
import os

import numpy as np
import pytest

import rollout_bitwise_cases as rc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rollout_parent.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as d:
        return {k: d[k] for k in d.files}


@pytest.mark.parametrize("shape", rc.SHAPES, ids=lambda s: f"N{s[0]}K{s[1]}")
@pytest.mark.parametrize("model", rc.MODELS)
def test_outputs_bitwise_equal_parent(cuda, golden, model, shape):
    N, K = shape
    got = rc.run(cuda, model, N, K)
    gold = golden[rc.key(model, N, K)]
    assert gold.size == sum(v.size for v in got.values()), (gold.size, {k: v.shape for k, v in got.items()})
    assert got["is/n_crit"].sum() > 0   # the scan's bisection and gradients ran
    off, bad = 0, []
    for name in sorted(got):
        v = got[name].astype(np.float64).ravel()
        g = gold[off:off + v.size]
        off += v.size
        eq = np.array_equal(v, g)
        first = ""
        if not eq:
            i = int(np.flatnonzero(v != g)[0])
            first = f": first difference at [{i}] {v[i]!r} (parent {g[i]!r}), {int((v != g).sum())} of {v.size} differ"
            bad.append(name)
        print(f"{model} N={N} K={K} {name}: bitwise equal {eq}{first}")
    assert not bad, (model, N, K, bad)
