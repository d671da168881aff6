"""The conditions the fixture of tests/test_pair_scan_bitwise_gpu.py must meet (tests/pair_scan_cases.py), asserted on
the numpy restatement of the two kernels without a device, on the samples the golden file holds."""
import os

import numpy as np
import pytest

import intersample_rows_ref as ir
import pair_scan_cases as pc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pair_scan_parent.npz")


@pytest.fixture(scope="module")
def P16():
    with np.load(GOLDEN) as d:
        return d["P16"]


def test_golden_holds_the_generators_samples(P16):
    mine = pc.make_p16()
    assert P16.shape == mine.shape == (pc.N, pc.K - 1, 17, 3) and P16.dtype == np.float64
    assert np.abs(P16 - mine).max() <= 1e-12 * np.abs(mine).max()        # another numpy build may round differently
    assert np.array_equal(P16[pc.TWIN], P16[pc.TWIN_OF])
    assert pc.N > 64 and pc.N % 64 == 6 and pc.N % 32 == 6                # a second block and a third tile of 6


@pytest.mark.parametrize("S", pc.S_ALL)
def test_fixture_conditions(P16, S):
    P, L = pc.samples(P16, S)
    assert P.shape == (pc.N, pc.K - 1, S + 1, 3) and np.array_equal(P[:, :, -1], P16[:, :, -1]) and (L > 0).all()
    Q, Sx, A, _ = ir.pair_minima(P)
    cand = ir.candidates(Q, Sx, A, S, pc.CULL)
    n = cand.sum(0)
    assert (n == 0).any() and all((n > J).any() for J in pc.J_ALL)
    other = ~np.eye(pc.N, dtype=bool)[:, :, None]
    # the coincident pair, in every segment and from both sides
    assert ((Q == 0.0) & other).sum() == 2 * (pc.K - 1) and (Q[pc.TWIN, pc.TWIN_OF] == 0.0).all()
    # exact ties among the candidates of one (agent, segment)
    ties = 0
    for a, k in zip(*np.nonzero(n > 1)):
        q = np.sort(Q[cand[:, a, k], a, k])
        ties += int((q[1:] == q[:-1]).sum())
    # closer than cull and not coincident, but with the minimum at a node: left to the node rows
    inner = ir.candidates(Q, Sx, A, S, np.inf)
    at_node = other & ~inner & (Q > 0.0) & (Q < pc.CULL ** 2)
    print(f"S={S}: {int((n == 0).sum())} of {n.size} segments without a candidate, more than J: "
          f"{[(J, int((n > J).sum())) for J in pc.J_ALL]}, {ties} ties, {int(at_node.sum())} minima at a node")
    assert ties > 0 and at_node.any()
