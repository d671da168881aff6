"""GPU: separation_scan (separation_scan_kernel) and intersample_pair_rows (intersample_pair_rows_kernel) after their
common part -- tile staging, chord closest approach, the squared norm, S dispatch, host checks -- became one header
(csrc/pair_scan.hpp), against goldens recorded with the build before that change (tests/golden/pair_scan_parent.npz,
written by tests/golden/make_pair_scan_goldens.py on an MI355X).

The expressions and the order of neighbours, chunks and sub-intervals are the kernels' own, so every output array of
every case is required to be equal byte for byte: the SHA-256 over the raw bytes, which tells -0.0 from 0.0 and covers
+inf and the -1 / zero unused slots.  The existing 1e-12 comparisons against numpy would let a reordered sum through.
The fixture and its cases: tests/pair_scan_cases.py (its conditions are asserted in
tests/test_pair_scan_fixture_cpu.py)."""
import os

import numpy as np
import pytest

import pair_scan_cases as pc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pair_scan_parent.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as d:
        return {k: d[k] for k in d.files}


@pytest.mark.parametrize("S", pc.S_ALL)
def test_outputs_bytewise_equal_parent(cuda, golden, S):
    want = {str(n): h.tobytes() for n, h in zip(golden["names"], golden["sha256"])}
    got = pc.run(cuda, golden["P16"], S)
    assert set(got) == {n for n in want if f"/S{S}/" in n} and len(got) == 2 * 2 * (3 + 4 * len(pc.J_ALL))
    bad = []
    for name, v in got.items():
        eq = pc.sha(v) == want[name]
        where = ""
        full = golden.get(name.replace("/unpruned/", "/pruned/"))
        if not eq:
            bad.append(name)
            if full is not None:
                a, b = (np.ascontiguousarray(x).view(np.uint8).reshape(x.size, -1) for x in (v, full))
                i = np.flatnonzero((a != b).any(1))
                where = (f": first difference at flat [{i[0]}] {v.ravel()[i[0]]!r} (parent {full.ravel()[i[0]]!r}), "
                         f"{i.size} of {v.size} differ")
        print(f"{name} {v.dtype}{v.shape}: bytewise equal {eq}{where}")
    assert not bad, bad
