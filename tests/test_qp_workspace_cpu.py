"""CPU, no GPU: scvx_qp_workspace_bytes (host only) returns, byte for byte, what it returned before the QP kernel's
layout was stated once (csrc/qp_layout.hpp): every built-in capacity class of csrc/qp_caps.hpp and three
runtime-compiled classes, each at K in {13, 50, 64} and N in {1, 3}, and one rejected template (K = 65 -> 0).
Expected values: tests/golden/qp_workspace_bytes.json, recorded by tests/golden/make_qp_workspace_goldens.py from
a build of the commit before the change."""
import ctypes
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "qp_workspace_bytes.json")

# (model_id, n_x, n_u): the rows of csrc/qp_caps.hpp as (NB, NO, NC, VC)
BUILTIN = {
    (0, 6, 3): [(2, 0, 0, 0), (2, 8, 0, 0), (2, 0, 8, 0), (2, 0, 16, 0), (2, 8, 8, 0), (4, 16, 32, 0), (2, 8, 0, 1)],
    (1, 3, 2): [(2, 4, 0, 0), (2, 0, 8, 0), (4, 16, 32, 0)],
    (2, 3, 3): [(4, 8, 0, 0), (4, 0, 8, 0), (4, 16, 32, 0)],
    (3, 12, 4): [(4, 8, 8, 0), (4, 16, 32, 0), (4, 8, 8, 1), (4, 16, 32, 1)],
}
# runtime-compiled classes (model_id 255): the kinematic car's, and the other user classes of
# tests/test_user_classes_cpu.py in their virtual-control variant
RUNTIME = [(4, 2, 2, 1, 0, 0), (5, 2, 2, 1, 0, 1), (9, 3, 2, 1, 0, 1)]
KS, NS = (13, 50, 64), (1, 3)


def cases():
    """(model_id, n_x, n_u, n_box, n_obs, j_max, vc, K, N) of every template; the last one is rejected (K = 65)."""
    classes = [(mid, nx, nu) + row for (mid, nx, nu), rows in BUILTIN.items() for row in rows]
    classes += [(255, nx, nu, nb, no, nc, vc) for nx, nu, nb, no, nc, vc in RUNTIME]
    out = [c + (K, N) for c in classes for K in KS for N in NS]
    out.append((0, 6, 3, 2, 0, 0, 0, 65, 1))
    return out


def key(case):
    return ",".join(str(v) for v in case)


def workspace_bytes(lib, QPTemplate, case):
    mid, nx, nu, nb, no, nc, vc, K, N = case
    T = QPTemplate()
    T.model_id, T.n_x, T.n_u, T.K, T.pos_dim = mid, nx, nu, K, 3
    T.n_box, T.n_obs, T.j_max, T.w_nu = nb, no, nc, (1.0 if vc else 0.0)
    T.max_iter, T.tol, T.w_last = 50, 1e-8, 1.0
    return int(lib.scvx_qp_workspace_bytes(ctypes.byref(T), N))


def test_qp_workspace_bytes_unchanged():
    from scvx_hip import _lib
    L = _lib.lib()
    with open(GOLDEN) as f:
        want = json.load(f)
    cs = cases()
    assert len(cs) == (17 + 3) * 6 + 1 and sorted(want) == sorted(key(c) for c in cs)
    got = {key(c): workspace_bytes(L, _lib.QPTemplate, c) for c in cs}
    assert got == want
    assert want[key(cs[-1])] == 0 and all(v > 0 for k, v in want.items() if k != key(cs[-1]))
