"""GPU: the selection kernel of the split QP launch (scvx_qp_dispatch_select, csrc/qp_dispatch.hip) against a numpy
restatement: all agents sorted by descending IPM iteration count, ties by index (stable); the first
min(T, #{iters >= thr}) -- with short_per_tail > 0 at most #{iters < thr} / short_per_tail -- form the tail list, the rest
the bulk list, unused entries are SCVX_QP_ORDER_SKIP."""
import ctypes

import numpy as np
import pytest

from scvx_hip import _lib

pytestmark = pytest.mark.gpu
SKIP = _lib.SCVX_QP_ORDER_SKIP


def restate(iters, thr, T, max_iter, spt=0):
    key = np.clip(iters, 0, max_iter)
    order = np.argsort(-key, kind="stable")
    nq = int((key >= thr).sum())
    nt = min(T, nq, (key.size - nq) // spt) if spt else min(T, nq)
    return (np.concatenate([order[:nt], np.full(T - nt, SKIP)]).astype(np.int64),
            np.concatenate([order[nt:], np.full(nt, SKIP)]).astype(np.int64))


def select(cuda, iters, thr, T, max_iter, spt=0):
    import torch
    N = iters.size
    it = torch.tensor(iters.astype(np.int32), device=cuda)
    tail = torch.full((max(T, 1),), 12345, dtype=torch.int32, device=cuda)
    bulk = torch.full((N,), 12345, dtype=torch.int32, device=cuda)
    rc = _lib.lib().scvx_qp_dispatch_select(N, ctypes.c_void_p(it.data_ptr()), thr, T, spt, max_iter,
                                            ctypes.c_void_p(tail.data_ptr()) if T else None,
                                            ctypes.c_void_p(bulk.data_ptr()), None)
    _lib.check(rc, "scvx_qp_dispatch_select")
    return tail.cpu().numpy()[:T].astype(np.int64), bulk.cpu().numpy().astype(np.int64)


def _cases():
    rng = np.random.default_rng(3)
    mx = 60
    yield "ties", rng.integers(3, 13, size=1024), 8, 32, mx            # ten distinct counts over 1024 agents
    yield "all_equal", np.full(256, 5), 5, 16, mx                      # every agent qualifies, T of them chosen by index
    yield "all_equal_below", np.full(256, 5), 6, 16, mx                # none qualifies
    yield "more_than_T", np.where(np.arange(300) % 3 == 0, 11, 3), 8, 16, mx   # 100 candidates, T = 16
    yield "odd_N", rng.integers(0, 20, size=1000), 7, 64, mx           # N no multiple of 64, last chunk part-filled
    yield "tiny", rng.integers(0, 9, size=5), 4, 5, mx                 # one part-filled chunk, T = N
    yield "at_max_iter", np.where(rng.random(777) < 0.05, mx, rng.integers(2, 9, size=777)), 8, 32, mx
    yield "beyond_max_iter", rng.integers(-2, 16, size=130), 8, 8, 12  # counts outside [0, max_iter] are clamped
    yield "order_only", rng.integers(2, 40, size=4096), mx + 1, 0, mx  # T = 0: the whole sort (64 chunks)


@pytest.mark.parametrize("spt", [0, 3], ids=["no_limit", "three_short_per_tail"])
@pytest.mark.parametrize("name,iters,thr,T,max_iter", [pytest.param(*c, id=c[0]) for c in _cases()])
def test_select_matches_restatement(cuda, name, iters, thr, T, max_iter, spt):
    tail, bulk = select(cuda, iters, thr, T, max_iter, spt)
    rt, rb = restate(iters, thr, T, max_iter, spt)
    assert np.array_equal(tail, rt) and np.array_equal(bulk, rb)
    # every agent exactly once across the two lists
    N = iters.size
    named = np.concatenate([tail[tail != SKIP], bulk[bulk != SKIP]])
    assert np.array_equal(np.sort(named), np.arange(N))
    # the bulk list: descending and stable, then only skip entries; the tail list likewise
    key = np.clip(iters, 0, max_iter)
    for lst in (tail, bulk):
        live = lst[lst != SKIP]
        assert (lst[:live.size] != SKIP).all()
        k = key[live]
        assert (np.diff(k) <= 0).all()
        assert (np.diff(live)[np.diff(k) == 0] > 0).all()
    if tail.size:
        live = tail[tail != SKIP]
        assert (key[live] >= thr).all()
        if not spt:
            assert live.size == T or (key[bulk[bulk != SKIP]] < thr).all()   # candidates stay in the bulk only past T
        else:
            short = int((key < thr).sum())
            assert spt * live.size <= short                                  # what a tail agent displaces is short
            assert live.size == min(T, int((key >= thr).sum()), short // spt)
    if name == "all_equal" and spt:
        assert (tail == SKIP).all() and np.array_equal(bulk, np.arange(iters.size))   # everyone qualifies: no tail


def test_select_is_deterministic_and_checks_arguments(cuda):
    rng = np.random.default_rng(4)
    iters = rng.integers(3, 13, size=1024)
    a = select(cuda, iters, 8, 32, 60)
    b = select(cuda, iters, 8, 32, 60)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    L = _lib.lib()
    assert L.scvx_qp_dispatch_select(16, None, 8, 4, 0, 60, None, None, None) == -1      # null buffers
    assert L.scvx_qp_dispatch_select(16, None, 8, 17, 0, 60, None, None, None) == -1     # T > N
    assert L.scvx_qp_dispatch_select(16, None, 8, 4, 0, 0, None, None, None) == -1       # max_iter < 1
    import torch
    buf = torch.zeros(8192, dtype=torch.int32, device=cuda)
    p = ctypes.c_void_p(buf.data_ptr())
    assert L.scvx_qp_dispatch_select(8192, p, 8, 4, 0, 200, p, p, None) == -2            # 128 chunks x 201 counts: no room
    assert L.scvx_qp_dispatch_select(64, p, 8, 4, 0, 1024, p, p, None) == -2             # more keys than threads
    assert L.scvx_qp_dispatch_select(0, None, 8, 0, 0, 60, None, None, None) == 0        # nothing to do
