"""Fixtures of the collision-kernel reference tests (tests/test_collision_kernels_gpu.py), shared with the CPU
test that proves their conditions on the reference alone (tests/test_collision_ref_cpu.py).

Every fixture is the smallest shape at which one mechanism of csrc/collision.hip is exercised: the 512-neighbour
LDS tiles and their 8-wide padded chunks, the wave-local bound tau, the [blo, bhi) block-mate exclusion, the JM
template classes, culling, exact ties, pos_dim < 3, K at its limits.  ROW_CASES / CHECK_CASES list them; a case is
a dict of the launch arguments plus `random` (False: integer coordinates, squared distances exact in double)."""
import functools

import numpy as np

import collision_ref as cr

R = 0.5
TOL = 1e-7
N_TILES = 1100          # 512 + 512 + 76, and 76 = 9 * 8 + 4: a padded last chunk
I0_TILES, NLOC_TILES = 450, 130   # blocks 450..513 (straddles the tile boundary 512), 514..577, 578..579 (2 lanes)


def _junk(rng, X, pos_dim):
    """Large values, different per agent and node, in the state components at and past pos_dim."""
    X[:, :, pos_dim:] = 1e6 * rng.normal(size=X[:, :, pos_dim:].shape) + 3e5
    return X


@functools.lru_cache(maxsize=None)
def multi_tile(K=3, seed=101):
    """1100 agents in 44 clusters whose membership is a random permutation of the indices, so an agent's nearest
    neighbours are spread over all three tiles and mostly are not its block-mates (loose tau); agents 520..559
    form one tight cluster of consecutive indices (tight tau in that wave)."""
    rng = np.random.default_rng(seed)
    N, C = N_TILES, 44
    member = rng.permutation(N) % C
    centre = rng.normal(scale=8.0, size=(C, 3))
    X = np.zeros((N, K, 6))
    X[:, :, :3] = centre[member][:, None, :] + rng.normal(scale=0.5, size=(N, K, 3))
    X[520:560, :, :3] = np.array([30.0, -30.0, 30.0]) + rng.normal(scale=0.2, size=(40, K, 3))
    X[:, :, 3:] = rng.normal(size=(N, K, 3))
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def cloud(N=100, K=3, seed=102, n_x=6, pos_dim=3, junk=False, coincident=False):
    """A sparse cloud with a dense cluster (agents 20..59 when N = 100): tau tight for some lanes, loose for others;
    with a cull radius, the number of eligible neighbours ranges from 0 to above j_max."""
    rng = np.random.default_rng(seed)
    X = np.zeros((N, K, n_x))
    X[:, :, :pos_dim] = rng.normal(scale=4.0, size=(N, K, pos_dim))
    lo, hi = N // 5, 3 * N // 5
    X[lo:hi, :, :pos_dim] = rng.normal(scale=0.5, size=(hi - lo, K, pos_dim))
    if junk:
        _junk(rng, X, pos_dim)
    if coincident:
        X[41, 1, :pos_dim] = X[40, 1, :pos_dim]
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def lattice(K=3, seed=103):
    """The 5 x 5 x 5 integer lattice with spacing 1 (coordinates -2..2): exact ties are the rule.  Node 0 numbers the
    sites in raster order, the later nodes in a random order."""
    rng = np.random.default_rng(seed)
    sites = np.indices((5, 5, 5)).reshape(3, -1).T.astype(np.float64) - 2.0
    X = np.zeros((125, K, 6))
    X[:, 0, :3] = sites
    for t in range(1, K):
        X[:, t, :3] = sites[rng.permutation(125)]
    X.setflags(write=False)
    return X


def _rows(name, X, i0, n_local, j_max, pos_dim=3, cull=0.0, random=True, idx=None, R=R):
    return dict(name=name, X=X, i0=i0, n_local=n_local, j_max=j_max, pos_dim=pos_dim, cull=cull, random=random,
                idx=idx, R=R)


CULL_CLOUD = 1.3        # cloud(): no neighbour in a sparse corner, a few at the cluster's rim, dozens inside it
CULL_TILES = 1.0
J_CLASSES = (1, 3, 8, 9, 16, 17, 32)


def indexed_agents():
    """70 distinct agents of the 1100, unsorted: two blocks of the indexed launch."""
    return np.random.default_rng(104).permutation(N_TILES)[:70].astype(np.int32)


def row_cases():
    c = [_rows("multi_tile", multi_tile(), I0_TILES, NLOC_TILES, 8)]
    c += [_rows(f"jmax{j}", cloud(), 13, 70, j) for j in J_CLASSES]
    c += [_rows(f"short_n{n}", cloud(N=n, seed=110 + n), 0, n, 8) for n in (1, 2, 5)]
    c += [_rows("exact_n33", cloud(N=33, seed=143), 0, 33, 32)]
    c += [_rows("cull", cloud(), 5, 90, 8, cull=CULL_CLOUD),
          _rows("cull_none", cloud(), 5, 90, 8, cull=1e-6)]
    c += [_rows("lattice_j8", lattice(), 0, 125, 8, random=False),
          _rows("lattice_j4", lattice(), 0, 125, 4, random=False),
          _rows("lattice_cull2_j8", lattice(), 0, 125, 8, cull=2.0, random=False),
          _rows("lattice_cull2_j32", lattice(), 0, 125, 32, cull=2.0, random=False)]
    for pd in (1, 2):
        c += [_rows(f"pd{pd}_junk", cloud(seed=120 + pd, pos_dim=pd, junk=True), 13, 70, 8, pos_dim=pd),
              _rows(f"pd{pd}_junk_cull", cloud(seed=120 + pd, pos_dim=pd, junk=True), 13, 70, 8, pos_dim=pd,
                    cull=0.2 if pd == 1 else 0.4),
              _rows(f"pd{pd}_nx{pd}", cloud(seed=130 + pd, n_x=pd, pos_dim=pd), 13, 70, 8, pos_dim=pd)]
    c += [_rows(f"K{K}", cloud(N=20, K=K, seed=150 + K), 0, 20, 8) for K in (2, 64)]
    c += [_rows("coincident", cloud(seed=161, coincident=True), 13, 70, 8)]
    c += [_rows("indexed", multi_tile(), 0, 70, 8, idx=indexed_agents()),
          _rows("indexed_cull", multi_tile(), 0, 70, 8, cull=CULL_TILES, idx=indexed_agents())]
    return c


ROW_CASES = {c["name"]: c for c in row_cases()}


def agents_of(case):
    """Global agent of every local agent of a case."""
    return case["idx"] if case["idx"] is not None else np.arange(case["i0"], case["i0"] + case["n_local"])


@functools.lru_cache(maxsize=None)
def _ref_cached(name, gi, t):
    c = ROW_CASES[name]
    return cr.rows_ref(c["X"], gi, t, c["R"], c["pos_dim"], c["cull"])


def row_ref(case, gi, t):
    """rows_ref of one (agent, node) of a case, computed once per session."""
    return _ref_cached(case["name"], int(gi), int(t))


# ---- the full-row check -------------------------------------------------------------------------------------------

def _check(name, X, i0, n_local, pos_dim=3, tol=TOL, noise=0.1, slack=None, seed=200, R=R):
    """X_new = X_all + noise (every component: the junk past pos_dim is perturbed too), slack |N(0, 0.2)| unless
    given as a constant."""
    rng = np.random.default_rng(seed)
    X_new = (X + noise * rng.normal(size=X.shape))[i0:i0 + n_local]
    if X.shape[2] > pos_dim and np.abs(X[:, :, pos_dim:]).max() > 1e3:   # a junk fixture: other junk in X_new
        X_new[:, :, pos_dim:] = 1e6 * rng.normal(size=X_new[:, :, pos_dim:].shape) - 2e5
    S = np.abs(rng.normal(scale=0.2, size=(n_local, X.shape[1])))
    if slack is not None:
        S[:] = slack
    return dict(name=name, X=X, X_new=np.ascontiguousarray(X_new), S=S, i0=i0, n_local=n_local, pos_dim=pos_dim,
                tol=tol, R=R)


def check_cases():
    c = [_check("tiles_shard", multi_tile(), I0_TILES, NLOC_TILES),
         _check("tiles_all", multi_tile(), 0, N_TILES, seed=201)]
    for pd in (1, 2):
        c += [_check(f"pd{pd}_junk", cloud(seed=120 + pd, pos_dim=pd, junk=True), 13, 70, pos_dim=pd, seed=202 + pd,
                     noise=0.02 if pd == 1 else 0.1)]
    c += [_check("slack0", cloud(), 13, 70, slack=0.0, seed=210),
          _check("slack1e3", cloud(), 13, 70, slack=1e3, seed=211),
          _check("slack_neg", cloud(), 13, 70, slack=-1e-12, seed=212),
          _check("dp0", cloud(), 13, 70, noise=0.0, seed=213),
          _check("dp0_slack0_tol0", cloud(), 13, 70, noise=0.0, slack=0.0, tol=0.0, seed=214),
          _check("dp_large", cloud(), 13, 70, noise=50.0, seed=215),
          _check("tol0", cloud(), 13, 70, tol=0.0, seed=216)]
    c += [_check(f"n{n}", cloud(N=n, seed=110 + n), 0, n, seed=220 + n) for n in (1, 2)]
    c += [_check("coincident_shard", cloud(seed=161, coincident=True), 13, 70, seed=230)]
    return c


CHECK_CASES = {c["name"]: c for c in check_cases()}
