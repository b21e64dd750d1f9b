"""What the ALS test modules share (test_gpu_als.py, test_gpu_als_implicit.py, test_gpu_als_ranks.py,
test_gpu_als_wide.py, test_gpu_als_cg.py): the context and id helpers, the numpy f64 references of the
explicit half-sweep, and the exactly solvable problems of the rank-bucket tests."""
import functools

import numpy as np

from mfhip import _lib as L
from mfhip.context import Context

MODES = [L.MODE_DETERMINISTIC_F64, L.MODE_FAST_F32]
REGS = [L.ALS_REG_WEIGHTED, L.ALS_REG_PLAIN]
TINY = 1e-300       # the lambda that vanishes: 0 in f32, absorbed by any non-zero integer in f64
EXACT = 1 << 20     # every entry of A, b and r of the planted problems stays below this (f32 holds integers up to 2^24)
N_ITEMS = 12        # solved rows of the exact-solve tests
FILLERS = 200       # zero-vector counterpart rows


def make_ctx(k, mode, **kw):
    p = L.default_params()
    p.num_factors = k
    p.mode = mode
    for a, b in kw.items():
        setattr(p, a, b)
    return Context(p)


def dtype_of(mode):
    return np.float64 if mode == L.MODE_DETERMINISTIC_F64 else np.float32


def shuffled_ids(rng, n, scale=3):
    """n distinct ids, about half of them negative, in random order (row order is call order)."""
    return (rng.permutation(n).astype(np.int32) - n // 2) * scale + 1


def rows_of(side_index, n_rows):
    """Per row the positions of its ratings, in input order (what the CSR must hold)."""
    order = np.argsort(side_index, kind="stable")
    cuts = np.searchsorted(side_index[order], np.arange(n_rows + 1))
    return [order[cuts[a]:cuts[a + 1]] for a in range(n_rows)]


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def first_difference(X, want):
    """'row a: got ... want ...' of the first row that differs (for the assertion message)."""
    for a in range(len(want)):
        if not np.array_equal(X[a], want[a]):
            cols = np.flatnonzero(X[a] != want[a])[:8]
            return f"row {a}, columns {cols.tolist()}: got {X[a][cols].tolist()} want {want[a][cols].tolist()}"
    return "equal"


# ---------------------------------------------------------------------------------------------
# the explicit half-sweep in numpy f64

def small_problem(rng, nu=40, ni=25, n=400):
    u = rng.integers(0, nu, n).astype(np.int32)
    i = rng.integers(0, ni, n).astype(np.int32)
    r = rng.integers(1, 11, n) / 2.0
    return u, i, r


def normal_eq_reference(F_other, other_index, r, pos, lam, reg, k):
    Qm = F_other[other_index[pos]]
    lam_row = lam * len(pos) if reg == L.ALS_REG_WEIGHTED else lam
    return Qm.T @ Qm + lam_row * np.eye(k), Qm.T @ r[pos]


def numpy_half_sweep(X, Y, x_rows, y_index, r, lam):
    for a, pos in enumerate(x_rows):
        if len(pos):
            Qm = Y[y_index[pos]]
            X[a] = np.linalg.solve(Qm.T @ Qm + lam * len(pos) * np.eye(X.shape[1]), Qm.T @ r[pos])


def objective(P, Q, pu, pi, r, lam):
    err = r - np.einsum("nk,nk->n", P[pu], Q[pi])
    nu, ni = np.bincount(pu, minlength=len(P)), np.bincount(pi, minlength=len(Q))
    return err @ err + lam * (nu @ (P * P).sum(1) + ni @ (Q * Q).sum(1))


# ---------------------------------------------------------------------------------------------
# planted problems whose half-sweep has an exact integer solution

@functools.lru_cache(maxsize=None)
def explicit_problem(k):
    """Three groups of k users (group g carries the rows of L_g^T), FILLERS zero-vector users, one user
    in the model but not in the data; N_ITEMS items, item t rating the whole group t % 3 with
    L_g^T x0_t plus 0, 1 or 200 fillers, and two items without ratings.  Verified in integers here."""
    rng = np.random.default_rng(9000 + k)
    Ls = [np.tril(rng.integers(-1, 2, (k, k)), -1) + np.diag(rng.integers(1, 4, k)) for _ in range(3)]
    nu = 3 * k + FILLERS + 1
    P = np.zeros((nu, k), np.int64)
    for g, Lg in enumerate(Ls):
        P[g * k:(g + 1) * k] = Lg.T
    P[-1] = 2                                          # not in the data
    X0 = rng.integers(-3, 4, (N_ITEMS, k))
    extras = [0, 1, FILLERS, 1, FILLERS, 0, FILLERS, 0, 1, 0, 1, 33]  # every group meets 0, 1 and 200
    pu, pi, r = [], [], []
    for t in range(N_ITEMS):
        g = t % 3
        fill = 3 * k + rng.choice(FILLERS, extras[t], replace=False)
        pu += list(range(g * k, (g + 1) * k)) + fill.tolist()
        pi += [t] * (k + extras[t])
        r += (Ls[g].T @ X0[t]).tolist() + rng.integers(1, 6, extras[t]).tolist()
    pu, pi, r = np.array(pu), np.array(pi), np.array(r, np.int64)
    perm = rng.permutation(len(pu))
    pu, pi, r = pu[perm], pi[perm], r[perm]
    Q0 = rng.integers(1, 4, (N_ITEMS + 2, k))          # the start: never a solution by accident of zeros
    irows = rows_of(pi, N_ITEMS + 2)
    counts = {len(x) for x in irows}
    assert {k, k + 1, k + FILLERS} <= counts and len(irows[-1]) == len(irows[-2]) == 0
    assert np.abs(r).max() < EXACT
    for t in range(N_ITEMS):
        Qm = P[pu[irows[t]]]
        A, b = Qm.T @ Qm, Qm.T @ r[irows[t]]
        assert np.array_equal(A, Ls[t % 3] @ Ls[t % 3].T)
        assert np.array_equal(A @ X0[t], b)
        assert max(np.abs(A).max(), np.abs(b).max()) < EXACT
    return frozen(dict(pu=pu, pi=pi, r=r.astype(np.float64), P=P.astype(np.float64), Q0=Q0.astype(np.float64),
                       X0=X0.astype(np.float64), uids=shuffled_ids(rng, nu), iids=shuffled_ids(rng, N_ITEMS + 2, 5)))


@functools.lru_cache(maxsize=None)
def implicit_problem(k):
    """One group of k users with Q = L^T, L = I + N, FILLERS zero-vector users, one user in the model
    with non-zero factors but not in the data (G must not count it); N_ITEMS items rating the whole
    group with ratings from {+-3, +-8, +-15} plus fillers, two items without ratings.  Item 0 has no
    positive rating at all (n+ = 0), item 1 only positive ones, item 2 only negative ones in the group
    and 200 positive fillers (n+ = 200, a zero right-hand side that is still solved)."""
    rng = np.random.default_rng(9500 + k)
    h = k // 2
    N = np.zeros((k, k), np.int64)
    N[h:, :h] = rng.integers(-1, 2, (k - h, h))
    Lm = np.eye(k, dtype=np.int64) + N
    assert not (N @ N).any()
    nu = k + FILLERS + 1
    P = np.zeros((nu, k), np.int64)
    P[:k] = Lm.T
    P[-1] = 2                                          # not in the data
    mags = np.array([3, 8, 15])
    R = rng.choice(mags, (N_ITEMS, k)) * rng.choice([-1, 1], (N_ITEMS, k))
    R[0] = -np.abs(R[0])
    R[1] = np.abs(R[1])
    R[2] = -np.abs(R[2])
    extras = [1, 0, FILLERS, 0, 1, FILLERS, 0, 1, FILLERS, 33, 0, 1]
    pu, pi, r = [], [], []
    for t in range(N_ITEMS):
        fill = k + rng.choice(FILLERS, extras[t], replace=False)
        fr = rng.integers(-2, 6, extras[t])
        if t == 0:
            fr = -np.abs(fr)
        if t == 2:
            fr = np.abs(fr) + 1
        pu += list(range(k)) + fill.tolist()
        pi += [t] * (k + extras[t])
        r += R[t].tolist() + fr.tolist()
    pu, pi, r = np.array(pu), np.array(pi), np.array(r, np.int64)
    perm = rng.permutation(len(pu))
    pu, pi, r = pu[perm], pi[perm], r[perm]
    Q0 = rng.integers(1, 4, (N_ITEMS + 2, k))
    X = (R > 0).astype(np.int64) @ (np.eye(k, dtype=np.int64) - N)   # rows x_t^T = [r > 0]^T (I - N)
    irows = rows_of(pi, N_ITEMS + 2)
    counts = {len(x) for x in irows}
    assert {k, k + 1, k + FILLERS} <= counts and len(irows[-1]) == len(irows[-2]) == 0
    rated = np.unique(pu)
    G = P[rated].T @ P[rated]
    assert np.array_equal(G, Lm @ Lm.T)
    for t in range(N_ITEMS):
        pos = irows[t]
        Qm, rt = P[pu[pos]], r[pos]
        A = G + (Qm * np.abs(rt)[:, None]).T @ Qm
        b = Qm.T @ np.where(rt > 0, 1 + np.abs(rt), 0)
        S = np.sqrt(1 + np.abs(R[t])).astype(np.int64)
        assert np.array_equal(S * S, 1 + np.abs(R[t]))
        assert np.array_equal(A, (Lm * S) @ (Lm * S).T)
        assert np.array_equal(A @ X[t], b)
        assert max(np.abs(A).max(), np.abs(b).max(), np.abs(rt).max()) < EXACT
    assert not (r[irows[0]] > 0).any() and not X[0].any()
    assert (r[irows[2]] > 0).sum() == FILLERS and not X[2].any()
    assert k == 1 or X[3:].any()
    return frozen(dict(pu=pu, pi=pi, r=r.astype(np.float64), P=P.astype(np.float64), Q0=Q0.astype(np.float64),
                       X=X.astype(np.float64), uids=shuffled_ids(rng, nu), iids=shuffled_ids(rng, N_ITEMS + 2, 5)))
