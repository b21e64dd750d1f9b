"""What the non-negative ALS test modules share (test_nnls_host.py, test_gpu_als_nonneg.py): the planted
systems, their tolerance and the KKT check.

The planted family.  A = diag(c^2) + w w^T with c in {2, 3} and w in {0, 1}: eigenvalues lie in
[4, 9 + k], so cond(A) <= (9 + k) / 4.  x* has integer entries in {0, 1, 2, 3}, about 40 % of them zero;
the multipliers mu >= 1 sit on the zero set and b = A x* - mu.  Strict complementarity makes x* the unique
solution of min 1/2 x^T A x - b^T x over x >= 0.  Everything is an integer far below 2^24, so f32 holds A
and b exactly.

As ALS data (planted_als): k counterpart rows c_f e_f, one row w and zero-vector fillers.  A solved row
rates every e_f row with r_f = c_f x*_f - m_f (m_f in {1, 2} on the zero set of x*, 0 elsewhere: mu_f =
c_f m_f), the w row with r_w = w . x* and fillers with anything; then sum q q^T = diag(c^2) [+ w w^T] and
sum r q = A x* - mu exactly.
"""
import functools

import numpy as np

from als_support import FILLERS, frozen, shuffled_ids

RANKS_HOST = [1, 2, 31, 32, 33, 64, 65, 128, 129, 160, 255, 256]
N_ROWS = 12


def eps_of(f64):
    return float(np.finfo(np.float64 if f64 else np.float32).eps)


def planted(k, seed, zero_share=0.4):
    """(A, b, x*, mu) of the family above."""
    rng = np.random.default_rng(seed)
    c = rng.integers(2, 4, k).astype(np.float64)
    w = rng.integers(0, 2, k).astype(np.float64)
    A = np.diag(c * c) + np.outer(w, w)
    x = rng.integers(1, 4, k).astype(np.float64)
    zero = rng.random(k) < zero_share
    x[zero] = 0.0
    mu = np.where(zero, rng.integers(1, 4, k), 0).astype(np.float64)
    return A, A @ x - mu, x, mu


def planted_tolerance(A, b, x_star, f64):
    """1e-6 |b| / lambda_min(A): what the stop rule guarantees once the support is right (the projected
    gradient is below 1e-6 |b|, and on the support x - x* = A_SS^-1 g_S); plus the rounding floor
    64 eps cond(A) |x*|.  Returns (tolerance, its first term, cond(A))."""
    ev = np.linalg.eigvalsh(A)
    cond = ev[-1] / ev[0]
    first = 1e-6 * np.linalg.norm(b) / ev[0]
    return first + 64 * eps_of(f64) * cond * np.linalg.norm(x_star), first, cond


def assert_planted(x, x_star, A, b, f64, what, family=True):
    """The assertions on a solved planted row (the reason code is the caller's).  family: A is
    diag(c^2) + w w^T itself, whose condition number is bounded."""
    assert (x >= 0).all() and not np.signbit(x).any(), (what, "negative or -0 entry")
    assert np.array_equal(x == 0, x_star == 0), (what, "zero set")
    tol, first, cond = planted_tolerance(A, b, x_star, f64)
    assert not family or cond <= (9 + len(b)) / 4 + 1e-9, (what, cond)
    err = np.linalg.norm(x - x_star)
    print(f"{what}: error {err:.3g} tolerance {tol:.3g} (first term {first:.3g})")
    assert err <= tol, (what, err, tol)


def assert_kkt(x, A, b, f64, what):
    """g = A x - b in f64; tau = (1e-6 + 32 k eps(T)) |b|: |g_i| <= tau where x_i > 0, g_i >= -tau where
    x_i = 0.  (1e-6 |b| is the stop rule's bound on the projected gradient; 32 k eps |b| covers the rounding
    of the solver's own k-term gradient, whose terms are of the size of b.)"""
    k = len(b)
    assert (x >= 0).all() and not np.signbit(x).any(), (what, "negative or -0 entry")
    g = A @ x - b
    tau = (1e-6 + 32 * k * eps_of(f64)) * np.linalg.norm(b)
    worst = max(np.abs(g[x > 0]).max(initial=0.0), (-g[x == 0]).max(initial=0.0))
    print(f"{what}: worst KKT violation {worst:.3g} tau {tau:.3g}")
    assert worst <= tau, (what, worst, tau)


def scipy_nnls(A, b):
    """argmin over x >= 0 of 1/2 x^T A x - b^T x by scipy's active-set NNLS on the Cholesky-transformed
    system |L^T x - L^-1 b|."""
    from scipy.optimize import nnls
    Lc = np.linalg.cholesky(A)
    return nnls(Lc.T, np.linalg.solve(Lc, b), maxiter=30 * len(b))[0]


def als_shaped(k, n, seed):
    """Q^T Q + 0.05 n I and Q^T r for n random ratings: what an ALS row looks like."""
    rng = np.random.default_rng(seed)
    Q = rng.standard_normal((n, k)) * 0.5
    r = rng.integers(1, 11, n) / 2.0 * rng.choice([-1.0, 1.0], n, p=[0.3, 0.7])
    return Q.T @ Q + 0.05 * n * np.eye(k), Q.T @ r


@functools.lru_cache(maxsize=None)
def planted_als(k):
    """The planted family as ALS data: N_ROWS items.  Item 0 is all zero (no positive rating, b <= 0);
    items 1 and 2 are strictly positive (the interior case); the counts are k (no w row), k + 1 and
    k + FILLERS and more.  Returns the ratings, the user factors P, the items' start Q0 and per item
    (A, b, x*) of the explicit system without lambda."""
    rng = np.random.default_rng(7700 + k)
    c = rng.integers(2, 4, k)
    w = rng.integers(0, 2, k)
    nu = k + 1 + FILLERS + 1
    P = np.zeros((nu, k), np.int64)
    P[:k] = np.diag(c)
    P[k] = w
    P[-1] = 2                                            # in the model, not in the data
    with_w = [1, 1, 0, 1, 0, 1, 1, 0, 1, 1, 0, 1]
    extras = [1, 0, 0, FILLERS, 1, 0, 33, FILLERS, 0, 1, 0, FILLERS]
    pu, pi, r, sysm = [], [], [], []
    for t in range(N_ROWS):
        x = rng.integers(1, 4, k)
        zero = rng.random(k) < 0.4
        if t == 0:
            zero[:] = True
        if t in (1, 2):
            zero[:] = False
        x[zero] = 0
        m = np.where(zero, rng.integers(1, 3, k), 0)
        wt = w if with_w[t] else np.zeros(k, np.int64)
        A = np.diag(c * c) + np.outer(wt, wt)
        b = A @ x - c * m
        fill = k + 1 + rng.choice(FILLERS, extras[t], replace=False)
        users = list(range(k)) + ([k] if with_w[t] else []) + fill.tolist()
        rat = (c * x - m).tolist() + ([int(w @ x)] if with_w[t] else []) + rng.integers(-2, 6, extras[t]).tolist()
        if t == 0:                                        # no positive rating at all
            rat[k + with_w[t]:] = [-abs(v) for v in rat[k + with_w[t]:]]
        pu += users
        pi += [t] * len(users)
        r += rat
        Qm = P[users]
        assert np.array_equal(Qm.T @ Qm, A) and np.array_equal(Qm.T @ np.array(rat), b)
        sysm.append((A.astype(np.float64), b.astype(np.float64), x.astype(np.float64)))
    pu, pi, r = np.array(pu), np.array(pi), np.array(r, np.int64)
    assert not (r[pi == 0] > 0).any()
    counts = np.bincount(pi)
    assert {k, k + 1, k + FILLERS} <= set(counts.tolist())
    perm = rng.permutation(len(pu))
    pu, pi, r = pu[perm], pi[perm], r[perm]
    Q0 = rng.integers(1, 4, (N_ROWS + 2, k))             # two items without ratings
    d = dict(pu=pu, pi=pi, r=r.astype(np.float64), P=P.astype(np.float64), Q0=Q0.astype(np.float64),
             uids=shuffled_ids(rng, nu), iids=shuffled_ids(rng, N_ROWS + 2, 5), counts=counts)
    frozen(d)
    d["systems"] = sysm
    return d
