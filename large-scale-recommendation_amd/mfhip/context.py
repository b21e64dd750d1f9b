"""Thin object wrapper of an mf_ctx (one model on one or more GPUs)."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np

from . import _lib as L
from ._lib import as_f64, as_i32, check, ptr, same_length


def nnls_solve(A, b, f64: bool = True):
    """mf_nnls_solve: (x [k], iterations, reason) of the non-negative ALS solve on the host, in the kernels'
    order of operations and in f32 or f64 arithmetic.  A is k x k symmetric.  No GPU needed."""
    A = np.ascontiguousarray(A, np.float64)
    b = np.ascontiguousarray(b, np.float64)
    k = b.shape[0]
    if b.ndim != 1 or A.shape != (k, k):
        raise ValueError("A must be k x k and b must hold k values")
    x = np.empty(k, np.float64)
    it, why = C.c_int32(0), C.c_int32(0)
    check(L.lib().mf_nnls_solve(k, ptr(A, C.c_double), ptr(b, C.c_double), 1 if f64 else 0, ptr(x, C.c_double),
                                C.byref(it), C.byref(why)))
    return x, int(it.value), int(why.value)


ALS_SOLVERS = {"cholesky": L.ALS_SOLVER_CHOLESKY, "cg": L.ALS_SOLVER_CG, "nnls": L.ALS_SOLVER_NNLS}


def als_solve(lam: float, reg: int = L.ALS_REG_WEIGHTED, implicit: bool = False, alpha: float = 0.0,
              solver: str = "cholesky", cg_steps: int = 3) -> L.mf_als_solve:
    """The mf_als_solve of als_run_rows / als_update: which of the eight kinds of half-sweep solves the rows."""
    if solver not in ALS_SOLVERS:
        raise ValueError(f"unknown ALS solver {solver!r}: one of {tuple(ALS_SOLVERS)}")
    how = L.mf_als_solve()
    how.lambda_, how.reg = float(lam), int(reg)
    how.implicit, how.alpha = int(bool(implicit)), float(alpha)
    how.solver, how.cg_steps = ALS_SOLVERS[solver], int(cg_steps)
    return how


@dataclass
class RankMetrics:
    """What mf_rank_eval returns (include/mfhip.h): counts, the six means over `queries`, and with
    per_query=True the evaluated queries' ids, (hits, g) and six values, rows in ascending id."""
    queries: int
    unknown_queries: int
    gt_pairs: int
    hits: int
    precision: float
    recall: float
    map: float
    ndcg: float
    mrr: float
    hit_rate: float
    ids: Optional[np.ndarray] = None
    counts: Optional[np.ndarray] = None
    values: Optional[np.ndarray] = None


@dataclass
class Prequential:
    """What mf_online_prequential returns (include/mfhip.h) for one micro-batch: the counts (events =
    evaluated + cold + excluded), the three sums over the evaluated events, their means, and with
    ranks=True every event's rank or negative code."""
    events: int
    evaluated: int
    cold: int
    excluded: int
    hits: int
    sum_ndcg: float
    sum_rr: float
    sum_pr: float
    ndcg: float
    mrr: float
    hit_rate: float
    mpr: float
    touched_users: int = 0
    touched_items: int = 0
    ranks: Optional[np.ndarray] = None


class Context:
    """Owns an mf_ctx.  mode: "deterministic" (bit-exact f64 replay) or "fast" (f32)."""

    def __init__(self, params: L.mf_params, devices: Optional[Sequence[int]] = None, n_devices: int = 1,
                 rank: Optional[Tuple[int, int, int, bytes]] = None):
        self.params = params
        self.k = int(params.num_factors)
        self._h = C.c_void_p(None)
        lib = L.lib()
        if rank is not None:  # (device, nranks, rank, uid)
            dev, nranks, r, uid = rank
            ub = (C.c_uint8 * L.UID_BYTES).from_buffer_copy(uid.ljust(L.UID_BYTES, b"\0"))
            check(lib.mf_create_rank(C.byref(params), dev, nranks, r, ub, C.byref(self._h)))
        else:
            if devices is not None:
                arr = (C.c_int * len(devices))(*devices)
                check(lib.mf_create(C.byref(params), arr, len(devices), C.byref(self._h)))
            else:
                check(lib.mf_create(C.byref(params), None, n_devices, C.byref(self._h)))

    # -- lifecycle -------------------------------------------------------------
    def close(self) -> None:
        if self._h and self._h.value:
            check(L.lib().mf_destroy(self._h))
            self._h = C.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @staticmethod
    def unique_id() -> bytes:
        buf = (C.c_uint8 * L.UID_BYTES)()
        check(L.lib().mf_comm_unique_id(buf))
        return bytes(buf)

    # -- DSGD ------------------------------------------------------------------
    def fit(self, u, i, r) -> None:
        u, i, r = as_i32(u), as_i32(i), as_f64(r)
        same_length(u, i, r)
        check(L.lib().mf_dsgd_fit(self._h, ptr(u, C.c_int32), ptr(i, C.c_int32), ptr(r, C.c_double), len(u)))

    def prepare(self, u, i, r) -> None:
        u, i, r = as_i32(u), as_i32(i), as_f64(r)
        same_length(u, i, r)
        check(L.lib().mf_dsgd_prepare(self._h, ptr(u, C.c_int32), ptr(i, C.c_int32), ptr(r, C.c_double), len(u)))

    def run(self, supersteps: int) -> None:
        check(L.lib().mf_dsgd_run(self._h, int(supersteps)))

    def sync(self) -> None:
        check(L.lib().mf_sync(self._h))

    def restart(self) -> None:
        """Factors back to their initial values and superstep 0; blocking and schedule kept."""
        check(L.lib().mf_dsgd_restart(self._h))

    @property
    def superstep(self) -> int:
        v = C.c_int64(0)
        check(L.lib().mf_dsgd_superstep(self._h, C.byref(v)))
        return v.value

    @superstep.setter
    def superstep(self, done: int) -> None:
        check(L.lib().mf_dsgd_set_superstep(self._h, int(done)))

    # -- ALS -------------------------------------------------------------------
    def als_prepare(self, u, i, r) -> None:
        """mf_als_prepare: ids resolved (unseen ones inserted), both CSRs on the device, counter 0."""
        u, i, r = as_i32(u), as_i32(i), as_f64(r)
        same_length(u, i, r)
        check(L.lib().mf_als_prepare(self._h, ptr(u, C.c_int32), ptr(i, C.c_int32), ptr(r, C.c_double), len(u)))

    def als_run(self, half_sweeps: int, lam: float, reg: int = L.ALS_REG_WEIGHTED) -> None:
        """mf_als_run: half-sweeps alternate, the item side first; the counter continues across calls."""
        check(L.lib().mf_als_run(self._h, int(half_sweeps), float(lam), int(reg)))

    def als_fit(self, u, i, r, iterations: int, lam: float, reg: int = L.ALS_REG_WEIGHTED) -> None:
        """mf_als_fit: als_prepare + als_run(2 * iterations) (ALS.train, OnlineSpark.scala:125-131)."""
        u, i, r = as_i32(u), as_i32(i), as_f64(r)
        same_length(u, i, r)
        check(L.lib().mf_als_fit(self._h, ptr(u, C.c_int32), ptr(i, C.c_int32), ptr(r, C.c_double), len(u),
                                 int(iterations), float(lam), int(reg)))

    def als_normal_eq(self, side: int, id_: int, lam: float, reg: int = L.ALS_REG_WEIGHTED):
        """(A [k, k], b [k]) of one row as the device accumulates them (mf_debug_als_normal_eq)."""
        A = np.empty((self.k, self.k), np.float64)
        b = np.empty(self.k, np.float64)
        check(L.lib().mf_debug_als_normal_eq(self._h, int(side), int(id_), float(lam), int(reg), ptr(A, C.c_double),
                                             ptr(b, C.c_double)))
        return A, b

    def als_run_implicit(self, half_sweeps: int, lam: float, alpha: float, reg: int = L.ALS_REG_WEIGHTED) -> None:
        """mf_als_run_implicit: confidence-weighted half-sweeps (w = alpha |r|) on the prepared data; the
        order and the counter are als_run's, and the two share the counter."""
        check(L.lib().mf_als_run_implicit(self._h, int(half_sweeps), float(lam), int(reg), float(alpha)))

    def als_fit_implicit(self, u, i, r, iterations: int, lam: float, alpha: float,
                         reg: int = L.ALS_REG_WEIGHTED) -> None:
        """mf_als_fit_implicit: als_prepare + als_run_implicit(2 * iterations) (ALS.trainImplicit)."""
        u, i, r = as_i32(u), as_i32(i), as_f64(r)
        same_length(u, i, r)
        check(L.lib().mf_als_fit_implicit(self._h, ptr(u, C.c_int32), ptr(i, C.c_int32), ptr(r, C.c_double), len(u),
                                          int(iterations), float(lam), int(reg), float(alpha)))

    def als_gram(self, side: int) -> np.ndarray:
        """G [k, k] = sum of y y^T over `side`'s rows rated in the prepared data (mf_debug_als_gram)."""
        G = np.empty((self.k, self.k), np.float64)
        check(L.lib().mf_debug_als_gram(self._h, int(side), ptr(G, C.c_double)))
        return G

    def als_normal_eq_implicit(self, side: int, id_: int, lam: float, alpha: float, reg: int = L.ALS_REG_WEIGHTED):
        """(A [k, k], b [k]) of one row of the implicit half-sweep (mf_debug_als_normal_eq_implicit)."""
        A = np.empty((self.k, self.k), np.float64)
        b = np.empty(self.k, np.float64)
        check(L.lib().mf_debug_als_normal_eq_implicit(self._h, int(side), int(id_), float(lam), int(reg), float(alpha),
                                                      ptr(A, C.c_double), ptr(b, C.c_double)))
        return A, b

    def als_run_cg(self, half_sweeps: int, lam: float, reg: int = L.ALS_REG_WEIGHTED, cg_steps: int = 3) -> None:
        """mf_als_run_cg: als_run's half-sweeps with cg_steps conjugate-gradient steps per row from its
        current value instead of a factorisation; the counter is als_run's."""
        check(L.lib().mf_als_run_cg(self._h, int(half_sweeps), float(lam), int(reg), int(cg_steps)))

    def als_run_implicit_cg(self, half_sweeps: int, lam: float, alpha: float, reg: int = L.ALS_REG_WEIGHTED,
                            cg_steps: int = 3) -> None:
        """mf_als_run_implicit_cg: als_run_implicit's half-sweeps by conjugate gradients."""
        check(L.lib().mf_als_run_implicit_cg(self._h, int(half_sweeps), float(lam), int(reg), float(alpha),
                                             int(cg_steps)))

    def als_fit_cg(self, u, i, r, iterations: int, lam: float, reg: int = L.ALS_REG_WEIGHTED, cg_steps: int = 3) -> None:
        """mf_als_fit_cg: als_prepare + als_run_cg(2 * iterations)."""
        u, i, r = as_i32(u), as_i32(i), as_f64(r)
        same_length(u, i, r)
        check(L.lib().mf_als_fit_cg(self._h, ptr(u, C.c_int32), ptr(i, C.c_int32), ptr(r, C.c_double), len(u),
                                    int(iterations), float(lam), int(reg), int(cg_steps)))

    def als_fit_implicit_cg(self, u, i, r, iterations: int, lam: float, alpha: float, reg: int = L.ALS_REG_WEIGHTED,
                            cg_steps: int = 3) -> None:
        """mf_als_fit_implicit_cg: als_prepare + als_run_implicit_cg(2 * iterations)."""
        u, i, r = as_i32(u), as_i32(i), as_f64(r)
        same_length(u, i, r)
        check(L.lib().mf_als_fit_implicit_cg(self._h, ptr(u, C.c_int32), ptr(i, C.c_int32), ptr(r, C.c_double),
                                             len(u), int(iterations), float(lam), int(reg), float(alpha),
                                             int(cg_steps)))

    def als_cg_matvec(self, side: int, id_: int, lam: float, v, alpha: float = -1.0, reg: int = L.ALS_REG_WEIGHTED):
        """(A v [k], b [k]) of one row through the conjugate-gradient half-sweep's kernels
        (mf_debug_als_cg_matvec); alpha < 0: the explicit system."""
        v = np.ascontiguousarray(v, np.float64)
        if v.shape != (self.k,):
            raise ValueError("v must hold k values")
        Av = np.empty(self.k, np.float64)
        b = np.empty(self.k, np.float64)
        check(L.lib().mf_debug_als_cg_matvec(self._h, int(side), int(id_), float(lam), int(reg), float(alpha),
                                             ptr(v, C.c_double), ptr(Av, C.c_double), ptr(b, C.c_double)))
        return Av, b

    def als_cg_capacity(self) -> int:
        """The most ratings of a row whose vectors the CG half-sweep stages in LDS (mf_debug_als_cg_capacity)."""
        n = C.c_int32(0)
        check(L.lib().mf_debug_als_cg_capacity(self._h, C.byref(n)))
        return int(n.value)

    def als_run_nonneg(self, half_sweeps: int, lam: float, reg: int = L.ALS_REG_WEIGHTED) -> None:
        """mf_als_run_nonneg: als_run's half-sweeps with every row solved for x >= 0 (projected
        conjugate-gradient NNLS); the counter is als_run's."""
        check(L.lib().mf_als_run_nonneg(self._h, int(half_sweeps), float(lam), int(reg)))

    def als_run_implicit_nonneg(self, half_sweeps: int, lam: float, alpha: float,
                                reg: int = L.ALS_REG_WEIGHTED) -> None:
        """mf_als_run_implicit_nonneg: als_run_implicit's half-sweeps with the non-negative solve."""
        check(L.lib().mf_als_run_implicit_nonneg(self._h, int(half_sweeps), float(lam), int(reg), float(alpha)))

    def als_fit_nonneg(self, u, i, r, iterations: int, lam: float, reg: int = L.ALS_REG_WEIGHTED) -> None:
        """mf_als_fit_nonneg: als_prepare + als_run_nonneg(2 * iterations)."""
        u, i, r = as_i32(u), as_i32(i), as_f64(r)
        same_length(u, i, r)
        check(L.lib().mf_als_fit_nonneg(self._h, ptr(u, C.c_int32), ptr(i, C.c_int32), ptr(r, C.c_double), len(u),
                                        int(iterations), float(lam), int(reg)))

    def als_fit_implicit_nonneg(self, u, i, r, iterations: int, lam: float, alpha: float,
                                reg: int = L.ALS_REG_WEIGHTED) -> None:
        """mf_als_fit_implicit_nonneg: als_prepare + als_run_implicit_nonneg(2 * iterations)."""
        u, i, r = as_i32(u), as_i32(i), as_f64(r)
        same_length(u, i, r)
        check(L.lib().mf_als_fit_implicit_nonneg(self._h, ptr(u, C.c_int32), ptr(i, C.c_int32), ptr(r, C.c_double),
                                                 len(u), int(iterations), float(lam), int(reg), float(alpha)))

    def als_nnls_row(self, side: int, id_: int, lam: float, alpha: float = -1.0, reg: int = L.ALS_REG_WEIGHTED):
        """(x [k], iterations, reason) of one row through the non-negative half-sweep's kernels
        (mf_debug_als_nnls_row); alpha < 0: the explicit system.  The model is not changed."""
        x = np.empty(self.k, np.float64)
        it, why = C.c_int32(0), C.c_int32(0)
        check(L.lib().mf_debug_als_nnls_row(self._h, int(side), int(id_), float(lam), int(reg), float(alpha),
                                            ptr(x, C.c_double), C.byref(it), C.byref(why)))
        return x, int(it.value), int(why.value)

    def als_nonneg_stats(self) -> dict:
        """mf_als_nonneg_stats: what the non-negative half-sweeps did since als_prepare."""
        st = L.mf_als_nonneg_stats()
        check(L.lib().mf_als_nonneg_stats(self._h, C.byref(st)))
        return {n: int(getattr(st, n)) for n, _ in st._fields_}

    @staticmethod
    def nnls_solve(A, b, f64: bool = True):
        """mf_nnls_solve: (x [k], iterations, reason) of the non-negative solve on the host, in the kernels'
        order and in f32 or f64 arithmetic.  No GPU needed."""
        return nnls_solve(A, b, f64)

    def als_append(self, u, i, r) -> None:
        """mf_als_append: the ratings join the resident CSRs, which are then what als_prepare would have
        built from everything so far; unseen ids are inserted as als_prepare inserts them."""
        u, i, r = as_i32(u), as_i32(i), as_f64(r)
        same_length(u, i, r)
        check(L.lib().mf_als_append(self._h, ptr(u, C.c_int32), ptr(i, C.c_int32), ptr(r, C.c_double), len(u)))

    def als_run_rows(self, side: int, ids, how: L.mf_als_solve) -> int:
        """mf_als_run_rows: the named rows of `side` solved as a full half-sweep with `how` (als_solve) would
        solve them now; returns the number of rows solved (unknown and unrated ids are skipped)."""
        ids = as_i32(ids)
        solved = C.c_int64(0)
        check(L.lib().mf_als_run_rows(self._h, int(side), ptr(ids, C.c_int32), len(ids), C.byref(how),
                                      C.byref(solved)))
        return int(solved.value)

    def als_objective(self, how: L.mf_als_solve) -> dict:
        """mf_als_objective: the value the half-sweeps of `how` (als_solve; lambda, reg, implicit and alpha are
        read) minimise, on the resident data at the factors as they stand: total, fit, unobserved, reg_user,
        reg_item and the counts ratings, user_rows, item_rows.  Nothing of the context changes."""
        out = L.mf_als_loss()
        check(L.lib().mf_als_objective(self._h, C.byref(how), C.byref(out)))
        return {n: (int if t is C.c_int64 else float)(getattr(out, n)) for n, t in out._fields_ if n != "reserved"}

    def als_run_until(self, how: L.mf_als_solve, max_iterations: int, rel_tol: float) -> Tuple[int, np.ndarray]:
        """mf_als_run_until: iterations (two half-sweeps each) of `how` until the objective falls by no more than
        rel_tol times its size, or max_iterations; returns (iterations, history [iterations + 1]) with
        history[0] the objective on entry."""
        max_iterations = int(max_iterations)
        hist = np.zeros(max(max_iterations, 0) + 1, np.float64)
        it = C.c_int32(0)
        check(L.lib().mf_als_run_until(self._h, C.byref(how), max_iterations, float(rel_tol), C.byref(it),
                                       ptr(hist, C.c_double)))
        return int(it.value), hist[:it.value + 1]

    def _foldin_lists(self, offsets, ids, ratings):
        off = np.ascontiguousarray(offsets, np.int64)
        if off.ndim != 1 or off.size < 1:
            raise ValueError("offsets must be a 1-d array of n_queries + 1 entries")
        ci, cr = as_i32(ids), np.ascontiguousarray(ratings, np.float64)
        ne = same_length(ci, cr)
        if int(off[-1]) != ne:
            raise ValueError(f"offsets end at {int(off[-1])} but the lists hold {ne} entries")
        return off, ci, cr, ne

    def als_foldin(self, side: int, offsets, ids, ratings, how: L.mf_als_solve) -> Tuple[np.ndarray, np.ndarray]:
        """mf_als_foldin: the vectors rows of `side` would get from mf_als_run_rows with `how` (als_solve) if
        their ratings were the lists -- query j owns entries offsets[j] .. offsets[j + 1] of ids / ratings, the
        ids naming the other side -- and nothing of the context changes.  Entries naming an id the model does
        not hold are dropped.  Returns (vecs [n, k] f64, used [n]: the kept entries per query)."""
        off, ci, cr, ne = self._foldin_lists(offsets, ids, ratings)
        n = off.size - 1
        vecs = np.zeros((max(n, 1), self.k), np.float64)
        used = np.zeros(max(n, 1), np.int32)
        check(L.lib().mf_als_foldin(self._h, int(side), ptr(off, C.c_int64), ptr(ci, C.c_int32) if ne else None,
                                    ptr(cr, C.c_double) if ne else None, n, C.byref(how), ptr(vecs, C.c_double),
                                    ptr(used, C.c_int32)))
        return vecs[:n], used[:n]

    def recommend_foldin(self, side: int, offsets, ids, ratings, how: L.mf_als_solve, top_n: int,
                         exclude_rated: bool = True, scores: bool = True, vectors: bool = False):
        """mf_recommend_foldin: als_foldin's vectors scored against every row of the other side on the device,
        as recommend_vectors(vecs, top_n, side=the other side) would; exclude_rated: a query's kept ids are
        never returned to it.  Returns (ids, scores or None, counts, vecs or None, used); a query with no kept
        entry has count 0."""
        off, ci, cr, ne = self._foldin_lists(offsets, ids, ratings)
        n, top_n = off.size - 1, int(top_n)
        rows = max(n, 1) * max(top_n, 1)
        out = np.zeros(rows, np.int32)
        sc = np.zeros(rows, np.float64) if scores else None
        counts = np.zeros(max(n, 1), np.int32)
        vecs = np.zeros((max(n, 1), self.k), np.float64) if vectors else None
        used = np.zeros(max(n, 1), np.int32)
        check(L.lib().mf_recommend_foldin(self._h, int(side), ptr(off, C.c_int64), ptr(ci, C.c_int32) if ne else None,
                                          ptr(cr, C.c_double) if ne else None, n, C.byref(how), top_n,
                                          1 if exclude_rated else 0, ptr(out, C.c_int32),
                                          ptr(sc, C.c_double) if scores else None, ptr(counts, C.c_int32),
                                          ptr(vecs, C.c_double) if vectors else None, ptr(used, C.c_int32)))
        shape = (n, max(top_n, 1))
        return (out[:n * shape[1]].reshape(shape), sc[:n * shape[1]].reshape(shape) if scores else None, counts[:n],
                vecs[:n] if vectors else None, used[:n])

    def als_update(self, u, i, r, how: L.mf_als_solve, rounds: int = 1) -> Tuple[int, int]:
        """mf_als_update: als_append, then `rounds` times the batch's users and then its items solved
        (users first: a new user's row is random until solved); returns the last round's (users, items)."""
        u, i, r = as_i32(u), as_i32(i), as_f64(r)
        same_length(u, i, r)
        su, si = C.c_int64(0), C.c_int64(0)
        check(L.lib().mf_als_update(self._h, ptr(u, C.c_int32), ptr(i, C.c_int32), ptr(r, C.c_double), len(u),
                                    C.byref(how), int(rounds), C.byref(su), C.byref(si)))
        return int(su.value), int(si.value)

    def als_remove(self, u, i) -> Tuple[np.ndarray, int]:
        """mf_als_remove: entry j removes the oldest rating of the pair (u[j], i[j]) still held; the resident
        CSRs are then what als_prepare would have built without the removed ratings.  Returns (found [n] as
        bool, ratings removed)."""
        u, i = as_i32(u), as_i32(i)
        n = same_length(u, i)
        found = np.zeros(max(n, 1), np.uint8)
        removed = C.c_int64(0)
        check(L.lib().mf_als_remove(self._h, ptr(u, C.c_int32) if n else None, ptr(i, C.c_int32) if n else None, n,
                                    ptr(found, C.c_uint8), C.byref(removed)))
        return found[:n].astype(bool), int(removed.value)

    def als_remove_rows(self, side: int, ids) -> int:
        """mf_als_remove_rows: every rating of the named rows of `side` leaves the resident data (the factor
        rows stay); returns the ratings removed."""
        ids = as_i32(ids)
        removed = C.c_int64(0)
        check(L.lib().mf_als_remove_rows(self._h, int(side), ptr(ids, C.c_int32) if len(ids) else None, len(ids),
                                         C.byref(removed)))
        return int(removed.value)

    def als_retract(self, u, i, how: L.mf_als_solve, rounds: int = 1) -> Tuple[np.ndarray, int, int, int]:
        """mf_als_retract: als_remove, then `rounds` times the batch's users and then its items solved; returns
        (found, ratings removed, users solved, items solved) with the last round's counts."""
        u, i = as_i32(u), as_i32(i)
        n = same_length(u, i)
        found = np.zeros(max(n, 1), np.uint8)
        removed, su, si = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        check(L.lib().mf_als_retract(self._h, ptr(u, C.c_int32) if n else None, ptr(i, C.c_int32) if n else None, n,
                                     C.byref(how), int(rounds), ptr(found, C.c_uint8), C.byref(removed), C.byref(su),
                                     C.byref(si)))
        return found[:n].astype(bool), int(removed.value), int(su.value), int(si.value)

    def als_csr(self, side: int):
        """(off [rows + 1], cols [nnz], vals [nnz] as f64, npos [rows]) of the resident CSR of `side`
        (mf_debug_als_csr)."""
        rows, nnz = C.c_int64(0), C.c_int64(0)
        one64, one32, onef = np.zeros(1, np.int64), np.zeros(1, np.int32), np.zeros(1, np.float64)
        st = L.lib().mf_debug_als_csr(self._h, int(side), ptr(one64, C.c_int64), ptr(one32, C.c_int32),
                                      ptr(onef, C.c_double), ptr(one32, C.c_int32), 0, 0,
                                      C.byref(rows), C.byref(nnz))
        if st not in (L.MF_OK, L.MF_ERR_CAPACITY):
            check(st)
        off = np.zeros(rows.value + 1, np.int64)
        cols = np.zeros(max(nnz.value, 1), np.int32)
        vals = np.zeros(max(nnz.value, 1), np.float64)
        npos = np.zeros(max(rows.value, 1), np.int32)
        check(L.lib().mf_debug_als_csr(self._h, int(side), ptr(off, C.c_int64), ptr(cols, C.c_int32),
                                       ptr(vals, C.c_double), ptr(npos, C.c_int32), rows.value, nnz.value,
                                       C.byref(rows), C.byref(nnz)))
        return off, cols[:nnz.value], vals[:nnz.value], npos[:rows.value]

    # -- factors ---------------------------------------------------------------
    def num_factors(self, side: int) -> int:
        v = C.c_int64(0)
        check(L.lib().mf_num_factors(self._h, side, C.byref(v)))
        return v.value

    def factors(self, side: int) -> Tuple[np.ndarray, np.ndarray]:
        n = self.num_factors(side)
        ids = np.empty(max(n, 1), np.int32)
        vecs = np.empty((max(n, 1), self.k), np.float64)
        w = C.c_int64(0)
        check(L.lib().mf_get_factors(self._h, side, ptr(ids, C.c_int32), ptr(vecs, C.c_double), n, C.byref(w)))
        return ids[:w.value], vecs[:w.value]

    def set_factors(self, side: int, ids, vecs) -> None:
        ids = as_i32(ids)
        vecs = as_f64(vecs)
        if vecs.size != len(ids) * self.k:
            raise ValueError(f"vecs must hold len(ids) x k = {len(ids)} x {self.k} values, got {vecs.size}")
        vecs = vecs.reshape(len(ids), self.k)
        check(L.lib().mf_set_factors(self._h, side, ptr(ids, C.c_int32), ptr(vecs, C.c_double), len(ids)))

    def lookup(self, side: int, ids) -> Tuple[np.ndarray, np.ndarray]:
        ids = as_i32(ids)
        n = len(ids)
        out = np.empty((max(n, 1), self.k), np.float64)
        found = np.empty(max(n, 1), np.uint8)
        check(L.lib().mf_lookup(self._h, side, ptr(ids, C.c_int32), n, ptr(out, C.c_double), ptr(found, C.c_uint8)))
        return out[:n], found[:n].astype(bool)

    # -- evaluation ------------------------------------------------------------
    def predict(self, u, i) -> Tuple[np.ndarray, np.ndarray]:
        u, i = as_i32(u), as_i32(i)
        n = same_length(u, i)
        out = np.empty(max(n, 1), np.float64)
        found = np.empty(max(n, 1), np.uint8)
        check(L.lib().mf_predict(self._h, ptr(u, C.c_int32), ptr(i, C.c_int32), n, ptr(out, C.c_double),
                                 ptr(found, C.c_uint8)))
        return out[:n], found[:n].astype(bool)

    def rmse(self, u, i, r) -> Tuple[float, int]:
        u, i, r = as_i32(u), as_i32(i), as_f64(r)
        same_length(u, i, r)
        v = C.c_double(0.0)
        m = C.c_int64(0)
        check(L.lib().mf_rmse(self._h, ptr(u, C.c_int32), ptr(i, C.c_int32), ptr(r, C.c_double), len(u),
                              C.byref(v), C.byref(m)))
        return v.value, m.value

    def empirical_risk(self, u, i, r, lam: float) -> float:
        u, i, r = as_i32(u), as_i32(i), as_f64(r)
        same_length(u, i, r)
        v = C.c_double(0.0)
        check(L.lib().mf_empirical_risk(self._h, ptr(u, C.c_int32), ptr(i, C.c_int32), ptr(r, C.c_double), len(u),
                                        float(lam), C.byref(v)))
        return v.value

    def recommend(self, queries, top_n: int, side: int = L.SIDE_USER, exclude=None, scores: bool = True):
        """mf_recommend: for every query id (users for side=SIDE_USER, items for SIDE_ITEM) the top_n ids
        of the other side by p.q, scored and selected on the device.  exclude: (query ids, candidate
        ids) pairs never returned.  Returns (ids [n, top_n], scores [n, top_n] or None, counts [n]):
        row j holds counts[j] valid entries, score descending, ties by id ascending; the rest is 0."""
        q = as_i32(queries)
        n, top_n = len(q), int(top_n)
        rows = max(n, 1) * max(top_n, 1)
        ids = np.zeros(rows, np.int32)
        sc = np.zeros(rows, np.float64) if scores else None
        counts = np.zeros(max(n, 1), np.int32)
        if exclude is L.SEEN:
            check(L.lib().mf_recommend_seen(self._h, int(side), ptr(q, C.c_int32), n, top_n, ptr(ids, C.c_int32),
                                            ptr(sc, C.c_double) if scores else None, ptr(counts, C.c_int32)))
            shape = (n, max(top_n, 1))
            return (ids[:n * shape[1]].reshape(shape), sc[:n * shape[1]].reshape(shape) if scores else None,
                    counts[:n])
        eq = ec = None
        ne = 0
        if exclude is not None:
            eq, ec = as_i32(exclude[0]), as_i32(exclude[1])
            ne = same_length(eq, ec)
        check(L.lib().mf_recommend(self._h, int(side), ptr(q, C.c_int32), n, top_n,
                                   ptr(eq, C.c_int32) if ne else None, ptr(ec, C.c_int32) if ne else None, ne,
                                   ptr(ids, C.c_int32), ptr(sc, C.c_double) if scores else None,
                                   ptr(counts, C.c_int32)))
        shape = (n, max(top_n, 1))
        return (ids[:n * shape[1]].reshape(shape), sc[:n * shape[1]].reshape(shape) if scores else None, counts[:n])

    def recommend_among(self, queries, top_n: int, candidates, offsets=None, side: int = L.SIDE_USER, exclude=None,
                        seen: bool = False, scores: bool = True):
        """mf_recommend_among: recommend() restricted to caller-given candidate ids.  offsets None: every query
        ranks the one list `candidates` (an allow-list); otherwise query j ranks candidates[offsets[j] :
        offsets[j + 1]] (len(queries) + 1 offsets from 0 to len(candidates)).  Ids the model does not hold are
        dropped, repeated ids count once.  exclude: (query ids, candidate ids) pairs never returned; seen=True:
        the resident seen set instead (exclude must then be None).  Returns (ids, scores or None, counts) laid
        out as recommend() lays them out."""
        q, cand = as_i32(queries), as_i32(candidates)
        n, top_n, nc = len(q), int(top_n), len(cand)
        off = None
        if offsets is not None:
            off = np.ascontiguousarray(offsets, np.int64)
            if off.ndim != 1 or len(off) != n + 1:
                raise ValueError(f"offsets must hold len(queries) + 1 = {n + 1} entries, got {off.shape}")
        rows = max(n, 1) * max(top_n, 1)
        ids = np.zeros(rows, np.int32)
        sc = np.zeros(rows, np.float64) if scores else None
        counts = np.zeros(max(n, 1), np.int32)
        eq = ec = None
        ne = 0
        if exclude is L.SEEN:
            seen, exclude = True, None
        if exclude is not None:
            eq, ec = as_i32(exclude[0]), as_i32(exclude[1])
            ne = same_length(eq, ec)
        check(L.lib().mf_recommend_among(self._h, int(side), ptr(q, C.c_int32), n, top_n,
                                         ptr(off, C.c_int64) if off is not None else None,
                                         ptr(cand, C.c_int32) if nc else None, nc, int(bool(seen)),
                                         ptr(eq, C.c_int32) if ne else None, ptr(ec, C.c_int32) if ne else None, ne,
                                         ptr(ids, C.c_int32), ptr(sc, C.c_double) if scores else None,
                                         ptr(counts, C.c_int32)))
        shape = (n, max(top_n, 1))
        return (ids[:n * shape[1]].reshape(shape), sc[:n * shape[1]].reshape(shape) if scores else None, counts[:n])

    def similar(self, queries, top_n: int, side: int = L.SIDE_ITEM, metric: int = L.METRIC_COSINE,
                include_self: bool = False, exclude=None, scores: bool = True):
        """mf_similar: for every query id of `side` the top_n nearest ids of the same side, by cosine
        (METRIC_COSINE) or by dot product (METRIC_DOT), scored and selected on the device.  The query's own
        row is left out unless include_self.  exclude: (query ids, candidate ids) pairs never returned.
        Returns (ids, scores or None, counts) laid out as recommend() lays them out."""
        q = as_i32(queries)
        n, top_n = len(q), int(top_n)
        rows = max(n, 1) * max(top_n, 1)
        ids = np.zeros(rows, np.int32)
        sc = np.zeros(rows, np.float64) if scores else None
        counts = np.zeros(max(n, 1), np.int32)
        eq = ec = None
        ne = 0
        if exclude is not None:
            eq, ec = as_i32(exclude[0]), as_i32(exclude[1])
            ne = same_length(eq, ec)
        check(L.lib().mf_similar(self._h, int(side), ptr(q, C.c_int32), n, top_n, int(metric), int(include_self),
                                 ptr(eq, C.c_int32) if ne else None, ptr(ec, C.c_int32) if ne else None, ne,
                                 ptr(ids, C.c_int32), ptr(sc, C.c_double) if scores else None, ptr(counts, C.c_int32)))
        shape = (n, max(top_n, 1))
        return (ids[:n * shape[1]].reshape(shape), sc[:n * shape[1]].reshape(shape) if scores else None, counts[:n])

    def recommend_vectors(self, vecs, top_n: int, side: int = L.SIDE_ITEM, metric: int = L.METRIC_DOT, exclude=None,
                          scores: bool = True):
        """mf_recommend_vectors: for every row of vecs ([n, k] f64, vectors the model need not hold) the top_n
        ids of `side`, by dot product or cosine.  exclude: (positions in vecs, candidate ids) pairs never
        returned; positions outside [0, n) are ignored.  Returns (ids, scores or None, counts) laid out as
        recommend() lays them out."""
        v = np.ascontiguousarray(vecs, np.float64)
        if v.ndim != 2 or v.shape[1] != self.k:
            raise ValueError(f"vecs must be [n, {self.k}], got {v.shape}")
        n, top_n = v.shape[0], int(top_n)
        rows = max(n, 1) * max(top_n, 1)
        ids = np.zeros(rows, np.int32)
        sc = np.zeros(rows, np.float64) if scores else None
        counts = np.zeros(max(n, 1), np.int32)
        eq = ec = None
        ne = 0
        if exclude is not None:
            eq, ec = np.ascontiguousarray(exclude[0], np.int64), as_i32(exclude[1])
            ne = same_length(eq, ec)
        check(L.lib().mf_recommend_vectors(self._h, int(side), ptr(v, C.c_double) if n else None, n, top_n, int(metric),
                                           ptr(eq, C.c_int64) if ne else None, ptr(ec, C.c_int32) if ne else None, ne,
                                           ptr(ids, C.c_int32), ptr(sc, C.c_double) if scores else None,
                                           ptr(counts, C.c_int32)))
        shape = (n, max(top_n, 1))
        return (ids[:n * shape[1]].reshape(shape), sc[:n * shape[1]].reshape(shape) if scores else None, counts[:n])

    def rank_eval(self, gt_queries, gt_cands, top_n: int, side: int = L.SIDE_USER, exclude=None,
                  per_query: bool = False) -> "RankMetrics":
        """mf_rank_eval: ranking metrics of the held-out pairs (gt_queries[j], gt_cands[j]) against the
        top_n lists recommend(..., exclude=exclude) would return, taken and summed on the device.
        per_query=True: also ids [n] (ascending), counts [n, 2] = (hits, g) and values [n, 6] =
        precision, recall, ap, ndcg, rr, hit of every evaluated query."""
        gq, gc = as_i32(gt_queries), as_i32(gt_cands)
        ng = same_length(gq, gc)
        eq = ec = None
        ne = 0
        if exclude is not None and exclude is not L.SEEN:
            eq, ec = as_i32(exclude[0]), as_i32(exclude[1])
            ne = same_length(eq, ec)
        out = L.mf_rank_metrics()
        cap = int(np.unique(gq).size) if per_query else 0
        ids = np.zeros(max(cap, 1), np.int32)
        counts = np.zeros((max(cap, 1), 2), np.int32)
        values = np.zeros((max(cap, 1), L.RANK_NMETRICS), np.float64)
        head = (self._h, int(side), ptr(gq, C.c_int32) if ng else None, ptr(gc, C.c_int32) if ng else None, ng,
                int(top_n))
        tail = (C.byref(out), ptr(ids, C.c_int32) if per_query else None,
                ptr(counts, C.c_int32) if per_query else None, ptr(values, C.c_double) if per_query else None, cap)
        if exclude is L.SEEN:
            check(L.lib().mf_rank_eval_seen(*head, *tail))
        else:
            check(L.lib().mf_rank_eval(*head, ptr(eq, C.c_int32) if ne else None, ptr(ec, C.c_int32) if ne else None,
                                       ne, *tail))
        m = RankMetrics(queries=out.queries, unknown_queries=out.unknown_queries, gt_pairs=out.gt_pairs, hits=out.hits,
                        precision=out.precision, recall=out.recall, map=out.map, ndcg=out.ndcg, mrr=out.mrr,
                        hit_rate=out.hit_rate)
        if per_query:
            n = int(out.queries)
            m.ids, m.counts, m.values = ids[:n], counts[:n], values[:n]
        return m

    def pair_ranks(self, queries, cands, side: int = L.SIDE_USER, exclude=None, scores: bool = False):
        """mf_pair_ranks: for every pair (queries[j], cands[j]) the 0-based position of the candidate in the
        query's complete list -- every row of the other side minus the query's exclusions, in recommend()'s
        order -- counted on the device without building the list.  Returns (ranks [n], valid [n], scores
        [n] or None): ranks[j] is PAIR_RANK_COLD for an id the model does not hold and PAIR_RANK_EXCLUDED for
        a pair in `exclude` (valid 0, score 0.0); valid[j] is the length of the list."""
        q, c = as_i32(queries), as_i32(cands)
        n = same_length(q, c)
        eq = ec = None
        ne = 0
        if exclude is not None and exclude is not L.SEEN:
            eq, ec = as_i32(exclude[0]), as_i32(exclude[1])
            ne = same_length(eq, ec)
        ranks = np.zeros(max(n, 1), np.int32)
        valid = np.zeros(max(n, 1), np.int32)
        sc = np.zeros(max(n, 1), np.float64) if scores else None
        if exclude is L.SEEN:
            check(L.lib().mf_pair_ranks_seen(self._h, int(side), ptr(q, C.c_int32) if n else None,
                                             ptr(c, C.c_int32) if n else None, n, ptr(ranks, C.c_int32),
                                             ptr(valid, C.c_int32), ptr(sc, C.c_double) if scores else None))
            return ranks[:n], valid[:n], (sc[:n] if scores else None)
        check(L.lib().mf_pair_ranks(self._h, int(side), ptr(q, C.c_int32) if n else None,
                                    ptr(c, C.c_int32) if n else None, n,
                                    ptr(eq, C.c_int32) if ne else None, ptr(ec, C.c_int32) if ne else None, ne,
                                    ptr(ranks, C.c_int32), ptr(valid, C.c_int32),
                                    ptr(sc, C.c_double) if scores else None))
        return ranks[:n], valid[:n], (sc[:n] if scores else None)

    def rank_csr(self, queries, cands, side: int = L.SIDE_USER, ground_truth: bool = True):
        """mf_debug_rank_csr: the pair table rank_eval builds on the device for one pair list, as (query
        ids in factor-row order, offsets [n + 1], entries): candidate ids (ground_truth) or candidate
        factor rows (the exclusion table)."""
        q, c = as_i32(queries), as_i32(cands)
        n = same_length(q, c)
        qids = np.zeros(max(n, 1), np.int32)
        off = np.zeros(max(n, 1) + 1, np.int64)
        ent = np.zeros(max(n, 1), np.int32)
        nq, ne = C.c_int64(0), C.c_int64(0)
        check(L.lib().mf_debug_rank_csr(self._h, int(side), 1 if ground_truth else 0, ptr(q, C.c_int32) if n else None,
                                        ptr(c, C.c_int32) if n else None, n, ptr(qids, C.c_int32), ptr(off, C.c_int64),
                                        ptr(ent, C.c_int32), max(n, 1), max(n, 1), C.byref(nq), C.byref(ne)))
        return qids[:nq.value], off[:nq.value + 1], ent[:ne.value]

    # -- the resident seen set ---------------------------------------------------
    def _seen_put(self, fn, u, i) -> int:
        u, i = as_i32(u), as_i32(i)
        n = same_length(u, i)
        ignored = C.c_int64(0)
        check(fn(self._h, ptr(u, C.c_int32) if n else None, ptr(i, C.c_int32) if n else None, n, C.byref(ignored)))
        return ignored.value

    def seen_set(self, u, i) -> int:
        """mf_seen_set: the resident seen set := the distinct pairs (u[j], i[j]) whose ids the model holds; the
        readers take it with exclude=SEEN.  Returns the pairs ignored for an unknown id."""
        return self._seen_put(L.lib().mf_seen_set, u, i)

    def seen_add(self, u, i) -> int:
        """mf_seen_add: the set's union with the pairs given (only the batch is sorted)."""
        return self._seen_put(L.lib().mf_seen_add, u, i)

    def seen_remove(self, u, i) -> Tuple[int, int]:
        """mf_seen_remove: the set minus the pairs given; returns (distinct held pairs removed, pairs ignored
        for an unknown id).  With no set nothing changes."""
        u, i = as_i32(u), as_i32(i)
        n = same_length(u, i)
        removed, ignored = C.c_int64(0), C.c_int64(0)
        check(L.lib().mf_seen_remove(self._h, ptr(u, C.c_int32) if n else None, ptr(i, C.c_int32) if n else None, n,
                                     C.byref(removed), C.byref(ignored)))
        return int(removed.value), int(ignored.value)

    def seen_from_als(self) -> None:
        """mf_seen_from_als: the set := the distinct pairs of the prepared ALS data; nothing is uploaded."""
        check(L.lib().mf_seen_from_als(self._h))

    def seen_clear(self) -> None:
        check(L.lib().mf_seen_clear(self._h))

    def seen_count(self) -> int:
        v = C.c_int64(0)
        check(L.lib().mf_seen_count(self._h, C.byref(v)))
        return v.value

    def debug_seen_csr(self, side: int = L.SIDE_USER):
        """mf_debug_seen_csr: the set's table of `side` as the readers see it: (row ids [rows], offsets
        [rows + 1], entries = counterpart factor rows, the ids of those rows)."""
        rows = max(self.num_factors(side), 1)
        nnz = max(self.seen_count(), 1)
        rid = np.zeros(rows, np.int32)
        off = np.zeros(rows + 1, np.int64)
        ent = np.zeros(nnz, np.int32)
        eid = np.zeros(nnz, np.int32)
        r, m = C.c_int64(0), C.c_int64(0)
        check(L.lib().mf_debug_seen_csr(self._h, int(side), ptr(rid, C.c_int32), ptr(off, C.c_int64),
                                        ptr(ent, C.c_int32), ptr(eid, C.c_int32), rows, nnz, C.byref(r), C.byref(m)))
        return rid[:r.value], off[:r.value + 1], ent[:m.value], eid[:m.value]

    # -- BPR training on the seen set ---------------------------------------------
    @staticmethod
    def bpr_params(lr: float, lam: float, batch: int = 1, scale: int = L.BPR_SCALE_SUM, redraws: int = 0,
                   seed: int = 0) -> L.mf_bpr_params:
        p = L.mf_bpr_params()
        p.lr, p.lambda_, p.batch, p.scale, p.redraws, p.seed = float(lr), float(lam), int(batch), int(scale), \
            int(redraws), int(seed)
        return p

    @staticmethod
    def _bpr_stats(st: L.mf_bpr_stats) -> dict:
        return {n: int(getattr(st, n)) for n, _ in L.mf_bpr_stats._fields_}

    def bpr_run(self, params: L.mf_bpr_params, first_step: int, steps: int) -> dict:
        """mf_bpr_run: minibatch steps first_step .. first_step + steps - 1 of BPR on the resident seen set, all
        queued at once.  The caller advances first_step.  Returns the call's mf_bpr_stats as a dict."""
        st = L.mf_bpr_stats()
        check(L.lib().mf_bpr_run(self._h, C.byref(params), int(first_step), int(steps), C.byref(st)))
        return self._bpr_stats(st)

    def bpr_step_triples(self, params: L.mf_bpr_params, users, pos_items, neg_items) -> dict:
        """mf_bpr_step_triples: one step on the caller's (user, positive, negative) ids; a triple with an unknown
        id or pos == neg is void.  params.batch / redraws / seed are not read."""
        u, a, b = as_i32(users), as_i32(pos_items), as_i32(neg_items)
        n = same_length(u, a, b)
        st = L.mf_bpr_stats()
        check(L.lib().mf_bpr_step_triples(self._h, C.byref(params), ptr(u, C.c_int32) if n else None,
                                          ptr(a, C.c_int32) if n else None, ptr(b, C.c_int32) if n else None, n,
                                          C.byref(st)))
        return self._bpr_stats(st)

    def bpr_fit(self, u, i, params: L.mf_bpr_params, steps: int, init_scale: float = 0.1) -> dict:
        """mf_bpr_fit: rows for the unseen ids (initial values times init_scale), the pairs as the seen set, then
        `steps` steps from step 0."""
        u, i = as_i32(u), as_i32(i)
        n = same_length(u, i)
        st = L.mf_bpr_stats()
        check(L.lib().mf_bpr_fit(self._h, ptr(u, C.c_int32) if n else None, ptr(i, C.c_int32) if n else None, n,
                                 float(init_scale), C.byref(params), int(steps), C.byref(st)))
        return self._bpr_stats(st)

    def debug_bpr_triples(self):
        """mf_debug_bpr_triples: the last step's triples as factor rows (users, positives, negatives), -1 in all
        three for a void slot."""
        n = C.c_int64(0)
        st = L.lib().mf_debug_bpr_triples(self._h, None, None, None, 0, C.byref(n))
        if st not in (L.MF_OK, L.MF_ERR_CAPACITY):
            check(st)
        m = max(int(n.value), 1)
        u, a, b = (np.zeros(m, np.int32) for _ in range(3))
        check(L.lib().mf_debug_bpr_triples(self._h, ptr(u, C.c_int32), ptr(a, C.c_int32), ptr(b, C.c_int32), m,
                                           C.byref(n)))
        return u[:n.value], a[:n.value], b[:n.value]

    # -- online ----------------------------------------------------------------
    def online_update(self, u, i, r, flavour: int = L.ONLINE_NEXT_FACTORS, num_partitions: int = 0):
        u, i, r = as_i32(u), as_i32(i), as_f64(r)
        same_length(u, i, r)
        tu, ti = C.c_int64(0), C.c_int64(0)
        check(L.lib().mf_online_update(self._h, ptr(u, C.c_int32), ptr(i, C.c_int32), ptr(r, C.c_double), len(u),
                                       flavour, num_partitions, C.byref(tu), C.byref(ti)))
        return tu.value, ti.value

    def online_prequential(self, u, i, r, top_n: int, flavour: int = L.ONLINE_NEXT_FACTORS, num_partitions: int = 0,
                           exclude=None, ranks: bool = False, add_events: bool = False) -> "Prequential":
        """mf_online_prequential: test-then-train on one micro-batch.  Every event (u[j], i[j]) is ranked
        among all items for its user with the model as it stands (pair_ranks; exclude = (user ids, item
        ids) never ranked above it), its ndcg / rr / hit at top_n and its percentile rank summed on the
        device in a fixed order, and only then online_update(u, i, r, flavour, num_partitions) runs.
        exclude=SEEN (mf_online_prequential_seen, arrival-order flavours): the resident seen set is the
        exclusions, and with add_events the batch joins it after the update."""
        if exclude is L.SEEN:
            return self.online_prequential_sampled(u, i, r, top_n, 0, flavour=flavour, exclude=L.SEEN, ranks=ranks,
                                                   add_events=add_events)
        u, i, r = as_i32(u), as_i32(i), as_f64(r)
        n = same_length(u, i, r)
        eq = ec = None
        ne = 0
        if exclude is not None:
            eq, ec = as_i32(exclude[0]), as_i32(exclude[1])
            ne = same_length(eq, ec)
        out = L.mf_prequential()
        rk = np.zeros(max(n, 1), np.int32) if ranks else None
        tu, ti = C.c_int64(0), C.c_int64(0)
        check(L.lib().mf_online_prequential(self._h, ptr(u, C.c_int32), ptr(i, C.c_int32), ptr(r, C.c_double), n,
                                            int(flavour), int(num_partitions), int(top_n),
                                            ptr(eq, C.c_int32) if ne else None, ptr(ec, C.c_int32) if ne else None, ne,
                                            C.byref(out), ptr(rk, C.c_int32) if ranks else None,
                                            C.byref(tu), C.byref(ti)))
        return Prequential(events=out.events, evaluated=out.evaluated, cold=out.cold, excluded=out.excluded,
                           hits=out.hits, sum_ndcg=out.sum_ndcg, sum_rr=out.sum_rr, sum_pr=out.sum_pr, ndcg=out.ndcg,
                           mrr=out.mrr, hit_rate=out.hit_rate, mpr=out.mpr, touched_users=tu.value,
                           touched_items=ti.value, ranks=rk[:n] if ranks else None)

    def _sampled_ids(self, buf, n: int, negatives: int):
        # a batch that leaves the model with one item has no negatives (mf_online_update_sampled)
        drawn = n > 0 and negatives > 0 and self.num_factors(L.SIDE_ITEM) >= 2
        return buf[:n * negatives].reshape(n, negatives) if drawn else np.zeros((n, 0), np.int32)

    def online_update_sampled(self, u, i, r, negatives: int, negative_rating: float = 0.0, seed: int = 0,
                              first_event: int = 0, flavour: int = L.ONLINE_NEXT_FACTORS, sampled: bool = False):
        """mf_online_update_sampled: online_update on the batch in which every event (u[j], i[j], r[j]) is
        followed by `negatives` updates (u[j], another item, negative_rating), drawn and expanded on the
        device (negsample.draws is the draw: event first_event + j, a row of the model's items other than
        the event's own).  The caller advances first_event by len(u) from call to call.  Returns (touched
        users, touched items) of the expanded batch, and with sampled=True also the drawn item ids
        [n, negatives] ([n, 0] when the model ends the batch with a single item: nothing to draw from)."""
        u, i, r = as_i32(u), as_i32(i), as_f64(r)
        n = same_length(u, i, r)
        negatives = int(negatives)
        ids = np.zeros(max(n * max(negatives, 0), 1), np.int32) if sampled else None
        tu, ti = C.c_int64(0), C.c_int64(0)
        check(L.lib().mf_online_update_sampled(self._h, ptr(u, C.c_int32), ptr(i, C.c_int32), ptr(r, C.c_double), n,
                                               int(flavour), negatives, float(negative_rating), int(seed),
                                               int(first_event), ptr(ids, C.c_int32) if sampled else None,
                                               C.byref(tu), C.byref(ti)))
        if sampled:
            return tu.value, ti.value, self._sampled_ids(ids, n, negatives)
        return tu.value, ti.value

    def online_prequential_sampled(self, u, i, r, top_n: int, negatives: int, negative_rating: float = 0.0,
                                   seed: int = 0, first_event: int = 0, flavour: int = L.ONLINE_NEXT_FACTORS,
                                   exclude=None, ranks: bool = False, sampled: bool = False,
                                   add_events: bool = False):
        """mf_online_prequential_sampled: online_prequential's step 1 unchanged (the events ranked against
        the model as it stands), then online_update_sampled.  Returns the Prequential record, and with
        sampled=True (record, drawn item ids [n, negatives]).  exclude=SEEN (mf_online_prequential_seen):
        the resident seen set is the exclusions, and with add_events the batch joins it after the update."""
        u, i, r = as_i32(u), as_i32(i), as_f64(r)
        n = same_length(u, i, r)
        negatives = int(negatives)
        eq = ec = None
        ne = 0
        if exclude is not None and exclude is not L.SEEN:
            eq, ec = as_i32(exclude[0]), as_i32(exclude[1])
            ne = same_length(eq, ec)
        out = L.mf_prequential()
        rk = np.zeros(max(n, 1), np.int32) if ranks else None
        ids = np.zeros(max(n * max(negatives, 0), 1), np.int32) if sampled else None
        tu, ti = C.c_int64(0), C.c_int64(0)
        head = (self._h, ptr(u, C.c_int32), ptr(i, C.c_int32), ptr(r, C.c_double), n, int(flavour), int(top_n))
        tail = (C.byref(out), ptr(rk, C.c_int32) if ranks else None, C.byref(tu), C.byref(ti), negatives,
                float(negative_rating), int(seed), int(first_event), ptr(ids, C.c_int32) if sampled else None)
        if exclude is L.SEEN:
            check(L.lib().mf_online_prequential_seen(*head, *tail, 1 if add_events else 0))
        else:
            if add_events:
                raise ValueError("add_events needs exclude=SEEN")
            check(L.lib().mf_online_prequential_sampled(
                *head, ptr(eq, C.c_int32) if ne else None, ptr(ec, C.c_int32) if ne else None, ne, *tail))
        rec = Prequential(events=out.events, evaluated=out.evaluated, cold=out.cold, excluded=out.excluded,
                          hits=out.hits, sum_ndcg=out.sum_ndcg, sum_rr=out.sum_rr, sum_pr=out.sum_pr, ndcg=out.ndcg,
                          mrr=out.mrr, hit_rate=out.hit_rate, mpr=out.mpr, touched_users=tu.value,
                          touched_items=ti.value, ranks=rk[:n] if ranks else None)
        return (rec, self._sampled_ids(ids, n, negatives)) if sampled else rec

    def online_update_out(self, u, i, r, flavour: int = L.ONLINE_NEXT_FACTORS, items: bool = True):
        """online_update plus the per-rating records the operators emit (mf_online_update_out):
        NEXT_FACTORS -> (user', item') per rating (FlinkOnlineMF.scala:131-135); DELTA ->
        (userVec + deltaItemVec, deltaItemVec) per rating (PSOfflineOnlineMF.scala:174-176).
        items=False: the item records are not produced (None; no n x k buffer, no copy back).
        Per-rating records need the level-by-level replay, slower than online_update's sweep."""
        u, i, r = as_i32(u), as_i32(i), as_f64(r)
        n = same_length(u, i, r)
        uo = np.empty((max(n, 1), self.k), np.float64)
        io = np.empty((max(n, 1), self.k), np.float64) if items else None
        tu, ti = C.c_int64(0), C.c_int64(0)
        check(L.lib().mf_online_update_out(self._h, ptr(u, C.c_int32), ptr(i, C.c_int32), ptr(r, C.c_double), n,
                                           flavour, 0, C.byref(tu), C.byref(ti), ptr(uo, C.c_double),
                                           ptr(io, C.c_double) if items else None))
        return uo[:n], (io[:n] if items else None)

    # -- snapshots (TemporaryPath persistence, DSGDforMF.scala:291-296, 330-349) --
    def save(self, path: str) -> None:
        check(L.lib().mf_save_model(self._h, path.encode()))

    def load(self, path: str) -> int:
        """Set both factor sides from a snapshot; returns the stored superstep counter (to resume
        a fit: prepare(same ratings), load(path), set_superstep(counter), run(...))."""
        step = C.c_int64(0)
        check(L.lib().mf_load_model(self._h, path.encode(), C.byref(step)))
        return step.value

    # -- stats -----------------------------------------------------------------
    def set_profiling(self, on: bool) -> None:
        check(L.lib().mf_set_profiling(self._h, 1 if on else 0))

    def stats(self) -> dict:
        s = L.mf_stats()
        check(L.lib().mf_get_stats(self._h, C.byref(s)))
        return {f: getattr(s, f) for f, _ in L.mf_stats._fields_ if not f.startswith("reserved")}

    def plan_digest(self) -> tuple:
        """(FNV digest of the device schedule, pair records) after prepare (mf_debug_plan_digest)."""
        out = (C.c_uint64 * 2)()
        check(L.lib().mf_debug_plan_digest(self._h, out))
        return int(out[0]), int(out[1])

    def reset_stats(self) -> None:
        check(L.lib().mf_reset_stats(self._h))


def block_update(r, uidx, iidx, users, uomega, items, iomega, k, iteration, rating_block_id, seed, lr,
                 lr_method=0, lr_arg=0.0, lam=1.0, ctx: Optional[Context] = None):
    """mf_block_update: exact updateLocalFactors (DSGDforMF.scala:378-418) on copies of users/items."""
    own = ctx is None
    if own:
        p = L.default_params()
        p.num_factors = k
        ctx = Context(p)
    try:
        r, uidx, iidx = as_f64(r), as_i32(uidx), as_i32(iidx)
        same_length(r, uidx, iidx)
        users = as_f64(users).copy()
        items = as_f64(items).copy()
        uomega, iomega = as_i32(uomega), as_i32(iomega)
        check(L.lib().mf_block_update(ctx._h, ptr(r, C.c_double), ptr(uidx, C.c_int32), ptr(iidx, C.c_int32), len(r),
                                      ptr(users, C.c_double), ptr(uomega, C.c_int32), users.shape[0],
                                      ptr(items, C.c_double), ptr(iomega, C.c_int32), items.shape[0], k, iteration,
                                      rating_block_id, seed, lr, lr_method, lr_arg, lam))
        return users, items
    finally:
        if own:
            ctx.close()
