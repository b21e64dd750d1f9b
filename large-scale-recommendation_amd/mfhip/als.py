"""Mirror of the Spark MLlib entry point the reference's offline "ALS" branch calls
(sp/OnlineSpark.scala:125-131): ALS.train(ratings, rank, iterations, lambda) returning a
MatrixFactorizationModel, backed by mf_als_fit (alternating least squares on the device).

    model = ALS.train(ratings, rank=10, iterations=10, lambda_=0.1)
    model.predict(user, product)
    model.recommendProducts(user, 10)

ALS.trainImplicit(ratings, rank, iterations, lambda, alpha) is the implicit-feedback sibling
(mf_als_fit_implicit): confidences 1 + alpha |r|, preferences r > 0.

ALS.withSolver("cg", cg_steps=3) gives the same two entry points on the conjugate-gradient half-sweeps
(mf_als_fit_cg / mf_als_fit_implicit_cg): a few CG steps per row from its current value instead of a
factorisation.  ALS.train / ALS.trainImplicit themselves keep the Cholesky solve.

    model = ALS.withSolver("cg", cg_steps=3).train(ratings, rank=128)

ALS.withSolver("nnls") is MLlib's nonnegative = true: every row is solved for x >= 0 by a projected
conjugate-gradient NNLS on the device (mf_als_fit_nonneg / mf_als_fit_implicit_nonneg); cg_steps is
ignored for it.

Weighted-lambda regularisation (ALS-WR), as ALS.train uses.  The initial factors are this library's
(k x nextDouble of new Random(id ^ seed)), not MLlib's partition-dependent XORShift draws.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np

from . import _lib as L
from .bpr import _dot64
from .context import Context, als_solve
from .dsgd import _columns, _pairs
from .ranking import RankingMetrics


class MatrixFactorizationModel:
    """org.apache.spark.mllib.recommendation.MatrixFactorizationModel over a fitted Context;
    Rating(user, product, rating) is the tuple (user, product, rating)."""

    def __init__(self, ctx: Context):
        self._ctx = ctx
        self.rank = ctx.k

    @property
    def context(self) -> Context:
        return self._ctx

    def close(self) -> None:
        self._ctx.close()

    def userFeatures(self) -> List[Tuple[int, np.ndarray]]:
        ids, vecs = self._ctx.factors(L.SIDE_USER)
        return [(int(x), v) for x, v in zip(ids, vecs)]

    def productFeatures(self) -> List[Tuple[int, np.ndarray]]:
        ids, vecs = self._ctx.factors(L.SIDE_ITEM)
        return [(int(x), v) for x, v in zip(ids, vecs)]

    def predict(self, user, product=None):
        """predict(user, product) -> float; predict(pairs) -> [(user, product, rating)], unknown ids dropped."""
        if product is not None:
            pred, found = self._ctx.predict([int(user)], [int(product)])
            if not found[0]:
                raise KeyError(f"unknown user or product: ({user}, {product})")
            return float(pred[0])
        u, i = _pairs(user)
        pred, found = self._ctx.predict(u, i)
        return [(int(a), int(b), float(c)) for a, b, c, f in zip(u, i, pred, found) if f]

    def recommendProducts(self, user: int, num: int) -> List[Tuple[int, int, float]]:
        ids, sc, cnt = self._ctx.recommend([int(user)], num, side=L.SIDE_USER)
        return [(int(user), int(ids[0, x]), float(sc[0, x])) for x in range(int(cnt[0]))]

    def recommendUsers(self, product: int, num: int) -> List[Tuple[int, int, float]]:
        ids, sc, cnt = self._ctx.recommend([int(product)], num, side=L.SIDE_ITEM)
        return [(int(ids[0, x]), int(product), float(sc[0, x])) for x in range(int(cnt[0]))]

    def similarProducts(self, product: int, num: int, metric: int = L.METRIC_COSINE) -> List[Tuple[int, float]]:
        """The num products nearest to `product` in factor space, the product itself left out: (id, score)."""
        ids, sc, cnt = self._ctx.similar([int(product)], num, side=L.SIDE_ITEM, metric=metric)
        return [(int(ids[0, x]), float(sc[0, x])) for x in range(int(cnt[0]))]

    def similarUsers(self, user: int, num: int, metric: int = L.METRIC_COSINE) -> List[Tuple[int, float]]:
        """The num users nearest to `user` in factor space, the user left out: (id, score)."""
        ids, sc, cnt = self._ctx.similar([int(user)], num, side=L.SIDE_USER, metric=metric)
        return [(int(ids[0, x]), float(sc[0, x])) for x in range(int(cnt[0]))]

    def recommendProductsForUsers(self, num: int, users=None, exclude=None) -> dict:
        """users=None: every user of the model.  exclude: (user ids, item ids) pairs never recommended."""
        if users is None:
            users, _ = self._ctx.factors(L.SIDE_USER)
        users = L.as_i32(users)
        ids, sc, cnt = self._ctx.recommend(users, num, side=L.SIDE_USER, exclude=exclude)
        return {int(u): [(int(u), int(ids[j, x]), float(sc[j, x])) for x in range(int(cnt[j]))]
                for j, u in enumerate(users)}

    def recommendProductsAmong(self, users, num: int, products, offsets=None) -> dict:
        """The num best products for each user among the given product ids only (mf_recommend_among).  offsets
        None: `products` is one list every user ranks (an allow-list); otherwise user j ranks products[offsets[j] :
        offsets[j + 1]].  Returns {position j: [(user, product, score), ...]} -- keyed by position, since a user
        may be asked twice with different lists."""
        users = L.as_i32(users)
        ids, sc, cnt = self._ctx.recommend_among(users, num, products, offsets=offsets, side=L.SIDE_USER)
        return {j: [(int(u), int(ids[j, x]), float(sc[j, x])) for x in range(int(cnt[j]))]
                for j, u in enumerate(users)}

    def recommendProductsForSessions(self, sessions, num: int, lambda_: float = 0.01, implicit: bool = False,
                                     alpha: float = 0.01, solver: str = "cholesky", cg_steps: int = 3,
                                     exclude_rated: bool = True) -> List[List[Tuple[int, float]]]:
        """Fold-in (mf_recommend_foldin): top-num products for users the model does not hold and does not
        take in -- a new visitor's basket, an anonymous session.  sessions: a list of (product ids, ratings);
        each is solved as a user with exactly those ratings would be (lambda_, implicit / alpha, solver as
        als_solve takes them), products the model does not know are dropped, and with exclude_rated a
        session's own products are never returned to it.  One list of (product, score) per session; a session
        with no known product gets an empty list.  The model is left exactly as it was."""
        off = np.zeros(len(sessions) + 1, np.int64)
        for j, (p, r) in enumerate(sessions):
            if len(p) != len(r):
                raise ValueError(f"session {j}: {len(p)} products but {len(r)} ratings")
            off[j + 1] = off[j] + len(p)
        ids = np.concatenate([L.as_i32(p) for p, _ in sessions]) if len(sessions) else np.zeros(0, np.int32)
        r = (np.concatenate([np.asarray(r, np.float64) for _, r in sessions]) if len(sessions)
             else np.zeros(0, np.float64))
        how = als_solve(lambda_, L.ALS_REG_WEIGHTED, implicit, alpha, solver, cg_steps)
        out, sc, cnt, _, _ = self._ctx.recommend_foldin(L.SIDE_USER, off, ids, r, how, num, exclude_rated=exclude_rated)
        return [[(int(out[j, x]), float(sc[j, x])) for x in range(int(cnt[j]))] for j in range(len(sessions))]

    def rankingMetrics(self, heldout_pairs, exclude=None) -> RankingMetrics:
        """RankingMetrics of the model's top-k product lists against held-out (user, product) pairs (tuples
        or two arrays); exclude: (user ids, item ids) pairs never recommended, e.g. the training pairs."""
        u, i = _pairs(heldout_pairs)
        return RankingMetrics(self._ctx, u, i, exclude=exclude, side=L.SIDE_USER)


def _sum64(v: np.ndarray) -> float:
    """sum64 of include/mfhip.h in f64: lane l chains v[l], v[l + 64], ... from 0.0, then the butterfly."""
    v = np.asarray(v, np.float64)
    pad = np.zeros((len(v) + 63) // 64 * 64, np.float64)   # x + 0.0 == x for every x a chain from +0.0 reaches
    pad[:len(v)] = v
    acc = np.zeros(64, np.float64)
    for tile in pad.reshape(-1, 64):
        acc = acc + tile
    lanes = np.arange(64)
    for b in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[lanes ^ b]
    return float(acc[0])


def replay_objective(P, Q, off, cols, vals, GU, GI, how: L.mf_als_solve, chunk: int, dtype) -> dict:
    """mf_als_objective's arithmetic in numpy, operation by operation (include/mfhip.h): the five doubles it
    must return bit for bit, and the three counts.  P / Q: the user / item factors by factor row; off / cols /
    vals: the USER side's resident CSR (Context.als_csr); GU / GI: the two Gram matrices [k, k] as the device
    forms them (Context.als_gram; read only when how.implicit); chunk: the prepare's als_chunk; dtype: the
    context's precision T."""
    T = np.dtype(dtype).type
    with np.errstate(all="ignore"):
        P, Q = np.ascontiguousarray(P, T), np.ascontiguousarray(Q, T)
        off, cols = np.asarray(off, np.int64), np.asarray(cols, np.int64)
        r = np.ascontiguousarray(vals, T)
        k, n, chunk = P.shape[1], int(off[-1]), int(chunk)
        implicit = bool(how.implicit)
        lam = float(T(how.lambda_))
        out = dict(total=0.0, fit=0.0, unobserved=0.0, reg_user=0.0, reg_item=0.0, ratings=n, user_rows=0, item_rows=0)
        if n == 0:
            return out
        counts = np.diff(off)
        urow = np.repeat(np.arange(len(counts)), counts)
        # fit: the terms in CSR order, a sum64 per work item, a sum64 over the work items
        d = _dot64(P[urow], Q[cols[:n]])
        if implicit:
            w = T(how.alpha) * np.abs(r[:n])
            c, e = T(1) + w, T(1) - d
            t = np.where(r[:n] > 0, (c * e) * e - d * d, (w * d) * d)
        else:
            e = r[:n] - d
            t = e * e
        t = t.astype(np.float64)
        sums = []
        for a in np.flatnonzero(counts):
            b0, b1 = int(off[a]), int(off[a + 1])
            step = b1 - b0 if b1 - b0 <= chunk else chunk
            sums += [_sum64(t[b:min(b + step, b1)]) for b in range(b0, b1, step)]
        out["fit"] = _sum64(np.array(sums))
        if implicit:
            g = (np.ascontiguousarray(GU, T) * np.ascontiguousarray(GI, T)).astype(np.float64)
            out["unobserved"] = _sum64(g.reshape(-1))
        # reg: the rated rows of each side ascending, weighted by the row's count (its ratings > 0 when implicit)
        weighted = how.reg == L.ALS_REG_WEIGHTED
        pos = (r[:n] > 0).astype(np.int64)
        for name, F, cnt, npos in (("user", P, counts, np.bincount(urow, pos, len(counts))),
                                   ("item", Q, np.bincount(cols[:n], minlength=len(Q)),
                                    np.bincount(cols[:n], pos, len(Q)))):
            rated = np.flatnonzero(cnt)
            out[name + "_rows"] = len(rated)
            nrm = _dot64(F[rated], F[rated]).astype(np.float64)
            if weighted:
                nrm = nrm * (npos if implicit else cnt)[rated].astype(np.float64)
            out["reg_" + name] = lam * _sum64(nrm)
        out["total"] = ((out["fit"] + out["unobserved"]) + out["reg_user"]) + out["reg_item"]
    return out


class ALS:
    @staticmethod
    def train(ratings, rank: int, iterations: int = 10, lambda_: float = 0.01, mode: str = "deterministic",
              seed: int = 0) -> MatrixFactorizationModel:
        """ALS.train(ratings, rank, iterations, lambda); ratings: (user, product, rating) tuples or
        three arrays."""
        u, i, r = _columns(ratings)
        ctx = ALS._context(rank, mode, seed)
        try:
            ctx.als_fit(u, i, r, int(iterations), float(lambda_), L.ALS_REG_WEIGHTED)
        except Exception:
            ctx.close()
            raise
        return MatrixFactorizationModel(ctx)

    @staticmethod
    def trainImplicit(ratings, rank: int, iterations: int = 10, lambda_: float = 0.01, alpha: float = 0.01,
                      mode: str = "deterministic", seed: int = 0) -> MatrixFactorizationModel:
        """ALS.trainImplicit(ratings, rank, iterations, lambda, alpha) with MLlib's defaults; the ratings
        are implicit feedback (counts, possibly zero or negative)."""
        u, i, r = _columns(ratings)
        ctx = ALS._context(rank, mode, seed)
        try:
            ctx.als_fit_implicit(u, i, r, int(iterations), float(lambda_), float(alpha), L.ALS_REG_WEIGHTED)
        except Exception:
            ctx.close()
            raise
        return MatrixFactorizationModel(ctx)

    @staticmethod
    def withSolver(solver: str = "cholesky", cg_steps: int = 3, tol: Optional[float] = None) -> "_SolverALS":
        """train / trainImplicit on the named solver: "cholesky" (ALS.train's own), "cg" or "nnls"
        (non-negative factors; cg_steps is ignored for it).  tol: training stops before `iterations` once an
        iteration lowers the objective by no more than tol times its size (mf_als_run_until)."""
        return _SolverALS(solver, cg_steps, tol)

    @staticmethod
    def _context(rank: int, mode: str, seed: int) -> Context:
        p = L.default_params()
        p.num_factors = int(rank)
        p.has_seed = 1
        p.seed = int(seed)
        p.mode = L.MODE_FAST_F32 if mode == "fast" else L.MODE_DETERMINISTIC_F64
        return Context(p)


SOLVERS = ("cholesky", "cg", "nnls")


class StreamingALS:
    """An ALS model that takes in new ratings (mf_als_append / mf_als_run_rows / mf_als_update): the rating
    history stays on the device, a micro-batch is appended to it there and only the rows it touches are
    solved again -- its users first, then its items.

        s = StreamingALS(rank=32, lambda_=0.05, mode="fast")
        s.fit(history, iterations=10)
        s.update(batch)              # (users solved, items solved); a new user's ratings: fold-in
        s.refit(2)                   # full half-sweeps over everything so far, nothing uploaded
        s.model.recommendProducts(user, 10)
    """

    def __init__(self, rank: int, lambda_: float = 0.01, implicit: bool = False, alpha: float = 0.01,
                 solver: str = "cholesky", cg_steps: int = 3, mode: str = "deterministic", seed: int = 0):
        if int(rank) < 1 or int(rank) > L.ALS_MAX_RANK:
            raise ValueError(f"rank must lie in 1 .. {L.ALS_MAX_RANK}")
        if not float(lambda_) > 0:
            raise ValueError("lambda_ must be > 0")
        if solver not in SOLVERS:
            raise ValueError(f"unknown ALS solver {solver!r}: one of {SOLVERS}")
        if not 1 <= int(cg_steps) <= L.ALS_CG_MAX_STEPS:
            raise ValueError(f"cg_steps must lie in 1 .. {L.ALS_CG_MAX_STEPS}")
        if implicit and not (float(alpha) >= 0 and np.isfinite(alpha)):
            raise ValueError("alpha must be finite and >= 0")
        if mode not in ("deterministic", "fast"):
            raise ValueError(f"unknown mode {mode!r}: 'deterministic' or 'fast'")
        self.how = als_solve(lambda_, L.ALS_REG_WEIGHTED, implicit, alpha, solver, cg_steps)
        self._rank, self._mode, self._seed = int(rank), mode, int(seed)
        self._ctx = None

    def _run(self, half_sweeps: int) -> None:
        h, c = self.how, self._ctx
        if h.solver == L.ALS_SOLVER_CG:
            if h.implicit:
                c.als_run_implicit_cg(half_sweeps, h.lambda_, h.alpha, h.reg, h.cg_steps)
            else:
                c.als_run_cg(half_sweeps, h.lambda_, h.reg, h.cg_steps)
        elif h.solver == L.ALS_SOLVER_NNLS:
            if h.implicit:
                c.als_run_implicit_nonneg(half_sweeps, h.lambda_, h.alpha, h.reg)
            else:
                c.als_run_nonneg(half_sweeps, h.lambda_, h.reg)
        elif h.implicit:
            c.als_run_implicit(half_sweeps, h.lambda_, h.alpha, h.reg)
        else:
            c.als_run(half_sweeps, h.lambda_, h.reg)

    def _fitted(self) -> Context:
        if self._ctx is None:
            raise RuntimeError("StreamingALS: call fit() first (an empty rating list is a valid start)")
        return self._ctx

    def fit(self, ratings, iterations: int = 10) -> "StreamingALS":
        """The history so far: upload it (als_prepare) and run `iterations` full iterations."""
        if int(iterations) < 0:
            raise ValueError("iterations must be >= 0")
        u, i, r = _columns(ratings)
        if self._ctx is None:
            self._ctx = ALS._context(self._rank, self._mode, self._seed)
        self._ctx.als_prepare(u, i, r)
        self._run(2 * int(iterations))
        return self

    def update(self, ratings, rounds: int = 1) -> Tuple[int, int]:
        """A micro-batch: appended on the device, then `rounds` times its users and its items solved.
        Returns the rows solved in the last round as (users, items)."""
        if int(rounds) < 0:
            raise ValueError("rounds must be >= 0")
        u, i, r = _columns(ratings)
        return self._fitted().als_update(u, i, r, self.how, int(rounds))

    def forget(self, pairs, rounds: int = 1) -> Tuple[int, int, int]:
        """Retraction (mf_als_retract): each (user, item) pair given removes the oldest rating of that pair
        still held, then `rounds` times the pairs' users and their items are solved again (rows left without
        a rating are skipped and keep their factors).  Returns (ratings removed, users solved, items solved)."""
        if int(rounds) < 0:
            raise ValueError("rounds must be >= 0")
        ctx = self._fitted()
        u, i = _pairs(pairs)
        _, removed, su, si = ctx.als_retract(u, i, self.how, int(rounds))
        return removed, su, si

    def refit(self, half_sweeps: int = 2) -> "StreamingALS":
        """Full half-sweeps over the resident data (the item side first, as a fit's); nothing is uploaded."""
        if int(half_sweeps) < 0:
            raise ValueError("half_sweeps must be >= 0")
        self._fitted()
        self._run(int(half_sweeps))
        return self

    def objective(self) -> dict:
        """mf_als_objective of this model's own half-sweeps on everything held so far (after every update and
        forget), at the factors as they stand: total, fit, unobserved, reg_user, reg_item and the counts."""
        return self._fitted().als_objective(self.how)

    @property
    def model(self) -> MatrixFactorizationModel:
        return MatrixFactorizationModel(self._fitted())

    def close(self) -> None:
        if self._ctx is not None:
            self._ctx.close()
            self._ctx = None


class _SolverALS:
    """ALS.train / ALS.trainImplicit with the solver of the half-sweeps chosen (ALS.withSolver), and with tol set
    training that stops by the objective (mf_als_run_until) instead of after a fixed count."""

    def __init__(self, solver: str = "cholesky", cg_steps: int = 3, tol: Optional[float] = None):
        if solver not in SOLVERS:
            raise ValueError(f"unknown ALS solver {solver!r}: one of {SOLVERS}")
        if not 1 <= int(cg_steps) <= L.ALS_CG_MAX_STEPS:
            raise ValueError(f"cg_steps must lie in 1 .. {L.ALS_CG_MAX_STEPS}")
        if tol is not None and not (float(tol) >= 0 and np.isfinite(tol)):
            raise ValueError("tol must be finite and >= 0")
        self.solver = solver
        self.cg_steps = int(cg_steps)
        self.tol = None if tol is None else float(tol)

    def _until(self, ratings, rank, iterations, mode, seed, how: L.mf_als_solve) -> MatrixFactorizationModel:
        """prepare, then at most `iterations` iterations, stopping once one lowers the objective by no more than
        tol times its size."""
        if int(iterations) < 0:
            raise ValueError("iterations must be >= 0")
        u, i, r = _columns(ratings)
        ctx = ALS._context(rank, mode, seed)
        try:
            if len(u):
                ctx.als_prepare(u, i, r)
                ctx.als_run_until(how, int(iterations), self.tol)
        except Exception:
            ctx.close()
            raise
        return MatrixFactorizationModel(ctx)

    def train(self, ratings, rank: int, iterations: int = 10, lambda_: float = 0.01, mode: str = "deterministic",
              seed: int = 0) -> MatrixFactorizationModel:
        if self.tol is not None:
            return self._until(ratings, rank, iterations, mode, seed,
                               als_solve(lambda_, solver=self.solver, cg_steps=self.cg_steps))
        if self.solver == "cholesky":
            return ALS.train(ratings, rank, iterations, lambda_, mode, seed)
        u, i, r = _columns(ratings)
        ctx = ALS._context(rank, mode, seed)
        try:
            if self.solver == "nnls":
                ctx.als_fit_nonneg(u, i, r, int(iterations), float(lambda_), L.ALS_REG_WEIGHTED)
            else:
                ctx.als_fit_cg(u, i, r, int(iterations), float(lambda_), L.ALS_REG_WEIGHTED, self.cg_steps)
        except Exception:
            ctx.close()
            raise
        return MatrixFactorizationModel(ctx)

    def trainImplicit(self, ratings, rank: int, iterations: int = 10, lambda_: float = 0.01, alpha: float = 0.01,
                      mode: str = "deterministic", seed: int = 0) -> MatrixFactorizationModel:
        if self.tol is not None:
            return self._until(ratings, rank, iterations, mode, seed,
                               als_solve(lambda_, implicit=True, alpha=alpha, solver=self.solver,
                                         cg_steps=self.cg_steps))
        if self.solver == "cholesky":
            return ALS.trainImplicit(ratings, rank, iterations, lambda_, alpha, mode, seed)
        u, i, r = _columns(ratings)
        ctx = ALS._context(rank, mode, seed)
        try:
            if self.solver == "nnls":
                ctx.als_fit_implicit_nonneg(u, i, r, int(iterations), float(lambda_), float(alpha),
                                            L.ALS_REG_WEIGHTED)
            else:
                ctx.als_fit_implicit_cg(u, i, r, int(iterations), float(lambda_), float(alpha), L.ALS_REG_WEIGHTED,
                                        self.cg_steps)
        except Exception:
            ctx.close()
            raise
        return MatrixFactorizationModel(ctx)
