"""What the two ALS-objective test modules share (test_gpu_als_objective.py, test_als_objective_api.py): the planted
integer problems of als_support in either orientation, the objective in integers, the objective by the dense
formula in extended precision with the forward bound of every field, and the CSR a prepare builds."""
import math

import numpy as np

from als_support import N_ITEMS, explicit_problem, implicit_problem
from mfhip import _lib as L
from mfhip.context import als_solve

RANKS = [1, 3, 16, 33, 63, 64, 65, 127, 128, 129, 192, 255, 256]
FIELDS = ("total", "fit", "unobserved", "reg_user", "reg_item")
COUNTS = ("ratings", "user_rows", "item_rows")
F32_INT = 1 << 24   # f32 holds every integer below this


def planted(implicit, k, exchanged):
    """explicit_problem(k) / implicit_problem(k) as (user ids, user factors, item ids, start item factors, planted
    item factors, u, i, r as positions into the id arrays).  exchanged: the problem's items are the users (rows of
    k, k + 1 and k + 200 ratings, which cross the 64-term tile edges) and its users the items; then `start` and
    `planted` are the USER side's factors."""
    d = implicit_problem(k) if implicit else explicit_problem(k)
    sol = d["Q0"].copy()
    sol[:N_ITEMS] = d["X"] if implicit else d["X0"]
    if not exchanged:
        return dict(uids=d["uids"], iids=d["iids"], P=d["P"], Q=d["Q0"], sol=sol, pu=d["pu"], pi=d["pi"], r=d["r"])
    return dict(uids=d["iids"], iids=d["uids"], P=d["Q0"], Q=d["P"], sol=sol, pu=d["pi"], pi=d["pu"], r=d["r"])


def integer_objective(P, Q, pu, pi, r, implicit, reg):
    """The objective with lambda = 1 and alpha = 1 in int64, every field exact, after asserting in integers that
    every intermediate of the device's arithmetic (dot partials, terms, Gram entries and products, row norms) is
    an integer below 2^24, so that f32 and f64 and any summation order give this value."""
    P, Q, r = (np.rint(x).astype(np.int64) for x in (P, Q, r))
    d = np.einsum("nk,nk->n", P[pu], Q[pi])
    dabs = np.einsum("nk,nk->n", np.abs(P[pu]), np.abs(Q[pi]))   # bounds every partial sum of the dot
    pos = r > 0
    if implicit:
        w = np.abs(r)
        t = np.where(pos, (1 + w) * (1 - d) ** 2 - d * d, w * d * d)
        tabs = (1 + w) * (1 + dabs) ** 2 + dabs ** 2             # bounds c e, (c e) e, d d and their difference
    else:
        t = (r - d) ** 2
        tabs = (np.abs(r) + dabs) ** 2
    assert tabs.max() < F32_INT, tabs.max()
    ru, ri = np.unique(pu), np.unique(pi)
    out = dict(fit=int(t.sum()), unobserved=0, ratings=len(r), user_rows=len(ru), item_rows=len(ri))
    if implicit:
        GU, GI = P[ru].T @ P[ru], Q[ri].T @ Q[ri]
        AU, AI = np.abs(P[ru]).T @ np.abs(P[ru]), np.abs(Q[ri]).T @ np.abs(Q[ri])
        assert max(AU.max(), AI.max(), (AU * AI).max()) < F32_INT
        out["unobserved"] = int((GU * GI).sum())
    for name, F, idx in (("reg_user", P, pu), ("reg_item", Q, pi)):
        nrm = (F * F).sum(1)
        assert nrm.max() < F32_INT
        cnt = np.bincount(idx, pos if implicit else None, len(F)).astype(np.int64)
        rated = np.bincount(idx, minlength=len(F)) > 0
        out[name] = int((nrm * (cnt if reg == L.ALS_REG_WEIGHTED else 1))[rated].sum())
    out["total"] = out["fit"] + out["unobserved"] + out["reg_user"] + out["reg_item"]
    assert out["total"] < 1 << 53
    return out


def csr_of(pu, pi, r, rows):
    """The user side's CSR as mf_als_prepare builds it: a row's ratings in the order of the arrays."""
    order = np.argsort(pu, kind="stable")
    off = np.zeros(rows + 1, np.int64)
    np.cumsum(np.bincount(pu, minlength=rows), out=off[1:])
    return off, np.asarray(pi)[order].astype(np.int32), np.asarray(r, np.float64)[order]


def exact_sum(v):
    """The sum of extended-precision values with one rounding (math.fsum over their f64 high and low parts)."""
    v = np.asarray(v, np.longdouble).reshape(-1)
    hi = v.astype(np.float64)
    lo = (v - hi).astype(np.float64)
    return np.longdouble(math.fsum(hi.tolist() + lo.tolist()))


def dense_objective(P, Q, off, cols, vals, how, dtype):
    """(value, bound) per field: the objective by the dense formula -- that of test_gpu_als_cg.objective plus the
    constant sum over r > 0 of (1 + w) it leaves out, with lambda and alpha as the device rounds them to T -- on
    factors by row and the user side's CSR, and the standard forward bound of the device's error for that field,
    from sums of absolute values:  u * ops * sum |terms|  with u = 2^-24 (f32) or 2^-53 (f64) and ops the longest
    chain behind the field, plus one rounding for each widened term:
        a dot              k / 64 + 7
        a Gram entry       rated rows + k
        a sum64 over n     n / 64 + 6   (always in f64)
    A term is a polynomial in d = x.q (or a product of two Gram entries); its absolute-value polynomial A bounds
    every intermediate, and its chain is twice the dot's (d enters as a square) plus the 6 operations of the
    longest term formula.
    Nothing is added for the reference's own error: it is computed in extended precision (a 64-bit significand,
    asserted) with every sum over terms rounded once (exact_sum), so a value is off by at most about (k + 8) *
    2^-64 * sum |terms|, under 2 % of the smallest bound here (k = 256 against 11 operations at 2^-53).  The
    values are returned in extended precision and compared there."""
    LD = np.longdouble
    assert np.finfo(LD).nmant >= 63, "the reference needs an extended-precision long double"
    T = np.dtype(dtype).type
    u = 2.0 ** -24 if T is np.float32 else 2.0 ** -53
    u64 = 2.0 ** -53
    P, Q = np.asarray(P, np.float64).astype(LD), np.asarray(Q, np.float64).astype(LD)
    k, n = P.shape[1], int(off[-1])
    counts = np.diff(off)
    urow = np.repeat(np.arange(len(counts)), counts)
    cols, r = np.asarray(cols[:n], np.int64), np.asarray(vals[:n], np.float64).astype(LD)
    lam, alpha = LD(float(T(how.lambda_))), LD(float(T(how.alpha)))
    implicit = bool(how.implicit)
    ops_dot = k / 64 + 7
    d = (P[urow] * Q[cols]).sum(1)
    dabs = (np.abs(P[urow]) * np.abs(Q[cols])).sum(1)
    pos = r > 0
    if implicit:
        w = alpha * np.abs(r)
        t = np.where(pos, (1 + w) * (1 - d) ** 2 - d * d, w * d * d)
        tabs = np.where(pos, (1 + w) * (1 + dabs) ** 2 + dabs ** 2, w * dabs ** 2)
    else:
        t = (r - d) ** 2
        tabs = (np.abs(r) + dabs) ** 2
    val, bound = {}, {}
    val["fit"] = exact_sum(t)
    sum_abs_t = float(np.abs(t).sum())
    bound["fit"] = u * (2 * ops_dot + 6) * float(tabs.sum()) + u64 * (n / 64 + 6 + len(counts) / 64 + 6) * sum_abs_t
    ru, ri = np.flatnonzero(counts), np.flatnonzero(np.bincount(cols, minlength=len(Q)))
    val["unobserved"], bound["unobserved"] = LD(0), 0.0
    if implicit:
        val["unobserved"] = exact_sum((P[ru] @ Q[ri].T) ** 2)
        AU, AI = np.abs(P[ru]).T @ np.abs(P[ru]), np.abs(Q[ri]).T @ np.abs(Q[ri])
        bound["unobserved"] = (u * (len(ru) + k + len(ri) + k + 1) + u64 * (k * k / 64 + 6)) * float((AU * AI).sum())
    for name, F, rated, idx in (("reg_user", P, ru, urow), ("reg_item", Q, ri, cols)):
        cnt = np.bincount(idx, np.asarray(pos, np.float64) if implicit else None, len(F))
        wgt = cnt[rated].astype(LD) if how.reg == L.ALS_REG_WEIGHTED else np.ones(len(rated), LD)
        s = exact_sum(wgt[:, None] * F[rated] ** 2)
        val[name] = lam * s
        bound[name] = float(lam * s) * (u * (ops_dot + 1) + u64 * (len(rated) / 64 + 6 + 2))
    val["total"] = val["fit"] + val["unobserved"] + val["reg_user"] + val["reg_item"]
    bound["total"] = sum(bound[f] for f in FIELDS[1:]) + u64 * 3 * float(sum_abs_t + val["unobserved"] +
                                                                       val["reg_user"] + val["reg_item"])
    return val, bound


def field_error(got, val):
    """|got - val| in extended precision, as a float."""
    return float(abs(np.longdouble(got) - val))


def how_of(lam, reg, implicit=False, alpha=0.0, **kw):
    return als_solve(lam, reg, implicit, alpha, **kw)
