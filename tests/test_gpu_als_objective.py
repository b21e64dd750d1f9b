"""mf_als_objective and mf_als_run_until on the device (csrc/kernels_als_objective.hip).

 1. exact on integer data       every rank bucket of the lane layout (k = 64 c + ...), both modes, both regs, both
                                orientations of the planted problems, whole rows, chunks, batches, Gram slices
 2. bit for bit                 against mfhip.als.replay_objective, the numpy restatement of the arithmetic
 3. against the dense formula   within the forward bound of als_objective_support.dense_objective (measured error
                                and bound are printed)
 4. invariances                 repeat, als_batch, append / remove against a fresh prepare, no side effects
 5. descent                     the value falls in every half-sweep of four solvers
 6. als_run_until               the manual loop, bit for bit, and its stopping rules
 7. errors                      each raised before anything changes
"""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest

import mfhip
from als_objective_support import (COUNTS, FIELDS, RANKS, dense_objective, field_error, how_of, integer_objective,
                                   planted)
from als_support import MODES, REGS, TINY, bits, dtype_of, make_ctx
from conftest import set_knob
from mfhip import _lib as L
from mfhip import synth
from mfhip.als import StreamingALS, replay_objective

pytestmark = pytest.mark.gpu

F64, F32 = L.MODE_DETERMINISTIC_F64, L.MODE_FAST_F32
LAM, ALPHA = 0.1, 0.7


@contextlib.contextmanager
def knob(key=None, value=None):
    """conftest.set_knob for a block (a prepare reads the cuts there); whatever MFHIP_TEST held stays beside it."""
    with pytest.MonkeyPatch.context() as mp:
        if key:
            set_knob(mp, key, value)
        yield


def first_touch(ids):
    """The distinct ids in order of first appearance: the factor rows a fresh context gives them."""
    return ids[np.sort(np.unique(ids, return_index=True)[1])]


def fields(d):
    return {f: d[f] for f in FIELDS + COUNTS}


def field_bits(d):
    return [int(bits(np.array([d[f]]))[0]) for f in FIELDS] + [d[f] for f in COUNTS]


def factor_bits(ctx):
    return [bits(ctx.factors(s)[1]).copy() for s in (0, 1)]


def run(ctx, half_sweeps, implicit, lam=LAM, alpha=ALPHA, cg=False):
    if cg:
        ctx.als_run_implicit_cg(half_sweeps, lam, alpha, cg_steps=3) if implicit else ctx.als_run_cg(half_sweeps, lam, cg_steps=3)
    else:
        ctx.als_run_implicit(half_sweeps, lam, alpha) if implicit else ctx.als_run(half_sweeps, lam)


@functools.lru_cache(maxsize=None)
def smoke_data(implicit):
    d = synth.generate(300, 120, 6000, seed=3)
    u, i, r = np.asarray(d.u, np.int32), np.asarray(d.i, np.int32), np.asarray(d.r, np.float64)
    out = (u, i, r - 3.0 if implicit else r)
    for a in out:
        a.setflags(write=False)
    return out


def seeded(k, mode):
    return make_ctx(k, mode, has_seed=1, seed=11)


# ---------------------------------------------------------------------------------------------
# 1. exact on integer data

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", RANKS)
def test_exact_on_integer_data(mode, k):
    """lambda = 1, alpha = 1 on explicit_problem(k) and implicit_problem(k), as given (user rows of at most 12
    ratings) and with the sides exchanged (user rows of k, k + 1 and k + 200 ratings).  Evaluated at the start
    factors and at the planted integer solution, which the device produces itself: one item half-sweep as given,
    mf_als_run_rows over the user side when exchanged (the planted rows are the users there).  integer_objective
    asserts in integers that every dot partial, term, Gram product and row norm stays below 2^24, so every field
    must equal the integer value exactly in f32 and f64, whatever the summation order -- with the default cuts,
    als_chunk=5 (a 12-rating row becomes chunks of 5, 5, 2), als_batch=7 and als_gram_slice=16."""
    for implicit in (False, True):
        for exchanged in (False, True):
            d = planted(implicit, k, exchanged)
            u, i = d["uids"][d["pu"]], d["iids"][d["pi"]]
            for cut in (None, ("als_chunk", 5), ("als_batch", 7), ("als_gram_slice", 16)):
                with knob(*(cut or ())), make_ctx(k, mode) as ctx:
                    ctx.set_factors(L.SIDE_USER, d["uids"], d["P"])
                    ctx.set_factors(L.SIDE_ITEM, d["iids"], d["Q"])
                    ctx.als_prepare(u, i, d["r"])
                    for at in ("start", "solution"):
                        P, Q = d["P"], d["Q"]
                        if at == "solution":
                            if exchanged:
                                ctx.als_run_rows(L.SIDE_USER, d["uids"], how_of(TINY, L.ALS_REG_WEIGHTED, implicit, 1.0))
                                P = d["sol"]
                                got = ctx.lookup(L.SIDE_USER, d["uids"])[0]
                            else:
                                run(ctx, 1, implicit, TINY, 1.0)
                                Q = d["sol"]
                                got = ctx.lookup(L.SIDE_ITEM, d["iids"])[0]
                            assert np.array_equal(got, d["sol"]), (k, mode, implicit, exchanged, cut)
                        for reg in REGS:
                            want = integer_objective(P, Q, d["pu"], d["pi"], d["r"], implicit, reg)
                            got = ctx.als_objective(how_of(1.0, reg, implicit, 1.0))
                            assert fields(got) == fields(want), (k, mode, implicit, exchanged, cut, at, reg)


# ---------------------------------------------------------------------------------------------
# 2. + 3. one trained state per (k, mode, implicit, chunk), downloaded once through the existing hooks

@functools.lru_cache(maxsize=None)
def trained(k, mode, implicit, chunk):
    u, i, r = smoke_data(implicit)
    with knob(*(("als_chunk", chunk) if chunk else ())), seeded(k, mode) as ctx:
        ctx.als_prepare(u, i, r)
        run(ctx, 2, implicit)
        got = {reg: ctx.als_objective(how_of(LAM, reg, implicit, ALPHA)) for reg in REGS}
        off, cols, vals, _ = ctx.als_csr(L.SIDE_USER)
        P, Q = ctx.lookup(L.SIDE_USER, first_touch(u))[0], ctx.lookup(L.SIDE_ITEM, first_touch(i))[0]
        GU, GI = (ctx.als_gram(L.SIDE_USER), ctx.als_gram(L.SIDE_ITEM)) if implicit else (None, None)
    assert len(off) - 1 == len(P) and cols.max() < len(Q)
    return dict(got=got, off=off, cols=cols, vals=vals, P=P, Q=Q, GU=GU, GI=GI)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", [3, 33, 64, 128, 160, 256])
def test_bit_for_bit_against_the_replay(mode, k):
    """synth.generate(300, 120, 6000, seed=3), explicit and implicit (r - 3, alpha 0.7), after one iteration, both
    regs, the default chunk and als_chunk=16: all five doubles equal replay_objective's in every bit."""
    for implicit in (False, True):
        for chunk in (None, 16):
            s = trained(k, mode, implicit, chunk)
            for reg in REGS:
                want = replay_objective(s["P"], s["Q"], s["off"], s["cols"], s["vals"], s["GU"], s["GI"],
                                        how_of(LAM, reg, implicit, ALPHA), chunk or 16384, dtype_of(mode))
                assert field_bits(s["got"][reg]) == field_bits(want), (k, mode, implicit, chunk, reg, s["got"][reg], want)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", [3, 33, 64, 128, 160, 256])
def test_within_the_forward_bound_of_dense_numpy(mode, k):
    """The same downloaded factors through the dense formula (evaluated in extended precision with exactly
    rounded sums, so that nothing need be added for the reference); per field |device - dense| <= the forward
    bound u * ops * sum |terms| that dense_objective computes from sums of absolute values (no chosen constant).  Every measured error is printed
    beside its bound; DESIGN 4.7.8 records them."""
    for implicit in (False, True):
        s = trained(k, mode, implicit, None)
        for reg in REGS:
            how = how_of(LAM, reg, implicit, ALPHA)
            val, bound = dense_objective(s["P"], s["Q"], s["off"], s["cols"], s["vals"], how, dtype_of(mode))
            for f in FIELDS:
                err = field_error(s["got"][reg][f], val[f])
                print(f"objective bound k={k} mode={mode} implicit={implicit} reg={reg} {f}: value {float(val[f]):.9g} "
                      f"error {err:.3g} bound {bound[f]:.3g} ratio {err / bound[f] if bound[f] else 0.0:.3g}")
                assert err <= bound[f], (k, mode, implicit, reg, f, s["got"][reg][f], float(val[f]), bound[f])


# ---------------------------------------------------------------------------------------------
# 4. invariances

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("implicit", [False, True])
def test_repeatable_and_batch_free(mode, implicit):
    """Two calls give equal bits, and als_batch (the rows per launch of the half-sweeps) changes nothing."""
    u, i, r = smoke_data(implicit)
    how = how_of(LAM, L.ALS_REG_WEIGHTED, implicit, ALPHA)
    seen = []
    for cut in (None, ("als_batch", 7)):
        with knob(*(cut or ())), seeded(33, mode) as ctx:
            ctx.als_prepare(u, i, r)
            seen += [field_bits(ctx.als_objective(how)), field_bits(ctx.als_objective(how))]
    assert seen[0] == seen[1] == seen[2] == seen[3]


def distinct_pairs(implicit):
    u, i, r = smoke_data(implicit)
    keep = np.sort(np.unique(u.astype(np.int64) * 1000 + i, return_index=True)[1])
    return u[keep], i[keep], r[keep]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("implicit", [False, True])
def test_append_and_remove_match_a_fresh_prepare(mode, implicit):
    """prepare(A) + als_append(B) and prepare(A ++ B) + als_remove(B) against fresh contexts holding the same
    factors in the same rows and prepare(A ++ B) / prepare(A): equal bits in every field."""
    u, i, r = distinct_pairs(implicit)
    cutoff = len(u) - 700
    A, B = slice(0, cutoff), slice(cutoff, None)
    how = how_of(LAM, L.ALS_REG_WEIGHTED, implicit, ALPHA)
    uids, iids = first_touch(u), first_touch(i)

    def fresh(src, part):
        ctx = seeded(65, mode)
        ctx.set_factors(L.SIDE_USER, uids, src.lookup(L.SIDE_USER, uids)[0])
        ctx.set_factors(L.SIDE_ITEM, iids, src.lookup(L.SIDE_ITEM, iids)[0])
        ctx.als_prepare(u[part], i[part], r[part])
        return ctx

    with seeded(65, mode) as grown:
        grown.als_prepare(u, i, r)            # rows in first-touch order of the whole list, as uids / iids
        run(grown, 2, implicit)
        with fresh(grown, A) as sub:
            sub.als_append(u[B], i[B], r[B])
            with fresh(grown, slice(None)) as whole:
                assert field_bits(sub.als_objective(how)) == field_bits(whole.als_objective(how))
                found, removed = whole.als_remove(u[B], i[B])
                assert found.all() and removed == len(u) - cutoff
                with fresh(grown, A) as part:
                    assert field_bits(whole.als_objective(how)) == field_bits(part.als_objective(how))


@pytest.mark.parametrize("implicit", [False, True])
def test_a_call_changes_nothing(implicit):
    """A twin that never asks for the objective is bit-identical after the next half-sweep; the seen set's count
    and the NNLS counters stay as they were."""
    u, i, r = smoke_data(implicit)
    how = how_of(LAM, L.ALS_REG_WEIGHTED, implicit, ALPHA)
    with seeded(33, F32) as ctx, seeded(33, F32) as twin:
        for c in (ctx, twin):
            c.als_prepare(u, i, r)
            c.als_run_implicit_nonneg(1, LAM, ALPHA) if implicit else c.als_run_nonneg(1, LAM)
            c.seen_from_als()
        before = (factor_bits(ctx), ctx.seen_count(), ctx.als_nonneg_stats())
        ctx.als_objective(how)
        after = (factor_bits(ctx), ctx.seen_count(), ctx.als_nonneg_stats())
        assert before[1:] == after[1:] and all(np.array_equal(a, b) for a, b in zip(before[0], after[0]))
        for c in (ctx, twin):
            run(c, 1, implicit)                # the counter is odd on both: the user side
        assert all(np.array_equal(a, b) for a, b in zip(factor_bits(ctx), factor_bits(twin)))


# ---------------------------------------------------------------------------------------------
# 5. descent

@pytest.mark.parametrize("cg", [False, True])
@pytest.mark.parametrize("implicit", [False, True])
def test_total_falls_in_every_half_sweep(implicit, cg):
    """k = 16, deterministic, lambda 0.1: Cholesky minimises each row's quadratic and 3 CG steps from the row's
    value cannot raise it, so total falls in each of 10 half-sweeps."""
    u, i, r = smoke_data(implicit)
    how = how_of(LAM, L.ALS_REG_WEIGHTED, implicit, 1.0)
    with seeded(16, F64) as ctx:
        ctx.als_prepare(u, i, r)
        J = [ctx.als_objective(how)["total"]]
        for _ in range(10):
            run(ctx, 1, implicit, LAM, 1.0, cg)
            J.append(ctx.als_objective(how)["total"])
    print(f"objective implicit={implicit} cg={cg}: " + " ".join(f"{x:.8g}" for x in J))
    assert all(b < a for a, b in zip(J, J[1:])), J


# ---------------------------------------------------------------------------------------------
# 6. als_run_until

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("implicit", [False, True])
def test_run_until_is_the_manual_loop(mode, implicit):
    u, i, r = smoke_data(implicit)
    how = how_of(LAM, L.ALS_REG_WEIGHTED, implicit, ALPHA, solver="cg", cg_steps=2)
    tol = 0.02
    with seeded(33, mode) as ctx, seeded(33, mode) as twin:
        for c in (ctx, twin):
            c.als_prepare(u, i, r)
        start = factor_bits(ctx)
        # max_iterations = 0: J_0 and no bit changes
        it, hist = ctx.als_run_until(how, 0, tol)
        assert it == 0 and len(hist) == 1 and all(np.array_equal(a, b) for a, b in zip(factor_bits(ctx), start))
        assert bits(hist)[0] == bits(np.array([twin.als_objective(how)["total"]]))[0]

        def manual(cap, rel_tol):
            J = [twin.als_objective(how)["total"]]
            while len(J) - 1 < cap:
                twin.als_run_implicit_cg(2, LAM, ALPHA, cg_steps=2) if implicit else twin.als_run_cg(2, LAM, cg_steps=2)
                J.append(twin.als_objective(how)["total"])
                if not np.isfinite(J[-1]) or J[-2] - J[-1] <= rel_tol * abs(J[-2]):
                    break
            return J

        # rel_tol = 0 runs to the cap while the value keeps falling (the first four iterations from the start)
        it, hist = ctx.als_run_until(how, 4, 0.0)
        J = manual(4, 0.0)
        assert it == 4 and np.array_equal(bits(hist), bits(np.array(J)))
        assert all(np.array_equal(a, b) for a, b in zip(factor_bits(ctx), factor_bits(twin)))
        it, hist = ctx.als_run_until(how, 12, tol)
        J = manual(12, tol)
        assert 1 <= it < 12, (it, hist)       # the tolerance, not the cap, ended it
        assert it == len(J) - 1 and np.array_equal(bits(hist), bits(np.array(J)))
        assert all(np.array_equal(a, b) for a, b in zip(factor_bits(ctx), factor_bits(twin)))
        # rel_tol = 1e30 stops after one iteration
        it, hist = ctx.als_run_until(how, 5, 1e30)
        assert it == 1 and len(hist) == 2
        # the counter moved by two per iteration: the item side is next on both
        manual(1, 1e30)
        for c in (ctx, twin):
            run(c, 1, implicit)
        assert all(np.array_equal(a, b) for a, b in zip(factor_bits(ctx), factor_bits(twin)))


def test_python_surface():
    """ALS.withSolver(tol=) is prepare + als_run_until and stops early; StreamingALS.objective follows an update."""
    u, i, r = smoke_data(False)
    how = how_of(LAM, L.ALS_REG_WEIGHTED)
    m = mfhip.als.ALS.withSolver("cholesky", tol=1e-2).train((u, i, r), 8, 50, LAM, mode="fast", seed=11)
    with make_ctx(8, F32, has_seed=1, seed=11) as twin:
        twin.als_prepare(u, i, r)
        it, _ = twin.als_run_until(how, 50, 1e-2)
        assert 1 <= it < 50
        assert field_bits(m.context.als_objective(how)) == field_bits(twin.als_objective(how))
        assert all(np.array_equal(a, b) for a, b in zip(factor_bits(m.context), factor_bits(twin)))
    m.close()
    s = StreamingALS(rank=8, lambda_=LAM, mode="fast", seed=11).fit((u[:5000], i[:5000], r[:5000]), 2)
    a = s.objective()
    s.update((u[5000:], i[5000:], r[5000:]))
    b = s.objective()
    assert (a["ratings"], b["ratings"]) == (5000, 6000)
    s.close()


# ---------------------------------------------------------------------------------------------
# 7. errors

def test_errors_are_raised_before_anything_changes():
    u, i, r = smoke_data(True)
    lib = L.lib()
    W = L.ALS_REG_WEIGHTED
    nan, inf = float("nan"), float("inf")
    out, it = L.mf_als_loss(), C.c_int32(0)

    def objective(ctx, how):
        return lib.mf_als_objective(ctx._h, C.byref(how) if how is not None else None, C.byref(out))

    def until(ctx, how, iters, tol):
        return lib.mf_als_run_until(ctx._h, C.byref(how) if how is not None else None, iters, tol, C.byref(it), None)

    with seeded(16, F32) as ctx, seeded(16, F32) as twin, seeded(16, F32) as bare, make_ctx(257, F32) as wide:
        good = how_of(LAM, W, True, ALPHA)
        # MF_ERR_STATE before a prepare; k above 256
        assert objective(bare, good) == L.MF_ERR_STATE and until(bare, good, 1, 0.0) == L.MF_ERR_STATE
        assert objective(wide, good) == L.MF_ERR_INVALID and until(wide, good, 1, 0.0) == L.MF_ERR_INVALID
        for c in (ctx, twin):
            c.als_prepare(u, i, r)
            run(c, 1, True)
        before = (factor_bits(ctx), field_bits(ctx.als_objective(good)))
        assert objective(ctx, None) == L.MF_ERR_INVALID
        assert lib.mf_als_objective(ctx._h, C.byref(good), None) == L.MF_ERR_INVALID
        bad = [how_of(-0.5, W), how_of(nan, W), how_of(inf, W), how_of(LAM, 7), how_of(LAM, W, True, -1.0),
               how_of(LAM, W, True, nan), how_of(LAM, W, True, inf)]
        for how in bad:
            assert objective(ctx, how) == L.MF_ERR_INVALID, (how.lambda_, how.reg, how.alpha)
            assert until(ctx, how, 3, 0.0) == L.MF_ERR_INVALID, (how.lambda_, how.reg, how.alpha)
        # what the objective does not read or allows: solver, cg_steps, lambda = 0, alpha when explicit
        odd = how_of(0.0, W, False, -1.0)
        odd.solver, odd.cg_steps = 9, -4
        assert objective(ctx, odd) == L.MF_OK and out.reg_user == 0.0 and out.reg_item == 0.0 and out.unobserved == 0.0
        # ... and the run call does not
        cg0 = how_of(LAM, W, True, ALPHA, solver="cg", cg_steps=3)
        cg0.cg_steps = 0
        for how, iters, tol in ((None, 3, 0.0), (how_of(0.0, W), 3, 0.0), (odd, 3, 0.0), (cg0, 3, 0.0), (good, -1, 0.0),
                                (good, 3, -1e-9), (good, 3, nan), (good, 3, inf)):
            assert until(ctx, how, iters, tol) == L.MF_ERR_INVALID, (iters, tol)
        assert lib.mf_als_run_until(None, C.byref(good), 1, 0.0, None, None) == L.MF_ERR_INVALID
        after = (factor_bits(ctx), field_bits(ctx.als_objective(good)))
        assert before[1] == after[1] and all(np.array_equal(a, b) for a, b in zip(before[0], after[0]))
        for c in (ctx, twin):                   # the half-sweep counter did not move either
            run(c, 1, True)
        assert all(np.array_equal(a, b) for a, b in zip(factor_bits(ctx), factor_bits(twin)))
        # a prepare with n = 0 gives all zeros
        empty = np.zeros(0, np.int32)
        bare.als_prepare(empty, empty, np.zeros(0))
        assert all(v == 0 for v in bare.als_objective(good).values())
        assert bare.als_run_until(good, 0, 0.0)[1].tolist() == [0.0]
