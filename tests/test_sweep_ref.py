# -*- coding: utf-8 -*-
"""tests/sweep_ref.py against itself, against NumPy / SciPy and against its mutants (no GPU): the packed layouts
round-trip and hit every index once; the long-double truths agree with a 50-digit evaluation; float64 evaluations of the
same operations (W @ k, solve_triangular) and the restated device order stay within the budgets on every input family
tests/test_gpu_sweep_budget.py uses, where the hollowing guards are asserted as well; each mutant of the restated order
exceeds the budget on EVERY row."""
import mpmath as mp
import numpy as np
import pytest
from scipy.linalg import solve_triangular

import factor_ref as fr
import kvalue_ref as kr
import sweep_ref as sr


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


# ----------------------------------------------------------------------------------------------------------------------
# layouts
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 17, 512, 513, 1025])
def test_pack_linv_round_trips_and_hits_every_index_once(n):
    W = sr.planted_w(n)
    W[np.tril_indices(n)] += 3.0                               # no zero in the lower triangle
    P = sr.pack_linv(W, n)
    assert len(P) == sr.packed_len(n)
    back, rest_zero = sr.unpack_linv(P, n)
    assert rest_zero and same_bits(back, W)
    row, col = sr.index_map(n)
    flat = row.astype(np.int64).reshape(-1) * (1 << 20) + col.reshape(-1)
    assert len(np.unique(flat)) == len(flat), "two packed doubles name the same (row, col)"
    # exactly the block-lower part of the padded matrix: row block ib has the columns 0 .. 512 (ib + 1) - 1
    want = np.zeros((sr.npad(n), sr.npad(n)), dtype=bool)
    for ib in range(sr.npad(n) // sr.ROWS):
        want[sr.ROWS * ib:sr.ROWS * (ib + 1), :sr.ROWS * (ib + 1)] = True
    got = np.zeros_like(want)
    got[row.reshape(-1), col.reshape(-1)] = True
    assert np.array_equal(got, want)
    rs = np.random.RandomState(n)
    for _ in range(200):
        r = rs.randint(n)
        c = rs.randint(r + 1)
        assert P[sr.packed_index(r, c)] == W[r, c]


def test_tile_decode_is_the_enumeration():
    """The sqrt-based decode of both pack kernels against plain enumeration, through 17 packed row blocks."""
    tiles = sr.tile_list(17 * sr.ROWS)
    for t in list(range(0, 2000)) + list(range(2000, len(tiles), 7)) + [len(tiles) - 1]:
        assert sr.tile_decode(t) == tiles[t]


@pytest.mark.parametrize("n", [1, 17, 513])
def test_pack_lsolve_index_map(n):
    """Off the prepared slots the image is -L on the packed positions whose 16-column block lies below the row's and
    +0.0 elsewhere; the slots hold -L left of the 4 x 4 diagonal blocks, whose inverses multiply back to the identity."""
    L, _ = fr.factor("planted", n)
    P = sr.pack_lsolve(L, n)
    slot = sr.lsolve_slot_mask(n)
    row, col = (a.reshape(-1) for a in sr.index_map(n))
    ok = (row < n) & ((col >> 4) < (row >> 4)) & ~slot
    assert same_bits(P[ok], -L[row[ok], col[ok]])
    assert np.all(P[~ok & ~slot].view(np.int64) == 0)
    assert slot.sum() == 256 * (sr.npad(n) // 16)
    for C in range((n + 15) // 16):
        Ts = sr.diag_slot(L, n, C).reshape(4, 4, 4, 4)        # [q][q'][i][k]
        for q in range(4):
            r0 = 16 * C + 4 * q
            if r0 >= n:
                assert not Ts[q].any()
                continue
            hi = min(n, r0 + 4) - r0
            X = Ts[q, q][:hi, :hi]
            assert np.allclose(np.tril(L[r0:r0 + hi, r0:r0 + hi]) @ X, np.eye(hi), rtol=0, atol=1e-13)
            for q2 in range(q):
                assert same_bits(Ts[q, q2][:hi], -L[r0:r0 + hi, 16 * C + 4 * q2:16 * C + 4 * q2 + 4])
            assert not Ts[q, q + 1:].any()


def test_inverted_block_off_by_one_ulp_moves_the_image_not_the_budget():
    """A 4 x 4 diagonal inverse off by one ulp in one entry: the bit-for-bit image test is what catches it; the error
    budget of the solve form does not (and need not): the entry's own rounding is already charged 5 u."""
    n = 129
    L, _ = fr.factor("planted", n)
    a, b = sr.pack_lsolve(L, n), sr.pack_lsolve(L, n, mutant="inv4_ulp")
    diff = np.nonzero(a.view(np.int64) != b.view(np.int64))[0]
    assert len(diff) == 1 and sr.lsolve_slot_mask(n)[diff[0]]
    assert abs(a[diff[0]] - b[diff[0]]) <= 2.0 * kr.ulp(a[diff[0]])


def probe_factor(n, r, c):
    L = np.diag(np.full(n, 2.0 ** 600))
    L[r, r] = 2.0 ** 152
    if r != c:
        L[r, c] = -2.0 ** 800
    else:
        L[c, c] = 2.0 ** -48
    return L


@pytest.mark.parametrize("r,c", [(5, 5), (7, 5), (14, 5), (21, 5), (261, 5), (768, 768)])
def test_probe_factor_has_exact_image(r, c):
    """The factor of the substitution form's k* probe: every entry of its image is a signed power of two or a zero,
    the row's inverted block carries 2^48 in column c (same 4 x 4 block) or the image carries 2^800 there, so that
    v_r = 2^48 k_c with no rounding."""
    n = 769
    L = probe_factor(n, r, c)
    P = sr.pack_lsolve(L, n)
    nz = P[P != 0.0]
    m, _ = np.frexp(np.abs(nz))
    assert np.all(m == 0.5)
    Ts = sr.diag_slot(L, n, r // 16).reshape(4, 4, 4, 4)
    q, i = (r % 16) // 4, r % 4
    assert Ts[q, q, i, i] == (2.0 ** 48 if r == c else 2.0 ** -152)
    if r != c and r // 4 == c // 4:
        assert Ts[q, q, i, c % 4] == 2.0 ** 48
    elif r != c and r // 16 == c // 16:
        assert Ts[q, (c % 16) // 4, i, c % 4] == 2.0 ** 800
    elif r != c:
        assert P[sr.packed_index(r, c)] == 2.0 ** 800


# ----------------------------------------------------------------------------------------------------------------------
# the truths against 50 digits
# ----------------------------------------------------------------------------------------------------------------------
def test_truths_against_50_digits():
    """mu, v and q of both forms at n = 24, D = 3: within 2^-9 ulp of a double of the scale each budget is relative to
    (sum |alpha||k^| for mu, (|A||k^|)_r resp. (|L^-1||k^|)_r for v, q for q)."""
    n, D = 24, 3
    X, alpha, T, k, mean = sr.case(n, D)
    T = T[:12]
    W = sr.planted_w(n)
    L, _ = fr.factor("planted", n)
    ti = sr.Truth(W, X, alpha, T, k, mean)
    ts = sr.Truth(L, X, alpha, T, k, mean, form="solve")
    tol = 2.0 ** -9 * 2.0 ** -52
    with mp.workdps(50):
        kt = kr.truth(T, X, k)
        Linv = np.abs(np.linalg.inv(L))
        for a in range(len(T)):
            kv = [kt[a, j] for j in range(n)]
            mu = sum(mp.mpf(float(alpha[j])) * kv[j] for j in range(n)) + mp.mpf(mean)
            assert abs(mp.mpf(float(ti.mu[a])) + mp.mpf(float(ti.mu[a] - np.longdouble(float(ti.mu[a])))) - mu) <= tol * ti.sabs[a]
            vi = [sum(mp.mpf(float(W[r, j])) * kv[j] for j in range(r + 1)) for r in range(n)]
            vs = []
            for r in range(n):
                vs.append((kv[r] - sum(mp.mpf(float(L[r, j])) * vs[j] for j in range(r))) / mp.mpf(float(L[r, r])))
            ak = np.array([float(abs(v)) for v in kv])
            for v_mp, tr, scale in ((vi, ti, np.abs(W) @ ak), (vs, ts, Linv @ ak)):
                for r in range(n):
                    got = mp.mpf(float(tr.v[a, r])) + mp.mpf(float(tr.v[a, r] - np.longdouble(float(tr.v[a, r]))))
                    assert abs(got - v_mp[r]) <= tol * scale[r]
                q = sum(v * v for v in v_mp)
                got = mp.mpf(float(tr.q[a])) + mp.mpf(float(tr.q[a] - np.longdouble(float(tr.q[a]))))
                assert abs(got - q) <= tol * float(q)


# ----------------------------------------------------------------------------------------------------------------------
# NumPy / SciPy and the restated order within the budgets, on the GPU file's cases; the guards
# ----------------------------------------------------------------------------------------------------------------------
INVERSE_CASES = ([(n, 8, None) for n in sr.ROW_BLOCK_N] + [(513, D, None) for D in sr.FEEDER_D if D != 8]
                 + [(513, D, P) for P, D in sr.LIN_CASES])
SOLVE_CASES = ([("planted", n, 8, None) for n in sr.ROW_BLOCK_N] + [("ill", 129, 8, None), ("ill", 449, 8, None)]
               + [("planted", 513, 2, None), ("planted", 513, 17, None), ("planted", 513, 8, 1)]
               + [("planted", n, D, None) for n in (2048, 2049) for D in (2, 8)])


def check_guards(tr, n):
    rel, decades, cancel = tr.guards()
    assert rel <= 1e-9
    assert decades >= 6.0
    assert cancel >= 20 or n == 1
    return rel, decades, cancel


@pytest.mark.parametrize("n,D,order", INVERSE_CASES)
def test_inverse_form_numpy_and_restated_order_within_budget(n, D, order):
    X, alpha, T, k, mean = sr.case(n, D, order)
    W = sr.planted_w(n)
    tr = sr.Truth(W, X, alpha, T, k, mean)
    g = check_guards(tr, n)
    kf = tr.kh.astype(np.float64)
    v = kf @ W.T
    r_np = (tr.mu_ratio(kf @ alpha + mean).max(), tr.var_ratio(np.asarray(tr.ktt, dtype=np.float64) - (v * v).sum(1)).max())
    mu, var = sr.restate(W, X, alpha, T, k, mean, kf=kf)
    r_re = (tr.mu_ratio(mu).max(), tr.var_ratio(var).max())
    print("inverse n=%-4d D=%-2d P=%-4s guards %.2g / %.1f / %-3d  NumPy mu %.3g var %.3g  restated mu %.3g var %.3g"
          % ((n, D, order) + g + r_np + r_re))
    assert max(r_np) <= 1.0 and max(r_re) <= 1.0


@pytest.mark.parametrize("family,n,D,order", SOLVE_CASES)
def test_solve_form_scipy_and_restated_order_within_budget(family, n, D, order):
    X, alpha, T, k, mean = sr.case(n, D, order)
    L, _ = fr.factor(family, n)
    la = np.abs(sr.inv_ld(L)).astype(np.float64) * (1.0 + 1e-9) if family == "ill" else None
    tr = sr.Truth(L, X, alpha, T, k, mean, form="solve", linv_abs=la)
    g = check_guards(tr, n)
    kf = tr.kh.astype(np.float64)
    v = solve_triangular(L, kf.T, lower=True).T
    r_sp = tr.var_ratio(np.asarray(tr.ktt, dtype=np.float64) - (v * v).sum(1)).max()
    mu, var = sr.restate(L, X, alpha, T, k, mean, kf=kf, form="solve")
    r_re = (tr.mu_ratio(mu).max(), tr.var_ratio(var).max())
    print("solve %-7s n=%-4d D=%-2d P=%-4s guards %.2g / %.1f / %-3d kappa4 %.3g  SciPy var %.3g  restated mu %.3g var %.3g"
          % ((family, n, D, order) + g + (sr.kappa4(L), r_sp) + r_re))
    assert r_sp <= 1.0 and max(r_re) <= 1.0


def test_long_double_inverse_matches_scipy():
    L, _ = fr.factor("ill", 129)
    ref = solve_triangular(L, np.eye(129), lower=True)
    got = sr.inv_ld(L).astype(np.float64)
    assert np.all(np.abs(got - ref) <= 1e-6 * (np.abs(np.tril(got)) @ np.abs(np.tril(L)) @ np.abs(np.tril(got))))


# ----------------------------------------------------------------------------------------------------------------------
# mutants
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [129, 449, 513, 769])
def test_mutants_exceed_the_budget_on_every_row(n):
    """Last row block of 129 rows (one block, predicated body), 193 (n = 449, predicated) and 1 (n = 513 and 769, the
    4-pair body).  Each mutant of the restated order must miss the var budget on every candidate row;
    "split_twice" the mu budget as well.  "parked_prev_block" and "split_twice" need a second row block."""
    X, alpha, T, k, mean = sr.case(n, 8)
    W = sr.planted_w(n)
    tr = sr.Truth(W, X, alpha, T, k, mean)
    kf = tr.kh.astype(np.float64)
    out = []
    for mt in sr.MUTANTS:
        if mt in ("parked_prev_block", "split_twice") and n <= 256:
            continue
        if mt == "stale_rows" and 32 * ((min(n - 256 * (sr.nrb(n) - 1), 256) + 31) >> 5) >= 256:
            continue
        mu, var = sr.restate(W, X, alpha, T, k, mean, kf=kf, mutant=mt)
        rv = tr.var_ratio(var)
        out.append("%s %.3g" % (mt, rv.min()))
        assert rv.min() > 1.0, (mt, rv.min())
        if mt == "split_twice":
            assert tr.mu_ratio(mu).min() > 1.0
    print("mutants n=%d: least |var - truth| / budget over the rows: %s" % (n, "  ".join(out)))


# ----------------------------------------------------------------------------------------------------------------------
# apgp_winv_apply
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trans", [0, 1])
@pytest.mark.parametrize("n", sr.WINV_N)
def test_winv_apply_numpy_restated_order_and_mutants(n, trans):
    W, b, shift = sr.winv_case(n)
    shift = 0.0 if trans else shift
    r_np = sr.winv_apply_ratio(W, (W.T if trans else W) @ (b - shift), b, shift, trans).max()
    r_re = sr.winv_apply_ratio(W, sr.winv_restate(W, b, shift, trans), b, shift, trans).max()
    out = []
    for mt in ("drop_last_row",) + (("chunk_twice",) if trans else ()):
        if n == 1:
            continue
        r = sr.winv_apply_ratio(W, sr.winv_restate(W, b, shift, trans, mutant=mt), b, shift, trans)
        # (trans = 0: row 0 has no column to lose; trans = 1: the last row / the last chunk reaches every column)
        hit = np.arange(n) >= (0 if trans else 1)
        out.append("%s %.3g" % (mt, r[hit].min()))
        assert r[hit].min() > 1.0, (mt, r[hit].min())
    print("winv_apply n=%-3d trans=%d NumPy %.3g restated %.3g %s" % (n, trans, r_np, r_re, "  ".join(out)))
    assert r_np <= 1.0 and r_re <= 1.0


# ----------------------------------------------------------------------------------------------------------------------
# the inverse's right residual
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,n", [("planted", n) for n in sr.TRTRI_N + (sr.TRTRI_BIG,)] + [("ill", n) for n in sr.TRTRI_N])
def test_trtri_bound_holds_for_scipy_and_the_restated_recursion(family, n):
    L, _ = fr.factor(family, n)
    big = n == sr.TRTRI_BIG
    rows = sr.trtri_big_rows(n) if big else None
    r_sp = sr.trtri_ratio(L, np.tril(solve_triangular(L, np.eye(n), lower=True)), rows).max()
    out = "trtri %-7s n=%-4d |L W - I| / bound: SciPy %.3g" % (family, n, r_sp)
    assert r_sp <= 1.0
    if not big:
        r_re = sr.trtri_ratio(L, sr.trtri_restate(L)).max()
        out += "  restated %.3g" % r_re
        assert r_re <= 1.0
        if n > 64:
            r_mt = sr.trtri_ratio(L, sr.trtri_restate(L, mutant="drop_k")).max()
            out += "  drop_k %.3g" % r_mt
            assert r_mt > 1.0
    print(out)


# ----------------------------------------------------------------------------------------------------------------------
# apgp_predict1_host
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["inverse", "solve"])
@pytest.mark.parametrize("n,D,order", sr.PRED1_CASES)
def test_predict1_numpy_and_restated_order_within_budget(n, D, order, form):
    X, alpha, T, k, mean = sr.case(n, D, order)
    T = T[:sr.PRED1_ROWS]
    A = sr.planted_w(n) if form == "inverse" else fr.factor("planted", n)[0]
    tr = sr.Truth(A, X, alpha, T, k, mean, form=form, consumer="predict1")
    kf = tr.kh.astype(np.float64)
    v = kf @ A.T if form == "inverse" else solve_triangular(A, kf.T, lower=True).T
    r_np = (tr.mu_ratio(kf @ alpha + mean).max(), tr.var_ratio(np.asarray(tr.ktt, dtype=np.float64) - (v * v).sum(1)).max())
    mu, var = sr.predict1_restate(A, X, alpha, T, k, mean, kf, form)
    r_re = (tr.mu_ratio(mu).max(), tr.var_ratio(var).max())
    print("predict1 %-7s n=%-3d D=%d P=%-4s NumPy mu %.3g var %.3g  restated mu %.3g var %.3g" % ((form, n, D, order) + r_np + r_re))
    assert max(r_np) <= 1.0 and max(r_re) <= 1.0


# ----------------------------------------------------------------------------------------------------------------------
# the sweep's own k*: site "sweep" of kvalue_ref
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 3, 8, 32])
def test_sweep_site_plain_is_cross_and_fused_is_within_budget(D):
    """The plain restatement of site "sweep" has "cross"'s bits; the fused one (the candidate's scaling contracted into
    the subtraction) differs from it on some rows, by a rounding of the exponent's argument only, is within
    kvalue_ref.budget of the truth like the plain one, and agrees with it bit for bit on a coincident point."""
    X, _, _, k, _ = sr.case(64, D)
    rs = np.random.RandomState(D)
    T = X[5] + rs.normal(size=(48, D)) * 1.5 / np.sqrt(k.inv_metric * D)
    T[0] = X[5]
    plain = kr.restate(T, X[5:6], k, site="sweep")
    fused = kr.restate(T, X[5:6], k, site="sweep", fused=True)
    assert same_bits(plain, kr.restate(T, X[5:6], k, site="cross"))
    assert plain[0, 0] == fused[0, 0] == k.amp
    assert np.any(plain != fused)
    for v in (plain, fused):
        r, _ = kr.err_over_budget(v, T, X[5:6], k)
        assert r <= 1.0
    with pytest.raises(ValueError):
        kr.restate(T, X[5:6], k._replace(lin_coef=0.1), site="sweep")
