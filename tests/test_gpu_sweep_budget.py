# -*- coding: utf-8 -*-
"""MI355X: the acquisition sweep's contraction and the two packed factor images it streams, each kernel alone through the
C ABI, each handed the bits it is judged on, against tests/sweep_ref.py (budgets derived from rounding counts read off
the kernel source, not fitted to device output; tests/test_sweep_ref.py holds NumPy / SciPy and the restated device
order to the same bars on the same inputs, and shows that each bar catches its mutants):

  1. apgp_trtri_pack    the packed image is pack_linv of the device's own dense panel, bit for bit, zeros included; the
                        right residual L W - I entry by entry against the bound of the inversion's own recursion;
  2. apgp_pack_lsolve   the image has the bits of the restated kernel everywhere (-L, the inverted 4 x 4 blocks, zeros);
  3. apgp_acquire       a PLANTED lower-triangular W (it need not be an inverse) and a planted alpha: mu and var of every
                        row within budget -- every row-block body, every launch path, every feeder instantiation, linear
                        terms, a box with a mask, a NaN row -- and the k* probe: one non-zero 2^48 in a zeroed image
                        makes -var == (2^48 mu)^2 exactly, so the B operand that reached the matrix cores is the value
                        the feeder produced, on the generating visit and on the parked reads; mu is then the sweep's own
                        k* and has the bits of one of kvalue_ref's two restatements of site "sweep" (hipcc contracts the
                        candidate's scaling into the subtraction on the first tile a workgroup generates);
  4. apgp_acquire_solve a planted factor through apgp_pack_lsolve's image: the same, with the forward bound of a solve
                        that multiplies by inverted 4 x 4 blocks; both sides of S2_STATIC_DIAG_NRB; the probe with a
                        factor of powers of two; the two forms against each other;
  5. apgp_winv_apply    both products from the bits of a planted W, NaN wherever the kernels promise not to read;
     apgp_predict1_host through a planted W (three launches, and the single launch at n <= 256) and through L.

Launch paths of the inverse form (launch_sweep, csrc/sweep.hip:1120-1145): with ``part`` given and n > 256 a call of at
most 184 candidate blocks is SPLIT by row block (m = 130 included); the persistent grid runs from 185 blocks on.  The
row-block and feeder cases therefore run twice, at m = 130 (split) and at 200 or 335 blocks (persistent, persistent +
split).

Worst figures are printed (pytest -s) and recorded in docs/experiments.md, round 14."""
import ctypes

import numpy as np
import pytest

import factor_ref as fr
import kvalue_ref as kr
import sweep_ref as sr

pytestmark = pytest.mark.gpu

SENTINEL = -1.2345678901234567e300
UTIL_NONE = 3
BIG = 2.0 ** 48


@pytest.fixture(scope="module")
def lib_loaded():
    from approxposterior_amd import _lib
    lib = _lib.load()
    assert lib.apgp_abi_version() == _lib.ABI_VERSION
    return lib


def _ks(k):
    from approxposterior_amd import _lib
    ks = _lib.KernelStruct()
    ks.ndim, ks.lin_order, ks.amp, ks.diag_add, ks.lin_coef = k.ndim, k.lin_order, k.amp, k.diag_add, k.lin_coef
    ks.inv_metric[:k.ndim] = k.inv_metric.tolist()
    return ks


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to("cuda:0")


def _full(shape, value=SENTINEL):
    import torch
    return torch.full(shape, value, dtype=torch.float64, device="cuda:0")


def _ok(lib, rc, what):
    assert rc == 0, (what, rc, lib.apgp_last_error())


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def padded(M, ld, fill=SENTINEL):
    n = len(M)
    buf = np.full((n, ld), fill)
    low = np.tril(np.ones((n, n), dtype=bool))
    buf[:, :n][low] = M[low]
    return buf


def image_families(n):
    return ("planted", "ill") if n <= 17 else ("planted",)


# ----------------------------------------------------------------------------------------------------------------------
# 1. apgp_trtri_pack: the image
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", sr.IMAGE_N + (sr.IMAGE_BIG,))
def test_trtri_pack_image_is_the_packed_panel(lib_loaded, n):
    import torch
    lib = lib_loaded
    assert int(lib.apgp_packed_linv_len(n)) == sr.packed_len(n)
    np64 = fr.TILE * fr.nblocks(n)
    for family in image_families(n):
        L, _ = fr.factor(family, n)
        seen = set()
        for ldl in ((n,) if n == sr.IMAGE_BIG else (n, n + 3)):
            Ld = _dev(padded(L, ldl))
            work = _full((int(lib.apgp_trtri_work_len(n)),))
            packed = _full((sr.packed_len(n),))
            Wd = _full((n, n))
            _ok(lib, lib.apgp_trtri_pack(Ld.data_ptr(), n, ldl, work.data_ptr(), packed.data_ptr(), Wd.data_ptr(), None),
                "apgp_trtri_pack")
            torch.cuda.synchronize()
            panel = work[:np64 * np64].cpu().numpy().reshape(np64, np64)
            assert np.all(np.isfinite(panel))
            assert same_bits(Wd.cpu().numpy(), panel[:n, :n]), "winv_dense is not the panel"
            assert not np.any(np.triu(panel, 1)), "the panel is not lower triangular"
            img = packed.cpu().numpy()
            assert same_bits(img, sr.pack_linv(panel, n)), "the packed image is not pack_linv of the panel"
            seen.add(img.tobytes())
            del Ld, work, packed, Wd
        assert len(seen) == 1, "the leading dimension changed a bit of the image"
        print("trtri_pack image %-7s n=%-4d %d tiles: bit for bit" % (family, n, sr.ntiles(n)))


@pytest.mark.parametrize("family,n", [("planted", n) for n in sr.TRTRI_N + (sr.TRTRI_BIG,)] + [("ill", n) for n in sr.TRTRI_N])
def test_trtri_right_residual_within_recursive_bound(lib_loaded, family, n):
    """n = 2100: 33 blocks, the level-16 merge takes two complementary tiles per workgroup; the residual is formed on
    sweep_ref.trtri_big_rows only (every 17th row of the blocks that merge writes, and the last)."""
    import torch
    lib = lib_loaded
    L, _ = fr.factor(family, n)
    rows = sr.trtri_big_rows(n) if n == sr.TRTRI_BIG else None
    seen = {}
    for ldl in (n, n + 3):
        Ld = _dev(padded(L, ldl))
        work = _full((int(lib.apgp_trtri_work_len(n)),))
        Wd = _full((n, n))
        _ok(lib, lib.apgp_trtri_pack(Ld.data_ptr(), n, ldl, work.data_ptr(), None, Wd.data_ptr(), None), "apgp_trtri_pack")
        torch.cuda.synchronize()
        W = Wd.cpu().numpy()
        assert not np.any(np.triu(W, 1))
        key = W.tobytes()
        if key not in seen:
            seen[key] = sr.trtri_ratio(L, W, rows).max()
        del Ld, work, Wd
    r = list(seen.values())[0]
    print("trtri %-7s n=%-4d worst |L W - I| / bound %.3f" % (family, n, r))
    assert r <= 1.0
    assert len(seen) == 1, "the leading dimension changed a bit of the inverse"


# ----------------------------------------------------------------------------------------------------------------------
# 2. apgp_pack_lsolve: the image
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", sr.IMAGE_N + (sr.IMAGE_BIG,))
def test_pack_lsolve_image_has_the_restated_bits(lib_loaded, n):
    import torch
    lib = lib_loaded
    assert int(lib.apgp_packed_lsolve_len(n)) == sr.packed_len(n)
    for family in image_families(n):
        L, _ = fr.factor(family, n)
        want = sr.pack_lsolve(L, n)
        for ldl in ((n,) if n == sr.IMAGE_BIG else (n, n + 3)):
            Ld = _dev(padded(L, ldl))
            packed = _full((sr.packed_len(n),))
            _ok(lib, lib.apgp_pack_lsolve(Ld.data_ptr(), n, ldl, packed.data_ptr(), None), "apgp_pack_lsolve")
            torch.cuda.synchronize()
            img = packed.cpu().numpy()
            bad = np.nonzero(img.view(np.int64) != want.view(np.int64))[0]
            assert len(bad) == 0, (family, n, ldl, len(bad), bad[:8], img[bad[:8]], want[bad[:8]])
            del Ld, packed
        print("pack_lsolve image %-7s n=%-4d %d tiles: bit for bit" % (family, n, sr.ntiles(n)))


# ----------------------------------------------------------------------------------------------------------------------
# the sweep through the C ABI
# ----------------------------------------------------------------------------------------------------------------------
class Model(object):
    """A planted model on the device: the packed image (of W, or of L through apgp_pack_lsolve) and the packed training
    stream; ``truth`` judges what comes back."""

    def __init__(self, lib, n, D, order=None, form="inverse", family="planted", A=None):
        import torch
        self.lib, self.n, self.form = lib, n, form
        self.X, self.alpha, self.T, self.k, self.mean = sr.case(n, D, order)
        if form == "inverse":
            self.A = sr.planted_w(n) if A is None else A
            self.packed = _dev(sr.pack_linv(self.A, n))
            self.truth = sr.Truth(self.A, self.X, self.alpha, self.T, self.k, self.mean)
        else:
            self.A = fr.factor(family, n)[0] if A is None else A
            self.packed = _full((sr.packed_len(n),))
            Ld = _dev(padded(self.A, n))
            _ok(lib, lib.apgp_pack_lsolve(Ld.data_ptr(), n, n, self.packed.data_ptr(), None), "apgp_pack_lsolve")
            la = np.abs(sr.inv_ld(self.A)).astype(np.float64) * (1.0 + 1e-9) if family == "ill" else None
            self.truth = sr.Truth(self.A, self.X, self.alpha, self.T, self.k, self.mean, form="solve", linv_abs=la)
        self.ks = _ks(self.k)
        self.xs = _full((int(lib.apgp_packed_train_len(n, D)),))
        Xd, ad = _dev(self.X), _dev(self.alpha)
        _ok(lib, lib.apgp_pack_train(Xd.data_ptr(), ad.data_ptr(), n, ctypes.byref(self.ks), self.xs.data_ptr(), None),
            "apgp_pack_train")
        torch.cuda.synchronize()

    def sweep(self, Tm, part=True, lo=None, hi=None, mask=None, mean=None, xs=None, packed=None):
        return run_sweep(self.lib, self.form != "inverse", self.packed if packed is None else packed,
                         self.xs if xs is None else xs, self.n, self.ks, self.mean if mean is None else mean, Tm,
                         part, lo, hi, mask)

    def check_guards(self, what):
        rel, decades, cancel = self.truth.guards()
        print("%s guards: worst dq / q %.3g, k^ spans %.1f decades, %d rows with sum|alpha||k^| >= 10 |mu|"
              % (what, rel, decades, cancel))
        assert rel <= 1e-9
        assert decades >= 6.0
        # (one training point: mu - mean is a single product and cannot cancel)
        assert cancel >= 20 or self.n == 1

    def judge(self, mu, var, what, skip=()):
        keep = np.ones(len(mu), dtype=bool)
        keep[list(skip)] = False
        rm = self.truth.mu_ratio(np.where(keep, mu, 0.0))
        rv = self.truth.var_ratio(np.where(keep, var, 0.0))
        rm, rv = rm[keep], rv[keep]
        print("%s m=%-5d worst |mu - truth| / budget %.3f, |var - truth| / budget %.3f" % (what, len(mu), rm.max(), rv.max()))
        assert rm.max() <= 1.0, (what, int(np.argmax(rm)), rm.max())
        assert rv.max() <= 1.0, (what, int(np.argmax(rv)), rv.max())
        return rm.max(), rv.max()


_MODELS = {}


def model(lib, n, D, order=None, form="inverse", family="planted"):
    """One Model (and one truth) per case, shared by the tests that use it and never changed."""
    key = (n, D, order, form, family)
    if key not in _MODELS:
        _MODELS[key] = Model(lib, n, D, order, form, family)
    return _MODELS[key]


def run_sweep(lib, solve, packed, xs, n, ks, mean, Tm, part=True, lo=None, hi=None, mask=None):
    """(mu, var) of apgp_acquire / apgp_acquire_solve with kind = APGP_UTIL_NONE, best = NULL; outputs and scratch
    pre-filled with the sentinel."""
    import torch
    from approxposterior_amd import _lib
    m = len(Tm)
    Td = _dev(Tm)
    mu, var = _full((m,)), _full((m,))
    pd = _full((max(int(lib.apgp_acquire_work_len(m, n)), 2),)) if part else None
    box = [None, None]
    if lo is not None:
        box = [(ctypes.c_double * _lib.MAX_DIM)(*(list(v) + [0.0] * (_lib.MAX_DIM - len(v)))) for v in (lo, hi)]
    md = torch.from_numpy(np.ascontiguousarray(mask, dtype=np.uint8)).to("cuda:0") if mask is not None else None
    fn = lib.apgp_acquire_solve if solve else lib.apgp_acquire
    _ok(lib, fn(Td.data_ptr(), m, 0, packed.data_ptr(), xs.data_ptr(), n, ctypes.byref(ks), mean, UTIL_NONE, box[0], box[1],
                md.data_ptr() if md is not None else None, 0.0, 0.0, mu.data_ptr(), var.data_ptr(), None,
                pd.data_ptr() if pd is not None else None, None, None), "apgp_acquire")
    torch.cuda.synchronize()
    return mu.cpu().numpy(), var.cpu().numpy()


M_PERSIST = sr.m_of_blocks(200)                  # one short persistent round, nothing split
M_PERSIST_SPLIT = sr.m_of_blocks(256 + 79)       # a full round, then 79 blocks split by row block + the finish kernel
M_THREE_ROUNDS = sr.m_of_blocks(2 * 256 + 213)   # three rounds: the parking slots are used again, nothing split


# ----------------------------------------------------------------------------------------------------------------------
# 3. the contraction, inverse form, planted W
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", sr.ROW_BLOCK_N)
def test_inverse_form_row_block_bodies(lib_loaded, n):
    """4-pair (<= 128 rows in the last block), 6-pair (<= 192), predicated and full bodies, one to four row blocks."""
    mdl = model(lib_loaded, n, 8)
    mdl.check_guards("inverse n=%d" % n)
    mu, var = mdl.sweep(sr.tiled(mdl.T, sr.M_SMALL))
    mdl.judge(mu, var, "inverse n=%-4d D=8 %s" % (n, "split" if n > 256 else "persistent"))
    if n <= 256:
        mu0, var0 = mdl.sweep(sr.tiled(mdl.T, sr.M_SMALL), part=False)
        assert same_bits(mu0, mu) and same_bits(var0, var), "part = NULL changed a bit"
    mu, var = mdl.sweep(sr.tiled(mdl.T, M_PERSIST))
    mdl.judge(mu, var, "inverse n=%-4d D=8 persistent" % n)


@pytest.mark.parametrize("m", [1, 63, 64, 65, M_PERSIST, M_PERSIST_SPLIT, M_THREE_ROUNDS])
def test_inverse_form_launch_paths(lib_loaded, m):
    mdl = model(lib_loaded, 513, 8)
    mu, var = mdl.sweep(sr.tiled(mdl.T, m))
    mdl.judge(mu, var, "inverse n=513 D=8 launch path")


@pytest.mark.parametrize("D", sr.FEEDER_D)
def test_inverse_form_feeder_instantiations(lib_loaded, D):
    """Every DPAD; the structured feeders at 2 / 4 / 16, the plain ones at 8 / 32."""
    mdl = model(lib_loaded, 513, D)
    mdl.check_guards("inverse n=513 D=%d" % D)
    for m in (sr.M_SMALL, M_PERSIST_SPLIT):
        mu, var = mdl.sweep(sr.tiled(mdl.T, m))
        mdl.judge(mu, var, "inverse n=513 D=%-2d" % D)


@pytest.mark.parametrize("order,D", sr.LIN_CASES)
def test_inverse_form_linear_term(lib_loaded, order, D):
    mdl = model(lib_loaded, 513, D, order)
    mdl.check_guards("inverse n=513 D=%d P=%d" % (D, order))
    for m in (sr.M_SMALL, M_PERSIST_SPLIT):
        mu, var = mdl.sweep(sr.tiled(mdl.T, m))
        mdl.judge(mu, var, "inverse n=513 D=%-2d P=%d" % (D, order))


@pytest.mark.parametrize("m", [sr.M_SMALL, M_PERSIST_SPLIT])
def test_inverse_form_box_mask_and_nan_row(lib_loaded, m):
    """kind = NONE: a box and a mask gate the utility only -- mu and var of gated rows are written all the same; a row
    with a NaN coordinate gives mu = var = NaN and leaves its neighbours alone."""
    mdl = model(lib_loaded, 513, 8)
    Tm = sr.tiled(mdl.T, m)
    lo, hi = np.median(mdl.T, axis=0) - 1e-3, mdl.T.max(0) + 1.0
    mask = (np.arange(m) % 3 != 1)
    mu, var = mdl.sweep(Tm, lo=lo, hi=hi, mask=mask)
    mdl.judge(mu, var, "inverse n=513 D=8 box+mask")
    mu_plain, var_plain = mdl.sweep(Tm)
    assert same_bits(mu, mu_plain) and same_bits(var, var_plain), "the gate changed a bit of mu / var"
    Tn = Tm.copy()
    bad = [77] + ([m - 5] if m > 200 else [])
    for b in bad:
        Tn[b, 3] = np.nan
    mu, var = mdl.sweep(Tn)
    assert np.all(np.isnan(mu[bad])) and np.all(np.isnan(var[bad]))
    keep = np.ones(m, dtype=bool)
    keep[bad] = False
    assert same_bits(mu[keep], mu_plain[keep]) and same_bits(var[keep], var_plain[keep]), "a NaN row touched another row"


# ---- the k* probe ----------------------------------------------------------------------------------------------------
PROBE_N = 769
PROBE_ALL_RESIDUES = tuple(17 * j for j in range(16))          # c mod 16 = 0 .. 15, sixteen different chunks, all < 256
PROBE_FEW = (0, 5, 15, PROBE_N - 1)


def probe_points(X, k, c, lin):
    """BASE candidates at most 3.5 length scales from x_c (a box: exp(-3.5^2 / 2) = 2^-8.8).  2^-20 <= |k_c| is
    asserted on the truth: q >= 2^56 then absorbs amp; |k_c| <= 16 is far from anything that could overflow."""
    rs = np.random.RandomState(8000 + c)
    ell = 1.0 / np.sqrt(k.inv_metric)
    T = X[c] + ell * rs.uniform(-1.0, 1.0, size=(sr.BASE, k.ndim)) * 3.5 / np.sqrt(k.ndim)
    T[0] = X[c]                                                 # the coincident point: k_c = amp exactly
    with np.errstate(all="ignore"):
        t = np.abs(kr.truth_ld(T, X[c:c + 1], k)[:, 0]).astype(np.float64)
    assert t.min() >= 2.0 ** -20 and t.max() <= 16.0
    return T


def probe_rows(c, n):
    return [r for r in (c, c + 256, c + 512) if r < n]


def check_probe(mu, var, want_mu, bud, what):
    m = len(mu)
    assert np.all(np.isfinite(mu)) and np.all(np.isfinite(var)), what
    sq = (BIG * mu) * (BIG * mu)                                # 2^48 mu is exact; the square rounds once
    bad = np.nonzero(-var != sq)[0]
    assert len(bad) == 0, (what, "the B operand is not the feeder's value", len(bad), bad[:8], mu[bad[:8]], var[bad[:8]])
    if bud is None:
        # want_mu: the two restatements of site "sweep" (plain, fused); a device value has the bits of one of them
        rep = [w[np.arange(m) % len(w)] for w in want_mu]
        hit = [mu.view(np.int64) == r.view(np.int64) for r in rep]
        bad = np.nonzero(~(hit[0] | hit[1]))[0]
        assert len(bad) == 0, (what, "k* has the bits of neither restatement", len(bad), bad[:8], mu[bad[:8]], rep[0][bad[:8]])
        return int((hit[1] & ~hit[0]).sum())
    rep = want_mu[np.arange(m) % len(want_mu)]
    assert np.all(np.abs(mu - rep) <= bud[np.arange(m) % len(bud)]), what
    return 0


def run_probe(lib, form, D, cols, order=None):
    import torch
    n = PROBE_N
    X, _, _, k, _ = sr.case(n, D, order)
    k = k._replace(amp=1.0)
    ks = _ks(k)
    lin = order is not None
    Xd = _dev(X)
    xs = _full((int(lib.apgp_packed_train_len(n, D)),))
    packed = torch.zeros(sr.packed_len(n), dtype=torch.float64, device="cuda:0")
    launches = 0
    fused_rows = {}
    for c in cols:
        T = probe_points(X, k, c, lin)
        if lin:
            want = kr.truth_ld(T, X[c:c + 1], k)[:, 0].astype(np.float64)
            bud = kr.budget(T, X[c:c + 1], k)[:, 0] + kr.ulp(want)     # (the truth was rounded to double)
        else:
            want = [kr.restate(T, X[c:c + 1], k, site="sweep", fused=f)[:, 0] for f in (False, True)]
            assert same_bits(want[0], kr.restate(T, X[c:c + 1], k, site="cross")[:, 0])
            bud = None
        alpha = np.zeros(n)
        alpha[c] = 1.0
        ad = _dev(alpha)
        _ok(lib, lib.apgp_pack_train(Xd.data_ptr(), ad.data_ptr(), n, ctypes.byref(ks), xs.data_ptr(), None), "apgp_pack_train")
        for r in probe_rows(c, n):
            if form == "inverse":
                idx = sr.packed_index(r, c)
                packed[idx] = BIG
            else:
                L = np.diag(np.full(n, 2.0 ** 600))
                L[r, r] = 2.0 ** 152
                if r != c:
                    L[r, c] = -2.0 ** 800
                else:                                           # v_c = 2^48 k_c from the pivot itself
                    L[c, c] = 2.0 ** -48
                Ld = _dev(L)
                _ok(lib, lib.apgp_pack_lsolve(Ld.data_ptr(), n, n, packed.data_ptr(), None), "apgp_pack_lsolve")
            for m in (65, M_PERSIST):
                mu, var = run_sweep(lib, form != "inverse", packed, xs, n, ks, 0.0, sr.tiled(T, m))
                nf = check_probe(mu, var, want, bud, (form, D, order, c, r, m))
                if nf:
                    fused_rows[(c, r, m)] = nf
                launches += 1
            if form == "inverse":
                packed[idx] = 0.0
    print("k* probe %s D=%-2d P=%s: %d columns, %d launches, -var == (2^48 mu)^2 and mu == k* on every row; rows that "
          "differ from the plain restatement and have the fused one's bits, by (column, row, m): %s"
          % (form, D, order, len(cols), launches, fused_rows))
    # the contraction is the compiler's and sits where produce_b follows load_candidates: the first chunk only
    assert all(c < 16 for c, _, _ in fused_rows), fused_rows


@pytest.mark.parametrize("D", sr.FEEDER_D)
def test_inverse_form_kstar_probe(lib_loaded, D):
    """All sixteen residues of c mod 16 for one structured (D = 3) and one plain (D = 8) feeder, four columns for the
    others; rows in c's row block (the generating visit) and one and two row blocks later (the parked read); a split
    launch (m = 65) and a persistent one (200 blocks)."""
    run_probe(lib_loaded, "inverse", D, PROBE_ALL_RESIDUES + (PROBE_N - 1,) if D in (3, 8) else PROBE_FEW)


def test_inverse_form_kstar_probe_linear_term(lib_loaded):
    run_probe(lib_loaded, "inverse", 3, PROBE_FEW, order=2)


# ----------------------------------------------------------------------------------------------------------------------
# 4. the contraction, substitution form, planted L
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", sr.ROW_BLOCK_N)
def test_solve_form_row_block_bodies(lib_loaded, n):
    mdl = model(lib_loaded, n, 8, form="solve")
    mdl.check_guards("solve n=%d" % n)
    print("solve n=%d kappa4 %.3g" % (n, sr.kappa4(mdl.A)))
    for m in (sr.M_SMALL, M_PERSIST):
        mu, var = mdl.sweep(sr.tiled(mdl.T, m))
        mdl.judge(mu, var, "solve planted n=%-4d D=8" % n)


@pytest.mark.parametrize("n", [129, 449])
def test_solve_form_ill_conditioned_factor(lib_loaded, n):
    mdl = model(lib_loaded, n, 8, form="solve", family="ill")
    mdl.check_guards("solve ill n=%d" % n)
    print("solve ill n=%d kappa4 %.3g" % (n, sr.kappa4(mdl.A)))
    for m in (sr.M_SMALL, M_PERSIST):
        mu, var = mdl.sweep(sr.tiled(mdl.T, m))
        mdl.judge(mu, var, "solve ill n=%-4d D=8" % n)


@pytest.mark.parametrize("D,order", [(2, None), (8, None), (17, None), (8, 1)])
def test_solve_form_feeders_and_linear_term(lib_loaded, D, order):
    """D = 2 is the solve form's only structured feeder."""
    mdl = model(lib_loaded, 513, D, order, form="solve")
    mdl.check_guards("solve n=513 D=%d P=%s" % (D, order))
    for m in (sr.M_SMALL, M_PERSIST_SPLIT):
        mu, var = mdl.sweep(sr.tiled(mdl.T, m))
        mdl.judge(mu, var, "solve planted n=513 D=%-2d P=%s" % (D, order))


@pytest.mark.parametrize("D", [2, 8])
@pytest.mark.parametrize("n", [2048, 2049])
def test_solve_form_either_side_of_the_static_diagonal(lib_loaded, n, D):
    """n = 2048: eight row blocks, the statically unrolled diagonal tiles; n = 2049: nine, the run-time-indexed ones.
    n = 2049, D = 8 once more with 256 + 40 candidate blocks: the parked V are used again in a second round."""
    mdl = model(lib_loaded, n, D, form="solve")
    mdl.check_guards("solve n=%d D=%d" % (n, D))
    for m in (sr.M_SMALL,) + ((sr.m_of_blocks(256 + 40),) if (n, D) == (2049, 8) else ()):
        mu, var = mdl.sweep(sr.tiled(mdl.T, m))
        mdl.judge(mu, var, "solve planted n=%-4d D=%d" % (n, D))


@pytest.mark.parametrize("D", [2, 8])
def test_solve_form_kstar_probe(lib_loaded, D):
    """L = 2^600 I with L_rr = 2^152 and L_rc = -2^800: v_r = 2^48 k_c exactly, every other v^2 underflows to zero,
    k*_r is absorbed by the 2^200 k_c it is added to (tests/test_sweep_ref.py checks the image's exponents)."""
    run_probe(lib_loaded, "solve", D, PROBE_FEW)


def test_the_two_forms_agree_within_their_budgets(lib_loaded):
    """One factor; W = the device's apgp_trtri_pack of it.  var of the two forms on the same rows differs by at most
    the sum of the two budgets (each taken against its own truth: the truths differ by the inverse's own error, which
    the right residual bounds -- added below as 2 |v| |W| |L W - I| |k^|)."""
    import torch
    lib = lib_loaded
    n, D = 513, 8
    slv = model(lib, n, D, form="solve")
    Ld = _dev(slv.A)
    work = _full((int(lib.apgp_trtri_work_len(n)),))
    Wd = _full((n, n))
    _ok(lib, lib.apgp_trtri_pack(Ld.data_ptr(), n, n, work.data_ptr(), None, Wd.data_ptr(), None), "apgp_trtri_pack")
    torch.cuda.synchronize()
    W = Wd.cpu().numpy()
    inv = Model(lib, n, D, form="inverse", A=W)
    Tm = sr.tiled(slv.T, sr.M_SMALL)
    _, var_s = slv.sweep(Tm)
    _, var_i = inv.sweep(Tm)
    slv.judge(np.asarray(slv.truth.mu, dtype=np.float64)[np.arange(len(Tm)) % sr.BASE], var_s, "forms: solve")
    inv.judge(np.asarray(inv.truth.mu, dtype=np.float64)[np.arange(len(Tm)) % sr.BASE], var_i, "forms: inverse")
    rep = np.arange(len(Tm)) % sr.BASE
    res = np.abs(np.tril(slv.A).astype(sr.LD) @ W.astype(sr.LD) - np.eye(n, dtype=sr.LD)).astype(np.float64)
    ak = np.abs(slv.truth.kh).astype(np.float64)
    gap = (2.0 * np.abs(slv.truth.v).astype(np.float64) * ((ak @ res.T) @ np.abs(W).T)).sum(1) * (1.0 + 1e-6)
    bound = (slv.truth.dq + inv.truth.dq + gap)[rep] + sr.U * (np.abs(var_s) + np.abs(var_i))
    r = np.abs(var_s - var_i) / bound
    print("forms n=513 D=8: worst |var_solve - var_inverse| / (sum of budgets) %.3f" % r.max())
    assert r.max() <= 1.0


# ----------------------------------------------------------------------------------------------------------------------
# 5. apgp_winv_apply
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trans", [0, 1])
@pytest.mark.parametrize("n", sr.WINV_N)
def test_winv_apply_within_depth_bound(lib_loaded, n, trans):
    """The panel is NaN above the diagonal and in its padding (sweep_ref.winv_panel: the one f64x2 partner the forward
    kernel loads keeps a zero): a NaN in x is a read outside the contract."""
    import torch
    lib = lib_loaded
    W, b, shift = sr.winv_case(n)
    shift = 0.0 if trans else shift
    P = sr.winv_panel(W)
    Pd, bd = _dev(P), _dev(b)
    x, ss = _full((n + 8,)), _full((1,))
    work = _full((max(int(lib.apgp_winv_apply_work_len(n)), 1),))
    _ok(lib, lib.apgp_winv_apply(Pd.data_ptr(), P.shape[1], n, bd.data_ptr(), shift, trans, x.data_ptr(), ss.data_ptr(),
                                 work.data_ptr(), None), "apgp_winv_apply")
    torch.cuda.synchronize()
    out = x.cpu().numpy()
    assert same_bits(out[n:], np.full(8, SENTINEL)), "written past n"
    assert same_bits(bd.cpu().numpy(), b) and same_bits(Pd.cpu().numpy(), P), "an input was written"
    r = sr.winv_apply_ratio(W, out[:n], b, shift, trans).max()
    t, bound = fr.sumsq_bound(out[:n])
    es = abs(float(np.longdouble(float(ss.item())) - t))
    print("winv_apply n=%-3d trans=%d worst |x - truth| / bound %.3f, |ss - x.x| / bound %.3f" % (n, trans, r, es / bound if bound else 0.0))
    assert r <= 1.0
    assert es <= bound


@pytest.mark.parametrize("form", ["inverse", "solve"])
@pytest.mark.parametrize("n,D,order", sr.PRED1_CASES)
def test_predict1_within_budget(lib_loaded, n, D, order, form):
    """One call per candidate.  Through winv the three-launch path (apgp_potrf_mode(1)) and, at n <= 256, the single
    launch: both within budget (test_gpu_parity.py holds them to the same bits)."""
    import torch
    lib = lib_loaded
    X, alpha, T, k, mean = sr.case(n, D, order)
    T = np.ascontiguousarray(T[:sr.PRED1_ROWS])
    ks = _ks(k)
    xs = _full((int(lib.apgp_packed_train_len(n, D)),))
    Xd, ad = _dev(X), _dev(alpha)
    _ok(lib, lib.apgp_pack_train(Xd.data_ptr(), ad.data_ptr(), n, ctypes.byref(ks), xs.data_ptr(), None), "apgp_pack_train")
    if form == "inverse":
        A = sr.planted_w(n)
        ld = (n + 63) // 64 * 64
        Ad = _dev(np.pad(A, ((0, 0), (0, ld - n))))
    else:
        A = fr.factor("planted", n)[0]
        ld = n
        Ad = _dev(padded(A, n))
    tr = sr.Truth(A, X, alpha, T, k, mean, form=form, consumer="predict1")
    work = _full((int(lib.apgp_predict1_work_len(n)),))
    torch.cuda.synchronize()
    modes = [1] + ([0] if form == "inverse" and n <= 256 else [])
    prev = lib.apgp_potrf_mode(-1)
    try:
        for mode in modes:
            lib.apgp_potrf_mode(mode)
            out = np.full((len(T), 2), np.nan)
            for a in range(len(T)):
                _ok(lib, lib.apgp_predict1_host(T[a].ctypes.data, xs.data_ptr(), n, ctypes.byref(ks), mean,
                                                Ad.data_ptr() if form == "inverse" else None, ld,
                                                Ad.data_ptr() if form != "inverse" else None, ld, work.data_ptr(),
                                                out[a].ctypes.data, None), "apgp_predict1_host")
            torch.cuda.synchronize()
            rm, rv = tr.mu_ratio(out[:, 0]).max(), tr.var_ratio(out[:, 1]).max()
            print("predict1 %-7s n=%-3d D=%d P=%-4s %s: worst |mu - truth| / budget %.3f, |var - truth| / budget %.3f"
                  % (form, n, D, order, "three launches" if mode == 1 or form != "inverse" else "one launch", rm, rv))
            assert rm <= 1.0 and rv <= 1.0
    finally:
        lib.apgp_potrf_mode(prev)
