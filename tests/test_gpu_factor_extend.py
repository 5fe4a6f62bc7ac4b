# -*- coding: utf-8 -*-
"""MI355X: the appended-row factor chain -- GP.compute(x, previous=gp), the only way the main loop grows its factor
between hyper-parameter refits -- against the condition-free budgets of tests/extend_ref.py (rounding counts read off
the kernel source; tests/test_extend_ref.py holds a restatement to the same bars on the same inputs and shows that
each bar catches its mutants):

  a. apgp_append_diag   alone through the C ABI: the pivot bar on success, *ljj == 1.0 and the FIRST failing order on
                        failure, over equal / smaller / NaN / infinite / subnormal operands and a set info word;
  b. apgp_fit_summary / apgp_logdet   planted factors, NaN everywhere off the lower triangle, three leading dimensions
                        with the same bits, with and without z and info;
  c. rows by substitution   one chain of GP objects per case, a fresh GP per appended row as ApproxPosterior._absorbPoint
                        makes them: every row and pivot inside its bar on the right-hand side the test obtains itself
                        (apgp_kernel_cross with _try_extend's arguments: the same call, the same bits), the parent's rows
                        bit for bit, exact zeros above the diagonal; the tip's |A - L L^T| entry by entry and its
                        log-determinant, condition estimate and constant from its own bits; the row-count rules;
  d. the W route        the first appended row has the bits of the test's own apgp_winv_apply on the parent's panel at
                        leading dimension (n0 + 63) // 64 * 64, inside the product's bar; "solve" keeps substitution;
  e. the store          in-place appends, a second child, growth, a failed pivot: who owns which buffer, and that no
                        owner's bits move;
  f. downstream         the tip at the store's leading dimension (256, every row 16-byte aligned) against a twin with
                        the same bits in a compact n x n factor: the same bits out of every consumer.

Worst figures are printed (pytest -s) and recorded in docs/experiments.md, round 28."""
import ctypes

import numpy as np
import pytest

import extend_ref as er
import factor_ref as fr

pytestmark = pytest.mark.gpu

NAN = float("nan")


@pytest.fixture(scope="module")
def lib_loaded():
    from approxposterior_amd import _lib
    lib = _lib.load()
    assert lib.apgp_abi_version() == _lib.ABI_VERSION
    return lib


def _dev(a, dtype=np.float64):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to("cuda:0")


def _ok(lib, rc, what):
    assert rc == 0, (what, rc, lib.apgp_last_error())


same_bits = er.fr_same_bits


def make_gp(D, wn, P=None, metric=None):
    from approxposterior_amd import gp as agp
    kernel = agp.ExpSquaredKernel(np.full(D, float(D)) if metric is None else metric, ndim=D)
    if P is not None:
        kernel = kernel + agp.LinearKernel(log_gamma2=-np.log(er.LIN_COEF), order=P, ndim=D)
    return agp.GP(kernel=kernel, fit_mean=True, mean=0.25, white_noise=wn, fit_white_noise=False)


def factor_bits(gp):
    """The n x n factor of ``gp`` as the host sees it through its (possibly strided) view."""
    import torch
    torch.cuda.synchronize()
    return gp._L.cpu().numpy()


def cross_row(lib, gp, j):
    """(k(x_j, X[:j]), kdiag) as GP._try_extend obtains them for row j of ``gp``: the same apgp_kernel_cross call on the
    grown GP's own device points, and the host's k(x, x) + diag_add."""
    import torch
    n1 = len(gp._x)
    ks = gp._kernel_struct()
    row = torch.full((n1,), NAN, dtype=torch.float64, device="cuda:0")
    _ok(lib, lib.apgp_kernel_cross(gp._x_d[j:].data_ptr(), 1, gp._x_d.data_ptr(), j, ctypes.byref(ks), row.data_ptr(),
                                   n1, None), "apgp_kernel_cross")
    torch.cuda.synchronize()
    kxx = ks.amp
    if ks.lin_coef != 0.0:
        kxx += ks.lin_coef * float(np.sum((gp._x[j] * gp._x[j]) ** ks.lin_order))
    return row.cpu().numpy()[:j], kxx + ks.diag_add


def check_rows(lib, child, Lp):
    """The row checks of (c) for every row ``child`` appended to a parent whose factor bits are ``Lp``: returns the
    child's factor bits, the cross rows, the diagonals and the worst (row, pivot) ratios."""
    n0, n1 = len(Lp), len(child._x)
    assert child._L_store is not None, "refactorised instead of extended"
    assert child._ld == child._L_store["buf"].shape[1] and child._L_store["used"] == n1
    Lc = factor_bits(child)
    assert Lc.shape == (n1, n1)
    assert same_bits(Lc[:n0, :n0], Lp), "the parent's rows changed on their way into the child"
    assert not np.triu(Lc, 1).view(np.int64).any(), "something above the diagonal is not +0.0"
    rows, diags, wr, wp = [], [], 0.0, 0.0
    for j in range(n0, n1):
        k, kdiag = cross_row(lib, child, j)
        rows.append(k)
        diags.append(kdiag)
        r, p = float(er.row_ratio(Lc, Lc[j, :j], k).max()), er.pivot_ratio(Lc[j, j], kdiag, Lc[j, :j])
        assert r <= 1.0, ("row", j, r)
        assert p <= 1.0, ("pivot", j, p)
        wr, wp = max(wr, r), max(wp, p)
    return Lc, rows, diags, wr, wp


# ----------------------------------------------------------------------------------------------------------------------
# a. apgp_append_diag alone
# ----------------------------------------------------------------------------------------------------------------------
def test_append_diag_alone(lib_loaded):
    import torch
    lib = lib_loaded

    def call(kdiag, ss, info, order):
        ljj = torch.full((3,), NAN, dtype=torch.float64, device="cuda:0")
        ssd = _dev([ss])
        _ok(lib, lib.apgp_append_diag(ljj[1:].data_ptr(), ssd.data_ptr(), kdiag, info.data_ptr(), order, None), "apgp_append_diag")
        torch.cuda.synchronize()
        out = ljj.cpu().numpy()
        assert np.isnan(out[0]) and np.isnan(out[2]), "written beside *ljj"
        assert same_bits(ssd.cpu().numpy(), np.array([ss])), "*ss was written"
        return float(out[1])

    for name, kdiag, ss, info0, order, ok in er.APPEND_DIAG:
        info = torch.tensor([info0, -77], dtype=torch.int32, device="cuda:0")
        d = call(kdiag, ss, info, order)
        got = info.cpu().numpy()
        assert got[1] == -77
        if ok:
            r = er.pivot_ratio(d, kdiag, None, ss=ss)
            print("append_diag %-22s d = %.17g, |d^2 - (kdiag - ss)| / (3 u d^2) = %.3f" % (name, d, r))
            assert r <= 1.0, (name, d, r)
            assert got[0] == info0, (name, "a success touched info")
        else:
            print("append_diag %-22s d = %r, info %d -> %d" % (name, d, info0, got[0]))
            assert np.float64(d).view(np.int64) == np.float64(1.0).view(np.int64), (name, d)
            assert got[0] == (info0 if info0 else order), (name, got[0])
    info = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    for kdiag, ss, order in er.APPEND_DIAG_TWICE:
        assert call(kdiag, ss, info, order) == 1.0
    assert int(info.item()) == er.APPEND_DIAG_TWICE[0][2], "info must keep the FIRST failing order"


# ----------------------------------------------------------------------------------------------------------------------
# b. apgp_fit_summary / apgp_logdet alone
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", er.SUMMARY_N)
def test_fit_summary_alone(lib_loaded, n):
    import torch
    lib = lib_loaded
    L, z = er.summary_case(n)
    low = np.tril(np.ones((n, n), dtype=bool))
    zd = _dev(z)
    info = torch.tensor([37], dtype=torch.int32, device="cuda:0")
    seen = {}
    worst = {"logdet": 0.0, "zz": 0.0}
    for ldl in er.summary_lds(n):
        buf = np.full((n, ldl), NAN)            # NaN above the diagonal and in the row padding: a read there surfaces
        buf[:, :n][low] = L[low]
        Ld = _dev(buf)
        for with_z in (True, False):
            for with_info in (True, False):
                out = torch.full((7,), NAN, dtype=torch.float64, device="cuda:0")
                _ok(lib, lib.apgp_fit_summary(Ld.data_ptr(), n, ldl, zd.data_ptr() if with_z else None,
                                              info.data_ptr() if with_info else None, out[1:].data_ptr(), None), "apgp_fit_summary")
                torch.cuda.synchronize()
                o = out.cpu().numpy()
                assert np.isnan(o[0]) and np.isnan(o[6]), "written outside the five doubles"
                o5 = o[1:6]
                assert np.all(np.isfinite(o5)), ("a NaN sentinel surfaced", ldl, o5)
                r = er.summary_ratios(o5, er.summary_bounds(L, z if with_z else None, 37 if with_info else None))
                assert r["logdet"] <= 1.0 and r["zz"] <= 1.0 and r["exact"], (ldl, with_z, with_info, r, o5)
                worst = {k: max(worst[k], r[k]) for k in worst}
                seen.setdefault((with_z, with_info), set()).add(o5.tobytes())
        out = torch.full((7,), NAN, dtype=torch.float64, device="cuda:0")
        _ok(lib, lib.apgp_logdet(Ld.data_ptr(), n, ldl, out[1:].data_ptr(), None), "apgp_logdet")
        torch.cuda.synchronize()
        o = out.cpu().numpy()
        assert np.isnan(o[0]) and np.isnan(o[6])
        seen.setdefault("logdet", set()).add(o[1:6].tobytes())
        seen[(False, False)].add(o[1:6].tobytes())          # the legacy entry is the summary without z and info
        assert same_bits(Ld.cpu().numpy(), buf), "the factor was written"
    print("fit_summary n=%-4d worst |logdet - truth| / bound %.3f, |z.z - truth| / bound %.3f" % (n, worst["logdet"], worst["zz"]))
    assert all(len(v) == 1 for v in seen.values()), "the leading dimension changed a bit of the record"


# ----------------------------------------------------------------------------------------------------------------------
# c. rows by substitution: a chain of GP objects
# ----------------------------------------------------------------------------------------------------------------------
_CHAIN_CACHE = {}


def run_chain(lib, name):
    """Runs (once per module) the chain ``name``: a fresh GP per appended row, every row judged.  Returns a dict with the
    GP objects, the tip's factor bits and the worst ratios."""
    if name in _CHAIN_CACHE:
        return _CHAIN_CACHE[name]
    import torch
    n0, n1, D, wn, P = er.CHAINS[name]
    X, y, metric, wn, P = er.chain_case(name)
    base = make_gp(D, wn, P)
    base.compute(X[:n0])
    assert base._L_store is None and base._work is None
    K0 = torch.zeros((n0, n0), dtype=torch.float64, device="cuda:0")
    _ok(lib, lib.apgp_gram(base._x_d.data_ptr(), n0, ctypes.byref(base._kernel_struct()), K0.data_ptr(), n0, None), "apgp_gram")
    A = np.zeros((n1, n1))
    A[:n0, :n0] = K0.cpu().numpy()
    gps, Lp = [base], factor_bits(base)
    stores, wr, wp = [], 0.0, 0.0
    for j in range(n0, n1):
        parent, child = gps[-1], make_gp(D, wn, P)
        child.compute(X[:j + 1], previous=parent)
        Lc, rows, diags, r, p = check_rows(lib, child, Lp)
        assert same_bits(factor_bits(parent), Lp), "the append changed the parent's factor"
        A[j, :j], A[j, j] = rows[0], diags[0]
        wr, wp = max(wr, r), max(wp, p)
        if not stores or child._L_store is not stores[-1]:
            stores.append(child._L_store)
        gps.append(child)
        Lp = Lc
    wc = float(fr.chol_ratio(A, Lp).max())
    out = {"gps": gps, "L": Lp, "A": A, "X": X, "y": y, "stores": stores, "row": wr, "pivot": wp, "chol": wc}
    _CHAIN_CACHE[name] = out
    return out


@pytest.mark.parametrize("name", sorted(er.CHAINS))
def test_chain_rows_pivots_and_tip(lib_loaded, name):
    from approxposterior_amd import gp as agp
    c = run_chain(lib_loaded, name)
    n0, n1 = er.CHAINS[name][:2]
    tip, L = c["gps"][-1], c["L"]
    caps = [s["buf"].shape[0] for s in c["stores"]]
    print("chain %-8s %d -> %d: worst row %.3f, pivot %.3f, |A - L L^T| / budget %.3f; store capacities %s"
          % (name, n0, n1, c["row"], c["pivot"], c["chol"], caps))
    assert c["chol"] <= 1.0
    if name == "readme":
        assert caps == [128]
    if name == "blocks":
        assert caps == [128, 256], "one grow-and-copy, when the first store is full at n1 = 129"
        assert c["gps"][128 - n0]._L_store is c["stores"][0] and c["gps"][129 - n0]._L_store is c["stores"][1]
    else:
        assert len(caps) == 1
    # the record of the last apgp_fit_summary, from the tip's own bits
    b = er.summary_bounds(L)
    t, bound = b["logdet"]
    e = abs(float(np.longdouble(tip.log_determinant) - t))
    print("chain %-8s tip: |log det - truth| / bound %.3f" % (name, e / bound))
    assert e <= bound
    assert tip.cond_estimate == float((b["max"] / b["min"]) ** 2)
    assert tip._const == -0.5 * (n1 * agp._LOG_2PI + tip.log_determinant)
    assert tip.computed


def test_many_rows_in_one_call(lib_loaded):
    """extend_max_rows = 64: 100 -> 164 extends (every row judged), 100 -> 165 refactorises."""
    lib = lib_loaded
    n0, n_ext, n_ref, D = er.MANY
    X = er.points(n_ref, D, 5900)
    base = make_gp(D, -12.0)
    base.compute(X[:n0])
    Lp = factor_bits(base)
    ext = make_gp(D, -12.0)
    ext.extend_max_rows = 64
    ext.compute(X[:n_ext], previous=base)
    Lc, rows, diags, wr, wp = check_rows(lib, ext, Lp)
    print("64 rows in one call, 100 -> 164: worst row %.3f, pivot %.3f" % (wr, wp))
    ref = make_gp(D, -12.0)
    ref.extend_max_rows = 64
    ref.compute(X[:n_ref], previous=base)
    assert ref._L_store is None and ref._L.shape == (n_ref, n_ref) and ref.computed
    assert same_bits(factor_bits(base), Lp)


def test_cost_rule(lib_loaded):
    """Without extend_max_rows two rows extend below n1 = 512 and refactorise from there on; three never extend."""
    lib = lib_loaded
    X = er.chain_case("rule")[0]
    D, wn = er.CHAINS["rule"][2:4]

    def child_of(n0, n1):
        p = make_gp(D, wn)
        p.compute(X[:n0])
        c = make_gp(D, wn)
        c.compute(X[:n1], previous=p)
        return p, c
    p, c = child_of(509, 511)
    _, _, _, wr, wp = check_rows(lib, c, factor_bits(p))
    print("two rows by the cost rule, 509 -> 511: worst row %.3f, pivot %.3f" % (wr, wp))
    for n0, n1 in ((510, 512), (511, 513), (100, 103)):
        p, c = child_of(n0, n1)
        assert c._L_store is None and c.computed and c._L.shape == (n1, n1), (n0, n1)
    p, c = child_of(511, 512)
    assert c._L_store is not None


# ----------------------------------------------------------------------------------------------------------------------
# d. the W route
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n0", er.W_N0)
def test_w_route_first_row(lib_loaded, n0):
    import torch
    lib = lib_loaded
    D, wn = 3, float(np.log(1e-6))
    X = er.points(n0 + 2, D, 6000 + n0)
    parent = make_gp(D, wn)
    parent.compute(X[:n0])
    parent._ensure_linv()
    assert parent._work is not None and parent._trust_inverse() and parent.variance_mode is None
    Lp = factor_bits(parent)
    child = make_gp(D, wn)
    child.extend_max_rows = 2
    child.compute(X, previous=parent)
    assert child._L_store is not None
    Lc = factor_bits(child)
    assert same_bits(Lc[:n0, :n0], Lp) and not np.triu(Lc, 1).view(np.int64).any()
    # the route and the panel's layout: the test's own product on parent._work at the leading dimension the route assumes
    ldw = (n0 + 63) // 64 * 64
    k0, kd0 = cross_row(lib, child, n0)
    mine = torch.full((n0,), NAN, dtype=torch.float64, device="cuda:0")
    ss = torch.full((1,), NAN, dtype=torch.float64, device="cuda:0")
    _ok(lib, lib.apgp_winv_apply(parent._work.data_ptr(), ldw, n0, _dev(k0).data_ptr(), 0.0, 0, mine.data_ptr(),
                                 ss.data_ptr(), None, None), "apgp_winv_apply")
    torch.cuda.synchronize()
    l0 = Lc[n0, :n0]
    assert same_bits(l0, mine.cpu().numpy()), "the first appended row is not apgp_winv_apply on the parent's panel"
    panel = parent._work[:ldw * ldw].cpu().numpy().reshape(ldw, ldw)
    rw = float(er.winv_row_ratio(panel, l0, k0).max())
    assert rw <= 1.0, rw
    assert er.pivot_ratio(Lc[n0, n0], kd0, l0) <= 1.0
    # the second row of the same call goes by substitution
    k1, kd1 = cross_row(lib, child, n0 + 1)
    r1 = float(er.row_ratio(Lc, Lc[n0 + 1, :n0 + 1], k1).max())
    assert r1 <= 1.0, r1
    assert er.pivot_ratio(Lc[n0 + 1, n0 + 1], kd1, Lc[n0 + 1, :n0 + 1]) <= 1.0
    # reported, not asserted: how far the inverse route's row sits from substitution's backward bound
    print("W route n0=%-3d cond_estimate %.3g: product / bar %.3f; the same row against substitution's bar: %.3g; second row "
          "(substitution) %.3f" % (n0, parent.cond_estimate, rw, float(er.row_ratio(Lc, l0, k0).max()), r1))
    # "solve" on the parent keeps substitution although W is resident
    parent.variance_mode = "solve"
    by_solve = make_gp(D, wn)
    by_solve.compute(X[:n0 + 1], previous=parent)
    fresh = make_gp(D, wn)
    fresh.compute(X[:n0])
    by_sub = make_gp(D, wn)
    by_sub.compute(X[:n0 + 1], previous=fresh)
    assert fresh._work is None and parent._work is not None
    Ls = factor_bits(by_solve)
    assert same_bits(Ls, factor_bits(by_sub)), "variance_mode = 'solve' did not take the substitution route"
    assert float(er.row_ratio(Ls, Ls[n0, :n0], k0).max()) <= 1.0


# ----------------------------------------------------------------------------------------------------------------------
# e. the store
# ----------------------------------------------------------------------------------------------------------------------
def _inside(t, buf):
    lo = buf.data_ptr()
    return lo <= t.data_ptr() < lo + buf.numel() * 8


def _outputs(gp, y, T):
    mu, var = gp.predict(y, T, return_var=True)
    return np.concatenate([mu, var, [gp.log_likelihood(y)]])


def _family(D=3, wn=-12.0, metric=None, extra=6):
    """(X, make, g0, g1): STORE_N + ``extra`` points, a GP factory, a fresh GP on STORE_N points and its first child on
    STORE_N + 1 (the owner of a shared store of capacity 192)."""
    X = er.points(er.STORE_N + extra, D, 7000)
    def make():
        return make_gp(D, wn, metric=metric)
    g0 = make()
    g0.compute(X[:er.STORE_N])
    g1 = make()
    g1.compute(X[:er.STORE_N + 1], previous=g0)
    assert g0._L_store is None and g1._L_store["buf"].shape[0] == 192
    g1.variance_mode = "solve"       # (its predictions leave no trusted W behind: appends go by substitution, as in (c))
    return X, make, g0, g1


def test_store_in_place_and_second_child(lib_loaded):
    lib = lib_loaded
    X, make, g0, g1 = _family()
    n = er.STORE_N + 1
    y, T = er.target(X), er.points(40, 3, 7001)
    store = g1._L_store
    L1 = factor_bits(g1)
    before = _outputs(g1, y[:n], T)
    # in place
    a = make()
    a.compute(X[:n + 1], previous=g1)
    assert a._L_store is store and store["used"] == n + 1 and _inside(a._L, store["buf"]) and a._L.data_ptr() == g1._L.data_ptr()
    La = check_rows(lib, a, L1)[0]
    assert same_bits(_outputs(g1, y[:n], T), before), "the child's append moved the parent's predictions"
    # a second child of the same parent: its own buffer, the first child's rows untouched
    Xb = np.vstack([X[:n], X[n + 2:n + 3]])
    b = make()
    b.compute(Xb, previous=g1)
    assert b._L_store is not store and not _inside(b._L, store["buf"]) and store["used"] == n + 1
    check_rows(lib, b, L1)
    assert same_bits(factor_bits(a), La), "the second child overwrote the first child's rows"
    assert same_bits(factor_bits(g1), L1)
    assert same_bits(_outputs(g1, y[:n], T), before)
    # and the first child's line goes on in place
    a2 = make()
    a2.compute(X[:n + 2], previous=a)
    assert a2._L_store is store and store["used"] == n + 2
    check_rows(lib, a2, La)
    assert same_bits(factor_bits(b)[:n, :n], L1)


def test_store_growth_leaves_the_old_buffer(lib_loaded):
    """A store of capacity 128 filled to its last row, then one more: a new buffer, the old one byte for byte as it was."""
    lib = lib_loaded
    D, wn = 3, -12.0
    X = er.points(130, D, 7100)
    y, T = er.target(X), er.points(40, 3, 7101)
    g0 = make_gp(D, wn)
    g0.compute(X[:64])
    first = make_gp(D, wn)
    first.compute(X[:65], previous=g0)                         # (the rule gives 65 rows a capacity of 128)
    g1 = make_gp(D, wn)
    g1.extend_max_rows = 64
    g1.compute(X[:128], previous=first)
    old = g1._L_store
    assert old is first._L_store and old["buf"].shape == (128, 128) and old["used"] == 128
    L1 = check_rows(lib, g1, factor_bits(first))[0]
    g1.variance_mode = "solve"                                 # (no W: the next append goes by substitution, as in (c))
    before = _outputs(g1, y[:128], T)
    image = old["buf"].cpu().numpy().copy()
    g2 = make_gp(D, wn)
    g2.compute(X[:129], previous=g1)
    assert g2._L_store is not old and g2._L_store["buf"].shape == (256, 256) and not _inside(g2._L, old["buf"])
    assert old["used"] == 128
    check_rows(lib, g2, L1)                                   # (the copied rows have the old bits)
    assert same_bits(old["buf"].cpu().numpy(), image), "the old store was written"
    assert same_bits(_outputs(g1, y[:128], T), before)
    rest = g2._L_store["buf"].cpu().numpy()
    rest[:129, :129] = 0.0
    assert not rest.view(np.int64).any(), "the grown store is not zero outside the factor"


def test_store_failed_append(lib_loaded):
    """No white noise, four rows in one call, the second and the fourth a copy of X[0]: both pivots fail exactly
    (extend_ref.failure_case); the first is the one reported."""
    lib = lib_loaded
    X, y = er.failure_case()
    n = er.STORE_N + 1
    T = er.points(40, 3, 7702)
    def make():
        g = make_gp(3, -800.0, metric=np.full(3, er.FAIL_METRIC))
        g.extend_max_rows = 4
        return g
    g0 = make()
    g0.compute(X[:er.STORE_N])
    parent = make()
    parent.compute(X[:n], previous=g0)
    store = parent._L_store
    assert store is not None and store["used"] == n
    Lp = factor_bits(parent)
    assert Lp[0, 0] == 1.0          # (so L[i, 0] = K_i0 exactly, whatever the bits of K_i0)
    parent.variance_mode = "solve"
    before = _outputs(parent, y[:n], T)
    bad = make()
    with pytest.raises(np.linalg.LinAlgError) as exc:
        bad.compute(X, previous=parent)
    assert str(exc.value).startswith("%d-th leading minor" % (n + 2)), str(exc.value)
    assert store["used"] == -1, "the shared store must be closed to further appends"
    assert not bad.computed and bad._L is None and bad._L_store is None
    assert same_bits(factor_bits(parent), Lp)
    assert same_bits(_outputs(parent, y[:n], T), before), "the failed append moved the parent's predictions"
    # the failed rows, as the device left them: (1, 0, ..., 0 | 1) at the two copies
    left = store["buf"][:n + 4, :n + 4].cpu().numpy()
    for r in (1, 3):
        assert left[n + r, 0] == 1.0 and not left[n + r, 1:n + r].any() and left[n + r, n + r] == 1.0
    # a later good append from the same parent: a fresh buffer
    good = make()
    good.compute(np.vstack([X[:n], X[n:n + 1], X[n + 2:n + 3]]), previous=parent)
    assert good._L_store is not store and not _inside(good._L, store["buf"]) and good._L_store["used"] == n + 2
    _, _, _, wr, wp = check_rows(lib, good, Lp)
    print("after a failed append: a good one from the same parent, worst row %.3f, pivot %.3f" % (wr, wp))
    assert same_bits(_outputs(parent, y[:n], T), before)


# ----------------------------------------------------------------------------------------------------------------------
# f. downstream at the store's leading dimension
# ----------------------------------------------------------------------------------------------------------------------
def test_downstream_bits_at_the_store_leading_dimension(lib_loaded):
    """The tip of the 60 -> 131 chain (n = 131 in a store of leading dimension 256: every row 16-byte aligned, which the
    ldl = n + 3 cases of the other budget tests never are) against a twin GP whose compact 131 x 131 factor holds the
    same bits: every consumer of the factor must give the same bits."""
    import torch
    c = run_chain(lib_loaded, "blocks")
    n0, n1, D, wn, P = er.CHAINS["blocks"]
    tip, X, y = c["gps"][-1], c["X"], c["y"]
    assert tip._ld == 256 and tip._L.data_ptr() % 16 == 0
    twin = make_gp(D, wn)
    twin.compute(X)
    assert twin._L_store is None and twin._ld == n1
    twin._L.copy_(tip._L)
    twin.log_determinant, twin.cond_estimate, twin._const = tip.log_determinant, tip.cond_estimate, tip._const
    torch.cuda.synchronize()
    assert same_bits(factor_bits(twin), c["L"])
    y2 = y + 0.5 * np.cos(X).sum(1)
    T = er.points(300, D, 7200)
    differ = []

    def both(what, f):
        a, b = f(tip), f(twin)
        a = np.concatenate([np.atleast_1d(np.asarray(v, dtype=np.float64)) for v in (a if isinstance(a, tuple) else (a,))])
        b = np.concatenate([np.atleast_1d(np.asarray(v, dtype=np.float64)) for v in (b if isinstance(b, tuple) else (b,))])
        assert np.all(np.isfinite(a))
        if not same_bits(a, b):
            differ.append((what, float(np.abs(a - b).max())))

    both("log_likelihood", lambda g: g.log_likelihood(y2))
    both("grad_log_likelihood", lambda g: g.grad_log_likelihood(y2))
    for mode in ("inverse", "solve"):
        tip.variance_mode = twin.variance_mode = mode
        both("predict one, " + mode, lambda g: g.predict(y2, T[:1], return_var=True))
        both("predict 300, " + mode, lambda g: g.predict(y2, T, return_var=True))
        for kind in ("agp", "bape", "jones"):
            both("acquire %s, %s" % (kind, mode), lambda g: g.acquire(y2, T, kind))
        both("grad_log_likelihood, " + mode, lambda g: g.grad_log_likelihood(y2))
    tip.variance_mode = twin.variance_mode = None
    print("downstream at ld 256 against a compact twin: %s" % (differ or "every consumer gives the same bits"))
    assert not differ, differ
