# -*- coding: utf-8 -*-
"""MI355X: the factor layer and the likelihood gradient, each kernel alone through the C ABI, each handed the bits it is
judged on, against the condition-free budgets of tests/factor_ref.py (derived from rounding counts read off the kernel
source, not fitted to device output; tests/test_factor_ref.py holds LAPACK and the restated device order to the same
bars on the same inputs, and shows that each bar catches its mutants):

  a. apgp_potrf         |A - L L^T| entry by entry, the right-hand side riding along, sentinels byte-identical;
  b. apgp_trsv[_ex]     the residual row by row and x.x, every path (one workgroup below n = 256, persistent and
                        launch-per-256-rows above), forward and transposed, aliased or not, ld = n and n + 3;
  c. apgp_kinv_solve    every lower tile against the truth of (L L^T)^-1, in cho_solve's error class; the tiles above
                        the block diagonal and everything past n untouched;
  d. W^T W              syrk_wtw_kernel entry by entry from the bits of the W that apgp_trtri_pack left;
  e. grad kernels       apgp_grad_loglik with a planted K^-1 (NaN above the block diagonal: a NaN in any output is a
                        read outside the contract), every padded width, linear terms of order 0 .. 3, and n = 2881;
  f. through GP         the gradient beyond one tile on both sides of the conditioning gate against a 60-digit truth.

The fused (apgp_nll_eval), persistent, hybrid, paired and deferred variants of the Cholesky are not repeated here:
test_gpu_parity.py ties each of them to the apgp_potrf path bit for bit (test_persistent_cholesky_bit_identical_to_
multi_launch, test_hybrid_cholesky_bit_identical_to_multi_launch, test_paired_trailing_updates_bit_identical), so the
budget asserted on this path holds for them.

Worst figures are printed (pytest -s) and recorded in docs/experiments.md, round 11."""
import ctypes
import os

import numpy as np
import pytest

import factor_ref as fr
import kvalue_ref as kr

pytestmark = pytest.mark.gpu

SENTINEL = -1.2345678901234567e300


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
    """n x ld buffer holding the lower triangle of M, ``fill`` above the diagonal and in the row padding."""
    n = len(M)
    buf = np.full((n, ld), fill)
    low = np.tril(np.ones((n, n), dtype=bool))
    buf[:, :n][low] = M[low]
    return buf


# ----------------------------------------------------------------------------------------------------------------------
# a. apgp_potrf
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", fr.POTRF_N)
@pytest.mark.parametrize("family", ["se", "ill"])
def test_potrf_residual_within_budget(lib_loaded, family, n):
    import torch
    lib = lib_loaded
    K, y = fr.gram(family, n)
    low = np.tril(np.ones((n, n), dtype=bool))
    yd = _dev(y)
    seen = {}
    for lda in (n, n + 3):
        A = padded(K, lda)
        Ad = _dev(A)
        zd = _full((n,))
        info = torch.full((1,), -5, dtype=torch.int32, device="cuda:0")
        _ok(lib, lib.apgp_potrf(Ad.data_ptr(), n, lda, yd.data_ptr(), 0.25, zd.data_ptr(), info.data_ptr(), None), "apgp_potrf")
        torch.cuda.synchronize()
        assert int(info.item()) == 0
        out = Ad.cpu().numpy()
        assert same_bits(out[:, :n][~low], A[:, :n][~low]), "written above the diagonal"
        assert same_bits(out[:, n:], A[:, n:]), "written into the row padding"
        L = np.tril(out[:, :n])
        z = zd.cpu().numpy()
        key = L.tobytes() + z.tobytes()
        if key not in seen:
            seen[key] = (fr.chol_ratio(K, L).max(), fr.trsv_ratio(L, z, y, 0.25, 0).max())
        r, rz = seen[key]
        print("potrf %-3s n=%-3d lda=%-3d worst |A - L L^T| / budget %.3f, rhs residual / budget %.3f" % (family, n, lda, r, rz))
        assert r <= 1.0
        assert rz <= 1.0
    assert len(seen) == 1, "the leading dimension changed a bit of the factor"


# ----------------------------------------------------------------------------------------------------------------------
# b. apgp_trsv / apgp_trsv_ex
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trans", [0, 1])
@pytest.mark.parametrize("n", fr.TRSV_N)
@pytest.mark.parametrize("family", ["planted", "ill"])
def test_trsv_residual_within_budget(lib_loaded, family, n, trans):
    import torch
    lib = lib_loaded
    L, b = fr.factor(family, n)
    shift = 0.125
    entries = [("trsv", None), ("ex", 0), ("ex", 1)] if n >= 256 else [("trsv", None), ("ex", -1)]
    seen = {}
    worst = (0.0, 0.0)
    for ldl in (n, n + 3):
        Ld = _dev(padded(L, ldl))                   # (what lies above the diagonal or in the padding must not be used)
        for alias in (False, True):
            for want_ss in (True, False):
                for entry, mode in entries:
                    bd = _dev(b)
                    xd = bd if alias else _full((n,))
                    ss = _full((1,))
                    ssp = ss.data_ptr() if want_ss else None
                    if entry == "trsv":
                        rc = lib.apgp_trsv(Ld.data_ptr(), n, ldl, bd.data_ptr(), shift, trans, xd.data_ptr(), ssp, None)
                    else:
                        rc = lib.apgp_trsv_ex(Ld.data_ptr(), n, ldl, bd.data_ptr(), shift, trans, xd.data_ptr(), ssp, mode, None)
                    _ok(lib, rc, "apgp_trsv")
                    torch.cuda.synchronize()
                    x = xd.cpu().numpy()
                    if not alias:
                        assert same_bits(bd.cpu().numpy(), b), "the right-hand side was written"
                    key = x.tobytes()
                    if key not in seen:
                        seen[key] = (fr.trsv_ratio(L, x, b, shift, trans).max(), fr.sumsq_bound(x))
                    r, (t, bound) = seen[key]
                    assert r <= 1.0, (ldl, alias, want_ss, entry, mode, r)
                    rs = 0.0
                    if want_ss:
                        s = float(ss.item())
                        assert np.isfinite(s)
                        es = abs(float(np.longdouble(s) - t))
                        assert es <= bound, (ldl, alias, entry, mode, es, bound)
                        rs = es / bound if bound > 0 else 0.0
                    worst = (max(worst[0], r), max(worst[1], rs))
    print("trsv %-7s n=%-3d trans=%d: worst residual / budget %.3f, |ss - x.x| / bound %.3f, %d distinct result(s)"
          % (family, n, trans, worst[0], worst[1], len(seen)))
    assert len(seen) == 1, "paths, leading dimensions or aliasing changed a bit of the solution"


# ----------------------------------------------------------------------------------------------------------------------
# c. K^-1 by apgp_kinv_solve
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", fr.KINV_N)
@pytest.mark.parametrize("family", ["planted", "ill"])
def test_kinv_solve_tiles_in_cho_solve_class(lib_loaded, family, n):
    import torch
    lib = lib_loaded
    L, _ = fr.factor(family, n)
    low = fr.lower_tile_mask(n)
    seen = {}
    for ldl in (n, n + 3):
        Ld = _dev(padded(L, ldl))
        xw = _full((int(lib.apgp_kinv_solve_work_len(n)),))
        buf = _full((n * n + 64,))
        _ok(lib, lib.apgp_kinv_solve(Ld.data_ptr(), n, ldl, xw.data_ptr(), buf.data_ptr(), None), "apgp_kinv_solve")
        torch.cuda.synchronize()
        out = buf.cpu().numpy()
        assert same_bits(out[n * n:], np.full(64, SENTINEL)), "written past row n"
        Y = out[:n * n].reshape(n, n)
        assert same_bits(Y[~low], np.full((~low).sum(), SENTINEL)), "a tile above the block diagonal was written"
        assert np.all(np.isfinite(Y[low]))
        key = Y.tobytes()
        if key not in seen:
            seen[key] = fr.kinv_bar_ratio(Y, L)
        r = seen[key]
        print("kinv_solve %-7s n=%-3d ldl=%-3d worst tile error / max(3 x cho_solve's, n u max|truth|) %.3f" % (family, n, ldl, r))
        assert r <= 1.0
    assert len(seen) == 1, "the leading dimension changed a bit of K^-1"


# ----------------------------------------------------------------------------------------------------------------------
# d. K^-1 = W^T W by the inverse route
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", fr.KINV_N)
def test_syrk_entries_within_bound(lib_loaded, n):
    import torch
    lib = lib_loaded
    L, _ = fr.factor("planted", n)
    npad = fr.TILE * fr.nblocks(n)
    Ld = _dev(L)
    twork = _full((int(lib.apgp_trtri_work_len(n)),))       # (GP hands over uninitialised memory: nothing unwritten may be used)
    Wd = _full((n, n))
    _ok(lib, lib.apgp_trtri_pack(Ld.data_ptr(), n, n, twork.data_ptr(), None, Wd.data_ptr(), None), "apgp_trtri_pack")
    torch.cuda.synchronize()
    W = Wd.cpu().numpy()
    panel = twork[:npad * npad].cpu().numpy().reshape(npad, npad)
    assert same_bits(panel[:n, :n], W), "winv_dense is not the panel the product reads"
    assert np.all(np.triu(W, 1) == 0.0)
    k = kr.kern([1.0])
    gwork = _full((int(lib.apgp_grad_work_len(n)),))
    out = _full((4 + fr.MAX_DIM,))
    Xd, ad = _dev(np.zeros((n, 1))), _dev(np.zeros(n))
    _ok(lib, lib.apgp_grad_loglik(Xd.data_ptr(), ad.data_ptr(), twork.data_ptr(), npad, n, ctypes.byref(_ks(k)),
                                  gwork.data_ptr(), out.data_ptr(), None), "apgp_grad_loglik")
    torch.cuda.synchronize()
    Kinv = gwork[:n * n].cpu().numpy().reshape(n, n)
    low = fr.lower_tile_mask(n)
    assert same_bits(Kinv[~low], np.full((~low).sum(), SENTINEL)), "a tile above the block diagonal was written"
    assert np.all(np.isfinite(Kinv[low]))
    T, B = fr.syrk_bound(W)
    err = np.abs(Kinv.astype(np.longdouble) - T).astype(np.float64)
    assert np.all((B[low] > 0) | (err[low] == 0))
    r = (err[low] / np.where(B[low] > 0, B[low], 1.0)).max()
    print("syrk n=%-3d worst |W^T W - truth| / bound %.3f" % (n, r))
    assert r <= 1.0


# ----------------------------------------------------------------------------------------------------------------------
# e. the gradient kernels alone
# ----------------------------------------------------------------------------------------------------------------------
def dev_grad(lib, X, alpha, Kinv, k):
    """``out`` (4 + MAX_DIM doubles, pre-filled with the sentinel) of apgp_grad_loglik with winv = NULL and ``work``
    planted with ``Kinv``."""
    import torch
    n = len(X)
    work = _full((int(lib.apgp_grad_work_len(n)),))
    work[:n * n] = _dev(Kinv).reshape(-1)
    out = _full((4 + fr.MAX_DIM,))
    Xd, ad = _dev(X), _dev(alpha)
    _ok(lib, lib.apgp_grad_loglik(Xd.data_ptr(), ad.data_ptr(), None, 0, n, ctypes.byref(_ks(k)), work.data_ptr(),
                                  out.data_ptr(), None), "apgp_grad_loglik")
    torch.cuda.synchronize()
    assert same_bits(work[:n * n].cpu().numpy(), np.asarray(Kinv).reshape(-1)), "the planted K^-1 was written"
    return out.cpu().numpy()


def check_grad(lib, n, D, order):
    X, alpha, Kinv, k = fr.grad_case(n, D, order)
    out = dev_grad(lib, X, alpha, Kinv, k)
    val, bud = fr.grad_record(X, alpha, Kinv, k)
    r = fr.grad_ratios(out, val, bud, D, order is not None)
    print("grad n=%-4d D=%-2d P=%-4s |out - truth| / budget: %s" % (n, D, order, "  ".join("%s %.3g" % kv for kv in sorted(r.items()))))
    assert max(r.values()) <= 1.0, r
    # the slots past ndim are not written, and without a linear term its slot is an exact zero
    assert same_bits(out[2 + D:2 + fr.MAX_DIM], np.full(fr.MAX_DIM - D, SENTINEL))
    if order is None:
        assert out[3 + fr.MAX_DIM] == 0.0


@pytest.mark.parametrize("D", fr.GRAD_D)
@pytest.mark.parametrize("n", fr.GRAD_N)
def test_gradient_kernels_within_budget(lib_loaded, n, D):
    check_grad(lib_loaded, n, D, None)


@pytest.mark.parametrize("order,n,D", fr.GRAD_LIN)
def test_gradient_kernels_linear_term_within_budget(lib_loaded, order, n, D):
    check_grad(lib_loaded, n, D, order)


def test_gradient_kernels_1081_tiles(lib_loaded):
    """n = 2881: 46 block rows, 1081 tiles -- the only size at which grad_final_kernel's strided loop over the tile
    partials takes a second trip (and the sqrt-based tile decode runs past 1024)."""
    check_grad(lib_loaded, fr.GRAD_BIG[0], fr.GRAD_BIG[1], None)


# ----------------------------------------------------------------------------------------------------------------------
# f. through GP, beyond one tile, on both sides of the gate
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["inverse", "solve", None])
@pytest.mark.parametrize("name", ["grad_n130_cond1e8", "grad_n130_cond1e13"])
def test_gradient_three_tiles_on_both_sides_of_the_gate(golden_dir, name, mode, lib_loaded):
    """test_gradient_on_the_conditioning_ladder's body at n = 130, D = 2 (three tiles, the last of two rows): the
    fixtures of tools/make_grad_golden.py carry the oracle's gradient and a 60-digit mpmath one.  Bar per component:
    error <= max(3 x the oracle's, 1e-3 cond eps max|truth|).  Left to itself the gate sends cond 1e13 to the solve
    route and 1e8 to the explicit inverse."""
    from approxposterior_amd import gp as agp
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    D, p = g["theta"].shape[1], g["p"]
    kernel = agp.Product(agp.ConstantKernel(p[1], ndim=D), agp.ExpSquaredKernel(np.exp(p[2:]), ndim=D))
    gp = agp.GP(kernel=kernel, fit_mean=True, mean=float(p[0]), white_noise=float(g["white_noise"]), fit_white_noise=False)
    gp.compute(g["theta"])
    gp.variance_mode = mode
    truth, ref = g["grad_truth"], g["grad"]
    hip = gp.grad_log_likelihood(g["y"])
    if mode is None:
        assert gp._trust_inverse() == (gp.cond_estimate <= agp.COND_SOLVE)
        assert gp._trust_inverse() == name.endswith("cond1e8")
    floor = 1e-3 * float(g["cond"]) * np.finfo(np.float64).eps * np.abs(truth).max()
    err, err_ref = np.abs(hip - truth), np.abs(ref - truth)
    print("grad through GP %s mode=%s: error %s, oracle's %s, floor %.3g" % (name, mode, err, err_ref, floor))
    assert np.all(err <= np.maximum(3.0 * err_ref, floor)), (err, err_ref, floor)
    assert np.linalg.norm(hip - truth) <= max(3.0 * np.linalg.norm(ref - truth), 2.0 * floor)
