# -*- coding: utf-8 -*-
"""CPU: apgp_path_importance refuses bad arguments with -1 and a message before any HIP call (there is no GPU here), and
apgp_path_importance_work_len agrees with the formula of include/apgp.h as tests/pathevidence_ref.py restates it -- in
the style of tests/test_evidence_arguments_host.py."""
import ctypes
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pathevidence_ref as per  # noqa: E402

from approxposterior_amd import _lib  # noqa: E402


@pytest.mark.parametrize("S", [1, 32])
@pytest.mark.parametrize("m", [1, 256, 257, per.ROW_CAP, per.ROW_CAP + 1])
def test_work_len_is_the_stated_formula(m, S):
    lib = _lib.load()
    assert lib.apgp_path_importance_work_len(m, S) == per.work_len(m, S) > 0


def test_work_len_limits():
    lib = _lib.load()
    assert per.ROW_CAP == _lib.IMP_BLOCK * _lib.IMP_MAX_BLOCKS
    assert lib.apgp_path_importance_work_len(0, 4) == 0 and lib.apgp_path_importance_work_len(-3, 4) == 0
    assert lib.apgp_path_importance_work_len(1 << 40, 1) == per.work_len(1 << 40, 1) > 0
    assert lib.apgp_path_importance_work_len((1 << 40) + 1, 1) == -1
    assert lib.apgp_path_importance_work_len(16, _lib.MAX_DRAWS + 1) == -1
    assert lib.apgp_path_importance_work_len(16, 0) == 0


def _setup():
    lib = _lib.load()
    ks = _lib.KernelStruct()
    ks.ndim, ks.amp = 2, 1.0
    ks.inv_metric[0] = ks.inv_metric[1] = 1.0
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    arr = ctypes.c_double * _lib.MAX_DIM
    lo, hi, c = arr(), arr(*([1.0] * _lib.MAX_DIM)), arr()
    ok = dict(T=p, m=4, lnq=None, xs=p, n=4, ks=ctypes.byref(ks), V=p, Z=p, b=p, W=p, Wl=None, nfeat=8, ndraws=2,
              lo=lo, hi=hi, c=ctypes.addressof(c), logw=None, stats=p, work=p)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.apgp_path_importance(a["T"], a["m"], a["lnq"], a["xs"], a["n"], a["ks"], 0.0, a["V"], a["Z"], a["b"],
                                        a["W"], a["Wl"], a["nfeat"], a["ndraws"], a["lo"], a["hi"], a["c"], a["logw"],
                                        a["stats"], a["work"], None)
    return lib, ks, call, (buf, lo, hi, c, arr)


def test_path_importance_refuses_null_pointers_before_any_launch():
    lib, ks, call, keep = _setup()
    for name in ("T", "Z", "b", "W", "c", "stats", "work"):
        assert call(**{name: None}) == -1, name
        err = lib.apgp_last_error()
        assert b"apgp_path_importance" in err and b"null pointer" in err, (name, err)
    assert call(ks=None) == -1 and b"null pointer" in lib.apgp_last_error()
    assert call(xs=None) == -1 and b"xs is required with V" in lib.apgp_last_error()     # V is given
    assert call(lo=None) == -1 and b"lo and hi" in lib.apgp_last_error()
    assert call(hi=None) == -1 and b"lo and hi" in lib.apgp_last_error()
    ks.lin_coef, ks.lin_order = 0.3, 1
    assert call(Wl=None) == -1 and b"Wl is required" in lib.apgp_last_error()
    ks.lin_coef = 0.0


def test_path_importance_refuses_sizes_beyond_the_limits():
    lib, ks, call, keep = _setup()
    for kw, word in ((dict(ndraws=0), b"ndraws"), (dict(ndraws=_lib.MAX_DRAWS + 1), b"ndraws"),
                     (dict(nfeat=0), b"nfeat"), (dict(nfeat=_lib.MAX_FEATURES + 1), b"nfeat"),
                     (dict(m=0), b"m <="), (dict(m=(1 << 40) + 1), b"m <="),
                     (dict(n=0), b"n <="), (dict(n=(1 << 24) + 1), b"n <="),
                     (dict(n=0, V=None, xs=None), b"n <=")):
        assert call(**kw) == -1, kw
        err = lib.apgp_last_error()
        assert b"apgp_path_importance" in err and word in err, (kw, err)


def test_path_importance_refuses_a_bad_centre_and_bad_kernels():
    lib, ks, call, keep = _setup()
    arr = keep[4]
    for bad in (float("nan"), float("inf"), -float("inf")):
        c = arr()
        c[1] = bad
        assert call(c=ctypes.addressof(c)) == -1 and b"centre must be finite" in lib.apgp_last_error()
    ks.ndim = _lib.MAX_DIM + 1
    assert call() == -1 and b"kernel parameters" in lib.apgp_last_error()
    ks.ndim, ks.amp = 2, 0.0
    assert call() == -1
    ks.amp = 1.0
