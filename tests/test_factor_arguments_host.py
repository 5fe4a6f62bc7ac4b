"""CPU: the factor entry points (apgp_potrf, apgp_nll_eval, apgp_nll_eval_batch, apgp_trsv) refuse a bad argument before
any HIP call, with the function's name in front of the message, and apgp_potrf_mode refuses a mode word it does not know
and leaves the word alone when asked for it."""
import ctypes

import pytest

from approxposterior_amd import _lib

N = 4
MODE_TEXT = b"apgp_potrf_mode: bad argument: mode 0 .. 3 (+ 16: no paired trailing updates, + 32: no deferred tiles)"


def _kernel():
    k = _lib.KernelStruct()
    k.ndim, k.lin_order, k.amp, k.diag_add, k.lin_coef = 2, 0, 1.0, 0.0, 0.0
    for d in range(2):
        k.inv_metric[d] = 1.0
    return k


def _calls(lib, p):
    """name -> (callable, expected message); every pointer is the one 2 KiB host buffer at p."""
    k = ctypes.byref(_kernel())
    null = b": bad argument: null pointer"
    together = b": bad argument: y and z must be given together"

    def potrf(A=p, n=N, lda=N, y=p, z=p, info=p):
        return lambda: lib.apgp_potrf(A, n, lda, y, 0.0, z, info, None)

    def nll(X=p, n=N, kern=k, y=p, K=p, z=p, info=p, out5=p, host=p):
        return lambda: lib.apgp_nll_eval(X, n, kern, y, 0.0, K, z, info, out5, host, None)

    def batch(X=p, n=N, b=2, kerns=k, y=p, means=p, host=p):
        return lambda: lib.apgp_nll_eval_batch(X, n, b, kerns, y, means, p, p, p, p, host, None)

    def trsv(L=p, n=N, ldl=N, b=p, x=p):
        return lambda: lib.apgp_trsv(L, n, ldl, b, 0.0, 0, x, None, None)

    size = b": bad argument: n >= 1 and lda >= n required"
    n1 = b": bad argument: n >= 1 required"
    nb = b": bad argument: 1 <= batch <= 65535 required"
    ldl = b": bad argument: n >= 1 and ldl >= n required"
    return {
        "potrf-null-A": (potrf(A=None), b"apgp_potrf" + null),
        "potrf-null-info": (potrf(info=None), b"apgp_potrf" + null),
        "potrf-y-without-z": (potrf(z=None), b"apgp_potrf" + together),
        "potrf-z-without-y": (potrf(y=None), b"apgp_potrf" + together),
        "potrf-n-0": (potrf(n=0), b"apgp_potrf" + size),
        "potrf-n-above-limit": (potrf(n=(1 << 24) + 1, lda=(1 << 24) + 1), b"apgp_potrf" + size),
        "potrf-lda-below-n": (potrf(lda=N - 1), b"apgp_potrf" + size),
        "nll-null-X": (nll(X=None), b"apgp_nll_eval" + null),
        "nll-null-kernel": (nll(kern=None), b"apgp_nll_eval" + null),
        "nll-null-host-record": (nll(host=None), b"apgp_nll_eval" + null),
        "nll-y-without-z": (nll(z=None), b"apgp_nll_eval" + together),
        "nll-n-0": (nll(n=0), b"apgp_nll_eval" + n1),
        "nll-n-above-limit": (nll(n=(1 << 24) + 1), b"apgp_nll_eval" + n1),
        "batch-null-X": (batch(X=None), b"apgp_nll_eval_batch" + null),
        "batch-null-y": (batch(y=None), b"apgp_nll_eval_batch" + null),
        "batch-null-means": (batch(means=None), b"apgp_nll_eval_batch" + null),
        "batch-0": (batch(b=0), b"apgp_nll_eval_batch" + nb),
        "batch-65536": (batch(b=65536), b"apgp_nll_eval_batch" + nb),
        "batch-n-0": (batch(n=0), b"apgp_nll_eval_batch" + n1),
        "trsv-null-L": (trsv(L=None), b"apgp_trsv" + null),
        "trsv-null-x": (trsv(x=None), b"apgp_trsv" + null),
        "trsv-n-0": (trsv(n=0), b"apgp_trsv" + ldl),
        "trsv-ldl-below-n": (trsv(ldl=N - 1), b"apgp_trsv" + ldl),
    }


NAMES = ["potrf-null-A", "potrf-null-info", "potrf-y-without-z", "potrf-z-without-y", "potrf-n-0", "potrf-n-above-limit",
         "potrf-lda-below-n", "nll-null-X", "nll-null-kernel", "nll-null-host-record", "nll-y-without-z", "nll-n-0",
         "nll-n-above-limit", "batch-null-X", "batch-null-y", "batch-null-means", "batch-0", "batch-65536", "batch-n-0",
         "trsv-null-L", "trsv-null-x", "trsv-n-0", "trsv-ldl-below-n"]


@pytest.mark.parametrize("name", NAMES)
def test_factor_entry_point_refuses_before_any_hip_call(name):
    lib = _lib.load()
    raw = (ctypes.c_char * (2048 + 64))()
    p = (ctypes.addressof(raw) + 63) & ~63
    call, message = _calls(lib, p)[name]
    assert call() == -1
    assert lib.apgp_last_error() == message


def test_calls_cover_every_name():
    assert sorted(_calls(_lib.load(), 64)) == sorted(NAMES)


@pytest.mark.parametrize("mode", [4, 64, 4 + 16, 7 + 32])
def test_potrf_mode_refuses_an_unknown_mode_and_keeps_the_word(mode):
    lib = _lib.load()
    before = lib.apgp_potrf_mode(-1)
    assert lib.apgp_potrf_mode(mode) == -1
    assert lib.apgp_last_error() == MODE_TEXT
    assert lib.apgp_potrf_mode(-1) == before


def test_potrf_mode_query_returns_the_word_and_leaves_it():
    """(setting the word touches host atomics only: no HIP call)"""
    lib = _lib.load()
    before = lib.apgp_potrf_mode(-1)
    try:
        for word in (0, 1, 2, 3, 1 + 16, 32, 3 + 16 + 32):
            lib.apgp_potrf_mode(word)
            assert lib.apgp_potrf_mode(-1) == word
            assert lib.apgp_potrf_mode(-1) == word
            assert lib.apgp_potrf_mode(-7) == word
        assert lib.apgp_potrf_mode(2 + 16) == 3 + 16 + 32          # (a set returns the previous word)
    finally:
        lib.apgp_potrf_mode(before)
    assert lib.apgp_potrf_mode(-1) == before
