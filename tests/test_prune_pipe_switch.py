# -*- coding: utf-8 -*-
"""The switch of the coarse bound's pipelined row loop (``apgp_set_prune_pipe`` / ``apgp_get_prune_pipe``,
``GP.prune_pipe``): host code only, no GPU.  It exists, is on by default, returns the previous value, takes any
non-zero value as on, and a GP leaves the process-wide setting alone unless told otherwise."""
import numpy as np


def test_the_library_switch_defaults_to_on_and_round_trips():
    from approxposterior_amd import _lib
    lib = _lib.load()
    assert lib.apgp_get_prune_pipe() == 1
    try:
        assert lib.apgp_set_prune_pipe(0) == 1 and lib.apgp_get_prune_pipe() == 0
        assert lib.apgp_set_prune_pipe(7) == 0 and lib.apgp_get_prune_pipe() == 1       # any non-zero value: on
        assert lib.apgp_set_prune_pipe(0) == 1
    finally:
        lib.apgp_set_prune_pipe(1)
    assert lib.apgp_get_prune_pipe() == 1
    assert lib.apgp_abi_version() == _lib.ABI_VERSION == 8


def test_a_gp_takes_the_library_setting_by_default():
    from approxposterior_amd import gp as agp
    gp = agp.GP(kernel=agp.ExpSquaredKernel(np.full(3, 8.0), ndim=3))
    assert gp.prune_pipe is None and gp.prune_signed is True
