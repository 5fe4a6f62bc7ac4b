# -*- coding: utf-8 -*-
"""The switch of the parked seed launch's prefetch distance (``apgp_set_seed_prefetch`` / ``apgp_get_seed_prefetch``,
``GP.seed_prefetch``): host code only, no GPU.  The two symbols are declared, the switch is on by default (6 tiles, as
far as the stage ring of the smallest part holds), returns the previous value, clamps to 0 .. 6, and a GP leaves the
process-wide setting alone unless told otherwise."""
import numpy as np


def test_the_library_switch_defaults_to_on_and_round_trips():
    from approxposterior_amd import _lib
    assert "apgp_set_seed_prefetch" in _lib.SIGNATURES and "apgp_get_seed_prefetch" in _lib.SIGNATURES
    lib = _lib.load()
    assert lib.apgp_get_seed_prefetch() == 6
    try:
        assert lib.apgp_set_seed_prefetch(0) == 6 and lib.apgp_get_seed_prefetch() == 0
        assert lib.apgp_set_seed_prefetch(3) == 0 and lib.apgp_get_seed_prefetch() == 3
        assert lib.apgp_set_seed_prefetch(99) == 3 and lib.apgp_get_seed_prefetch() == 6     # more than the ring holds: 6
        assert lib.apgp_set_seed_prefetch(-2) == 6 and lib.apgp_get_seed_prefetch() == 0     # negative: off
    finally:
        lib.apgp_set_seed_prefetch(6)
    assert lib.apgp_get_seed_prefetch() == 6
    assert lib.apgp_abi_version() == _lib.ABI_VERSION == 8


def test_a_gp_takes_the_library_setting_by_default():
    from approxposterior_amd import gp as agp
    gp = agp.GP(kernel=agp.ExpSquaredKernel(np.full(3, 8.0), ndim=3))
    assert gp.seed_prefetch is None and gp.seed_park is None
