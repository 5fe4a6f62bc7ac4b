# -*- coding: utf-8 -*-
"""Static checks of the built gfx950 code objects (no GPU needed: the library is disassembled, not run)."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_no_wide_store_has_its_data_registers_overwritten_at_once():
    """A 16-byte VMEM store reads its data registers late; LLVM exempts MUBUF stores with an SGPR soffset from the
    wait state, MI355X does not (round 4: wrong low words under valid tags in the persistent Cholesky's granule
    stream, csrc/apgp_common.h APGP_STORE16).  Every wide store in the shipped library must keep its data registers
    untouched for the next two issue slots."""
    from approxposterior_amd import _lib
    tools = "/opt/rocm/lib/llvm/bin"
    if not (os.path.exists(_lib.LIB_PATH) and os.path.exists(os.path.join(tools, "llvm-objdump"))
            and os.path.exists(os.path.join(tools, "clang-offload-bundler"))):
        # (a host-only box without the ROCm toolchain or the built library: nothing to disassemble -- the GPU suite's
        # test_cabi_symbols / every -m gpu test still fails loudly without the library)
        pytest.skip("libapgp.so or the ROCm LLVM tools are missing")
    n_objects, wide, found = _tool("check_store_hazard").check(_lib.LIB_PATH)
    assert n_objects >= 6 and wide > 100          # every translation unit was looked at
    assert not found, "\n".join(found[:10])
