"""``morl_lcn_select`` is declared in include/morl_hip.h, exported by the gfx950 library and by the host-emulated build, bound in
native.py with the header's argument types, documented in INTEGRATION.md -- and refuses what is outside its limits with
``MORL_ERR_ARG`` (-1) and a message before any device call.  No GPU: the refusals come before anything is launched."""
import ctypes as C
import os
import re

import pytest

import simlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "morl_hip.h")
ERR_ARG = -1


@pytest.fixture(scope="module")
def sim():
    return simlib.load_sim()


def libs(sim):
    from morl_baselines_amd.native import load_library
    return [sim, load_library()]


def test_declared_with_the_documented_signature_and_limit():
    src = open(HEADER).read()
    m = re.search(r"int morl_lcn_select\(([^)]*)\);", src)
    assert m, "morl_lcn_select is not declared in include/morl_hip.h"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    # lcn_lambda is a double: the kernel needs float(1.0 - lcn_lambda) of the reference's Python float, which a float cannot carry
    assert args == ["const float* returns", "int N", "int R", "int mode", "double lcn_lambda", "const uint8_t* crowded",
                    "float* l2_out", "uint8_t* nd_out", "void* stream"]
    limit = int(re.search(r"#define MORL_LCN_MAX_N (\d+)", src).group(1))
    from morl_baselines_amd import lcn
    assert limit == lcn.MAX_EPISODES and limit >= 2048, "the header states the upper limit of N (at least 2 048 at R = 8)"
    assert int(re.search(r"#define MORL_ABI_VERSION (\d+)", src).group(1)) == 13, "an additive entry leaves the ABI version"
    kernels = open(os.path.join(ROOT, "morl-baselines_amd", "csrc", "lcn_kernels.h")).read()
    assert f"LCN_MAX_N = {limit};" in kernels


def test_bound_exported_and_documented(sim):
    import morl_baselines_amd.native as native
    assert "morl_lcn_select" in native.EXPORTED_SYMBOLS
    for lib in libs(sim):
        fn = lib.lib.morl_lcn_select
        assert fn.restype is C.c_int
        assert fn.argtypes == [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        assert lib.lib.morl_abi_version() == native.ABI_VERSION == 13
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    row = [ln for ln in doc.splitlines() if ln.startswith("| `morl_lcn_select`")]
    assert len(row) == 1 and "lcn.py" in row[0] and "_nlargest" in row[0], "the symbol <-> call-site row"
    assert "from morl_baselines_amd.lcn import LCN" in doc, "the registration line"
    for name in ("README.md", "DESIGN.md"):
        assert "morl_lcn_select" in open(os.path.join(ROOT, name)).read(), name


def test_refusals_need_no_device(sim):
    for lib in libs(sim):
        L, err = lib.lib.morl_lcn_select, lib.lib.morl_last_error
        p = 4096            # (never dereferenced: every call below is refused first)
        assert L(None, 4, 2, 1, 0.0, None, None, p, None) == ERR_ARG and b"NULL" in err()
        assert L(p, 4, 2, 1, 0.0, None, None, None, None) == ERR_ARG and b"NULL" in err()
        assert L(p, 4, 2, 1, 0.0, p, None, p, None) == ERR_ARG and b"together" in err()
        assert L(p, 0, 2, 1, 0.0, None, None, p, None) == ERR_ARG and b"N=0" in err()
        assert L(p, 2049, 8, 1, 0.0, p, p, p, None) == ERR_ARG and b"N=2049 outside 1..2048" in err()
        assert L(p, -1, 8, 1, 0.0, p, p, p, None) == ERR_ARG and b"N=-1" in err()
        assert L(p, 4, 0, 1, 0.0, p, p, p, None) == ERR_ARG and b"R=0" in err()
        assert L(p, 4, 9, 1, 0.0, p, p, p, None) == ERR_ARG and b"R=9 outside 1..8" in err()
        assert L(p, 4, 2, 3, 0.0, p, p, p, None) == ERR_ARG and b"mode=3" in err()
        assert L(p, 4, 2, 2, float("inf"), p, p, p, None) == ERR_ARG and b"lcn_lambda" in err()
