"""The boundary of the gradient moves (CPU only): include/gen_hip.h declares
gh_pf_choice_gradients, gh_pf_mala and gh_pf_hmc, libgen_hip.so exports them,
the ctypes binding has their signatures and the package their Python forms.
"""
import ctypes
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gen_hip.h")
SYMS = ["gh_pf_choice_gradients", "gh_pf_mala", "gh_pf_hmc"]


def test_boundary_of_the_gradient_moves():
    import gen_amd as gen
    from gen_amd import _lib

    text = open(HEADER).read()
    table = text[: text.index("Conventions")]
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.load()
    for s in SYMS:
        assert re.search(r"\bint\s+%s\s*\(\s*gh_pf\s*\*" % s, code), s  # declared
        assert s in table, s  # and listed in the table of replaced reference functions
        assert hasattr(lib, s), s
        assert s in _lib.SIGNATURES, s
    c_int, c_double, c_void_p, u32 = ctypes.c_int, ctypes.c_double, ctypes.c_void_p, ctypes.c_uint32
    pd, pi64 = ctypes.POINTER(c_double), ctypes.POINTER(ctypes.c_int64)
    assert _lib.SIGNATURES["gh_pf_choice_gradients"] == (c_int, [c_void_p, u32, pd, pd])
    assert _lib.SIGNATURES["gh_pf_mala"] == (c_int, [c_void_p, u32, c_double, c_int, pi64])
    assert _lib.SIGNATURES["gh_pf_hmc"] == (c_int, [c_void_p, u32, c_int, c_double, c_int, pi64])
    for f in ("choice_gradients", "mala", "hmc"):
        assert callable(getattr(gen, f)) and f in gen.__all__
    # the reference's defaults (hmc.jl:25: L=10, eps=0.1)
    p = inspect.signature(gen.hmc).parameters
    assert (p["L"].default, p["eps"].default, p["n_moves"].default) == (10, 0.1, 1)
    assert inspect.signature(gen.mala).parameters["n_moves"].default == 1


def test_null_filter_is_refused_before_the_device():
    from gen_amd import _lib

    lib = _lib.load()
    g = (ctypes.c_double * 1)()
    assert lib.gh_pf_choice_gradients(None, 1, None, g) == 1
    assert lib.gh_pf_mala(None, 1, 0.1, 1, None) == 1
    assert lib.gh_pf_hmc(None, 1, 10, 0.1, 1, None) == 1
    assert b"null" in lib.gh_last_error()
