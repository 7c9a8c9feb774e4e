"""The boundary of elliptical_slice and map_optimize (CPU only):
include/gen_hip.h declares gh_pf_elliptical_slice and gh_pf_map_optimize,
libgen_hip.so exports them, the ctypes binding has their signatures and the
package their Python forms.
"""
import ctypes
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gen_hip.h")
SYMS = ["gh_pf_elliptical_slice", "gh_pf_map_optimize"]


def test_boundary_of_the_slice_moves():
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
    assert "elliptical_slice.jl:13-45" in table and "map_optimize.jl:9-41" in table
    c_int, c_double, c_void_p, u32 = ctypes.c_int, ctypes.c_double, ctypes.c_void_p, ctypes.c_uint32
    pi64 = ctypes.POINTER(ctypes.c_int64)
    assert _lib.SIGNATURES["gh_pf_elliptical_slice"] == (c_int, [c_void_p, u32, c_int, pi64, pi64])
    assert _lib.SIGNATURES["gh_pf_map_optimize"] == (c_int, [c_void_p, u32, c_double, c_double, c_double, c_int, pi64])
    for f in ("elliptical_slice", "map_optimize"):
        assert callable(getattr(gen, f)) and f in gen.__all__
    # the reference's defaults (map_optimize.jl:9-10)
    p = inspect.signature(gen.map_optimize).parameters
    assert list(p)[:2] == ["state", "selection"]
    assert (p["max_step_size"].default, p["tau"].default, p["min_step_size"].default, p["n_iters"].default) == \
        (0.1, 0.5, 1e-16, 1)
    p = inspect.signature(gen.elliptical_slice).parameters
    assert list(p) == ["state", "selection", "n_moves"] and p["n_moves"].default == 1
    doc = " ".join(gen.elliptical_slice.__doc__.split())
    assert "not arguments" in doc and "likelihood only" in doc


def test_null_filter_is_refused_before_the_device():
    from gen_amd import _lib

    lib = _lib.load()
    assert lib.gh_pf_elliptical_slice(None, 1, 1, None, None) == 1
    assert b"null" in lib.gh_last_error()
    assert lib.gh_pf_map_optimize(None, 1, 0.1, 0.5, 1e-16, 1, None) == 1
    assert b"null" in lib.gh_last_error()
