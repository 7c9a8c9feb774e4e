"""The boundary of forecast (CPU only): include/gen_hip.h declares
gh_pf_forecast and lists it in the table of replaced reference functions with
the Gen functions it stands for, libgen_hip.so exports it, the ctypes binding
has its signature, the package its Python forms, and a null filter is refused
before the device is touched.
"""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gen_hip.h")


def test_boundary_of_the_forecast():
    import gen_amd as gen
    from gen_amd import _lib

    text = open(HEADER).read()
    table = text[: text.index("Conventions")]
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    s = "gh_pf_forecast"
    assert re.search(r"\bint\s+%s\s*\(\s*gh_pf\s*\*\s*pf\s*,\s*int\s+horizon\s*,\s*const\s+double\s*\*\s*inputs" % s, code)
    row = table[table.index(s):]
    row = row[: row.index("gh_pf_get_scores")]
    for ref in ("particle_filter_step!", "EmptyChoiceMap", "particle_filter.jl:139-160", "unfold/update.jl:54-78",
                "static_ir/simulate.jl:23-34"):
        assert ref in row, ref
    assert "1..64" in text[text.index("The posterior predictive"):]  # the interface limit is stated
    lib = _lib.load()
    assert hasattr(lib, s)
    c_int, c_void_p, pd = ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)
    assert _lib.SIGNATURES[s] == (c_int, [c_void_p, c_int, pd, pd, pd, pd, pd, pd, pd])
    for f in ("forecast", "ParticleForecast"):
        assert callable(getattr(gen, f)) and f in gen.__all__
    assert gen.ParticleForecast._fields == ("x_mean", "x_cov", "y_mean", "y_cov", "xs", "ys")


def test_null_filter_is_refused_before_the_device():
    from gen_amd import _lib

    lib = _lib.load()
    out = (ctypes.c_double * 4)()
    assert lib.gh_pf_forecast(None, 1, None, out, None, None, None, None, None) == 1
    assert b"null" in lib.gh_last_error()
