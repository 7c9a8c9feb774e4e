"""The boundary of the weight history and of backward simulation (CPU only):
include/gen_hip.h declares gh_pf_get_log_weights_at, gh_pf_backward_weights
and gh_pf_smooth and lists them among the replaced reference functions,
libgen_hip.so exports them, the ctypes binding has their signatures and the
package their Python forms; gh_pf_opts keeps its size with record_weights in
the first reserved word; and `reference_pick` / `reference_u53`, the host
restatements of the header's selection that tests/test_smooth.py compares the
device against bit for bit, are pinned here on cases worked by hand.

The restatement uses Python integers for q, S and the target (nothing rounds),
the oracle's orc_exp for the exp (tests/test_gpu_parity.py pins it bit for bit
to the device's) and the oracle's Philox with the engine's counter layout
(rng_block: counter = (id lo, id hi, step, stream << 16 | draw), key = seed).
"""
import ctypes
import math
import re

import numpy as np

from tests.test_quantiles_abi import HEADER, quant_shift

STREAM_SMOOTH = 8
SYMBOLS = ("gh_pf_get_log_weights_at", "gh_pf_backward_weights", "gh_pf_smooth")


# ----------------------------------------------------------- the reference
def reference_u53(seed, m, t):
    """The 53-bit uniform of trajectory m at step t: u53_bits of the first two
    words of rng_block(seed, m, t, STREAM_SMOOTH, 0)."""
    from oracle import oracle as O

    seed, m = int(seed) & (2 ** 64 - 1), int(m)
    w = O.philox([m & 0xFFFFFFFF, m >> 32, int(t), STREAM_SMOOTH << 16], [seed & 0xFFFFFFFF, seed >> 32])
    return ((w[0] >> 5) << 26) | (w[1] >> 6)


def reference_q(b, n=None, pending=False):
    """q_i = floor(exp(b_i - B) 2^shift), B = max b, as Python ints (2^shift
    each while a resample is pending); b_i = -inf gives 0."""
    from oracle import oracle as O

    n = len(b) if n is None else n
    shift = quant_shift(n)
    if pending:
        return [1 << shift] * len(b)
    L = O.lib()
    B = float(np.max(b))
    assert math.isfinite(B) and not np.isnan(b).any()
    scale = 2.0 ** shift
    return [0 if v == -math.inf else int(math.floor(L.orc_exp(float(v) - B) * scale)) for v in b]


def reference_pick_q(q, u):
    """The first i whose inclusive sum exceeds target = floor(u S / 2^53)."""
    S = sum(q)
    assert S > 0 and 0 <= u < 2 ** 53
    target = (u * S) >> 53
    c = 0
    for i, v in enumerate(q):
        c += v
        if c > target:
            return i
    raise AssertionError("target < S: some inclusive sum exceeds it")


def reference_pick(b, u, n, pending=False):
    """The pick among n particles of log-weights b under the 53-bit uniform u."""
    assert len(b) == n
    return reference_pick_q(reference_q(np.asarray(b, dtype=np.float64), n, pending), int(u))


# ------------------------------------------------------------ the boundary
def test_boundary_of_the_smoother():
    import gen_amd as gen
    from gen_amd import _lib

    text = open(HEADER).read()
    table = text[: text.index("Conventions")]
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.load()
    for s in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(\s*gh_pf\s*\*" % s, code), s  # declared
        assert s in table, s
        assert hasattr(lib, s), s
    c_int, c_void_p, pd = ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)
    assert _lib.SIGNATURES["gh_pf_get_log_weights_at"] == (c_int, [c_void_p, c_int, pd])
    assert _lib.SIGNATURES["gh_pf_backward_weights"] == (c_int, [c_void_p, c_int, pd, pd])
    assert _lib.SIGNATURES["gh_pf_smooth"] == (c_int, [c_void_p, c_int, ctypes.c_int64, ctypes.c_uint64, pd,
                                                       ctypes.POINTER(ctypes.c_int32)])
    for f in ("smooth", "SmoothedTrajectories", "backward_weights"):
        assert hasattr(gen, f) and f in gen.__all__
    assert "record_weights" in code


def test_opts_keep_their_size():
    from gen_amd import _lib

    assert ctypes.sizeof(_lib.PFOpts) == 32 and _lib.PFOpts.record_weights.offset == 20
    o = _lib.PFOpts()
    o.record_weights = 7
    _lib.load().gh_pf_opts_default(ctypes.byref(o))
    assert o.record_weights == 0 and o.record_history == 1


def test_null_arguments_are_refused_before_the_device():
    from gen_amd import _lib

    lib = _lib.load()
    x, out = (ctypes.c_double * 1)(0.5), (ctypes.c_double * 1)()
    assert lib.gh_pf_get_log_weights_at(None, 1, out) == 1 and b"null" in lib.gh_last_error()
    assert lib.gh_pf_backward_weights(None, 1, x, out) == 1 and b"null" in lib.gh_last_error()
    assert lib.gh_pf_smooth(None, 1, 1, 0, out, None) == 1 and b"null" in lib.gh_last_error()


# ------------------------------------- the reference, on cases worked by hand
def test_reference_equal_weights():
    """n = 4: shift = 52, q = 2^52 each, S = 2^54, target = floor(u 2^54 / 2^53)
    = 2 u, and the inclusive sums are (i + 1) 2^52: the first one that EXCEEDS
    2 u is i = floor(u / 2^51).  u = 0 -> 0; u = 2^51 - 1 -> 0 (the last u of
    the first quarter); u = 2^51 -> target 2^52, which the first sum equals and
    does not exceed -> 1; u = 2^52 -> 2; u = 2^53 - 1 -> 3.

    The rule is "exceeds", cdf_search's: with "reaches", u = 0 would pick a
    first particle of weight 0 (the next case)."""
    b = np.full(4, -3.5)
    assert reference_q(b) == [1 << 52] * 4
    us = (0, (1 << 51) - 1, 1 << 51, 1 << 52, (1 << 53) - 1)
    assert [reference_pick(b, u, 4) for u in us] == [0, 0, 1, 2, 3]
    # pending: every q = 2^shift, the weights are not read
    assert reference_pick(np.array([-1.0, -9.0, 0.0, -2.0]), 3 << 51, 4, pending=True) == 3


def test_reference_one_particle_carries_the_weight():
    """exp(-2000) is 0 and -inf is 0 by definition: q = 0, 2^52, 0; every u picks 1."""
    b = np.array([-2000.0, 0.0, -math.inf])
    assert reference_q(b) == [0, 1 << 52, 0]
    for u in (0, 1, 1 << 52, (1 << 53) - 1):
        assert reference_pick(b, u, 3) == 1


def test_reference_a_block_of_minus_inf_is_never_picked():
    """n = 9: shift = 52 still; four particles of weight 2^52 around five of
    weight 0.  S = 2^54; u = 2^52 gives target 2^53, the second inclusive sum,
    which is not exceeded until particle 7."""
    b = np.array([0.0, 0.0] + [-math.inf] * 5 + [0.0, 0.0])
    assert quant_shift(9) == 52
    assert reference_q(b) == [1 << 52 if v == 0.0 else 0 for v in b]
    assert {reference_pick(b, u, 9) for u in range(0, 1 << 53, 1 << 44)} == {0, 1, 7, 8}
    assert reference_pick(b, (1 << 52) - 1, 9) == 1 and reference_pick(b, 1 << 52, 9) == 7


def test_reference_u53_is_the_engines_counter_layout():
    """Distinct (seed, m, t) give distinct uniforms below 2^53, and the words
    are those of Philox4x32-10 on (m lo, m hi, t, 8 << 16) keyed by the seed."""
    from oracle import oracle as O

    us = {reference_u53(s, m, t) for s in (0, 1, 2 ** 40 + 3) for m in (0, 1, 65535) for t in (1, 2, 50)}
    assert len(us) == 27 and all(0 <= u < 2 ** 53 for u in us)
    w = O.philox([5, 0, 3, 8 << 16], [7, 0])
    assert reference_u53(7, 5, 3) == ((w[0] >> 5) << 26) | (w[1] >> 6)
    assert reference_u53(7, 5, 3) != reference_u53(7, 3, 5)
