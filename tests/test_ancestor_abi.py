"""The boundary of ancestor sampling (CPU only): gh_pf_opts keeps its size with
ancestor_sampling in the first of the two words that were reserved,
include/gen_hip.h declares and documents the option, the Python forms carry
the keyword, and `reference_u53`, the host restatement of the uniform that
tests/test_ancestor.py feeds to tests/test_smooth_abi.py's `reference_pick`,
is pinned on a counter worked by hand.

The uniform of the distinguished particle's parent at step t is u53_bits of
the first two words of Philox4x32-10 on the engine's counter layout
(rng_block: counter = (id lo, id hi, step, stream << 16 | draw), key = seed)
with id 0, stream 10 (STREAM_ANCESTOR) and draw 0, keyed by the filter's seed.
"""
import ctypes
import inspect
import re

from tests.test_quantiles_abi import HEADER
from tests.test_smooth_abi import reference_u53 as smooth_u53

STREAM_ANCESTOR = 10


def reference_u53(seed, m, t):
    """The 53-bit uniform of id m (the filter: 0) at step t on stream 10."""
    from oracle import oracle as O

    seed, m = int(seed) & (2 ** 64 - 1), int(m)
    w = O.philox([m & 0xFFFFFFFF, m >> 32, int(t), STREAM_ANCESTOR << 16], [seed & 0xFFFFFFFF, seed >> 32])
    return ((w[0] >> 5) << 26) | (w[1] >> 6)


def test_opts_keep_their_size_and_default():
    from gen_amd import _lib

    assert ctypes.sizeof(_lib.PFOpts) == 32
    assert _lib.PFOpts.record_weights.offset == 20 and _lib.PFOpts.ancestor_sampling.offset == 24
    assert _lib.PFOpts.reserved.offset == 28 and _lib.PFOpts.reserved.size == 4
    o = _lib.PFOpts()
    o.ancestor_sampling = 7
    _lib.load().gh_pf_opts_default(ctypes.byref(o))
    assert o.ancestor_sampling == 0 and o.record_weights == 0 and o.record_history == 1


def test_header_declares_and_documents_the_option():
    text = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\} gh_pf_opts;", code).group(1)
    fields = re.findall(r"int32_t\s+(\w+)(\[\d+\])?;", body)
    assert [f for f, _ in fields] == ["resampler", "record_history", "history_capacity", "block_size", "time_kernels",
                                      "record_weights", "ancestor_sampling", "reserved"]
    assert fields[-1][1] == ""  # one reserved word left
    table = text[: text.index("Conventions")]
    assert "ancestor_sampling" in table
    doc = text[text.index("Conditional SMC (examples/pmmh/smc.jl"):]
    doc = doc[: doc.index("gh_pf_step_conditional(gh_pf* pf")]
    for word in ("ancestor_sampling", "Lindsten", "gh_pf_backward_weights", "10 << 16", "GH_E_NUMERIC",
                 "gh_pf_step_params_conditional", "no random variable"):
        assert word in doc, word


def test_reference_u53_is_stream_10_of_the_engines_counter_layout():
    """Seed 7, id 0, step 3: the words of Philox4x32-10 on (0, 0, 3, 10 << 16) =
    (0, 0, 3, 0xA0000) keyed by (7, 0); the same (seed, 0, t) on stream 8 (the
    smoother's trajectory 0) gives another uniform."""
    from oracle import oracle as O

    w = O.philox([0, 0, 3, 0xA0000], [7, 0])
    assert w[:2] == [15474949, 1528831464]  # (the literal words: a pin, not the helper's own call again)
    # (15474949 >> 5) << 26 = 483592 * 2^26, 1528831464 >> 6 = 23887991
    assert reference_u53(7, 0, 3) == 483592 * 2 ** 26 + 23887991 == 32453333647479
    assert smooth_u53(7, 0, 3) == 2713443934628465  # stream 8 on the same (seed, 0, t)
    us = {reference_u53(s, 0, t) for s in (0, 1, 2 ** 40 + 3) for t in (2, 3, 50)}
    assert len(us) == 9 and all(0 <= u < 2 ** 53 for u in us)
    for s, t in ((7, 3), (0, 2), (2 ** 40 + 3, 50)):
        assert reference_u53(s, 0, t) != smooth_u53(s, 0, t)


def test_python_forms_carry_the_keyword():
    import gen_amd as gen
    from gen_amd import pf

    for f in (gen.initialize_conditional_particle_filter, gen.conditional_smc, gen.particle_gibbs):
        p = inspect.signature(f).parameters["ancestor_sampling"]
        assert p.default is False, f.__name__
        assert "smc.jl" in f.__doc__ and "Lindsten" in f.__doc__, f.__name__
    assert "record_weights" in inspect.signature(gen.conditional_smc).parameters
    assert "ancestor_sampling" in inspect.signature(pf._opts).parameters
    assert pf._opts("multinomial", True, 0, 0, False, True).ancestor_sampling == 1
    assert pf._opts("multinomial", True, 0, 0).ancestor_sampling == 0
