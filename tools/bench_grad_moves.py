"""Gradient moves against the drift move: the C2 model (10-d LG-SSM) at 2^20
particles, after 5 steps.

python tools/bench_grad_moves.py [--particles N] [--steps T] [--moves M] [--reps R]
Prints one JSON line: microseconds per move (event-timed median of R
repetitions of M moves each, after one untimed warm-up call of each) of
gh_pf_mh_drift, gh_pf_mala, gh_pf_hmc with L = 1 and with L = 10, their ratios
to the drift move and the acceptance rates.  All in one process on one filter.
"""
import argparse
import json
import os
import statistics
import sys
from ctypes import byref, c_int64

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--particles", type=int, default=1 << 20)
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--moves", type=int, default=10)
    p.add_argument("--reps", type=int, default=5)
    a = p.parse_args()
    import torch

    import gen_amd as gen
    from gen_amd import _lib

    ctx = gen.Context(device=0)
    gen.set_default_context(ctx)
    lib = _lib.load()
    m = gen.LinearGaussianSSM.benchmark(10)
    _, ys = m.simulate(a.steps, np.random.default_rng(2))
    st = gen.initialize_particle_filter(m, (1,), ys[0], a.particles, seed=42)
    for t in range(2, a.steps + 1):
        gen.maybe_resample(st)
        gen.particle_filter_step(st, (t,), (gen.UnknownChange(),), ys[t - 1])
    h = ctx.stream()
    stream = torch.cuda.ExternalStream(h) if h else torch.cuda.default_stream()
    sd = np.full(m.d, 0.2)
    # step sizes in the regime of the tests (acceptance 0.3-0.97 at t > 1)
    moves = {
        "mh_drift": lambda n, acc: lib.gh_pf_mh_drift(st.h, 1, _lib.dptr(sd), n, acc),
        "mala": lambda n, acc: lib.gh_pf_mala(st.h, 1, 0.04, n, acc),
        "hmc_L1": lambda n, acc: lib.gh_pf_hmc(st.h, 1, 1, 0.3, n, acc),
        "hmc_L10": lambda n, acc: lib.gh_pf_hmc(st.h, 1, 10, 0.1, n, acc),
    }
    us, rate = {}, {}
    for name, f in moves.items():
        acc = c_int64()
        _lib.check(f(a.moves, byref(acc)))  # warm-up (synchronises)
        rate[name] = acc.value / (a.moves * a.particles)
        ts = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            _lib.check(f(a.moves, None))
            e1.record(stream)
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3 / a.moves)
        us[name] = statistics.median(ts)
    print(json.dumps({
        "metric": "rejuvenation moves on every particle, us per move (C2 model)",
        "config": {"particles": a.particles, "steps": a.steps, "moves_per_call": a.moves, "reps": a.reps},
        "us_per_move": us,
        "ratio_to_drift": {k: v / us["mh_drift"] for k, v in us.items()},
        "accept_rate": rate,
    }), flush=True)


if __name__ == "__main__":
    main()
