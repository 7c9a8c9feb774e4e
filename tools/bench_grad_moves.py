"""Gradient, slice and map_optimize moves against the drift move: the C2 model
(10-d LG-SSM) or the nonlinear SSM at 2^20 particles, after 5 steps.

python tools/bench_grad_moves.py [--model lg10|kit] [--particles N] [--steps T] [--moves M] [--reps R]
Prints one JSON line: microseconds per move (event-timed median of R
repetitions of M moves each, after one untimed warm-up call of each) of
gh_pf_mh_drift, gh_pf_mala, gh_pf_hmc with L = 1 and with L = 10,
gh_pf_elliptical_slice and gh_pf_map_optimize (per iteration), their ratios to
the drift move, particle-moves per second and a rate per move: accepted moves
per particle-move, shrinks per particle-move (elliptical_slice), improved
iterations per particle-iteration (map_optimize).  All in one process.  Every
call, the warm-up included, starts from a fresh filter with the same seed, so
each repetition times the same work (map_optimize converges: a second call
on the same filter would time particles that sit on their mode).
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
    p.add_argument("--model", choices=["lg10", "kit"], default="lg10")
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
    m = gen.LinearGaussianSSM.benchmark(10) if a.model == "lg10" else gen.KitagawaSSM(10.0, 1.0)
    _, ys = m.simulate(a.steps, np.random.default_rng(2))
    ys = [np.atleast_1d(y) for y in ys]

    def fresh():
        st = gen.initialize_particle_filter(m, (1,), ys[0], a.particles, seed=42)
        for t in range(2, a.steps + 1):
            gen.maybe_resample(st)
            gen.particle_filter_step(st, (t,), (gen.UnknownChange(),), ys[t - 1])
        return st

    h = ctx.stream()
    stream = torch.cuda.ExternalStream(h) if h else torch.cuda.default_stream()
    lg = a.model == "lg10"
    sd = np.full(m.d, 0.2 if lg else 1.0)
    tau, eps1, eps10, step = (0.04, 0.3, 0.1, 0.05) if lg else (0.6, 1.2, 0.15, 0.5)
    # step sizes in the regime of the tests (acceptance 0.3-0.97 at t > 1); map_optimize's
    # max_step_size below the stability limit of every particle, so an iteration is one evaluation
    moves = {
        "mh_drift": lambda st, n, acc: lib.gh_pf_mh_drift(st.h, 1, _lib.dptr(sd), n, acc),
        "mala": lambda st, n, acc: lib.gh_pf_mala(st.h, 1, tau, n, acc),
        "hmc_L1": lambda st, n, acc: lib.gh_pf_hmc(st.h, 1, 1, eps1, n, acc),
        "hmc_L10": lambda st, n, acc: lib.gh_pf_hmc(st.h, 1, 10, eps10, n, acc),
        "elliptical_slice": lambda st, n, acc: lib.gh_pf_elliptical_slice(st.h, 1, n, acc, None),
        "map_optimize": lambda st, n, acc: lib.gh_pf_map_optimize(st.h, 1, step, 0.5, 1e-16, n, acc),
    }
    us, rate = {}, {}
    for name, f in moves.items():
        acc = c_int64()
        st = fresh()
        _lib.check(f(st, a.moves, byref(acc)))  # warm-up (synchronises)
        st.close()
        rate[name] = acc.value / (a.moves * a.particles)
        ts = []
        for _ in range(a.reps):
            st = fresh()
            st.states()  # (synchronises: the filter's steps are not in the timed span)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            _lib.check(f(st, a.moves, None))
            e1.record(stream)
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3 / a.moves)
            st.close()
        us[name] = statistics.median(ts)
    print(json.dumps({
        "metric": "rejuvenation moves on every particle, us per move",
        "config": {"model": a.model, "particles": a.particles, "steps": a.steps, "moves_per_call": a.moves,
                   "reps": a.reps},
        "us_per_move": us,
        "ratio_to_drift": {k: v / us["mh_drift"] for k, v in us.items()},
        "particle_moves_per_s": {k: a.particles / (v * 1e-6) for k, v in us.items()},
        "rate": rate,
    }), flush=True)


if __name__ == "__main__":
    main()
