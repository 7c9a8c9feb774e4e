"""Every step's summary in one walk against the per-step loop: the C2 model
(10-d LG-SSM) at 2^20 particles, T = 64 steps with maybe_resample before each.

python tools/bench_path.py [--particles N] [--steps T] [--calls C] [--windows W]
Prints one JSON line.  Milliseconds per whole path (all T steps; the median of
W windows, the four routes alternating inside every window, all in one
process, by the host clock around C rounds — every route ends each call in a
device synchronise) of
  (a) estimate_path(st)                         one sweep, one synchronise
  (b) [estimate(st, t) for t in 1..T]           T walks from T, T synchronises
  (c) quantiles_path(st, [0.05, 0.5, 0.95])
  (d) [quantiles(st, [0.05, 0.5, 0.95], t) for t in 1..T]
the ratios (b) / (a) and (d) / (c), every window's figures (their spread is
the noise a ratio has to clear), the ancestor hops of one pass of each route
(n times the step boundaries a resample preceded, counted from the decisions),
and `distinct` along the path.  Before timing, the routes are checked to agree
bit for bit.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PROBS = [0.05, 0.5, 0.95]


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--particles", type=int, default=1 << 20)
    p.add_argument("--steps", type=int, default=64)
    p.add_argument("--calls", type=int, default=3)
    p.add_argument("--windows", type=int, default=5)
    a = p.parse_args()

    import gen_amd as gen

    ctx = gen.Context(device=0)
    gen.set_default_context(ctx)
    m = gen.LinearGaussianSSM.benchmark(10)
    T, n = a.steps, a.particles
    _, ys = m.simulate(T, np.random.default_rng(2))
    st = gen.initialize_particle_filter(m, (1,), {m.obs_address(1): ys[0]}, n, seed=42)
    fired = [False, False]  # fired[t]: a resample preceded step t
    for t in range(2, T + 1):
        fired.append(bool(gen.maybe_resample(st)))
        gen.particle_filter_step(st, (t,), (gen.UnknownChange(),), {m.obs_address(t): ys[t - 1]})

    routes = {
        "estimate_path": lambda: gen.estimate_path(st),
        "estimate_loop": lambda: [gen.estimate(st, t) for t in range(1, T + 1)],
        "quantiles_path": lambda: gen.quantiles_path(st, PROBS),
        "quantiles_loop": lambda: [gen.quantiles(st, PROBS, t) for t in range(1, T + 1)],
    }
    # warm-up of every route, and they agree
    path, loop = routes["estimate_path"](), routes["estimate_loop"]()
    qpath, qloop = routes["quantiles_path"](), routes["quantiles_loop"]()
    bits = lambda x, y: np.array_equal(np.asarray(x).view(np.uint64), np.asarray(y).view(np.uint64))
    for t in range(T):
        assert bits(path.mean[t], loop[t].mean) and bits(path.cov[t], loop[t].cov) and bits(qpath[t], qloop[t]), t

    def window(f):
        t0 = time.perf_counter()
        for _ in range(a.calls):
            f()
        return (time.perf_counter() - t0) * 1e3 / a.calls

    w = {k: [] for k in routes}
    for _ in range(a.windows):
        for k, f in routes.items():
            w[k].append(window(f))
    ms = {k: statistics.median(v) for k, v in w.items()}
    hops_sweep = n * sum(fired[2:])
    hops_loop = n * sum(sum(fired[t + 1:]) for t in range(1, T + 1))
    st.close()
    print(json.dumps({
        "metric": "the summaries of all T steps of a filter's path, ms per path",
        "config": {"particles": n, "steps": T, "calls": a.calls, "windows": a.windows, "probs": PROBS, "d": m.d},
        "resamples": sum(fired),
        "hops_per_pass": {"sweep": hops_sweep, "loop": hops_loop},
        "ms": ms,
        "estimate_loop_over_path": ms["estimate_loop"] / ms["estimate_path"],
        "quantiles_loop_over_path": ms["quantiles_loop"] / ms["quantiles_path"],
        "windows_ms": w,
        "distinct": path.distinct.tolist(),
        "path_ess": [round(float(v), 1) for v in path.ess],
    }), flush=True)


if __name__ == "__main__":
    main()
