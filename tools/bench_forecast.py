"""forecast against the route without it: the C2 model (10-d LG-SSM) at 2^20
particles, horizon 8, means and covariances, no draws.

python tools/bench_forecast.py [--particles N] [--steps T] [--horizon H] [--calls C]
Prints one JSON line: microseconds per call, the median of C event-timed calls
after one warm-up of each route, of
  (a) forecast(st, H, cov=True) on the filter at step T,
  (b) the only route to the same numbers without gh_pf_forecast: H times an
      unobserved particle_filter_step and estimate(cov=True) on a scratch
      filter (same model, seed and steps, record_history off so that no history
      slot is allocated inside the timed window; it keeps stepping from call to
      call, every call the same work),
both in one process, alternating, in both orders (call i runs (a) first when i
is even, (b) first when odd); their ratio (b) / (a) and each route's spread
(min, max).  The x moments of (a) and of (b)'s first call are compared, so the
two routes are timed on the same computation.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--particles", type=int, default=1 << 20)
    p.add_argument("--steps", type=int, default=6)
    p.add_argument("--horizon", type=int, default=8)
    p.add_argument("--calls", type=int, default=5)
    a = p.parse_args()
    import torch

    import gen_amd as gen

    ctx = gen.Context(device=0)
    gen.set_default_context(ctx)
    m = gen.LinearGaussianSSM.benchmark(10)
    _, ys = m.simulate(a.steps, np.random.default_rng(2))

    def make(**kw):
        st = gen.initialize_particle_filter(m, (1,), ys[0], a.particles, seed=42, **kw)
        for t in range(2, a.steps + 1):
            gen.maybe_resample(st)
            gen.particle_filter_step(st, (t,), (gen.UnknownChange(),), ys[t - 1])
        return st

    st, scratch = make(), make(record_history=False)
    h = ctx.stream()
    stream = torch.cuda.ExternalStream(h) if h else torch.cuda.default_stream()
    H = a.horizon

    def route_forecast():
        return gen.forecast(st, H)

    def route_steps():
        out = []
        for _ in range(H):
            t = scratch.t + 1
            gen.particle_filter_step(scratch, (t,), (gen.UnknownChange(),), None)
            out.append(gen.estimate(scratch))
        return out

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        f()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3

    fc, ref = route_forecast(), route_steps()  # the warm-up of each route, and the two agree
    for k in range(H):
        assert np.allclose(fc.x_mean[k], ref[k].mean, rtol=1e-9, atol=1e-12), k
        assert np.allclose(fc.x_cov[k], ref[k].cov, rtol=1e-8, atol=1e-12), k
    ta, tb = [], []
    for i in range(a.calls):
        if i % 2 == 0:
            ta.append(timed(route_forecast))
            tb.append(timed(route_steps))
        else:
            tb.append(timed(route_steps))
            ta.append(timed(route_forecast))
    us = {"forecast": statistics.median(ta), "steps_and_estimates": statistics.median(tb)}
    print(json.dumps({
        "metric": "h-step-ahead predictive means and covariances of x and y, us per call",
        "config": {"model": "lg10", "particles": a.particles, "steps": a.steps, "horizon": H, "calls": a.calls},
        "us_per_call": us,
        "calls_us": {"forecast": ta, "steps_and_estimates": tb},
        "spread_us": {"forecast": [min(ta), max(ta)], "steps_and_estimates": [min(tb), max(tb)]},
        "steps_over_forecast": us["steps_and_estimates"] / us["forecast"],
    }), flush=True)
    st.close()
    scratch.close()


if __name__ == "__main__":
    main()
