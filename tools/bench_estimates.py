"""On-device estimates against the host route: the C2 model (10-d LG-SSM) at
2^20 particles, after 5 warm steps.

python tools/bench_estimates.py [--particles N] [--steps T] [--calls C] [--host-calls H] [--windows W]
Prints one JSON line: microseconds per call (median of W windows; the three
routes alternate inside every window, all in one process) of
  (a) estimate(cov=False): the ESS and the weighted mean, one pass over the states,
  (b) estimate(cov=True): and the covariance, a second pass,
      both event-timed over C calls (every call ends in its own synchronise),
  (c) the route without gh_pf_estimate: state.states() + get_log_weights and
      the numpy reduction, by the host clock around H such rounds (each ends in
      synchronising copies),
the algorithmic bytes of one pass, N (8 d + 8), (a)'s share of the 8 TB/s HBM
peak (bytes over peak bandwidth, over the call time: a call's launches, copy
and synchronise included, so a lower bound of the kernel's share), and (b)/(a).
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

HBM_PEAK = 8e12  # bytes/s


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--particles", type=int, default=1 << 20)
    p.add_argument("--steps", type=int, default=6)
    p.add_argument("--calls", type=int, default=200)
    p.add_argument("--host-calls", type=int, default=200)
    p.add_argument("--windows", type=int, default=5)
    a = p.parse_args()
    import torch

    import gen_amd as gen

    ctx = gen.Context(device=0)
    gen.set_default_context(ctx)
    m = gen.LinearGaussianSSM.benchmark(10)
    _, ys = m.simulate(a.steps, np.random.default_rng(2))
    st = gen.initialize_particle_filter(m, (1,), ys[0], a.particles, seed=42)
    for t in range(2, a.steps + 1):  # steps - 1 >= 5 warm steps
        gen.maybe_resample(st)
        gen.particle_filter_step(st, (t,), (gen.UnknownChange(),), ys[t - 1])
    h = ctx.stream()
    stream = torch.cuda.ExternalStream(h) if h else torch.cuda.default_stream()

    def host_route():
        x, lw = st.states(), gen.get_log_weights(st)
        w = np.exp(lw - lw.max())
        W = w.sum()
        mean = w @ x / W
        dx = x - mean
        return W * W / (w * w).sum(), mean, (dx * w[:, None]).T @ dx / W

    def device_window(cov):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(a.calls):
            gen.estimate(st, cov=cov)
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.calls

    def host_window():
        t0 = time.perf_counter()
        for _ in range(a.host_calls):
            host_route()
        return (time.perf_counter() - t0) * 1e6 / a.host_calls

    est, ref = gen.estimate(st), host_route()  # warm-up of every route, and the two agree
    gen.estimate(st, cov=False)
    assert abs(est.ess - ref[0]) <= 1e-9 * ref[0] and np.allclose(est.mean, ref[1], rtol=1e-9, atol=1e-12)
    assert np.allclose(est.cov, ref[2], rtol=1e-8, atol=1e-12)
    ta, tb, tc = [], [], []
    for _ in range(a.windows):
        ta.append(device_window(False))
        tb.append(device_window(True))
        tc.append(host_window())
    us = {"estimate_mean": statistics.median(ta), "estimate_mean_cov": statistics.median(tb),
          "host_route": statistics.median(tc)}
    nbytes = a.particles * (8 * m.d + 8)
    print(json.dumps({
        "metric": "ESS + weighted mean (+ covariance) of a filter's particles, us per call",
        "config": {"model": "lg10", "particles": a.particles, "steps": a.steps, "calls": a.calls,
                   "host_calls": a.host_calls, "windows": a.windows, "ess": est.ess},
        "us_per_call": us,
        "windows_us": {"estimate_mean": ta, "estimate_mean_cov": tb, "host_route": tc},
        "bytes_per_pass": nbytes,
        "hbm_peak_share_mean": nbytes / HBM_PEAK / (us["estimate_mean"] * 1e-6),
        "cov_over_mean": us["estimate_mean_cov"] / us["estimate_mean"],
        "host_over_mean_cov": us["host_route"] / us["estimate_mean_cov"],
    }), flush=True)
    st.close()


if __name__ == "__main__":
    main()
