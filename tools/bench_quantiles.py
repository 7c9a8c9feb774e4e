"""On-device quantiles against the host route: the C2 model (10-d LG-SSM) and
the Kitagawa model (d = 1) at 2^20 particles, after 5 warm steps with
maybe_resample before each.

python tools/bench_quantiles.py [--particles N] [--steps T] [--calls C] [--host-calls H] [--windows W]
Prints one JSON line.  Per model, for the current step and for an earlier step
(t = 2: the walk crosses the resamples since), microseconds per call (median
of W windows; the two routes alternate inside every window, all in one
process) of
  (a) quantiles(st, [0.05, 0.5, 0.95], t), event-timed over C calls (every
      call ends in its own synchronise),
  (b) the route without gh_pf_quantiles: state.states(t) + get_log_weights and
      a numpy sort per component with the cumulative weights searched, by the
      host clock around H such rounds (each ends in synchronising copies),
their ratio, the algorithmic bytes of one pass over the state, N (8 d + 8),
and that pass's share of the 8 TB/s HBM peak with the pass time taken as the
call time over the 8 passes (a call's 17 launches, copy and synchronise
included, and a dense d = 10 pass reads the state once per probability: a
lower bound of the histogram kernel's share).
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
PROBS = [0.05, 0.5, 0.95]
PASSES = 8


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--particles", type=int, default=1 << 20)
    p.add_argument("--steps", type=int, default=6)
    p.add_argument("--calls", type=int, default=50)
    p.add_argument("--host-calls", type=int, default=2)
    p.add_argument("--windows", type=int, default=3)
    a = p.parse_args()
    import torch

    import gen_amd as gen

    ctx = gen.Context(device=0)
    gen.set_default_context(ctx)
    h = ctx.stream()
    stream = torch.cuda.ExternalStream(h) if h else torch.cuda.default_stream()

    def host_route(st, t):
        x, lw = st.states(t), gen.get_log_weights(st)
        w = np.exp(lw - lw.max())
        out = np.empty((len(PROBS), x.shape[1]))
        for k in range(x.shape[1]):
            order = np.argsort(x[:, k], kind="stable")
            cum = np.cumsum(w[order])
            idx = np.minimum(np.searchsorted(cum, np.array(PROBS) * cum[-1], side="left"), len(cum) - 1)
            out[:, k] = x[order[idx], k]
        return out

    def device_window(st, t):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(a.calls):
            gen.quantiles(st, PROBS, t)
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.calls

    def host_window(st, t):
        t0 = time.perf_counter()
        for _ in range(a.host_calls):
            host_route(st, t)
        return (time.perf_counter() - t0) * 1e6 / a.host_calls

    results = {}
    for name, m in (("lg10", gen.LinearGaussianSSM.benchmark(10)), ("kitagawa", gen.KitagawaSSM(10.0, 1.0))):
        _, ys = m.simulate(a.steps, np.random.default_rng(2))
        st = gen.initialize_particle_filter(m, (1,), {m.obs_address(1): ys[0]}, a.particles, seed=42)
        fired = 0
        for t in range(2, a.steps + 1):  # steps - 1 >= 5 warm steps
            fired += bool(gen.maybe_resample(st))
            gen.particle_filter_step(st, (t,), (gen.UnknownChange(),), {m.obs_address(t): ys[t - 1]})
        d = m.d
        nbytes = a.particles * (8 * d + 8)
        for label, t in (("current", None), ("earlier", 2)):
            dev, ref = gen.quantiles(st, PROBS, t), host_route(st, t)  # warm-up of both routes, and they agree
            # (the host route's weights are rounded sums: it may pick a neighbouring order statistic)
            spread = st.states(t).std(axis=0)
            assert (np.abs(dev - ref) <= 1e-3 * spread).all(), (name, label, dev, ref)
            ta, tb = [], []
            for _ in range(a.windows):
                ta.append(device_window(st, t))
                tb.append(host_window(st, t))
            us_dev, us_host = statistics.median(ta), statistics.median(tb)
            results[f"{name}_{label}"] = {
                "d": d, "resamples": fired, "quantiles_us": us_dev, "host_route_us": us_host,
                "host_over_quantiles": us_host / us_dev, "windows_us": {"quantiles": ta, "host_route": tb},
                "bytes_per_pass": nbytes, "pass_us_upper_bound": us_dev / PASSES,
                "hbm_peak_share_per_pass": nbytes / HBM_PEAK / (us_dev / PASSES * 1e-6),
            }
        st.close()
    print(json.dumps({
        "metric": "quantiles(st, [0.05, 0.5, 0.95]) of a filter's particles, us per call",
        "config": {"particles": a.particles, "steps": a.steps, "calls": a.calls, "host_calls": a.host_calls,
                   "windows": a.windows, "probs": PROBS},
        "results": results,
    }), flush=True)


if __name__ == "__main__":
    main()
