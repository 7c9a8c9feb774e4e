"""The price of ancestor sampling in a conditional step, and the same pick
through the backward-simulation kernels.

python tools/bench_ancestor.py [--windows W] [--steps K] [--lg-particles N] [--kit-particles N]
Prints one JSON line.

  conditional_step   per model (the 10-d LG-SSM of C2 at 2^20 particles, the
                     nonlinear SSM of C4 at 2^21): microseconds per
                     {maybe_resample; conditional step} with ancestor_sampling
                     on and off, two filters in one process on the same build,
                     a resample at every step (threshold n), event-timed
                     windows of K steps alternating between the two; the median
                     of W windows each, the windows themselves and the
                     difference: the three launches of gh_ancestor.h.
  bytes              what the three launches move per particle, from the shapes:
                     the row and the weight read once and b written (8 d + 8 +
                     8), b read again by the sum pass (8); the pick pass reads
                     one block.  Against the route below: the row and the
                     weight read twice, 2 (8 d + 8).
  smooth_one         the same pick through k_bs_max / k_bs_fold / k_bs_sum /
                     k_bs_pick: a filter with record_weights at the same n, an
                     event-timed smooth(st, 1, t0 = T - 1) (the start draw and
                     one backward step) minus smooth(st, 1, t0 = T) (the start
                     draw alone), medians of W calls each after a warm-up.
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
    p.add_argument("--windows", type=int, default=5)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--lg-particles", type=int, default=1 << 20)
    p.add_argument("--kit-particles", type=int, default=1 << 21)
    a = p.parse_args()
    import torch

    import gen_amd as gen

    ctx = gen.Context(device=0)
    gen.set_default_context(ctx)
    h = ctx.stream()
    stream = torch.cuda.ExternalStream(h) if h else torch.cuda.default_stream()

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        f()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3

    K, W = a.steps, a.windows
    out = {"metric": "ancestor sampling, us per conditional step", "config": {"windows": W, "steps_per_window": K}}
    for name, m, n in (("lg10", gen.LinearGaussianSSM.benchmark(10), a.lg_particles),
                       ("kitagawa", gen.KitagawaSSM(10.0, 1.0), a.kit_particles)):
        T = 6 + (1 + W) * K
        xs, ys = m.simulate(T, np.random.default_rng(2))
        ref = np.asarray(xs, dtype=np.float64).reshape(T, -1) * 0.9
        obs = lambda t: {m.obs_address(t): ys[t - 1]}
        mk = lambda on: gen.initialize_conditional_particle_filter(m, (1,), obs(1), n, ref[0], seed=42,
                                                                   record_history=False, ancestor_sampling=on)
        on, off = mk(True), mk(False)

        def window(st, k):
            def run():
                for _ in range(k):
                    t = st.t + 1
                    gen.maybe_resample_async(st, n)
                    gen.conditional_particle_filter_step(st, (t,), (gen.UnknownChange(),), obs(t), ref[t - 1])
            return timed(run) / k

        for st in (on, off):
            window(st, 5 + K)  # the warm-up
        t_on, t_off = [], []
        for i in range(W):
            for st, acc in ((on, t_on), (off, t_off)) if i % 2 == 0 else ((off, t_off), (on, t_on)):
                acc.append(window(st, K))
        fired = [bool(st.ess_history()[1][:st.t - 1].all()) for st in (on, off)]  # (entry s - 1: decided after step s)
        d = m.d
        r = {"particles": n, "on_us_per_step": statistics.median(t_on), "off_us_per_step": statistics.median(t_off),
             "on_windows_us": t_on, "off_windows_us": t_off,
             "added_us_per_step": statistics.median(t_on) - statistics.median(t_off),
             "every_resample_fired": fired,
             "bytes_per_particle": {"ancestor": (8 * d + 8) + 8 + 8, "smooth_route": 2 * (8 * d + 8)}}
        for st in (on, off):
            gen.log_ml_estimate(st)  # (a device error would surface here)
            st.close()

        # the same pick through the backward-simulation kernels, one trajectory
        Ts = 4
        st = gen.initialize_particle_filter(m, (1,), obs(1), n, seed=42, resampler="multinomial", record_weights=True)
        for t in range(2, Ts + 1):
            gen.maybe_resample(st, n)
            gen.particle_filter_step(st, (t,), (gen.UnknownChange(),), obs(t))
        for t0 in (Ts - 1, Ts):
            gen.smooth(st, 1, seed=1, t0=t0)  # the warm-up
        both = [timed(lambda: gen.smooth(st, 1, seed=2 + i, t0=Ts - 1)) for i in range(W)]
        start = [timed(lambda: gen.smooth(st, 1, seed=2 + i, t0=Ts)) for i in range(W)]
        st.close()
        r["smooth_one"] = {"start_and_one_backward_step_us": both, "start_alone_us": start,
                           "one_backward_step_us": statistics.median(both) - statistics.median(start)}
        out[name] = r
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
