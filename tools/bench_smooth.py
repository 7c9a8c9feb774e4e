"""smooth (backward simulation on the device) against the route without it, and
the price of the weight history it reads.

python tools/bench_smooth.py [--particles N] [--traj M] [--steps T] [--windows W] [--no-host]
Prints one JSON line.  Per model (the 10-d LG-SSM of C2, whose Q is diagonal;
the same model with a dense Q; the nonlinear SSM of C4) at N = 2^16 particles
and M = 256 trajectories over T steps:

  device    microseconds per backward step: an event-timed gen.smooth(st, M) call
            (the start draw, T - 1 backward steps of four launches each, the copy
            of the draws to the host) divided by T - 1; the median of W windows
            after one warm-up call, with the windows' spread.
  host      the same draws' distribution without gh_pf_smooth: every step's
            particles as the caller kept them while filtering (states() after
            each step: states(t) of the finished filter follows the surviving
            genealogy, not step t's particles), get_log_weights(st, t) and a
            numpy FFBSi — per step the n x M matrix of backward weights in
            trajectory blocks, a softmax-free cumulative sum per trajectory and
            a searchsorted.  Host clock, per backward step, W windows.
  fp64      the transition densities' floating-point operations per (particle,
            trajectory) pair that the model's instantiation executes (an FMA
            counts 2; a diagonal chol(Q) skips the forward substitution), times
            2 n M per backward step (the maximum pass and the sum pass evaluate
            every pair once each), over the device time per backward step, as a
            share of the part's vector fp64 peak (78.6 TFLOP/s).  The time is
            the whole call's, so the figure is a floor for the kernels' own.

and for the C2 loop (run_particle_filter, the 10-d LG-SSM at 2^20 particles):

  record_weights   microseconds per {maybe_resample; step} with the option on
                   and off, two filters in one process, event-timed windows of
                   20 steps alternating between them; the median of W windows
                   each and their difference (one 8 n-byte copy per step).
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

FP64_VECTOR_PEAK = 78.6e12


def lg_flops(d, dense_q):
    """What LGModel<d, S>::score executes for the latent at t >= 2: mean = A x +
    b (d^2 FMA), r = x~ - mean (d), the forward substitution with chol(Q) (d (d
    - 1) / 2 FMA) only when chol(Q) is not diagonal (the host then picks a
    structure without bit 0), d divisions, the quadratic form (d FMA), the
    constant and the weight (3).  d = 10: 243 with a diagonal Q, 333 with a
    dense one."""
    return 2 * d * d + d + (d * (d - 1) if dense_q else 0) + d + 2 * d + 3


KIT_FLOPS = 14  # x / 2 + 25 x / (1 + x^2) + ct (7, a division), the normal log-density (5), the weight (2)


def host_ffbsi(rows, lws, logpdf, M, rng, block=16):
    """numpy FFBSi over the kept particles rows[t] [n, d] and weights lws[t]
    [n], t = 1..T: idx [T, M].  logpdf(t, X, Y) -> [n, m]: the density of step
    t + 1's states Y [m, d] given step t's X [n, d]."""
    T = len(rows)
    n = rows[1].shape[0]
    idx = np.empty((T, M), dtype=np.int64)
    w = np.exp(lws[T] - lws[T].max())
    idx[T - 1] = np.searchsorted(np.cumsum(w), rng.random(M) * w.sum(), side="right").clip(0, n - 1)
    per_step = []
    for t in range(T - 1, 0, -1):
        t0 = time.perf_counter()
        Y = rows[t + 1][idx[t]]
        for m0 in range(0, M, block):
            b = lws[t][:, None] + logpdf(t, rows[t], Y[m0:m0 + block])
            c = np.cumsum(np.exp(b - b.max(axis=0)), axis=0)
            u = rng.random(c.shape[1]) * c[-1]
            idx[t - 1, m0:m0 + block] = (c <= u).sum(axis=0).clip(0, n - 1)
        per_step.append((time.perf_counter() - t0) * 1e6)
    return idx, per_step


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--particles", type=int, default=1 << 16)
    p.add_argument("--traj", type=int, default=256)
    p.add_argument("--steps", type=int, default=6)
    p.add_argument("--windows", type=int, default=3)
    p.add_argument("--c2-particles", type=int, default=1 << 20)
    p.add_argument("--no-host", action="store_true")
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

    n, M, T = a.particles, a.traj, a.steps
    out = {"metric": "backward simulation, us per backward step",
           "config": {"particles": n, "trajectories": M, "steps": T, "windows": a.windows}}

    lg = gen.LinearGaussianSSM.benchmark(10)
    assert not np.any(lg.Q - np.diag(np.diag(lg.Q)))  # (the C2 model: a diagonal Q, LGModel<10, 3>)
    G = 0.1 * np.random.default_rng(7).standard_normal((10, 10))
    lgd = gen.LinearGaussianSSM(lg.A, lg.Q + G @ G.T, lg.H, lg.R, lg.mu0, lg.P0, b=lg.b, c=lg.c)
    kit = gen.KitagawaSSM(10.0, 1.0)

    def lg_logpdf_of(m):
        Linv = np.linalg.inv(np.linalg.cholesky(m.Q))
        cst = -0.5 * (m.d * np.log(2 * np.pi) + np.linalg.slogdet(m.Q)[1])

        def logpdf(t, X, Y):
            mean = X @ m.A.T + m.b                        # [n, d]: the per-particle part, once per step
            z = (Y[None, :, :] - mean[:, None, :]) @ Linv.T
            return cst - 0.5 * np.einsum("nmd,nmd->nm", z, z)
        return logpdf

    def kit_logpdf(t, X, Y):
        x = X[:, 0]
        mean = x / 2 + 25 * x / (1 + x * x) + 8 * np.cos(1.2 * (t + 1))
        r = Y[None, :, 0] - mean[:, None]
        return -r * r / (2 * kit.var_x) - 0.5 * np.log(2 * np.pi * kit.var_x)

    for name, m, flops, logpdf in (("lg10", lg, lg_flops(10, False), lg_logpdf_of(lg)),
                                   ("lg10_dense_q", lgd, lg_flops(10, True), lg_logpdf_of(lgd)),
                                   ("kitagawa", kit, KIT_FLOPS, kit_logpdf)):
        _, ys = m.simulate(T, np.random.default_rng(2))
        st = gen.initialize_particle_filter(m, (1,), {m.obs_address(1): ys[0]}, n, seed=42, record_weights=True)
        rows = {1: st.states()}
        for t in range(2, T + 1):
            gen.maybe_resample(st)
            gen.particle_filter_step(st, (t,), (gen.UnknownChange(),), {m.obs_address(t): ys[t - 1]})
            rows[t] = st.states()
        sm = gen.smooth(st, M, seed=1)  # the warm-up
        calls = [timed(lambda: gen.smooth(st, M, seed=2 + i)) for i in range(a.windows)]
        per_step = [c / (T - 1) for c in calls]
        dev = statistics.median(per_step)
        r = {"device_us_per_backward_step": dev, "device_windows_us": per_step, "device_call_us": calls,
             "flops_per_pair": flops,
             "fp64_tflops": 2.0 * n * M * flops / (dev * 1e-6) / 1e12,
             "fp64_share_of_vector_peak": 2.0 * n * M * flops / (dev * 1e-6) / FP64_VECTOR_PEAK,
             "pairs_per_second": 2.0 * n * M / (dev * 1e-6)}
        if not a.no_host:
            rng = np.random.default_rng(3)
            wins = []
            for _ in range(a.windows):
                t0 = time.perf_counter()
                lws = {t: gen.get_log_weights(st, t) for t in range(1, T + 1)}
                fetch = (time.perf_counter() - t0) * 1e6
                hidx, steps_us = host_ffbsi(rows, lws, logpdf, M, rng)
                wins.append((fetch + sum(steps_us)) / (T - 1))
            host = statistics.median(wins)
            r.update({"host_us_per_backward_step": host, "host_windows_us": wins, "host_over_device": host / dev,
                      # the two routes draw from the same distribution: the smoothed means of step 1 side by side
                      "mean_step1_device": sm.xs[0].mean(axis=0)[:2].tolist(),
                      "mean_step1_host": rows[1][hidx[0]].mean(axis=0)[:2].tolist()})
        out[name] = r
        st.close()

    # the price of record_weights in the C2 loop
    nc, K = a.c2_particles, 20
    _, ys = lg.simulate(6 + (1 + a.windows) * K, np.random.default_rng(2))
    ys = [np.asarray(y) for y in ys]
    mk = lambda rw: gen.initialize_particle_filter(lg, (1,), {lg.obs_address(1): ys[0]}, nc, seed=42,
                                                   record_weights=rw, history_capacity=len(ys) + 2)
    on, off = mk(True), mk(False)
    pos = {id(on): 1, id(off): 1}

    def window(st, k):
        i = pos[id(st)]
        pos[id(st)] = i + k
        return timed(lambda: gen.run_particle_filter(st, ys[i:i + k])) / k

    for st in (on, off):
        window(st, 5 + K)  # the warm-up
    t_on, t_off = [], []
    for i in range(a.windows):
        for st, acc in ((on, t_on), (off, t_off)) if i % 2 == 0 else ((off, t_off), (on, t_on)):
            acc.append(window(st, K))
    out["record_weights"] = {"particles": nc, "steps_per_window": K, "on_us_per_step": statistics.median(t_on),
                             "off_us_per_step": statistics.median(t_off), "on_windows_us": t_on, "off_windows_us": t_off,
                             "difference_us": statistics.median(t_on) - statistics.median(t_off),
                             "copy_bytes_per_step": 8 * nc}
    on.close()
    off.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
