"""A numpy restatement of the particle-Gibbs chain of tests/test_ancestor.py
(no GPU): the figures that DESIGN.md 7t and the test's docstring cite, and the
source of the test's bounds.

python tools/pgas_chain.py [T] [seeds]      (default 40 30)

Model tests/test_csmc.py::_lg1 (A = 0.9, Q = 0.5, H = 1, R = 0.8), observations
m.simulate(T, default_rng(12)), 16 particles, a multinomial resample at every
step, 600 sweeps from a zero reference of which 100 are burn-in.  Per variant
(with ancestor sampling over `seeds` chain seeds, without over 5): the largest
error of the mean references against the RTS means, worst and best seed, and
the share of sweeps after burn-in in which x_1 differs from the sweep before.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests.test_csmc import _lg1, _rts_means  # noqa: E402


def chain(ys, T, N, sweeps, burn, seed, anc):
    a, q, h, r = 0.9, 0.5, 1.0, 0.8
    rng = np.random.default_rng(seed)
    ref = np.zeros(T)
    acc = np.zeros(T)
    moved = 0
    for k in range(sweeps):
        X = np.empty((T, N))
        P = np.zeros((T, N), dtype=int)
        x = rng.standard_normal(N) * 1.0
        x[0] = ref[0]
        lw = -0.5 * (ys[0] - h * x) ** 2 / r
        X[0] = x
        for t in range(1, T):
            w = np.exp(lw - lw.max())
            par = rng.choice(N, size=N, p=w / w.sum())
            if anc:
                b = lw - 0.5 * (ref[t] - a * x) ** 2 / q
                wb = np.exp(b - b.max())
                par[0] = rng.choice(N, p=wb / wb.sum())
            else:
                par[0] = 0
            xn = a * x[par] + np.sqrt(q) * rng.standard_normal(N)
            xn[0] = ref[t]
            x = xn
            lw = -0.5 * (ys[t] - h * x) ** 2 / r
            X[t] = x
            P[t] = par
        w = np.exp(lw - lw.max())
        i = rng.choice(N, p=w / w.sum())
        new = np.empty(T)
        for t in range(T - 1, -1, -1):
            new[t] = X[t, i]
            i = P[t, i]
        if k >= burn:
            moved += new[0] != ref[0]
            acc += new
        ref = new
    return acc / (sweeps - burn), moved / (sweeps - burn)


if __name__ == "__main__":
    T = int(sys.argv[1]) if len(sys.argv) > 1 else 40
    seeds = int(sys.argv[2]) if len(sys.argv) > 2 else 30
    m = _lg1()
    _, ys = m.simulate(T, np.random.default_rng(12))
    ys = np.asarray(ys).ravel()
    exact = _rts_means(m, ys)
    for anc in (True, False):
        errs, mv = [], []
        for s in range(seeds if anc else min(seeds, 5)):
            est, moved = chain(ys, T, 16, 600, 100, s, anc)
            errs.append(np.max(np.abs(est - exact)))
            mv.append(moved)
        print(f"T={T} anc={anc}: max err worst {max(errs):.3f} best {min(errs):.3f}; moved {min(mv):.3f}..{max(mv):.3f}", flush=True)
