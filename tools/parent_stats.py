"""Which lines of x_{t-1} a C2 step reads: the survivors of every resample of
the bench's run, from the product's own parents.

  python tools/parent_stats.py [--steps 25] [--particles 1048576] [--out ANC.bin]

The bench's C2 filter (d = 10 `LinearGaussianSSM.benchmark`, observations of
numpy seed 2, filter seed 42, systematic resampling at ESS < N/2), stepped
call by call; after each step that followed a resample `st.parents` gives the
ancestors the step gathered.  Prints per step the share of particles with at
least one offspring and the share of the state bytes fetched under each
placement of a particle's 80 bytes:
  pair    wave tiles of 16-byte component pairs: a 128-B line holds one pair of
          8 consecutive particles (64-B sector: 4)
  row     one contiguous 80-byte row per particle
  chunk   32-byte chunks (4 particles per line) for components 0-7, a pair
          word for 8-9
--out writes the ancestors (int32, one block of N per resampled step) for
tools/ubench_layout.
"""
import argparse
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import gen_amd as gen  # noqa: E402
from gen_amd import _lib  # noqa: E402


def shares(parents, n):
    alive = np.unique(parents)
    row = alive * 80
    out = {"survivors": len(alive) / n}
    for name, g in (("line", 128), ("sector", 64)):
        per = g // 16  # particles per unit of one pair word
        out[f"pair_{name}"] = len(np.unique(alive // per)) / -(-n // per)
        first, last = row // g, (row + 79) // g
        out[f"row_{name}"] = len(np.unique(np.concatenate([first, last]))) * g / (80.0 * n)
        per32 = g // 32
        out[f"chunk_{name}"] = 0.8 * len(np.unique(alive // per32)) / -(-n // per32) + 0.2 * out[f"pair_{name}"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--particles", type=int, default=1 << 20)
    ap.add_argument("--d", type=int, default=10)
    ap.add_argument("--out")
    a = ap.parse_args()
    n = a.particles
    model = gen.LinearGaussianSSM.benchmark(a.d)
    _, ys = model.simulate(a.steps + 1, np.random.default_rng(2))
    st = gen.initialize_particle_filter(model, (1,), {model.obs_address(1): ys[0]}, n, seed=42,
                                        history_capacity=a.steps + 3)
    keys = ["survivors", "pair_line", "pair_sector", "row_line", "row_sector", "chunk_line", "chunk_sector"]
    print("step  ess/N   " + "  ".join(f"{k:>12s}" for k in keys))
    rows, out = [], open(a.out, "wb") if a.out else None
    for t in range(2, a.steps + 2):
        did, ess = ctypes.c_int(), ctypes.c_double()
        _lib.check(_lib.load().gh_pf_maybe_resample(st.h, n / 2, ctypes.byref(did), ctypes.byref(ess)))
        did, ess = bool(did.value), ess.value
        gen.particle_filter_step(st, (t,), (gen.UnknownChange(),), {model.obs_address(t): ys[t - 1]})
        if not did:
            print(f"{t:4d}  (no resample)")
            continue
        par = st.parents
        assert par.min() >= 0 and par.max() < n
        s = shares(par, n)
        rows.append([s[k] for k in keys])
        print(f"{t:4d}  {ess / n:6.4f}  " + "  ".join(f"{s[k]:12.3f}" for k in keys))
        if out:
            par.astype(np.int32).tofile(out)
    st.close()
    r = np.array(rows[1:])  # (the first resample follows the prior: degenerate)
    print(f"steps after the first resample: {len(r)}")
    for name, v in (("min", r.min(0)), ("median", np.median(r, 0)), ("mean", r.mean(0)), ("max", r.max(0))):
        print(f"{name:>6s}        " + "  ".join(f"{x:12.3f}" for x in v))


if __name__ == "__main__":
    main()
