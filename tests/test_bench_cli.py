"""bench.py's command line: a plain run measures the headline alone, --full
adds the rest, and --dump-outputs writes the timed filter's final outputs.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

DUMPED = ("particle_index", "states", "log_weights", "parents", "log_ml", "ess", "resampled")


def test_plain_run_is_the_default():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    a = bench.parse(["--full", "--dump-outputs", "somewhere"])
    assert a.full and a.dump_outputs == "somewhere"


class _FakeState:
    """The accessors dump_outputs reads, on host arrays."""

    def __init__(self, n, d, t):
        self.n_local = n
        self.model = type("Model", (), {"d": d})
        self._x = np.arange(n * d, dtype=np.float64).reshape(n, d)
        self._t = t

    def states(self):
        return self._x

    @property
    def log_weights(self):
        return -self._x[:, 0]

    @property
    def parents(self):
        return np.arange(self.n_local, dtype=np.int64)[::-1]

    def ess_history(self):
        return np.linspace(1.0, 2.0, self._t), np.arange(self._t) % 2 == 0


class _FakeGen:
    @staticmethod
    def log_ml_estimate(st):
        return -12.5


@pytest.mark.parametrize("n,d", [(100, 3), (bench.DUMP_SAMPLE + 3, 3), (bench.DUMP_SAMPLE, 40)])
def test_dump_outputs_files(tmp_path, n, d):
    t = 5
    st = _FakeState(n, d, t)
    bench.dump_outputs(_FakeGen, st, str(tmp_path / "a"), 0, 1)
    bench.dump_outputs(_FakeGen, st, str(tmp_path / "b"), 0, 1)
    got = {k: np.load(tmp_path / "a" / f"{k}.npy") for k in DUMPED}
    assert sorted(os.listdir(tmp_path / "a")) == sorted(f"{k}.npy" for k in DUMPED)
    assert all(v.dtype == np.float64 for v in got.values())
    assert sum(v.nbytes for v in got.values()) <= 64 << 20
    m = min(n, bench.DUMP_SAMPLE, bench.DUMP_BYTES // (8 * (d + 3)))
    idx = got["particle_index"].astype(np.int64)
    assert idx.shape == (m,) and np.all(np.diff(idx) > 0) and 0 <= idx[0] and idx[-1] < n
    assert np.array_equal(got["states"], st.states()[idx])
    assert np.array_equal(got["log_weights"], st.log_weights[idx])
    assert np.array_equal(got["parents"], st.parents[idx])
    assert got["log_ml"].tolist() == [-12.5]
    assert got["ess"].shape == (t,) and got["resampled"].tolist() == [1.0, 0.0, 1.0, 0.0, 1.0]
    for k in DUMPED:  # the sample is fixed: a second dump writes the same files
        assert np.array_equal(got[k], np.load(tmp_path / "b" / f"{k}.npy"))


@pytest.mark.gpu
def test_plain_bench_line_and_dump(gh_ctx, tmp_path):
    """A plain run in a process of its own: the result line holds the headline
    and none of the --full sections, --steps sets the timed steps (the
    filter's history holds the init, the warm-up and exactly that many), and
    the dumped arrays are those of the same filter built here through the
    package's own calls."""
    import gen_amd as gen

    n, d, steps, warmup = 4096 + 640, 4, 3, 2
    argv = ["--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--particles", str(n), "--d", str(d)]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv, "--dump-outputs", str(tmp_path / "a")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "roofline"):
        assert k in out
    assert out["steps"] == steps and out["warmup"] == warmup and out["ms_per_step"] > 0
    assert out["value"] == pytest.approx(n * 1e3 / out["ms_per_step"], rel=1e-9)
    assert out["log_ml_error"] is None and "cpu_baseline" not in out and "secondary" not in out

    assert out["config"]["filters"] == 1
    got = {k: np.load(tmp_path / "a" / f"{k}.npy") for k in DUMPED}
    assert all(v.dtype == np.float64 for v in got.values())
    assert got["ess"].shape == got["resampled"].shape == (1 + warmup + steps,)
    assert int(got["resampled"][warmup : warmup + steps].sum()) == out["config"]["resample_steps_timed"]
    assert got["log_ml"][0] == out["config"]["log_ml"]
    assert np.array_equal(got["particle_index"], np.arange(n))

    model = gen.LinearGaussianSSM.benchmark(d)
    _, ys = model.simulate(warmup + steps + 1, np.random.default_rng(2))
    st = gen.initialize_particle_filter(model, (1,), {("chain", 1, "y"): ys[0]}, n, seed=42, ctx=gh_ctx)
    gen.run_particle_filter(st, list(ys[1:]), None)
    ess, did = st.ess_history()
    assert np.array_equal(got["states"], st.states())
    assert np.array_equal(got["log_weights"], st.log_weights)
    assert np.array_equal(got["parents"], st.parents)
    assert np.array_equal(got["ess"], ess) and np.array_equal(got["resampled"], did.astype(np.float64))
    assert got["log_ml"][0] == gen.log_ml_estimate(st)
    st.close()


def test_filter_plan():
    cap = bench.MAX_FILTER_STEPS
    # one filter, warm-up then the timed steps, while they fit
    assert bench.filter_plan(5, 20) == [(5, 20)]
    assert bench.filter_plan(0, cap) == [(0, cap)]
    assert bench.filter_plan(12, cap - 12) == [(12, cap - 12)]
    # beyond: every filter within the cap, the timed steps summing to --steps
    assert bench.filter_plan(12, cap - 11) == [(12, cap - 12), (12, 1)]
    assert bench.filter_plan(cap, 5) == [(cap, 0), (16, 5)]
    assert bench.filter_plan(2 * cap + 7, 1) == [(cap, 0), (16, 1)]
    for w, n in ((10, 16384), (0, 1000), (100, 5 * cap + 1)):
        plan = bench.filter_plan(w, n)
        assert all(ws + ns <= cap for ws, ns in plan) and sum(ns for _, ns in plan) == n
        assert plan[0][0] == min(w, cap) and all(ws == min(w, 16) and ns > 0 for ws, ns in plan[1:])


@pytest.mark.gpu
def test_long_run_goes_through_bounded_filters(gh_ctx, tmp_path):
    """More timed steps than one filter's history takes: the run continues in
    a second filter over the same observation series, and what it dumps is
    that filter's state (here rebuilt directly from the series)."""
    import gen_amd as gen

    n, d, warmup = 4096 + 640, 4, 3
    steps = bench.MAX_FILTER_STEPS + 8
    a = bench.parse(["--steps", str(steps), "--warmup", str(warmup), "--particles", str(n), "--d", str(d)])
    a.time_every = 10
    model = gen.LinearGaussianSSM.benchmark(d)
    r = bench.pf_run(gen, gh_ctx, None, 1, a, model, n, "", lambda n_res: 16 * d + 16, dump=str(tmp_path))
    plan = bench.filter_plan(warmup, steps)
    assert r["filters"] == len(plan) == 2 and r["dt"] > 0 and 0 <= r["n_res"] <= steps
    assert r["roofline"]["kernel_launches"] > 0 and r["roofline"]["kernel_avg_ms"] > 0
    T = warmup + steps + 1
    _, ys = model.simulate(T, np.random.default_rng(2))
    first = T - sum(plan[-1])  # the last filter ends with the series; ys[first] is its first step
    assert np.array_equal(np.asarray(r["ys_last"]), np.asarray(ys[first - 1 :]))
    st = gen.initialize_particle_filter(model, (1,), {("chain", 1, "y"): ys[first - 1]}, n, seed=42, ctx=gh_ctx)
    gen.run_particle_filter(st, list(ys[first:]), None)
    assert gen.log_ml_estimate(st) == r["lml"] == np.load(tmp_path / "log_ml.npy")[0]
    assert np.array_equal(st.states(), np.load(tmp_path / "states.npy"))
    assert np.array_equal(st.log_weights, np.load(tmp_path / "log_weights.npy"))
    assert np.array_equal(st.parents, np.load(tmp_path / "parents.npy"))
    st.close()
