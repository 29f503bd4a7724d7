"""bench.py's own options: a plain run is the headline alone (--full brings back the secondary legs), --steps is the number of
timed steps, and --dump-outputs writes what the last timed step computed -- a fixed, seeded column sample within 64 MB."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTPUTS = ("u", "u0", "flux_up", "flux_down_diffuse", "flux_down_direct")


def _bench_module():
    sys.path[:0] = [ROOT]
    import bench
    return bench


def _stub_bench(args, **env_over):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env.update(RTD_BENCH_STUB="1", RTD_BENCH_TIMEOUT="240")
    env.update(env_over)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True, timeout=300)


def _line(r):
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0 and len(lines) == 1, (r.returncode, r.stderr[-2000:])
    return json.loads(lines[0])


class _FakePlan:
    """fetch() as Plan.fetch returns it for cfg4 (32 streams, 21 depths, 3 azimuths); every value carries its column index."""

    def __init__(self, C):
        col = np.arange(C, dtype=np.float64)
        flux = col[:, None] + np.zeros((1, 21))
        self.res = dict(u=col[:, None, None, None] + np.linspace(0, 0.5, 32 * 21 * 3).reshape(1, 32, 21, 3),
                        u0=col[:, None, None] + np.zeros((1, 32, 21)), flux_up=flux, flux_down_diffuse=flux + 0.25,
                        flux_down_direct=flux + 0.75)

    def fetch(self):
        return {k: v.copy() for k, v in self.res.items()}


def test_dump_outputs_writes_the_same_seeded_sample_within_64_mb(tmp_path):
    bench = _bench_module()
    C = 3000
    plan = _FakePlan(C)
    for d in ("a", "b"):
        bench.dump_outputs(plan, str(tmp_path / d))
    assert sorted(os.listdir(tmp_path / "a")) == sorted(n + ".npy" for n in OUTPUTS)
    total = 0
    cols = None
    for n in OUTPUTS:
        x, y = np.load(tmp_path / "a" / (n + ".npy")), np.load(tmp_path / "b" / (n + ".npy"))
        assert x.dtype == np.float64 and np.array_equal(x, y)                  # same arguments, same files
        assert x.shape == (bench.DUMP_COLUMNS,) + plan.res[n].shape[1:]
        rows = np.floor(x.reshape(len(x), -1)[:, 0]).astype(int)
        assert cols is None or np.array_equal(rows, cols)                       # one sample of columns for every array
        cols = rows
        assert np.array_equal(x, plan.res[n][rows])                             # the rows ARE those columns' results
        total += os.path.getsize(tmp_path / "a" / (n + ".npy"))
    assert np.all(np.diff(cols) > 0) and cols[0] >= 0 and cols[-1] < C
    assert total <= 64 << 20


def test_dump_outputs_keeps_every_column_of_a_small_batch(tmp_path):
    bench = _bench_module()
    plan = _FakePlan(100)
    bench.dump_outputs(plan, str(tmp_path))
    for n in OUTPUTS:
        assert np.array_equal(np.load(tmp_path / (n + ".npy")), plan.res[n])


def test_plain_run_is_the_headline_alone_and_full_adds_the_secondary_legs():
    args = ["--gpus", "2", "--steps", "3", "--warmup", "1", "--columns", "3", "--total-columns", "0"]
    plain = _line(_stub_bench(args))
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in plain, key
    assert plain["steps"] == 3 and "value_cached_tables" not in plain
    # the stand-in rank sleeps 1 ms per step: --steps 3 -> 3 timed steps, ms_per_step = timed seconds / 3
    assert plain["ms_per_step"] >= 1.0 and abs(plain["ms_per_step"] - 1e3 * plain["timed_seconds"] / 3) < 1e-9
    full = _line(_stub_bench(args[:2] + ["--full"] + args[2:]))
    assert full["steps"] == 3 and full["value_cached_tables"] > 0


def test_steps_must_be_positive():
    r = _stub_bench(["--gpus", "2", "--steps", "0", "--warmup", "0", "--columns", "3", "--total-columns", "0"])
    assert r.returncode == 2 and "--steps" in r.stderr


@pytest.mark.gpu
def test_plain_run_dumps_what_its_last_timed_step_computed(tmp_path):
    """A plain one-GPU run with --dump-outputs: one line without the secondary legs, and the dumped rows equal a separate
    one-window solve of the same regenerated columns, bit for bit (windowing does not change a column's result)."""
    bench = _bench_module()
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    C = 4096
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--total-columns", str(C), "--dump-outputs", str(tmp_path)], env=env, capture_output=True, text=True, timeout=600)
    out = _line(r)
    assert out["n_gpus"] == 1 and out["steps"] == 3 and out["ms_per_step"] > 0 and out["value"] > 0
    for key in ("roofline", "other_configs", "e2e", "value_cached_tables"):
        assert key not in out, key
    assert out["cpu_baseline"] is None and "n_rank_check" not in out["multi_gpu"]
    got = {n: np.load(tmp_path / (n + ".npy")) for n in OUTPUTS}
    cols = bench.dump_sample(C, sum(v[0].nbytes for v in got.values()))
    assert all(v.shape[0] == len(cols) == bench.DUMP_COLUMNS and v.dtype == np.float64 for v in got.values())
    assert sum(os.path.getsize(tmp_path / (n + ".npy")) for n in OUTPUTS) <= 64 << 20
    sys.path[:0] = [os.path.join(ROOT, "pythonic-disort_amd")]
    from pydisort_amd._engine import Plan
    cfg, _, count = bench.shard_config(0, 1, 256, C)
    pick = [0, 1, len(cols) // 2, len(cols) - 1]
    idx = cols[pick]
    sub = {k: (v[idx] if isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == count else v) for k, v in cfg.items()}
    small = Plan(bench.prepare_cfg4(sub), device=0)
    try:
        small.set_eval_points(np.concatenate((np.zeros((len(idx), 1)), sub["tau_arr"]), axis=1), np.array([0.0, np.pi / 2, np.pi]))
        small.run()
        want = small.fetch()
    finally:
        small.close()
    for n in OUTPUTS:
        assert np.array_equal(got[n][pick], want[n]), n
