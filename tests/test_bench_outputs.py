"""bench.py --dump-outputs: what the headline leg's last step left for its caller, written as .npy files so that two builds
can be compared output for output; and the plain run (no --full) times the headline leg only.  The helper is checked on
the CPU; one GPU test runs bench.py and replays the same passes through the C ABI."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_dump_outputs_writes_every_array_whole_under_the_limit(tmp_path):
    rng = np.random.default_rng(1)
    arrays = {"u0": rng.normal(size=(16, 3)), "ut": rng.normal(size=(16, 20, 3)).astype(np.float32)}
    bench.dump_outputs(str(tmp_path), arrays)
    assert sorted(os.listdir(tmp_path)) == ["u0.npy", "ut.npy"]
    for name, a in arrays.items():
        b = np.load(tmp_path / (name + ".npy"))
        assert b.dtype == a.dtype and np.array_equal(a, b)


def test_dump_outputs_samples_rows_past_the_limit_and_stays_under_it(tmp_path):
    rng = np.random.default_rng(2)
    arrays = {"u0": rng.normal(size=(1000, 3)), "ut": rng.normal(size=(1000, 50, 3))}
    limit = 300_000   # ut alone is 1.2 MB
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays, limit=limit)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["u0.npy", "ut.npy", "ut_rows.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= limit
    assert np.array_equal(np.load(tmp_path / "a" / "u0.npy"), arrays["u0"])
    rows = np.load(tmp_path / "a" / "ut_rows.npy")
    ut = np.load(tmp_path / "a" / "ut.npy")
    assert rows.dtype == np.float64 and len(rows) == len(ut) > 100 and np.all(np.diff(rows) > 0)
    assert np.array_equal(ut, arrays["ut"][rows.astype(np.int64)])
    # a fixed sample: the same rows every time
    for f in files:
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))


def test_bench_has_full_and_dump_outputs_options():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], cwd=ROOT, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--full" in r.stdout and "--dump-outputs" in r.stdout


@pytest.mark.gpu
def test_plain_run_dumps_what_its_last_step_computed(tmp_path):
    """A plain run (no --full): the line holds the headline and ms_per_step, no secondary leg ran; the dumped u0 / ut are
    the same bits on a second run and what the same passes give through eea_control_batch one call at a time"""
    torch = pytest.importorskip("torch")
    from ergodic_exploration_amd import capi
    from bench_legs import MAP_BOUNDS, MEANS, SIGMAS

    B, R, steps, warmup = 256, 10, 2, 1
    env = dict(os.environ, EEA_BENCH_SPINUP_PASSES="0", EEA_BENCH_DETAIL_DIR=str(tmp_path))
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    recs = []
    for d in ("a", "b"):
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
               "--passes-per-step", str(R), "--agents", str(B), "--dump-outputs", str(tmp_path / d)]
        r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        recs.append(json.loads(r.stdout.rstrip("\n").splitlines()[-1]))
    rec = recs[0]
    assert rec["steps"] == steps and rec["value"] > 0 and rec["dtype"] == "f64" and rec["higher_is_better"] is True
    assert rec["ms_per_step"] == pytest.approx(1e3 * rec["timed_region_s"] / steps, rel=1e-4)
    with open(tmp_path / "bench_detail.json") as f:
        detail = json.load(f)
    assert detail["config"]["optimisations_per_step"] == B * R
    for leg in ("single_launch_per_pass", "other_configs", "latency_mode", "single_robot_tick", "fleet_tick", "roofline_phik",
                "exchange", "grid_tile", "cpu_baseline", "cpu_baseline_all_cores"):
        assert leg not in detail, leg
    for name in ("u0", "ut"):
        assert np.array_equal(np.load(tmp_path / "a" / (name + ".npy")), np.load(tmp_path / "b" / (name + ".npy"))), name

    # the same (warmup + steps) x R passes from a zero warm start, one eea_control_batch call per pass
    lim = np.array([1.0, 0.0, 2.0])
    eng = capi.Engine(capi.make_config(capi.MODEL_SIMPLE_CART, 0.1, 20.0, 0.1, 1.0, 10, np.diag([1.0, 0.0, 2.0]), -lim, lim))
    try:
        eng.set_target_gaussians(MEANS, SIGMAS)
        eng.config_domain(MAP_BOUNDS)
        rng = np.random.default_rng(12345)
        poses = np.stack([rng.uniform(0.5, 11.5, B) - 1.0, rng.uniform(0.5, 5.5, B) - 1.0, rng.uniform(-np.pi, np.pi, B)], 1)
        d_pose = torch.as_tensor(poses).cuda()
        d_ut = torch.zeros((B, eng.T, 3), dtype=torch.float64, device="cuda")
        d_u0 = torch.empty((B, 3), dtype=torch.float64, device="cuda")
        for _ in range((warmup + steps) * R):
            eng.control_batch(B, d_pose, d_ut, d_u0)
        torch.cuda.synchronize()
        u0, ut = d_u0.cpu().numpy(), d_ut.cpu().numpy()
    finally:
        eng.close()
    got_u0, got_ut = np.load(tmp_path / "a" / "u0.npy"), np.load(tmp_path / "a" / "ut.npy")
    assert got_u0.dtype == np.float64 and got_u0.shape == u0.shape and got_ut.shape == ut.shape
    assert np.abs(got_u0 - u0).max() <= 1e-9 and np.abs(got_ut - ut).max() <= 1e-9
