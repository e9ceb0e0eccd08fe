"""bench.py as the driver runs it: the JSON contract, roofline / parity fields on a small workload, the N > 1 code path
(tile-set dispatch + RCCL gather behind the C ABI) forced onto one GPU -- also with HIP-graph replay on, the
configuration that faulted in round 1 -- and the launcher-less `--gpus N` form."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--scene", "cornellbox", "--width", "256", "--height", "256", "--bounces", "8"]


def run_bench(extra_env, *args, check=True):
    env = dict(os.environ)
    env.update(extra_env)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True, env=env, timeout=900)
    if not check:
        return p
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_line_contract(built):
    d = run_bench({}, "--steps", "4", "--warmup", "2", "--full", *SMALL)
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "dtype", "data", "config", "roofline", "cpu_baseline", "parity"):
        assert key in d, key
    assert d["n_gpus"] == 1 and d["steps"] == 4 and d["warmup"] == 2 and d["value"] > 0 and d["higher_is_better"] is True
    assert "workload" in d["config"] and d["vs_baseline"] is None and d["scaling"] == "strong"
    assert d["cpu_baseline"]["kind"] == "port" and d["cpu_baseline"]["cores"] >= 1 and d["cpu_baseline"]["value"] > 0
    assert d["parity"]["differing_f16_words"] == 0 and d["parity"]["rmse_vs_cpu_restatement"] == 0.0
    r = d["roofline"]
    # the Cornell box is staged in LDS: its tracer is not an HBM kernel and the line says so
    assert r["bound"] == "lds/issue" and r["peak"] == 8000.0 and r["achieved"] > 0 and r["bytes_per_unit"] > 56 and r["peak_measured"] > 1000
    assert d["config"]["frames_in_flight"] == 4 and d["config"]["traversal"] == "binary"   # reported by the library (LDS-resident scene: four lanes)
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    assert d["hip_runtime"]["num_hip_runtimes_mapped"] == 1


@pytest.mark.gpu
def test_plain_line_and_dumped_outputs(built, tmp_path):
    """Without --full the line holds the headline only; --dump-outputs writes the last timed frame, the same from run to run."""
    import numpy as np
    runs = []
    for k in range(2):
        out = tmp_path / f"run{k}"
        d = run_bench({}, "--steps", "3", "--warmup", "1", "--dump-outputs", str(out), *SMALL)
        assert d["steps"] == 3 and d["value"] > 0 and d["ms_per_step"] > 0 and abs(d["ms_per_step"] - d["timed_seconds"] / 3 * 1e3) < 1e-6
        assert d["roofline"] is None and d["cpu_baseline"] is None and d["parity"] is None and "configs" not in d
        runs.append({n[:-len(".npy")]: np.load(out / n) for n in os.listdir(out)})
    a, b = runs
    assert sorted(a) == ["frame_block_mean", "frame_pixel_index", "frame_pixels"]
    assert a["frame_pixels"].dtype == np.float32 and a["frame_pixels"].shape == (256 * 256, 4)   # a small frame is written whole
    assert a["frame_block_mean"].dtype == np.float64 and a["frame_block_mean"].shape == (32, 32, 4)
    assert np.array_equal(a["frame_pixel_index"], np.arange(256 * 256)) and a["frame_pixels"][:, :3].max() > 0
    for n in a:
        assert np.array_equal(a[n], b[n]), n


@pytest.mark.gpu
@pytest.mark.parametrize("graph,gather", [("0", "root"), ("1", "all")])
def test_distributed_bench_path_on_one_gpu(built, graph, gather):
    """world_size 1 through the rendezvous file + RCCL: warm-up gather, timed steps, final gather; graph = "1" is the
    configuration that died with a memory fault in round 1 (then on a PyTorch wheel's HIP 7.0 runtime)."""
    env = {"LUPIN_BENCH_FORCE_DIST": "1", "LUPIN_GRAPH": graph, "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": "29533", "RANK": "0",
           "WORLD_SIZE": "1", "LOCAL_RANK": "0"}
    d = run_bench(env, "--steps", "6", "--warmup", "4", "--no-cpu-baseline", "--gather", gather, *SMALL)
    assert d["n_gpus"] == 1 and d["value"] > 0 and d["path_bounces"] > 0 and "tile-sharded" in d["config"]["sharding"]
    ph = d["config"]["rank_phases"]
    assert ph["render_ms_min_max"][0] > 0 and ph["gather_ms_min_max"][1] >= 0 and ph["gather_payload_bytes"] == 256 * 256 * 8


@pytest.mark.gpu
@pytest.mark.parametrize("graph", ["0", "1"])
def test_gather_through_the_c_abi(built, graph):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_gather_worker.py")], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, LUPIN_GRAPH=graph))
    assert p.returncode == 0 and all(tag in p.stdout for tag in ("SCATTER OK", "GATHER OK", "F32 UNPACK OK", "INIT_ALL OK")), p.stdout[-1500:] + p.stderr[-1500:]


def test_gpus_n_without_launcher_spawns_ranks_or_fails(built):
    """`python bench.py --gpus 2` with no launcher must not print a 1-GPU line: it starts two rank processes itself; where
    they cannot run (no second GPU / no GPU at all) the command fails."""
    from lupinpathtracer_amd import api
    if api.device_count() >= 2:
        pytest.skip("two GPUs present: the spawned job would run")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0", "--no-cpu-baseline", *SMALL],
                       capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode != 0
    assert not [l for l in p.stdout.splitlines() if l.startswith("{")]


def test_options_are_listed():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and "--full" in p.stdout and "--dump-outputs" in p.stdout


def test_dump_outputs_sample_and_block_means(tmp_path):
    """The dump of a frame larger than the sample: at most 2^20 pixels, the same ones every time, every pixel in a block mean."""
    from unittest import mock
    import numpy as np
    with mock.patch.dict(os.environ):   # bench.py sets its default GPU_MAX_HW_QUEUES on import: not for this process
        import bench
    frame = np.random.default_rng(3).random((1100, 1000, 4)).astype(np.float16)
    for k in range(2):
        bench.dump_outputs(frame, str(tmp_path / str(k)))
    px, idx, mean = (np.load(tmp_path / "0" / f"frame_{n}.npy") for n in ("pixels", "pixel_index", "block_mean"))
    assert px.dtype == np.float32 and idx.dtype == np.float64 and mean.dtype == np.float64
    assert px.shape == (1 << 20, 4) and np.all(np.diff(idx) > 0)
    assert np.array_equal(px, frame.reshape(-1, 4)[idx.astype(np.int64)].astype(np.float32))
    assert mean.shape == (138, 125, 4) and np.allclose(mean[-1, -1], frame[1096:, 992:].astype(np.float64).mean(axis=(0, 1)))
    assert sum(os.path.getsize(p) for p in (tmp_path / "0").iterdir()) <= 64 << 20
    assert np.array_equal(idx, np.load(tmp_path / "1" / "frame_pixel_index.npy"))


def test_world_size_mismatch_is_an_error(built):
    p = run_bench({"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"}, "--gpus", "1", *SMALL, check=False)
    assert p.returncode != 0 and "WORLD_SIZE" in (p.stderr + p.stdout)
