"""bench.py's rank handling, checked without a GPU: `--gpus N` with no launcher must START N child ranks (each of which
then reports that no GPU is visible here), and a launcher whose WORLD_SIZE disagrees with --gpus must be refused."""
import json
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _env(**extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env.update(extra)
    return env


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only check of the spawn path")
def test_gpus_flag_spawns_child_ranks():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                       env=_env(), capture_output=True, text=True, timeout=600)
    errs = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]
    assert p.returncode != 0
    # (the launcher stops the other rank as soon as one has failed, so one or two rank records arrive) ...
    ranks = [e for e in errs if "rank" in e]
    assert 1 <= len(ranks) <= 2 and all("no GPU visible" in e["error"] and e["world"] == 2 for e in ranks), p.stdout + p.stderr[-1500:]
    # ... followed by the parent's own record: exit status and the tail of the children's stderr (round 4: a multi-GPU run that dies
    # must be diagnosable from the one line a driver keeps)
    last = errs[-1]
    assert "rank" not in last and last["n_gpus"] == 2 and "child ranks exited with status" in last["error"]
    assert "exitcode" in last["stderr_tail"] and len(last["stderr_tail"]) <= 1500
    assert last["stderr_tail"][-200:] in p.stderr          # relayed as well as recorded


def test_world_size_mismatch_is_refused():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4"], env=_env(WORLD_SIZE="2", RANK="0"),
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 2
    assert "--gpus 4 but WORLD_SIZE=2" in p.stdout


def test_steps_below_one_is_refused():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], env=_env(), capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 2 and "--steps must be at least 1" in p.stderr


def test_dump_sample_is_a_fixed_bounded_row_sample():
    import bench
    y = torch.randn(4096, 4096).to(torch.bfloat16)
    a, b = bench.dump_sample(y), bench.dump_sample(y.clone())
    assert a.dtype.name == "float32" and a.size <= bench.DUMP_MAX_ELEMS and a.shape[1] == 4096
    assert (a == b).all()
    # whole rows of the output, in ascending row order
    rows = [int(torch.nonzero((y.float() == torch.from_numpy(r)).all(1))[0]) for r in a[:: len(a) // 8]]
    assert rows == sorted(rows)
    small = [torch.randn(1, 64) for _ in range(3)]
    assert (bench.dump_sample(small) == torch.stack(small).numpy()).all()


@pytest.mark.gpu
def test_dump_outputs_hold_the_last_timed_step(tmp_path):
    """--dump-outputs writes what the timed matmul_4bit returned, as the same call on the same seeded inputs computes it here."""
    import numpy as np
    import bench
    import mps_bitsandbytes_amd as bnb
    from mps_bitsandbytes_amd import synthetic
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--reps", "1",
                        "--prewarm-ms", "0", "--no-cpu-baseline", "--no-gemv", "--no-empirical", "--no-secondary",
                        "--dump-outputs", str(tmp_path)], env=_env(), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    rec = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert rec["steps"] == 2 and rec["ms_per_step"] > 0 and rec["dumped_outputs"] == {"nf4_m4096": [768, 4096]}
    got = np.load(tmp_path / "nf4_m4096.npy")
    dev = torch.device("cuda")
    W = synthetic.normal_device((4096, 4096), torch.bfloat16, seed=1234, std=1.0, device=dev)
    packed, state = bnb.quantize_nf4(W, blocksize=64)
    X = synthetic.normal_device((4096, 4096), torch.bfloat16, seed=4321, std=1.0, device=dev)
    want = bench.dump_sample(bnb.matmul_4bit(X, packed, state))
    assert got.dtype == np.float32 and np.array_equal(got, want)


def test_full_flag_is_accepted():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--full"], env=_env(WORLD_SIZE="2", RANK="0"),
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 2 and "--gpus 4 but WORLD_SIZE=2" in p.stdout, p.stderr[-1500:]


@pytest.mark.gpu
def test_plain_run_times_the_headline_alone_and_dumps_what_full_dumps(tmp_path):
    """A plain run measures only the headline; --full adds the rest.  Both write the same four arrays, bit for bit (the plain run
    computes the secondary workloads' outputs with one untimed step each)."""
    import numpy as np
    common = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--reps", "1", "--prewarm-ms", "0"]
    recs = {}
    for form, extra in (("plain", []), ("full", ["--full", "--no-cpu-baseline", "--no-gemv", "--no-empirical"])):
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + common + extra + ["--dump-outputs", str(tmp_path / form)],
                           env=_env(), capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        recs[form] = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    plain, full = recs["plain"], recs["full"]
    for key in ("metric", "unit", "higher_is_better", "dtype", "steps", "warmup"):
        assert plain[key] == full[key], key
    assert plain["value"] > 0 and plain["ms_per_step"] > 0 and plain["roofline"]["kernel_us"] > 0
    assert not {"secondary", "no_prewarm", "cpu_baseline", "gemv", "batch_sweep"} & set(plain)
    assert "dominant_kernel" not in plain["roofline"] and "empirical" not in plain["roofline"]
    assert [o["workload_key"] for o in full["secondary"]] == ["nf4dq_ffn", "int8_4096", "nf4_m1"]
    assert not [o["error"] for o in full["secondary"] if "error" in o]
    assert "no_prewarm" in full and "dominant_kernel" in full["roofline"]
    names = ["nf4_m4096", "nf4dq_ffn", "int8_4096", "nf4_m1"]
    assert list(plain["dumped_outputs"]) == names and plain["dumped_outputs"] == full["dumped_outputs"]
    for n in names:
        a, b = np.load(tmp_path / "plain" / (n + ".npy")), np.load(tmp_path / "full" / (n + ".npy"))
        assert a.dtype == np.float32 and np.array_equal(a, b), n
