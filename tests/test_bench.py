"""bench.py's bookkeeping (no GPU): the algorithmic FLOP and byte counts its
roofline uses, and that the kernel names it quotes traffic for exist in the
newest committed PMC summaries (a renamed kernel would silently drop
roofline.traffic to null)."""
import importlib
import sys

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def bench():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    return importlib.import_module("bench")


def test_flops_per_frame_matches_survey(bench):
    # 2 * (200*1024 + 4*3072*1024 + 1024*1024 + 1024*3456)
    assert bench.FLOPS_PER_FRAME == 34_750_464


def test_split_algorithmic_bytes(bench):
    rows = 4072
    layers = ((256, 1024),) + ((3072, 1024),) * 4 + ((1024, 1024), (1024, 3456))
    want = sum(4 * rows * k + 4 * k * n + 4 * rows * n for k, n in layers) / len(layers)
    assert bench.split_algorithmic_bytes(rows, 4) == pytest.approx(want)
    # planes: 6-byte operands and hidden outputs, fp32 last layer
    want6 = sum(6 * rows * k + 6 * k * n + (4 if i == 6 else 6) * rows * n
                for i, (k, n) in enumerate(layers)) / len(layers)
    assert bench.split_algorithmic_bytes(rows, 6) == pytest.approx(want6)


@pytest.mark.parametrize("workload,kernel", [
    ("c3", "SPLIT_BF16X6"),
    ("c5", "I8"),
])
def test_roofline_kernels_have_committed_traffic(bench, workload, kernel):
    name = bench.SPLIT_ROOFLINE_KERNEL["bf16x6"] if kernel == "SPLIT_BF16X6" else bench.I8_ROOFLINE_KERNEL
    traffic, src = bench.pmc_traffic(name, workload)
    assert src is not None, f"no committed PMC summary for {workload}"
    assert traffic is not None and traffic > 0, f"{name} not in {src}"


@pytest.mark.parametrize("workload,kernel", [
    ("c3", "SPLIT_BF16X6"),
    ("c5", "I8"),
])
def test_roofline_kernels_have_committed_mfma_util(bench, workload, kernel):
    """The rocprof MFMA-utilisation figure (north star) exists for the
    dominant GEMM of C3 and C5 and is a fraction."""
    name = bench.SPLIT_ROOFLINE_KERNEL["bf16x6"] if kernel == "SPLIT_BF16X6" else bench.I8_ROOFLINE_KERNEL
    u = bench.pmc_mfma(name, workload)
    assert u is not None, f"no committed MFMA-utilisation summary for {name} ({workload})"
    assert 0.0 < u["chip"] <= u["active_cus"] <= 1.0


@pytest.mark.parametrize("kernel", ["fbank_kernel<float*", "fbank_fma_kernel<float*"])
def test_c2_valu_counters_are_committed(bench, kernel):
    """C2's measured VALU occupancy (roofline.valu_counters) reads the
    committed PMC counter summary (tools/pmc_valu.py) of both fbank kernels;
    a renamed kernel or a missing summary would silently drop it."""
    v = bench.pmc_valu(kernel)
    assert v is not None, f"no committed c2 PMC VALU summary with {kernel}"
    # a few hundred wave instructions per frame for either lane program
    assert 100 < v["valu_insts_per_dispatch"] / 998000 < 400
    assert 0 < v["valu_active_per_simd"] < 4 and 0 < v["wave_active"] < 1


def _clean_env(**extra):
    import os
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT",
                        "GROUP_RANK", "TORCHELASTIC_RUN_ID")}
    env.update(PYTHONPATH=ROOT, **extra)
    return env


def _lines(out):
    import json
    return [json.loads(ln) for ln in out.splitlines() if ln.startswith("{")]


def test_bench_gpus_n_self_launches_n_ranks():
    """`bench.py --gpus 2` with no launcher starts the two ranks itself, as a
    child torch.distributed.run (the parent never touches the GPU), and the
    line reports n_gpus 2 from two distinct rank processes (VERDICT r4 item
    2).  --launch-check stops after the gloo process group: no GPU here."""
    import subprocess
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--dist-backend", "gloo", "--launch-check"],
                       cwd=ROOT, env=_clean_env(CATEARS_BENCH_DEVICE="0"), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = _lines(r.stdout)
    assert len(lines) == 1, r.stdout
    line = lines[0]
    assert line["n_gpus"] == 2 and line["launch_check"]
    assert sorted(x["rank"] for x in line["ranks"]) == [0, 1]
    assert sorted(x["local_rank"] for x in line["ranks"]) == [0, 1]
    assert len({x["pid"] for x in line["ranks"]}) == 2


def test_bench_one_gpu_runs_in_process():
    import subprocess
    r = subprocess.run([sys.executable, "bench.py", "--launch-check"], cwd=ROOT, env=_clean_env(),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    (line,) = _lines(r.stdout)
    assert line["n_gpus"] == 1 and len(line["ranks"]) == 1


def test_bench_world_size_mismatch_fails():
    """Under an external launcher whose world differs from --gpus the bench
    exits non-zero instead of printing a mislabelled line."""
    import subprocess
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--launch-check"], cwd=ROOT,
                       env=_clean_env(WORLD_SIZE="1", RANK="0", LOCAL_RANK="0"), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode != 0
    assert "WORLD_SIZE 1" in r.stderr
    assert not _lines(r.stdout)


def test_sink_share_default_balances_rank0_with_senders(bench):
    """rank 0's rehearsed step (0.61 + 0.034 (N - 1) ms at a
    full share, 0.71 ms per unit of share) is brought to a sender's 0.65-0.66
    ms (profiles/r05z3_sender_rehearsal.txt); never below half a share."""
    assert bench.sink_share_default(1) == 1.0
    assert bench.sink_share_default(2) == 1.0
    assert abs(bench.sink_share_default(8) - 0.681) < 1e-9
    for n in range(2, 9):
        f = bench.sink_share_default(n)
        assert 0.5 <= f <= 1.0
        rank0 = 0.61 + 0.034 * (n - 1) - 0.71 * (1.0 - f)
        assert rank0 <= 0.67
    assert bench.sink_share_default(64) == 0.5


def test_full_is_off_by_default(bench):
    """A plain run does only what the headline figure needs: the CPU baseline
    and the int8-against-fp32 leg wait for --full."""
    assert bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"]).full is False
    a = bench.parse(["--full", "--dump-outputs", "d"])
    assert a.full is True and a.dump_outputs == "d" and a.steps == 200


def test_dump_outputs_sample_is_fixed_and_bounded(bench, tmp_path):
    """--dump-outputs: a small array is written whole; one above the bound as
    a sample of rows that depends on the row count alone (same rows from run
    to run and from build to build), in row order, as float32."""
    import numpy as np
    import torch
    small = torch.arange(12, dtype=torch.float32).reshape(4, 3)
    bench.dump_outputs(str(tmp_path / "a"), "x", small)
    assert np.array_equal(np.load(tmp_path / "a" / "x.npy"), small.numpy())
    cols = 3456
    n = bench.DUMP_MAX_BYTES // (4 * cols) + 1000
    big = (torch.arange(n, dtype=torch.float32)[:, None] + torch.zeros(cols)).contiguous()
    bench.dump_outputs(str(tmp_path / "a"), "y", big)
    bench.dump_outputs(str(tmp_path / "b"), "y", big.clone(), rank=1)
    y = np.load(tmp_path / "a" / "y.npy")
    assert y.dtype == np.float32 and y.nbytes <= bench.DUMP_MAX_BYTES < 64e6
    assert y.shape == (bench.DUMP_MAX_BYTES // (4 * cols), cols)
    assert np.all(np.diff(y[:, 0]) > 0) and np.all(y[:, 0] == y[:, -1])
    assert np.array_equal(y, np.load(tmp_path / "b" / "y.rank1.npy"))
