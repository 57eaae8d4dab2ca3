"""BASELINE config C4 end to end on one GPU: bench.py --workload c4 shards a
length-mixed corpus over 2 ranks (gloo, both on device 0 -- the one-GPU
rehearsal of the N-GPU run; the processes are started by torchrun before any
GPU call), packs each rank's utterances into ragged <= 4096-row batches,
scores them and streams every batch to rank 0.  Rank 0's consumed rows --
its own and the peer's, per utterance -- must be bit-identical to one process
scoring the whole corpus alone: sharding and batching may not change a bit
(per-utterance state only, src/ce_stt.cc:53-60; chunk-invariant AM,
src/am.cc:73-80,115-164)."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

UTTS = 24  # 24 x 2-18 s (4 min of audio): several ragged batches per rank


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _bench(extra, dump, nproc):
    env = dict(os.environ, PYTHONPATH=ROOT, CATEARS_BENCH_DEVICE="0")
    args = ["bench.py", "--workload", "c4", "--c4-utts", str(UTTS), "--model", "tdnn-xs", "--warmup", "2",
            "--no-cpu-baseline", "--c4-dump", str(dump)] + extra  # (later --model / --c4-utts win)
    if nproc > 1:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes", "1", "--nproc-per-node", str(nproc),
               "--master-addr", "127.0.0.1", "--master-port", str(_port())] + args + ["--dist-backend", "gloo",
                                                                                       "--gpus", str(nproc)]
    else:
        cmd = [sys.executable] + args
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(line) == 1, r.stdout[-2000:]
    return json.loads(line[0])


_ONE = {}


def _one_process(model, utts, tmp_dir):
    """bench.py --workload c4 in one process (cached per model): the line and
    the rows rank 0 consumed, per utterance."""
    if model not in _ONE:
        dump = os.path.join(str(tmp_dir), f"one_{model}.npz")
        line = _bench(["--model", model, "--c4-utts", str(utts)], dump, 1)
        _ONE[model] = (line, dict(np.load(dump)))
    return _ONE[model]


def test_c4_two_ranks_bit_identical_to_one_process(tmp_path_factory, tmp_path):
    from catears_amd.shard import c4_corpus, num_frames
    one, _ = _one_process("tdnn-xs", UTTS, tmp_path_factory.mktemp("c4"))
    np.savez(tmp_path / "one.npz", **_ONE["tdnn-xs"][1])
    two = _bench([], tmp_path / "two.npz", 2)
    frames = [num_frames(int(n)) for n in c4_corpus(UTTS)]
    assert one["config"]["frames_total"] == two["config"]["frames_total"] == sum(frames)
    assert two["n_gpus"] == 2 and two["config"]["gather"]
    assert sum(two["config"]["frames_per_rank"]) == sum(frames)
    assert two["config"]["rows_gathered_to_rank0"] == two["config"]["frames_per_rank"][1] > 0
    assert max(two["config"]["batches_per_rank"]) >= 2
    a, b = np.load(tmp_path / "one.npz"), np.load(tmp_path / "two.npz")
    assert sorted(a.files) == sorted(b.files) == sorted(f"u{u}" for u in range(UTTS))
    for k in a.files:
        u = int(k[1:])
        assert a[k].shape == (frames[u], 512)
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
    # the checksums fold every row of every utterance: equal up to fp64 order
    assert two["checksum"] == pytest.approx(one["checksum"], rel=1e-12)


def _bench_c3(extra, nproc):
    env = dict(os.environ, PYTHONPATH=ROOT, CATEARS_BENCH_DEVICE="0")
    args = ["bench.py", "--model", "tdnn-xs", "--steps", "6", "--warmup", "2", "--pool", "8",
            "--no-cpu-baseline"] + extra
    if nproc > 1:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes", "1", "--nproc-per-node", str(nproc),
               "--master-addr", "127.0.0.1", "--master-port", str(_port())] + args + ["--gpus", str(nproc),
                                                                                     "--dist-backend", "gloo"]
    else:
        cmd = [sys.executable] + args
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(line) == 1, r.stdout[-2000:]
    return json.loads(line[0])


def test_c3_two_ranks_gather_every_row(tmp_path):
    """The driver's N > 1 C3 command (bench.py main: three nnet streams,
    per-batch events, the comm stream, RowGather's receive ring and
    wait_slot), rehearsed with 2 gloo ranks on device 0.  Within the run:
    every batch rank 1 sends (its rows as scored, copied on the stream that
    hands them to the gather) arrives at rank 0 bit for bit, and rank 0's
    checksum folds exactly its own batches and the received ones, warm-up
    included -- no batch lost, duplicated or read before it was written."""
    steps = 6 + 2
    two = _bench_c3(["--c3-dump", str(tmp_path / "d.npz"), "--verify-serial"], 2)
    assert two["n_gpus"] == 2 and two["config"]["gather"] and two["finite"]
    # end to end: every batch each rank scored in the pipelined run (three
    # nnet streams + the front stream + the comm stream) equals the same
    # batch re-scored serially on one stream in the same process -- fbank,
    # CMVN and every log-likelihood row
    for r, v in enumerate(two["verify_ranks"]):
        assert v["batches"] == steps and v["differing"] == 0, (r, v)
    r0, r1 = np.load(tmp_path / "d.rank0.npz"), np.load(tmp_path / "d.rank1.npz")
    assert sorted(r1.files) == sorted(f"r1s{s}" for s in range(steps))
    want = 0.0
    for s in range(steps):
        sent, got, own = r1[f"r1s{s}"], r0[f"r1s{s}"], r0[f"r0s{s}"]
        assert sent.shape == got.shape == own.shape
        assert np.array_equal(sent.view(np.uint32), got.view(np.uint32)), s
        want += float(own.astype(np.float64).sum()) + float(got.astype(np.float64).sum())
    assert two["checksum"] == pytest.approx(want, rel=1e-12)
    # the two ranks score different audio: a gather that dropped the peer's
    # rows (or sent rank 0's twice) would miss by a whole rank's sum
    assert not np.array_equal(r0["r0s0"], r0["r1s0"])


@pytest.mark.parametrize("model,utts", [("tdnn-xs", UTTS), ("tdnn-s", 8)])
def test_c4_rows_match_oracle(tmp_path_factory, model, utts):
    """C4's gathered rows against the oracle: for the shortest and the
    longest utterance of the length-mixed corpus, and for the utterances on
    either side of a batch boundary (the last of one <= 4096-row batch, the
    first of the next), rank 0's consumed rows are within the north star's
    1e-4 of oracle.am_whole(oracle.cmvn(oracle fbank)) with an fp64 network
    (src/am.cc:115-164 per utterance, src/ce_stt.cc:53-60: an utterance's
    rows depend on nothing but its own samples)."""
    import tempfile

    from catears_amd import formats, synth
    from catears_amd.shard import c4_corpus, num_frames, pack_batches, shard_utterances
    from oracle import pyoracle
    line, rows = _one_process(model, utts, tmp_path_factory.mktemp("c4"))
    conf = synth.write_model(os.path.join(tempfile.gettempdir(), f"catears_bench_{os.getuid()}"), model)
    am = formats.read_am(conf)
    samples = c4_corpus(utts)
    frames = [num_frames(int(n)) for n in samples]
    mine = shard_utterances(frames, 1, 0)
    batches = [[mine[i] for i in b] for b in pack_batches([frames[u] for u in mine], am["left"], am["right"], 4096)]
    assert len(batches) >= 2 and line["config"]["batches_per_rank"] == [len(batches)]
    pick = {int(np.argmin(samples)), int(np.argmax(samples)), int(batches[0][-1]), int(batches[1][0])}
    plen = int(samples.max())
    gstats = synth.cmvn_stats_synthetic()
    fb = pyoracle.Fbank()
    f64 = lambda a, w: (a.astype(np.float64) @ w.astype(np.float64)).astype(np.float32)
    for u in sorted(pick):
        wave = synth.pcm(600000 + u % 48, plen)[:int(samples[u])]  # bench.py main_c4's resident pool
        ref = pyoracle.am_whole(am, pyoracle.cmvn(gstats, fb.compute(wave)), gemm=f64)
        got = rows[f"u{u}"]
        assert got.shape == ref.shape == (frames[u], am["log_prior"].shape[0])
        err = float(np.abs(got - ref).max())
        assert err <= 1e-4, (u, err)


def test_c4_full_corpus_sampled_rows_match_oracle(tmp_path):
    """The whole C4 corpus (36 000 utterances, 100 h, TDNN-S, ~9 000 ragged
    <= 4096-row batches) in one process, one utterance in 3 000 kept: every
    kept utterance has its frame count, and four of them -- the shortest,
    the longest, and the first and last kept -- are within 1e-4 of the
    oracle (fp64 network).  Exercises the full-size batching the small
    corpora above do not reach."""
    import tempfile

    from catears_amd import formats, synth
    from catears_amd.shard import c4_corpus, num_frames, pack_batches, shard_utterances
    from oracle import pyoracle
    every = 3000
    dump = tmp_path / "full.npz"
    env = dict(os.environ, PYTHONPATH=ROOT, CATEARS_BENCH_DEVICE="0")
    r = subprocess.run([sys.executable, "bench.py", "--workload", "c4", "--model", "tdnn-s", "--warmup", "2",
                        "--no-cpu-baseline", "--c4-dump", str(dump), "--c4-dump-every", str(every)],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    conf = synth.write_model(os.path.join(tempfile.gettempdir(), f"catears_bench_{os.getuid()}"), "tdnn-s")
    am = formats.read_am(conf)
    samples = c4_corpus(36000)
    frames = [num_frames(int(n)) for n in samples]
    batches = pack_batches([frames[u] for u in shard_utterances(frames, 1, 0)], am["left"], am["right"], 4096)
    assert line["config"]["batches_per_rank"] == [len(batches)] and len(batches) > 8000
    rows = dict(np.load(dump))
    kept = sorted(int(k[1:]) for k in rows)
    assert kept == list(range(0, 36000, every))
    for u in kept:
        assert rows[f"u{u}"].shape == (frames[u], am["log_prior"].shape[0]), u
    by_len = sorted(kept, key=lambda u: samples[u])
    pick = {by_len[0], by_len[-1], kept[0], kept[-1]}
    plen = int(samples.max())
    gstats = synth.cmvn_stats_synthetic()
    fb = pyoracle.Fbank()
    f64 = lambda a, w: (a.astype(np.float64) @ w.astype(np.float64)).astype(np.float32)
    for u in sorted(pick):
        wave = synth.pcm(600000 + u % 48, plen)[:int(samples[u])]  # bench.py main_c4's resident pool
        ref = pyoracle.am_whole(am, pyoracle.cmvn(gstats, fb.compute(wave)), gemm=f64)
        err = float(np.abs(rows[f"u{u}"] - ref).max())
        assert err <= 1e-4, (u, err)


def test_c3_gpus_2_self_launched():
    """`bench.py --gpus 2` with no external launcher: the bench starts its two
    ranks itself (gloo, both on device 0 here) and the line is a 2-rank line
    with the gather to rank 0."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(PYTHONPATH=ROOT, CATEARS_BENCH_DEVICE="0")
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--dist-backend", "gloo", "--steps", "6",
                        "--warmup", "2", "--no-cpu-baseline", "--prewarm-ms", "0"],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(line) == 1, r.stdout[-2000:]
    line = line[0]
    assert line["n_gpus"] == 2 and line["config"]["gather"] and line["finite"]
    assert line["value"] > 0


def test_c3_sink_share_rank0_scores_part_of_the_steps(tmp_path):
    """--sink-share 0.5: rank 0 (the gather sink) scores a batch on every
    other step and on the rest only receives; the line counts exactly the
    batches scored, every batch rank 1 sends still arrives bit for bit, and
    the checksum folds rank 0's own scored batches and every received one."""
    steps = 6 + 2
    two = _bench_c3(["--c3-dump", str(tmp_path / "d.npz"), "--sink-share", "0.5"], 2)
    cfg = two["config"]
    assert cfg["sink_share"] == 0.5 and cfg["rank0_scored_steps"] == 3  # timed steps 2..7: 3, 5, 7
    assert cfg["frames_total"] == cfg["frames_per_step_per_gpu"] * (6 + 3)
    r0, r1 = np.load(tmp_path / "d.rank0.npz"), np.load(tmp_path / "d.rank1.npz")
    scored = [s for s in range(steps) if int((s + 1) * 0.5) > int(s * 0.5)]
    assert sorted(f for f in r0.files if f.startswith("r0s")) == sorted(f"r0s{s}" for s in scored)
    want = 0.0
    for s in range(steps):
        sent, got = r1[f"r1s{s}"], r0[f"r1s{s}"]
        assert np.array_equal(sent.view(np.uint32), got.view(np.uint32)), s
        want += float(got.astype(np.float64).sum())
        if s in scored:
            want += float(r0[f"r0s{s}"].astype(np.float64).sum())
    assert two["checksum"] == pytest.approx(want, rel=1e-12)


def test_c3_sink_share_serial_scores_the_right_steps(tmp_path):
    """--serial with --sink-share 0.5 (two front slots; rank 0's scored steps
    two apart): the next scored step's fbank + CMVN is staged before the
    current one's nnet runs, so the front slots must go by the scored
    ordinal, not the step -- every batch rank 0 scored matches a
    serial re-score of the same step's utterances bit for bit."""
    two = _bench_c3(["--serial", "--sink-share", "0.5", "--verify-serial"], 2)
    assert two["config"]["rank0_scored_steps"] == 3
    ver = two["verify_ranks"] if "verify_ranks" in two else [two["verify"]]
    assert ver[0]["batches"] > 0 and all(v["differing"] == 0 for v in ver), ver


def test_rehearse_peers_runs_and_reports():
    """bench.py --rehearse-peers (the one-GPU rehearsal of rank 0's receive +
    fold load behind the default sink share): it runs the
    pipeline with the extra copies and folds and says so in the line."""
    line = _bench_c3(["--rehearse-peers", "2"], 1)
    assert line["rehearse_peers"]["peers"] == 2 and line["finite"]
    assert line["config"]["frames_total"] == line["config"]["frames_per_step_per_gpu"] * 6


def test_dump_outputs_writes_the_last_timed_step(tmp_path):
    """bench.py --dump-outputs DIR: DIR/loglik.npy holds the rows of the last
    timed step (step warmup + steps - 1 = 7 here), as float32, bit for bit
    what --c3-dump kept of that step; a run without --full carries no CPU
    baseline, and --steps is the number of timed steps."""
    d = tmp_path / "out"
    line = _bench_c3(["--fold-all", "--c3-dump", str(tmp_path / "all.npz"), "--dump-outputs", str(d)], 1)
    assert line["steps"] == 6 and line["ms_per_step"] > 0 and line["cpu_baseline"] is None
    assert sorted(os.listdir(d)) == ["loglik.npy"]
    got, every = np.load(d / "loglik.npy"), np.load(tmp_path / "all.npz")
    assert got.dtype == np.float32 and got.shape == (line["config"]["frames_per_step_per_gpu"], 512)
    assert got.nbytes <= 64e6
    assert np.array_equal(got.view(np.uint32), every["r0s7"].view(np.uint32))
    assert not np.array_equal(got, every["r0s6"])  # (each step scores other utterances)
