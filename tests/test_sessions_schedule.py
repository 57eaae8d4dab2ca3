"""Sessions.schedule (catears_amd/gpu.py): the frames and rows each push of a
slot produces, by arithmetic alone -- what Sessions.push sizes its output
with and what ce_gpu_sessions_push reports in h_rows_out
(tests/test_gpu_sessions.py compares the two on the device).  Checked here
against a brute-force restatement, without a GPU."""
import numpy as np
import pytest

L = R = 10


def brute(oracle, right, counts, eos_at):
    samples = frames = rows = 0
    out_f, out_r = [], []
    for i, c in enumerate(counts):
        samples += c
        f = oracle.Fbank.num_frames(samples)
        total = f if i == eos_at else max(0, f - right)
        out_f.append(f - frames)
        out_r.append(total - rows)
        frames, rows = f, total
    return out_f, out_r


def constant(total, chunk):
    return [min(chunk, total - at) for at in range(0, total, chunk)]


def sequences():
    seqs = [constant(48000, c) for c in (159, 160, 161, 399, 400, 401, 777, 1600, 48000)]
    seqs.append([1] * 1000)
    rng = np.random.default_rng(902)
    counts, left = [], 48000
    while left:
        c = min(left, int(rng.choice([0, 0, 1, 37, 160, 399, 400, 1599, 3000])))
        counts.append(c)
        left -= c
    seqs.append(counts)
    cuts = sorted(set(range(0, 240001, 1600)) | {400 + 160 * (f - 1) for f in (598, 599, 600, 601)})
    seqs.append([b - a for a, b in zip(cuts, cuts[1:])])
    seqs.append([160000, 80000])
    seqs += [[399], [400], [400] + [160] * 9, [400] + [160] * 9 + [0], [777, 1063]]
    seqs += [constant(n, c) for n, c in zip([8000, 16000, 32000, 52800, 112000], [160, 777, 1600, 4000, 333])]
    return seqs


@pytest.mark.parametrize("right", [0, 3, R])
def test_schedule_matches_brute_force(oracle, right):
    from catears_amd.gpu import Sessions
    for counts in sequences():
        for eos_at in (len(counts) - 1, None):
            got = Sessions.schedule(L, right, counts, eos_at)
            assert got == brute(oracle, right, counts, eos_at), (counts[:8], eos_at)
            assert sum(got[0]) == oracle.Fbank.num_frames(sum(counts))
            if eos_at is not None:
                assert sum(got[1]) == sum(got[0])
            assert min(got[1]) >= 0


def test_schedule_refuses_a_push_after_the_end():
    from catears_amd.gpu import Sessions
    with pytest.raises(ValueError):
        Sessions.schedule(L, R, [400, 160, 160], 1)


def test_session_symbols_in_abi():
    from catears_amd import gpu
    for name in ("ce_gpu_sessions_create", "ce_gpu_sessions_destroy", "ce_gpu_sessions_reset",
                 "ce_gpu_sessions_push", "ce_gpu_sessions_push_s16", "ce_gpu_debug_counters"):
        assert name in gpu.ABI
        assert hasattr(gpu.lib(), name)
    a, f = gpu.debug_counters()
    assert a >= 0 and f >= 0
