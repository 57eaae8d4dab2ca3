"""ce_gpu_plan_create's geometry restated in numpy, for the reusable-plan tests
(tests/test_plan_reusable_cpu.py, tests/test_gpu_plan_reusable.py): the frame
rule, the packing of utterances into chunks of at most max_rows rows, and the
six device tables word for word (catears_amd/csrc/capi.cc, ce_gpu_plan_create).
A third statement of the rule beside the host loops of ce_gpu_plan_create and
the expansion kernel of ce_gpu_plan_assign: the two are compared with each
other and with this one.

The two constants a test must not copy are read back from the sources:
frames_per_block() (the granularity of block_utt) and ring_depth() (the
pinned descriptor buffers of a reusable plan)."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "catears_amd", "csrc")
FRAME_LENGTH, FRAME_SHIFT = 400, 160


def _constant(path, name):
    m = re.search(r"constexpr\s+int\s+" + name + r"\s*=\s*(\d+)\s*;", open(path).read())
    assert m, f"{name} not found in {path}"
    return int(m.group(1))


def frames_per_block():
    return _constant(os.path.join(CSRC, "kernels", "fbank.hip"), "kFramesPerBlock")


def ring_depth():
    return _constant(os.path.join(CSRC, "internal.h"), "kPlanRing")


def frames(n):
    return 0 if n < FRAME_LENGTH else 1 + (n - FRAME_LENGTH) // FRAME_SHIFT


def samples(t, extra=0):
    """A sample count that gives t frames (extra < 160 more samples, or for
    t = 0 any count below 400)."""
    return extra if t == 0 else FRAME_LENGTH + FRAME_SHIFT * (t - 1) + extra


def pack(lengths, left, right, max_rows):
    """(segments, chunks): segments (utt, t, n, base) in packed order, chunks
    (rows, map_base)."""
    segs, chunks = [], []
    rows, base, at = 0, 0, 0
    for u, ns in enumerate(lengths):
        T, t = frames(int(ns)), 0
        while t < T:
            room = max_rows - rows - left - right
            if room < T - t and rows > 0:
                chunks.append((rows, base))
                rows, base = 0, at
                room = max_rows - left - right
            n = min(T - t, room)
            segs.append((u, t, n, at))
            at += n + left + right
            rows += n + left + right
            t += n
    if rows > 0:
        chunks.append((rows, base))
    return segs, chunks


def tables(lengths, left=None, right=None, max_rows=4096):
    """The six tables (names of gpu.PLAN_TABLES) and the plan_info tuple
    (n_utt, total_samples, total_frames, n_chunks, max_chunk_rows) of a plan;
    left is None: a plan without a model."""
    lengths = [int(n) for n in lengths]
    soff = np.concatenate([[0], np.cumsum(lengths, dtype=np.int64)]).astype(np.int64)
    foff = np.concatenate([[0], np.cumsum([frames(n) for n in lengths], dtype=np.int64)]).astype(np.int64)
    total = int(foff[-1])
    fpb = frames_per_block()
    blocks = (total + fpb - 1) // fpb
    # the first utterance whose frames end behind frame b * fpb
    butt = np.searchsorted(foff[1:], np.arange(blocks, dtype=np.int64) * fpb, side="right").astype(np.int32)
    if blocks == 0:
        butt = np.zeros(1, np.int32)
    src, dst, edge, chunks = [], [], [], []
    if left is not None:
        segs, chunks = pack(lengths, left, right, max_rows)
        for u, t, n, _ in segs:
            T = int(foff[u + 1] - foff[u])
            j = np.arange(n + left + right, dtype=np.int64)
            src.append(foff[u] + np.clip(t - left + j, 0, T - 1))
            dst.append(np.where((j >= left) & (j < left + n), foff[u] + t + j - left, -1))
            edge.append(np.minimum(j, 0xffff) | (np.minimum(n + left + right - 1 - j, 0xffff) << 16))
    cat = lambda parts, dt: (np.concatenate(parts) if parts else np.zeros(0, np.int64)).astype(dt)
    tab = {"sample_off": soff, "frame_off": foff, "block_utt": butt, "row_src": cat(src, np.int32),
           "row_dst": cat(dst, np.int32), "row_edge": cat(edge, np.uint32)}
    info = (len(lengths), int(soff[-1]), total, len(chunks), max([c[0] for c in chunks], default=0))
    return tab, info
