"""The front end's seam cases, shared by tests/test_oracle_vs_reference.py (the
oracle against the reference's own code, CPU) and
tests/test_gpu_frontend_seams.py (the kernels against the oracle).

Online CMVN (src/cmvn.cc) has three regimes per frame t (count = t + 1 while
the window fills): up to count 400 the global stats enter with the capped
weight 200, from there with 600 - count, at t = 599 not at all, and from
t = 600 on frame t - 600 leaves the sum.  cmvn_kernel walks them in tiles of
48 frames, so the frame counts sit on both sides of every regime change and
of the tile boundaries next to them.

chain_f32 restates the chain in numpy with the two constants as parameters:
with the defaults it must give the oracle's bits, and with a constant off by
one it must not -- on exactly the rows that constant governs.  That is the
evidence that these frame counts would catch such a mistake in a kernel.
"""
import numpy as np

SEAM_T = (1, 2, 47, 48, 49, 95, 96, 97, 399, 400, 401, 576, 598, 599, 600, 601, 647, 648, 649, 695, 696, 697,
          1199, 1200, 1201, 1561)
T_MAX = max(SEAM_T)
CPU_COUNTS = (36162480.0, 1e6, 599.0, 200.0, 100.0, 3.0, 1.0, 0.5)
GPU_COUNTS = (36162480.0, 200.0, 100.0, 1.0)
WINDOW, GLOBAL_FRAMES = 600, 200


def rescaled_stats(global_stats, count):
    """The fixture's stats with its means kept and the frame count `count`:
    alpha = min(600 - n, 200) / count is 1.0f at 200 (while n <= 400) and
    above 1 below that."""
    g = np.asarray(global_stats, np.float64)
    mean = g[:40] / g[40]
    return np.concatenate([mean * count, [count]]).astype(np.float32)


def rows(seed=5, scale=1.0):
    """T_MAX feature rows ~ N(12, 4) (log-mel sized); every case of T frames
    reads the first T.  scale 1e4: sums beyond 2^24 ulps of a row, so the
    float carry rounds at every step.  Read-only."""
    x = (np.random.default_rng(seed).normal(12.0, 4.0, size=(T_MAX, 40)) * scale).astype(np.float32)
    x.setflags(write=False)
    return x


def chain_f32(global_stats, feats, window=WINDOW, cap=GLOBAL_FRAMES, leave_shift=0):
    """CMVN::GetFrame for frames 0 .. T-1 in numpy: double temporaries, float
    carry, one float rounding per float operation.  window: the count at
    which a frame starts to leave; cap: the most the global stats weigh;
    leave_shift: the leaving frame is t - WINDOW + leave_shift."""
    g = np.asarray(global_stats, np.float32)
    x = np.asarray(feats, np.float32)
    out = np.zeros_like(x)
    carry = np.zeros(41, np.float32)
    for t in range(len(x)):
        acc = carry.astype(np.float64)
        acc[:40] += x[t].astype(np.float64)
        acc[40] += 1.0
        if t - window >= 0:
            acc[:40] += -1.0 * x[t - window + leave_shift].astype(np.float64)
            acc[40] -= 1.0
        st = acc.astype(np.float32)
        carry = st.copy()
        cnt = float(st[40])
        if cnt < WINDOW:
            alpha = np.float32(min(WINDOW - cnt, float(cap)) / float(g[40]))
            st = st + alpha * g                       # float product, float sum
        neg = -np.float32(1.0 / float(st[40]))
        out[t] = x[t] + neg * st[:40]
    return out
