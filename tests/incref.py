"""The incremental session scheme (CE_GPU_SESSIONS_INCREMENTAL,
catears_amd/csrc/sessions.cc) restated on the CPU over oracle.layer_forward,
so that the scheme itself -- positions, blocks of H lead rows, causal splice
offsets, per-layer caches -- is held to the one-shot evaluation
(oracle.am_whole) without a device.

A model is the dict of formats.read_am / oracle.am_whole: layers, left,
right, log_prior.  Caches start filled with NaN: a valid row that ever read
a row it must not would show it."""
import numpy as np


def stages(layers):
    """The net as [(splice indices, [the Linear and the row ops behind it])]:
    one stage per Linear, the Splice in front of it ([0] without one), the
    Narrow dropped (the causal form needs none)."""
    out, idx = [], [0]
    for layer in layers:
        kind = layer["kind"]
        if kind == "splice":
            idx = list(layer["indices"])
        elif kind == "narrow":
            continue
        elif kind == "linear":
            out.append((idx, [layer]))
            idx = [0]
        else:
            out[-1][1].append(layer)
    return out


def spans(layers):
    """c_i = max(idx_i) - min(idx_i) per Linear."""
    return [max(idx) - min(idx) for idx, _ in stages(layers)]


def lead_rows(layers):
    return max(spans(layers))


class Stream:
    """One slot.  push(new frames, eos) returns the rows the push completes
    (prior subtracted) and adds the packed rows it used to self.packed."""

    def __init__(self, oracle, model, max_rows=4096):
        self.oracle, self.model, self.max_rows = oracle, model, max_rows
        self.L, self.R = model["left"], model["right"]
        self.stages = stages(model["layers"])
        self.c = [max(idx) - min(idx) for idx, _ in self.stages]
        self.H = max(self.c)
        assert sum(-min(idx) for idx, _ in self.stages) == self.L
        assert sum(max(idx) for idx, _ in self.stages) == self.R
        idx0, ops0 = self.stages[0]
        self.frames = np.zeros((0, ops0[0]["W"].shape[0] // len(idx0)), np.float32)
        self.P = 0          # padded frames (positions) fed so far
        self.ended = False
        self.caches = None  # per stage: c_i rows of that stage's input
        self.packed = 0

    def _block(self, p0, k):
        """Positions p0 .. p0 + k - 1 behind H lead rows: (rows of position
        >= L + R, in order)."""
        H, L, R = self.H, self.L, self.R
        last = len(self.frames) - 1
        fr = np.clip(np.arange(p0 - H, p0 + k) - L, 0, last)
        x = self.frames[fr]
        fresh = p0 == 0
        for i, (idx, ops) in enumerate(self.stages):
            c = self.c[i]
            if i > 0 and c > 0:
                if self.caches[i] is None:
                    self.caches[i] = np.full((c, x.shape[1]), np.nan, np.float32)
                x = x.copy()
                x[H - c:H] = 0.0 if fresh else self.caches[i]
                self.caches[i] = x[H + k - c:H + k].copy()
            causal = {"kind": "splice", "indices": [v - max(idx) for v in idx]}
            x = self.oracle.layer_forward(causal, x)
            for op in ops:
                x = self.oracle.layer_forward(op, x)
        self.packed += H + k
        keep = np.arange(p0, p0 + k) >= L + R
        return (x[H:] - self.model["log_prior"][None, :])[keep]

    def push(self, new_frames, eos=False):
        assert not self.ended
        if self.caches is None:
            self.caches = [None] * len(self.stages)
        self.frames = np.concatenate([self.frames, np.asarray(new_frames, np.float32).reshape(-1, self.frames.shape[1])])
        self.ended = eos
        n = len(self.frames)
        p1 = 0 if n == 0 else self.L + n + (self.R if eos else 0)
        out = []
        while self.P < p1:
            k = min(p1 - self.P, self.max_rows - self.H)
            out.append(self._block(self.P, k))
            self.P += k
        if not out:
            return np.zeros((0, self.model["log_prior"].shape[0]), np.float32)
        return np.concatenate(out)


def stream(oracle, model, feats, counts, eos_at, max_rows=4096):
    """feats pushed as counts[i] frames per push (EOS with push eos_at):
    (all rows, packed rows)."""
    s = Stream(oracle, model, max_rows)
    at, out = 0, []
    for i, c in enumerate(counts):
        out.append(s.push(feats[at:at + c], eos=i == eos_at))
        at += c
    assert at == len(feats)
    return np.concatenate(out), s.packed
