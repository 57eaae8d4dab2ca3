"""Hostile residue for device memory the library owns (the helpers of
tests/test_gpu_stale_memory.py; tests/test_devfill.py checks on the CPU what
is said here about the two words).

The library's debug entries ce_gpu_debug_fill_allocs / _fill_ctx /
_fill_sessions overwrite its own device buffers with one 32-bit word.  A call
that reads such memory before it has written it then computes on that word.
Two words, because no single one is hostile to every reader:

NAN_WORD  0xFFFFFFFF  a NaN as fp32, as either bf16 half and as either fp16
                      half; -1 as int8 and int32, 255 as u8.  Anything that
                      multiplies, adds or converts it shows it -- a zero
                      weight pad does not hide it (0 * NaN = NaN).
BIG_WORD  0x7F617F61  about 2.997e38 as fp32 and as either bf16 half: finite,
                      so the readers that swallow a NaN see it -- a min / max
                      reduction skips NaN but is moved by a finite outlier,
                      the int8 quantizer clamps it to a byte that changes a
                      row sum.  0x7F61 is a NaN as fp16; 97 / 127 as bytes.
"""
import contextlib

import numpy as np

NAN_WORD = 0xFFFFFFFF
BIG_WORD = 0x7F617F61
WORDS = {"nan": NAN_WORD, "big": BIG_WORD}


def readings(word):
    """What a buffer filled with `word` holds, per element type."""
    w = np.array([word], np.uint32)
    return {"fp32": w.view(np.float32)[0], "bf16": (w & np.uint32(0xffff0000)).view(np.float32)[0],
            "bf16_low": (w << np.uint32(16)).view(np.float32)[0], "fp16": w.view(np.float16)[0],
            "fp16_high": w.view(np.float16)[1], "int8": w.view(np.int8)[0], "u8": w.view(np.uint8)[0],
            "int32": w.view(np.int32)[0]}


@contextlib.contextmanager
def fresh_allocations(G, word):
    """Every device allocation the library makes inside the block arrives
    filled with `word`; off again behind it, whatever happens inside."""
    G.debug_fill_allocs(True, word)
    try:
        yield
    finally:
        G.debug_fill_allocs(False)


def fill_ctx(G, ctx, word):
    """The context's call-scoped buffers filled with `word`; returns the
    bytes filled."""
    return G.debug_fill_ctx(ctx, word)


def fill_slots(G, sess, word, slots=()):
    """The set's per-push scratch and the listed slots' regions filled."""
    G.debug_fill_sessions(sess, word, slots)


def same_bits(torch, got, want):
    """Bit equality of two float32 device tensors."""
    return got.shape == want.shape and bool(torch.equal(got.contiguous().view(torch.int32),
                                                        want.contiguous().view(torch.int32)))
