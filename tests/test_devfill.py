"""What needs no GPU of the stale-memory tests (tests/devfill.py,
tests/test_gpu_stale_memory.py): the two fill words read as devfill says in
every element type the library keeps in its buffers, and the three debug
entries exist, check their arguments and touch no device."""
import math
import os
import re

import numpy as np
import pytest

import devfill
from conftest import ROOT

ENTRIES = ("ce_gpu_debug_fill_allocs", "ce_gpu_debug_fill_ctx", "ce_gpu_debug_fill_sessions")


def test_nan_word_is_a_nan_in_every_float_type_and_minus_one_as_integer():
    r = devfill.readings(devfill.NAN_WORD)
    for t in ("fp32", "bf16", "bf16_low", "fp16", "fp16_high"):
        assert math.isnan(float(r[t])), t
    assert (r["int8"], r["int32"], r["u8"]) == (-1, -1, 255)


def test_big_word_is_finite_where_a_nan_would_be_swallowed():
    r = devfill.readings(devfill.BIG_WORD)
    assert np.isfinite(r["fp32"]) and 2.99e38 < r["fp32"] < 3.0e38 < np.finfo(np.float32).max
    assert np.isfinite(r["bf16"]) and np.isfinite(r["bf16_low"]) and r["bf16"] == r["bf16_low"] > 2.99e38
    assert math.isnan(float(r["fp16"])) and math.isnan(float(r["fp16_high"]))
    # a min / max reduction skips a NaN and is moved by this; the int8
    # quantizer clamps it to the top byte
    assert np.fmax(np.float32(1.0), np.float32(np.nan)) == 1.0 and np.fmax(np.float32(1.0), r["fp32"]) == r["fp32"]
    assert (r["int8"], r["u8"]) == (0x61, 0x61)


def test_entries_are_declared_bound_and_debug_only():
    from catears_amd import gpu
    header = open(os.path.join(ROOT, "include", "catears_gpu.h")).read()
    for name in ENTRIES:
        assert name in gpu.ABI and hasattr(gpu.lib(), name)
        assert re.search(r"\bint " + name + r"\(", header), name
    assert re.search(r"int ce_gpu_debug_fill_allocs\(int on, uint32_t word\);", header)
    # the product library still reads no environment switch (tests/test_abi.py
    # asserts it on the binary); the header says which buffers are left alone
    for kept in ("fbank tables", "overflow word", "tickets"):
        assert kept in header, kept
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "ce_gpu_debug_fill_" in integration and "debug" in integration


def test_entries_check_their_arguments_without_a_device():
    from catears_amd import gpu
    L = gpu.lib()
    # process-wide switch: no device call when nothing is allocated
    assert L.ce_gpu_debug_fill_allocs(1, devfill.NAN_WORD) == 0
    assert L.ce_gpu_debug_fill_allocs(0, 0) == 0
    assert L.ce_gpu_debug_fill_ctx(None, devfill.NAN_WORD, None) == -2
    assert b"NULL" in L.ce_gpu_last_error()
    assert L.ce_gpu_debug_fill_sessions(None, devfill.BIG_WORD, 0, None) == -2
    with pytest.raises(gpu.CatearsError, match="EINVAL"):
        gpu.check(L.ce_gpu_debug_fill_sessions(None, 0, 1, None))
