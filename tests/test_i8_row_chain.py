"""Row steps of a static int8 model that write the next Linear's bytes
(ce_gpu_debug_rowop_chain_q, ce_gpu_debug_i8_static_launches): what needs no
GPU -- the two entries, the refusals of the first (decided before the context
is touched), and the hand-over rule restated on layer lists
(tests/i8rowref.py).  tests/test_gpu_i8_row_chain.py runs it."""
import ctypes

import numpy as np

import i8rowref
import rownet

EINVAL = -2


def test_abi_lists_the_new_entries():
    from catears_amd import gpu
    for name in ("ce_gpu_debug_rowop_chain_q", "ce_gpu_debug_i8_static_launches"):
        assert name in gpu.ABI and hasattr(gpu.lib(), name)
    assert b" 0.7 " in gpu.lib().ce_gpu_version()
    counts = gpu.debug_i8_static_launches()
    assert len(counts) == 3 and all(c >= 0 for c in counts)
    q = ctypes.c_int64(-1)
    assert gpu.lib().ce_gpu_debug_i8_static_launches(None, ctypes.byref(q), None) == 0 and q.value >= 0
    assert gpu.lib().ce_gpu_debug_i8_static_launches(None, None, None) == 0


def test_rowop_chain_q_refuses_bad_arguments():
    """Every refusal comes before the context or a buffer is read: a block of
    host memory stands in for each here, and none of it may be touched."""
    from catears_amd import gpu
    fn = gpu.lib().ce_gpu_debug_rowop_chain_q
    blk = lambda: ctypes.create_string_buffer(4096)
    ctx, x, q, rs, zero = blk(), blk(), blk(), blk(), blk()
    ops = (ctypes.c_int * 5)(0, 4, 0, 4, 0)

    def call(ctx=ctx, n=2, rows=3, dim=128, x=x, ld=128, q=q, ldq=128, rs=rs, zero=zero, h_ops=ops):
        return fn(ctx, n, h_ops, rows, dim, x, ld, None, None, 0.03125, 7, q, ldq, rs, zero)

    assert call(n=5) == EINVAL and "bad argument" in gpu.lib().ce_gpu_last_error().decode()
    assert call(n=-1) == EINVAL
    assert call(ldq=127) == EINVAL
    assert call(ld=127) == EINVAL
    assert call(dim=0, ld=0, ldq=0) == EINVAL
    assert call(rows=-1) == EINVAL
    assert call(ctx=None) == EINVAL
    assert call(h_ops=None) == EINVAL
    for name in ("x", "q", "rs", "zero"):
        assert call(**{name: None}) == EINVAL, name
        assert "NULL" in gpu.lib().ce_gpu_last_error().decode(), name
    for b in (ctx, x, q, rs, zero):
        assert b.raw == bytes(4096)


def test_launch_counts_of_the_renorm_nets():
    """Hidden width 128: every hidden Linear reads plain 128-byte rows, so the
    Normalize before it stores them; one quantize pass is left, on the
    features.  Hidden width 96: every Linear's operand is written spliced by
    its quantize pass."""
    layers, _, _ = rownet.renorm_tdnn(128, 52)
    how, runs = i8rowref.hand_overs(layers)
    assert len(how) == 7 and runs == [1] * 6 + [0]
    assert rownet.steps(layers).count("normalize") == 6
    assert how == ["quantize"] + ["chain"] * 6
    assert i8rowref.launch_counts(layers) == (1, 6, 6)
    assert i8rowref.launch_counts(layers, fused=False) == (7, 6, 0)
    layers, _, _ = rownet.renorm_tdnn(96, 52)
    assert i8rowref.hand_overs(layers)[0] == ["quantize"] * 7
    assert i8rowref.launch_counts(layers) == (7, 6, 0)


def test_launch_counts_of_other_shapes():
    from catears_amd import synth
    # no row step: the requantize epilogues, as tests/i8ref.py::paths has them
    layers = synth.tdnn_layers(128, 52)[0]
    assert not rownet.has_row_steps(layers)
    assert i8rowref.launch_counts(layers) == (1, 0, 0)
    # a second BatchNorm and a ReLU as row steps behind the hidden width 64:
    # one run of two steps, one launch, the 64-wide consumer spliced
    layers, _ = rownet.exact_cases()["second-bn"]
    how, runs = i8rowref.hand_overs(layers)
    assert runs == [2, 0, 0] and how == ["quantize"] * 3
    assert i8rowref.launch_counts(layers) == (3, 1, 0)
    # a run of five steps is two launches, the second of which stores
    five = rownet.renorm_tdnn(128, 52)[0]
    at = [i for i, L in enumerate(five) if L["kind"] == "normalize"][0]
    five = five[:at] + [{"kind": "normalize"}] * 4 + five[at:]
    assert i8rowref.launch_counts(five) == (1, 7, 6)
    # a row step behind the last Linear stores nothing
    layers, _ = rownet.exact_cases()["row-last"]
    assert i8rowref.launch_counts(layers)[2] == 0


def test_static_rows_equal_the_oracle_on_a_net_without_a_sum(oracle):
    """On ReLU / BatchNorm row steps (element-wise) static_rows is
    tests/test_int8_static.py's static_oracle bit for bit."""
    from test_int8_static import fp32_ranges, static_oracle
    layers, x = rownet.exact_cases()["second-bn"]
    x = np.array(x[:40])
    ranges = fp32_ranges(oracle, layers, x)
    got = i8rowref.static_rows(oracle, layers, x, ranges)
    want = static_oracle(oracle, layers, x, ranges)
    assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))
