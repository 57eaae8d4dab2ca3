"""Static int8 on nets with row steps of their own (tests/rownet.py): the rows
a model must give, and which hand-over each of its Linears takes.

static_rows is tests/test_int8_static.py::static_oracle -- per Linear
Quantize's parameters of the two-element tensor [min, max], Quantize's
elementwise step with them, MatMat_U8U8F32, bias -- with every other layer
evaluated by rownet.row_op, the row kernel's lane order restated, instead of
oracle.layer_forward: a Normalize's sum then has the device's order, so the
rows ahead of a final LogSoftmax are exact arithmetic and the bar is bit for
bit.

hand_overs restates run_steps_i8_static's choice (csrc/nnet_programs.cc) on a
layer list: a Linear's input arrives by the quantize pass ("quantize"), from
the requantize epilogue of the GEMM before it ("gemm"), or from the last
launch of the row steps before it ("chain": i8_rows_can_quantize).  The
Linear behind a hand-over reads plain bytes when its input width is a multiple
of the int8 K-tile (128 bytes: I8Layer::spliced otherwise), which is also all
that i8_gemm_can_requantize asks of the producer of that width.
launch_counts turns that into the three figures of
ce_gpu_debug_i8_static_launches for one chunk."""
import numpy as np

import netgen
import rownet

K_ALIGN = 128      # i8_k_align
ROW_CHAIN_MAX = 4  # kRowChainMax

ROW_KINDS = ("relu", "batchnorm", "normalize", "softmax", "log_softmax")


def static_rows(oracle, layers, x, ranges, taps=None):
    """The net's rows with Linear i on the frozen parameters of ranges[i];
    taps: a list that receives every Linear's quantized input (uint8)."""
    x = np.ascontiguousarray(x, np.float32)
    li, i = 0, 0
    while i < len(layers):
        L = layers[i]
        k = L["kind"]
        if k == "splice":
            nar = layers[i + 1]
            idx, left, right = L["indices"], nar["left"], nar["right"]
            assert nar["kind"] == "narrow" and left == -min(min(idx), 0) and right == max(max(idx), 0)
            rows = x.shape[0] - left - right
            assert rows > 0, "input does not cover the context"
            x = np.concatenate([x[left + o:left + o + rows] for o in idx], axis=1)
            i += 1
        elif k == "narrow":
            assert L["left"] == 0 and L["right"] == 0
        elif k == "linear":
            _, s, z = oracle.quantize(np.float32([ranges[li][0], ranges[li][1]]))
            xq = oracle._quantize_with(x, s, z)
            if taps is not None:
                taps.append(xq)
            wq, sw, zw = oracle.quantize(L["W"])
            small = xq.shape[1] * (255 + abs(z)) * (255 + abs(zw)) < 2 ** 31 and 0 <= z <= 255 and 0 <= zw <= 255
            y = (oracle.gemm_u8u8f32_f64 if small else oracle.gemm_u8u8f32)(xq, s, z, wq, sw, zw)
            x = (y + np.asarray(L["b"], np.float32)[None, :]).astype(np.float32)
            li += 1
        else:
            assert k in ROW_KINDS, k
            x = rownet.row_op(k, x, L.get("scale"), L.get("offset"))
        i += 1
    return x


def without_final_log_softmax(layers):
    return layers[:-1] if layers[-1]["kind"] == "log_softmax" else layers


def log_softmax_f64(rows):
    v = np.asarray(rows, np.float64)
    m = v.max(axis=1, keepdims=True)
    return v - (m + np.log(np.exp(v - m).sum(axis=1, keepdims=True)))


def hand_overs(layers, fused=True):
    """Per Linear "quantize", "gemm" or "chain"; and per Linear the number of
    row steps behind it."""
    lin = netgen.linears(layers)
    runs, cur = [], -1
    for s in rownet.steps(layers):
        if s == "gemm":
            cur += 1
            runs.append(0)
        else:
            runs[cur] += 1
    assert len(runs) == len(lin)
    how = ["quantize"]
    for g, run, nxt in zip(lin, runs, lin[1:]):
        plain = nxt["din"] % K_ALIGN == 0 and nxt["din"] == g["n"]
        how.append("quantize" if not (fused and plain) else "chain" if run else "gemm")
    return how, runs


def launch_counts(layers, fused=True):
    """(quantize passes, row-step launches, row-step launches that store
    bytes) of one chunk of the static int8 program."""
    how, runs = hand_overs(layers, fused)
    row_launches = sum(-(-r // ROW_CHAIN_MAX) for r in runs)
    return how.count("quantize"), row_launches, how.count("chain")
