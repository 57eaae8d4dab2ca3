"""CPU restatement of the plain bf16 GEMM mode (CE_GPU_GEMM_BF16,
include/catears_gpu.h) for tests/test_gemm_bf16.py and
tests/test_gpu_gemm_bf16.py.

Every Linear computes bf16(a) @ bf16(W) with round-to-nearest-even operands
and exact products; a hidden output is rounded to bf16 by its consumer (the
same function as the GPU's rounding at the producer, since the only consumer
of a hidden Linear is the next Linear).  bias / ReLU / BatchNorm are float32
operations in the reference's rounding order.

The host's tile rule (kernels/gemm_bf16.hip bf16_small_tile) is restated in
tile() / tiles(), as netgen.kernels does for the other modes.
"""
import numpy as np

import netgen


def rne_bf16(x):
    """float32 -> the nearest bf16 (ties to even), returned as float32.
    On the uint32 bits, as weight_images.cc's bf16_rne / v_cvt_pk_bf16_f32."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    nan = (u & np.uint32(0x7fffffff)) > np.uint32(0x7f800000)
    r = (u + np.uint32(0x7fff) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xffff0000)
    r = np.where(nan, (u & np.uint32(0xffff0000)) | np.uint32(0x00400000), r)
    return r.astype(np.uint32).view(np.float32)


def trunc_bf16(x):
    """float32 -> bf16 by dropping the low 16 bits (what the mode must NOT do)."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return (u & np.uint32(0xffff0000)).view(np.float32)


def walk(layers, x, acc=np.float64, k_reversed=False, visit=None, log_softmax=True, rnd=rne_bf16):
    """netgen._walk's topology under the mode's definition.  Every Linear is
    rnd(a) @ rnd(W) accumulated in dtype `acc` (numpy's matmul on K ascending,
    or on K reversed), cast to float32; bias and every post op are float32
    operations.  A final LogSoftmax is evaluated in float64 on the float32
    activations (log_softmax=False: left out).  visit(layer, a16, w16) is
    called per Linear with the rounded operands.  Returns float32, or float64
    after a LogSoftmax."""
    x = np.asarray(x, np.float32)
    i = 0
    while i < len(layers):
        L = layers[i]
        k = L["kind"]
        if k == "splice":
            nar = layers[i + 1]
            assert nar["kind"] == "narrow"
            idx, left, right = L["indices"], nar["left"], nar["right"]
            assert left == -min(min(idx), 0) and right == max(max(idx), 0)
            rows = x.shape[0] - left - right
            assert rows > 0, "input does not cover the context"
            x = np.concatenate([x[left + o:left + o + rows] for o in idx], axis=1)
            i += 1
        elif k == "narrow":
            assert L["left"] == 0 and L["right"] == 0
        elif k == "linear":
            a16, w16 = rnd(x), rnd(L["W"])
            if visit:
                visit(L, a16, w16)
            a, w = a16.astype(acc), w16.astype(acc)
            if k_reversed:
                a, w = np.ascontiguousarray(a[:, ::-1]), np.ascontiguousarray(w[::-1])
            x = (a @ w).astype(np.float32)
            x = x + L["b"].astype(np.float32)
        elif k == "relu":
            x = np.where(x < 0.0, np.float32(0.0), x)
        elif k == "batchnorm":
            x = x * L["scale"].astype(np.float32)
            x = x + L["offset"].astype(np.float32)
        elif k == "log_softmax":
            if log_softmax:
                assert i + 1 == len(layers)
                x = x.astype(np.float64)
                m = x.max(axis=1, keepdims=True)
                x = x - (m + np.log(np.exp(x - m).sum(axis=1, keepdims=True)))
        else:
            raise ValueError(k)
        assert x.dtype == (np.float64 if k == "log_softmax" and log_softmax else np.float32)
        i += 1
    return x


def exact_bounds(layers, x):
    """log2 of max_ij (sum_k |bf16(a_ik)| |bf16(w_kj)| + |b_j|) per Linear on
    input x: below 24, every partial sum of every order is an integer float32
    holds exactly (the rounded operands of an integer net are integers)."""
    out = []

    def visit(L, a16, w16):
        # every product is an integer (the operands are integers, or integers
        # scaled by 2^e and 2^-e in netgen's binade-shifted cases)
        col = int(np.abs(w16).sum(axis=0).argmax())
        prod = a16.astype(np.float64)[:64] * w16.astype(np.float64)[:, col]
        bias = np.asarray(L["b"], np.float64)
        assert np.all(np.isfinite(prod)) and np.array_equal(prod, np.rint(prod)), "products are not integers"
        assert np.array_equal(bias, np.rint(bias)), "bias is not integers"
        bound = (np.abs(a16).astype(np.float64) @ np.abs(w16).astype(np.float64) + np.abs(bias)).max()
        out.append(float(np.log2(max(bound, 1.0))))

    walk(layers, x, np.float64, visit=visit)
    return out


# ------------------------------------------------ the dispatch rule, read --

LARGE_MIN_TILES = 64  # internal.h kB16LargeMinTiles


def tile(m, n):
    """bf16_small_tile: the tile shape of one Linear of n outputs on a block
    of m rows -- a function of (rows, n) only, K plays no part."""
    return "b16_32x32" if ((m + 127) // 128) * ((n + 127) // 128) < LARGE_MIN_TILES else "b16_128x128"


def tiles(layers, out_rows):
    """Per Linear (tile, K-tiles of 32, n) for a block of out_rows output rows
    (the GEMMs see out_rows + left + right rows)."""
    left, right = netgen.context(layers)
    m = out_rows + left + right
    out = []
    for i, g in enumerate(netgen.linears(layers)):
        k = (g["k"] + 63) // 64 * 64 if i == 0 else g["k"]  # the loader pads the first layer's K to 64
        out.append((tile(m, g["n"]), k // 32, g["n"]))
    return out
