"""The exact cases of tests/rownet.py are exact, as tests/test_netgen.py shows
for netgen's: for every case the oracle (the reference's layer loop) in three
GEMM orders -- its naive fp32 loop, an fp64 GEMM, the fp32 loop with K
reversed -- gives the bits of rownet.walk, and the plain bf16 restatement
gives the same bits in its three orders.  A GPU mismatch on these nets is
then the library's.  Also: the restated row steps against the oracle's, and
the restated loader rule on the cases."""
import numpy as np
import pytest

import bf16ref
import netgen
import rownet

ORDER_ROWS = 40


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _f64(a, w):
    return (a.astype(np.float64) @ w.astype(np.float64)).astype(np.float32)


def all_cases():
    cases = dict(rownet.exact_cases())
    cases.update({f"pad-{k}": v for k, v in rownet.pad_cases().items()})
    cases["big"] = rownet.big_case()
    return cases


@pytest.mark.parametrize("name", sorted(all_cases()))
def test_exact_cases_are_order_independent(oracle, name):
    layers, x = all_cases()[name]
    left, right = netgen.context(layers)
    want = rownet.check_exact(layers, x)
    assert want.shape[0] == x.shape[0] - left - right and np.all(np.isfinite(want))
    xs = np.array(x[:ORDER_ROWS + left + right])
    naive = oracle.nnet_propagate(layers, xs)
    assert np.array_equal(bits(naive), bits(want[:ORDER_ROWS])), f"{name}: naive fp32"
    f64 = oracle.nnet_propagate(layers, xs, gemm=_f64)
    assert np.array_equal(bits(f64), bits(naive)), f"{name}: fp64 GEMM"
    rev = oracle.nnet_propagate(layers, xs, gemm=lambda a, w: oracle.sgemm(a[:, ::-1], w[::-1]))
    assert np.array_equal(bits(rev), bits(naive)), f"{name}: K reversed"
    assert np.array_equal(bits(rownet.walk(layers, xs, acc=np.float32, k_reversed=True)), bits(naive))


@pytest.mark.parametrize("name", sorted(all_cases()))
def test_the_bf16_restatement_is_order_independent(name):
    """The plain bf16 definition on the exact cases: three orders, one result;
    it differs from the fp32 rows only behind a Normalize (whose output is
    rounded once), and there it does differ."""
    layers, x = all_cases()[name]
    left, right = netgen.context(layers)
    xs = np.array(x[:ORDER_ROWS + left + right])
    w64 = rownet.walk(layers, xs, rnd=bf16ref.rne_bf16)
    for kw in (dict(acc=np.float32), dict(acc=np.float32, k_reversed=True)):
        assert np.array_equal(bits(rownet.walk(layers, xs, rnd=bf16ref.rne_bf16, **kw)), bits(w64)), (name, kw)
    same = np.array_equal(bits(w64), bits(rownet.walk(layers, xs)))
    norm_feeds_linear = any(L["kind"] == "normalize" for L in layers[:-1])
    assert same == (not norm_feeds_linear), name


def test_row_steps_restated(oracle):
    """rownet.row_op against the oracle's layers: the same bits for ReLU and
    BatchNorm on any row and for Normalize on integer rows (an exact sum); on
    real rows the two summation orders differ by rounding only."""
    rng = np.random.default_rng(8400)
    for dim in (32, 96, 100, 1000):
        x = rng.normal(0.0, 2.0, size=(9, dim)).astype(np.float32)
        sc, of = rng.normal(1.0, 0.1, dim).astype(np.float32), rng.normal(0.0, 0.1, dim).astype(np.float32)
        assert np.array_equal(bits(rownet.row_op("relu", x)), bits(oracle.nnet_propagate([{"kind": "relu"}], x)))
        bn = {"kind": "batchnorm", "scale": sc, "offset": of}
        assert np.array_equal(bits(rownet.row_op("batchnorm", x, sc, of)), bits(oracle.nnet_propagate([bn], x)))
        xi = rng.integers(-50, 51, size=(9, dim)).astype(np.float32)
        assert np.array_equal(bits(rownet.row_op("normalize", xi)),
                              bits(oracle.nnet_propagate([{"kind": "normalize"}], xi)))
        for kind in ("normalize", "softmax", "log_softmax"):
            got, ref = rownet.row_op(kind, x), oracle.nnet_propagate([{"kind": kind}], x)
            assert np.allclose(got, ref, rtol=1e-5, atol=1e-6), kind
            assert np.allclose(got, rownet.eval_f64([{"kind": kind}], x), rtol=1e-5, atol=1e-6), kind
    # the order itself: lane sums over c = l (mod 64), then the xor tree
    t = rng.normal(0.0, 1.0, size=(3, 200)).astype(np.float32)
    for r in range(3):
        lanes = [np.float32(0.0)] * 64
        for c in range(200):
            lanes[c % 64] = np.float32(lanes[c % 64] + t[r, c])
        d = 32
        while d:
            lanes = [np.float32(lanes[l] + lanes[l ^ d]) for l in range(64)]
            d >>= 1
        assert bits(np.array(lanes[:1]))[0] == bits(rownet.lane_sum(t)[r:r + 1])[0]


def test_the_cases_are_what_the_issue_names():
    cases = rownet.exact_cases()
    assert rownet.steps(cases["five-posts"][0]) == ["gemm", "relu", "gemm", "gemm"]
    assert [L["kind"] for L in cases["five-posts"][0]][3:8] == ["relu", "batchnorm", "relu", "relu", "relu"]
    assert rownet.steps(cases["second-bn"][0]) == ["gemm", "batchnorm", "relu", "gemm", "gemm"]
    assert rownet.steps(cases["row-last"][0]) == ["gemm", "gemm", "gemm", "normalize"]
    for h in (64, 96):
        layers = cases[f"normalize-{h}"][0]
        assert rownet.steps(layers) == ["gemm", "normalize", "gemm"]
        assert [g["n"] for g in netgen.linears(layers)] == [h, rownet.PDFS]
    for layers, _ in cases.values():
        # inside the envelope but for the row steps: admitted, the model is bf16x6
        assert netgen.x6_ok(layers) and rownet.has_row_steps(layers)
    for layers, _ in rownet.pad_cases().values():
        assert not netgen.x6_ok(layers) and rownet.has_row_steps(layers)
    big, x = rownet.big_case()
    assert [g["n"] for g in netgen.linears(big)] == [1024, 36] and x.shape[0] == 1024 + 4
    assert bf16ref.tile(x.shape[0], 1024) == "b16_128x128"
    # netgen's own nets have no row step
    for geom in netgen.GEOMETRIES:
        assert not rownet.has_row_steps(netgen.exact_cases(geom)[0][1])


def test_renorm_tdnn_shape():
    layers, left, right = rownet.renorm_tdnn(64, 36)
    assert not any(L["kind"] == "batchnorm" for L in layers) and any(L["kind"] == "normalize" for L in layers)
    assert rownet.has_row_steps(layers) and netgen.context(layers) == (left, right)
