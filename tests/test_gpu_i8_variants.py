"""The int8 GEMM variants the experiments library keeps give the product's
bits.  CATEARS_I8_GEMM is read once per process by libcatears_hip_exp.so (the
product library compiles its one kernel in and reads no environment): one
child process per value.  The accumulators are int32 sums of exact products,
so the tile shape (128 x 128 of variant 0, 256 x 128, 256 x 256), the K-tile
(64 or 128 bytes), the stage count, the loop's schedule (10 / 11 through
registers, 15 plain LDS-DMA, 16 software-pipelined, 17 staggered) and, under
static int8, whether the next
layer's bytes come from the requantize epilogue (16, 17) or from a Quantize
pass (the others) cannot change any bit: the tolerance is zero.

Every variant scores the dynamic and the static int8 model of i8ref's I1 (8
asymmetric gathered segments of 128: another segment on every K-tile; fused
min / max; n = 100) and I3 (width 130, spliced: the scalar epilogue) at 70
rows (one partial row tile) and 300 rows (two row tiles of 256, the second
ragged); tests/test_i8ref.py::test_variant_cases_cover_the_gemm_paths shows
what these reach.  The DIAG values 61-71 give wrong results by design and are
not run.  A value the library no longer carries fails with CE_GPU_EINVAL
instead of running something else."""
import os
import subprocess
import sys

import numpy as np
import pytest

import i8ref
import netgen
from conftest import ROOT
from test_int8_static import central_half, fp32_ranges

pytestmark = pytest.mark.gpu

VARIANTS = (0, 10, 11, 15, 16, 17, 40, 41, 44)

# score(cases, out): cases.npz holds per geometry g the NN02 image `g.image`,
# the static ranges `g.ranges` and the blocks `g.x<rows>`; out.npz gets
# `g.dynamic.<rows>` and `g.static.<rows>`.  The same code in the parent (on
# the product library) and in every child.
SCORE = r"""
import numpy as np, torch
from catears_amd import gpu

def score(cases, out):
    c = np.load(cases)
    ctx = gpu.Context(0)
    got = {}
    for g in sorted({k.split(".")[0] for k in c.files}):
        image = c[g + ".image"].tobytes()
        models = {"dynamic": gpu.Model(ctx, image=image).quantize(ctx),
                  "static": gpu.Model(ctx, image=image).quantize_static(ctx, c[g + ".ranges"])}
        for k in c.files:
            if k.startswith(g + ".x"):
                x = torch.from_numpy(c[k]).to("cuda:0")
                for form, model in models.items():
                    got[f"{g}.{form}.{k[len(g) + 2:]}"] = gpu.nnet_propagate(ctx, model, x).cpu().numpy()
    np.savez(out, **got)
"""


@pytest.fixture(scope="module")
def cases(oracle, tmp_path_factory):
    """(cases.npz, the product library's outputs computed in this process)."""
    d = tmp_path_factory.mktemp("i8_variants")
    c = {}
    for g in i8ref.VARIANT_GEOMS:
        layers = i8ref.net(g)
        c[g + ".image"] = np.frombuffer(netgen.image(layers), np.uint8)
        c[g + ".ranges"] = central_half(fp32_ranges(oracle, layers, i8ref.calibration_input(g)))
        for rows in i8ref.VARIANT_ROWS:
            c[f"{g}.x{rows}"] = i8ref.block_input(g, rows)
    path = str(d / "cases.npz")
    np.savez(path, **c)
    ns = {}
    exec(SCORE, ns)
    ns["score"](path, str(d / "product.npz"))
    base = dict(np.load(str(d / "product.npz")))
    assert len(base) == 2 * len(i8ref.VARIANT_GEOMS) * len(i8ref.VARIANT_ROWS)
    assert all(a.size and np.isfinite(a).all() for a in base.values())
    return path, base


def _child(variant, cases_path, out, lib):
    env = dict(os.environ, CATEARS_I8_GEMM=str(variant), PYTHONPATH=ROOT, CATEARS_HIP_LIB=lib)
    return subprocess.run([sys.executable, "-c", SCORE + "import sys\nscore(sys.argv[1], sys.argv[2])\n",
                           cases_path, str(out)], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)


@pytest.mark.parametrize("variant", VARIANTS)
def test_i8_variant_bit_identical(tmp_path, cases, exp_lib, variant):
    path, base = cases
    r = _child(variant, path, tmp_path / "out.npz", exp_lib)
    assert r.returncode == 0, r.stderr[-3000:]
    got = np.load(str(tmp_path / "out.npz"))
    assert sorted(got.files) == sorted(base)
    for k in sorted(base):
        assert got[k].shape == base[k].shape, k
        assert np.array_equal(got[k].view(np.uint32), base[k].view(np.uint32)), \
            f"CATEARS_I8_GEMM={variant} differs from the product library on {k}"


def test_removed_variant_fails_loudly(tmp_path, cases, exp_lib):
    """20 was gemm_i8_q_kernel, removed: an error return, nothing runs."""
    r = _child(20, cases[0], tmp_path / "out.npz", exp_lib)
    assert r.returncode != 0
    assert "EINVAL" in r.stderr and "variant 20 is not in this build" in r.stderr, r.stderr[-2000:]
    assert not os.path.exists(tmp_path / "out.npz")
