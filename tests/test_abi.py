"""The C-ABI library (no GPU needed): it loads, exports exactly the entry
points include/catears_gpu.h declares, and its host-only functions behave."""
import ctypes
import os
import re

import pytest

from conftest import ROOT


def header_symbols():
    text = open(os.path.join(ROOT, "include", "catears_gpu.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(ce_gpu_\w+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    from catears_amd import gpu
    lib = gpu.lib()
    syms = header_symbols()
    assert len(syms) >= 20
    missing = [s for s in syms if not hasattr(lib, s)]
    assert not missing, missing
    assert sorted(gpu.ABI) == syms


def test_frame_count_matches_reference_rule(oracle):
    from catears_amd import gpu
    for n in [0, 1, 399, 400, 401, 559, 560, 7802, 160000, 1600000]:
        assert gpu.num_frames(n) == oracle.Fbank.num_frames(n)


def test_version_and_error_string():
    from catears_amd import gpu
    assert b"gfx950" in gpu.lib().ce_gpu_version()
    assert gpu.lib().ce_gpu_last_error() is not None


def test_only_gfx950_code_objects():
    # the library carries gfx950 code only (no CUDA/other-arch fallbacks)
    data = open(os.path.join(ROOT, "catears_amd", "lib", "libcatears_hip.so"), "rb").read()
    assert b"gfx950" in data
    for other in (b"gfx942", b"gfx90a", b"sm_80", b"sm_90"):
        assert other not in data


def test_product_library_has_no_ablation_kernels():
    """The product library carries the bf16x6 kernels its dispatch
    (kernels/gemm_bf16x6.hip) can reach and no other: the measurement
    variants and the DIAG ablation builds (wrong results, timing only) are
    compiled only into `make EXPERIMENTS=1`'s separate library
    (kernels/gemm_bf16x6_exp.hip).  Exactly seven kernels: the direct-weight
    kernel d on 128 x 128 tiles (the gathered FIRST layer, and wide tiles)
    and on 256 x 128, the one-wave-per-SIMD kernel w on 512 x 128, the plane
    kernel q with fp32 and with split output, and splice_pad_split.  Every d
    has DIAG = 0, KS = 1, PIN = OUT16 = false; there is no f, ws or r
    kernel.  The int8 GEMM likewise (kernels/nnet_i8.hip against
    kernels/nnet_i8_exp.hip): exactly gemm_i8_pipe_kernel<256, 128, 3, 4, 2,
    false> and the two Quantize kernels."""
    data = open(os.path.join(ROOT, "catears_amd", "lib", "libcatears_hip.so"), "rb").read()
    syms = set(re.findall(rb"_ZN7catears12_GLOBAL__N_1\d+(?:gemm_bf16x6\w*?_kernel|splice_pad_split_kernel)\w*", data))
    # name + template arguments of each: the scope in front and the return
    # type and parameter list behind cut off
    kern = sorted({re.sub(rb"^_ZN7catears12_GLOBAL__N_1\d+", b"", re.sub(rb"EEvNS0_6X6ArgsE$|EPKf\w+$", b"", s))
                   for s in syms})
    x6, w6 = b"INS0_5X6CfgI", b"INS0_5W6CfgI"
    assert kern == sorted([
        b"gemm_bf16x6d_kernel" + x6 + b"Li128ELi128ELi2ELi4ELi2EEELb1ELi0ELi1ELb0ELb0E",
        b"gemm_bf16x6d_kernel" + x6 + b"Li128ELi128ELi2ELi4ELi2EEELb0ELi0ELi1ELb0ELb0E",
        b"gemm_bf16x6d_kernel" + x6 + b"Li256ELi128ELi4ELi2ELi2EEELb0ELi0ELi1ELb0ELb0E",
        b"gemm_bf16x6w_kernel" + w6 + b"Li512ELi128ELi4ELi2EEELb1ELi4E",
        b"gemm_bf16x6q_kernel" + x6 + b"Li128ELi128ELi4ELi2ELi3EEELb1ELi0E",
        b"gemm_bf16x6q_kernel" + x6 + b"Li128ELi128ELi4ELi2ELi3EEELb0ELi0E",
        b"splice_pad_split_kernel",
    ]), kern
    for gone in (b"gemm_bf16x6f_kernel", b"gemm_bf16x6ws_kernel", b"gemm_bf16x6r_kernel"):
        assert gone not in data, gone
    # every d: <Cfg, FIRST, DIAG = 0, KS = 1, PIN = false, OUT16 = false>
    d = re.findall(rb"gemm_bf16x6d_kernelINS0_5X6CfgI(?:Li\d+E)+EELb[01]E(Li\d+E)(Li\d+E)(Lb[01]E)(Lb[01]E)", data)
    assert d and set(d) == {(b"Li0E", b"Li1E", b"Lb0E", b"Lb0E")}, sorted(set(d))
    # the int8 GEMM likewise (kernels/nnet_i8.hip): the one kernel
    # launch_i8_gemm launches and the two Quantize kernels; the plain LDS-DMA
    # kernel with its DIAG ablation builds, the first kernel (once the
    # fallback) and the removed ones are not in the library at all
    syms = set(re.findall(rb"_ZN7catears12_GLOBAL__N_1\d+(?:gemm_i8_\w*?_kernel|quantize\w*?_kernel)\w*", data))
    # (kernels/quant.hip's u8 quantize_kernel shares the name: one entry)
    i8 = sorted({re.sub(rb"^_ZN7catears12_GLOBAL__N_1\d+", b"",
                        re.sub(rb"(?:EEv|E)(?:NS0_6I8ArgsE|PKf\w+)$", b"", s)) for s in syms})
    assert i8 == sorted([b"gemm_i8_pipe_kernelILi256ELi128ELi3ELi4ELi2ELb0E", b"quantize_kernel",
                         b"quantize_fast_kernelILi1E"]), i8
    for gone in (b"gemm_i8_glds_kernel", b"gemm_i8_nnet_kernel", b"gemm_i8_q_kernel", b"gemm_i8_reg_kernel",
                 b"quantize_fast_kernelILi2E"):
        assert gone not in data, gone
    assert b"gemm_i8_pipe_kernel" in data and b"lat_gemm_kernel" in data
    assert b"gemm_bf16x6r_kernel" not in data


def test_product_library_reads_no_environment_switch():
    """The tuning switches of the measurement tools (CE_KNOB, internal.h) are
    read from the environment only by the experiments library; the product
    library compiles their defaults in, so no CATEARS_* name
    -- and no getenv call -- is in it.  Mode choices go through the C-ABI
    (ce_gpu_model_set_gemm, ce_gpu_ctx_set_*).  The drop-in layer's
    CATEARS_DEVICE / CATEARS_LANES / CATEARS_FBANK (host/src/runtime.cc,
    libcatears_pk.so) are its documented configuration, not switches here."""
    data = open(os.path.join(ROOT, "catears_amd", "lib", "libcatears_hip.so"), "rb").read()
    assert re.findall(rb"CATEARS_[A-Z0-9_]+", data) == []
    assert b"getenv" not in data


def test_dropin_library_defines_no_test_hook():
    """The drop-in's failure injection is test-only: libcatears_pk.so holds an
    undefined weak reference to catears_test_inject_failure (null in every
    product binary) and no definition; only the test driver defines it."""
    import subprocess
    pk = os.path.join(ROOT, "catears_amd", "lib", "libcatears_pk.so")
    out = subprocess.run(["nm", "-D", pk], capture_output=True, text=True, check=True).stdout
    hook = [ln.split() for ln in out.splitlines() if ln.endswith(" catears_test_inject_failure")]
    assert hook and all(f[-2] == "w" for f in hook), hook
    assert "InjectDeviceFailures" not in out


def _code_objects(path):
    """Every gfx950 code object in a HIP shared library: the .hip_fatbin
    section holds one clang offload bundle per translation unit."""
    import struct
    data = open(path, "rb").read()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    objs, at = [], data.find(magic)
    while at >= 0:
        n = struct.unpack_from("<Q", data, at + 24)[0]
        p = at + 32
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", data, p)
            triple = data[p + 24:p + 24 + tlen].decode()
            p += 24 + tlen
            if "gfx950" in triple:
                objs.append(data[at + off:at + off + size])
        at = data.find(magic, p)
    return objs


def kernel_private_segments(path):
    """{kernel symbol: .private_segment_fixed_size} from the code objects'
    AMDGPU metadata notes (llvm-readelf --notes)."""
    import subprocess
    import tempfile
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not os.path.exists(readelf):
        pytest.skip("llvm-readelf not in this image")
    out = {}
    for co in _code_objects(path):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(co)
            f.flush()
            notes = subprocess.check_output([readelf, "--notes", f.name], text=True)
        name = None
        for ln in notes.splitlines():
            m = re.match(r"\s+\.name:\s+(\S+)", ln)
            if m:
                name = m.group(1)
            m = re.match(r"\s+\.private_segment_fixed_size:\s+(\d+)", ln)
            if m and name:
                out[name] = int(m.group(1))
    return out


def test_product_kernels_use_no_scratch():
    """No kernel of the product library has a private (scratch) segment.
    The exact fbank kernel once spilled 3 VGPRs to scratch under a forced
    5-waves-per-SIMD budget and, only in the multi-stream pipeline, gave a
    different value for one frame in some runs; every kernel
    on the path now keeps its state in registers and LDS."""
    segs = kernel_private_segments(os.path.join(ROOT, "catears_amd", "lib", "libcatears_hip.so"))
    assert len(segs) >= 20, sorted(segs)
    assert any("fbank_kernel" in k for k in segs)
    scratch = {k: v for k, v in segs.items() if v}
    assert not scratch, scratch


def kernel_instruction_counts(path, pattern):
    """{kernel symbol: count of instructions whose mnemonic matches pattern}
    from llvm-objdump of the library's gfx950 code objects."""
    import collections
    import subprocess
    import tempfile
    objdump = "/opt/rocm/lib/llvm/bin/llvm-objdump"
    if not os.path.exists(objdump):
        pytest.skip("llvm-objdump not in this image")
    rx = re.compile(pattern)
    out = collections.Counter()
    n_kernels = 0
    for co in _code_objects(path):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(co)
            f.flush()
            asm = subprocess.check_output([objdump, "-d", "--mcpu=gfx950", f.name], text=True)
        name = None
        for ln in asm.splitlines():
            m = re.match(r"^[0-9a-f]+ <(.+)>:", ln)
            if m:
                name = m.group(1)
                n_kernels += 1
                continue
            m = re.match(r"^\s+([a-z_0-9]+)", ln)
            if m and name and rx.fullmatch(m.group(1)):
                out[name] += 1
    return out, n_kernels


def test_product_kernels_use_no_packed_fp32_valu():
    """No kernel of the product library issues packed-FP32 VALU instructions
    (v_pk_add_f32, v_pk_mul_f32, v_pk_fma_f32, v_pk_mov_b32).  With them, the
    fast fbank kernel's lanes 48-63 computed wrong values in about 2 % of its
    launches while bf16 MFMA GEMMs ran beside it on other streams (round 4's
    GPUTEST failure; tools/experiments/lds_race_stress.py: 2 x 126 k launches
    without a difference once they were gone).  The Makefile
    builds every kernel with the packed-fp32-ops target feature off."""
    counts, n = kernel_instruction_counts(os.path.join(ROOT, "catears_amd", "lib", "libcatears_hip.so"),
                                          r"v_pk_(add|mul|fma)_f32|v_pk_mov_b32")
    assert n >= 20
    assert not counts, dict(counts)
