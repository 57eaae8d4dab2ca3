"""ctypes binding of libcatears_hip.so (include/catears_gpu.h).

This is the Python side of the drop-in boundary: the same C-ABI a C++ host
(the reference's ce_stt.cc) links against.  Device memory and streams come
from PyTorch (plumbing only); every compute call goes through the HIP library.
There is no CPU fallback: if the library or a GPU is missing, calls raise.
"""
import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# CATEARS_HIP_LIB: development override (e.g. an instrumented build)
LIB_PATH = os.environ.get("CATEARS_HIP_LIB") or os.path.join(HERE, "lib", "libcatears_hip.so")

CE_GPU_OK = 0
ERRORS = {-2: "EINVAL", -3: "EHIP", -4: "EIO", -5: "ECORRUPT", -6: "ENOTSUP", -7: "ENOMEM"}

# Every symbol include/catears_gpu.h declares (checked by tests).
ABI = [
    "ce_gpu_last_error", "ce_gpu_version", "ce_gpu_ctx_create", "ce_gpu_ctx_destroy",
    "ce_gpu_ctx_set_stream", "ce_gpu_ctx_synchronize", "ce_gpu_ctx_profile", "ce_gpu_ctx_profile_classes",
    "ce_gpu_ctx_profile_read", "ce_gpu_model_load_config",
    "ce_gpu_model_load", "ce_gpu_model_info", "ce_gpu_model_tid2pdf", "ce_gpu_model_destroy",
    "ce_gpu_fbank_num_frames", "ce_gpu_plan_create", "ce_gpu_plan_info",
    "ce_gpu_plan_frame_offsets", "ce_gpu_plan_destroy", "ce_gpu_fbank", "ce_gpu_cmvn",
    "ce_gpu_am_forward", "ce_gpu_score", "ce_gpu_sgemm", "ce_gpu_quantize",
    "ce_gpu_gemm_u8u8f32", "ce_gpu_gemm_u8u8i32", "ce_gpu_model_load_mem",
    "ce_gpu_nnet_propagate", "ce_gpu_linear", "ce_gpu_splice", "ce_gpu_rowwise",
    "ce_gpu_profile_anchor", "ce_gpu_ctx_profile_intervals", "ce_gpu_model_quantize",
    "ce_gpu_nnet_propagate_blocks", "ce_gpu_loglik_gather", "ce_gpu_loglik_columns",
    "ce_gpu_model_set_gemm", "ce_gpu_model_get_gemm", "ce_gpu_ctx_overflow", "ce_gpu_ctx_set_latency",
    "ce_gpu_fbank_s16", "ce_gpu_score_s16", "ce_gpu_ctx_set_fbank", "ce_gpu_sum_f64", "ce_gpu_ctx_set_wide_tiles",
    "ce_gpu_sum_f64_many", "ce_gpu_trace_mark", "ce_gpu_nnet_check_mem",
    "ce_gpu_sessions_create", "ce_gpu_sessions_destroy", "ce_gpu_sessions_reset", "ce_gpu_sessions_push",
    "ce_gpu_sessions_push_s16", "ce_gpu_debug_counters",
    "ce_gpu_quant_params_from_range", "ce_gpu_model_calibrate", "ce_gpu_model_quantize_static",
    "ce_gpu_model_quant_params",
    "ce_gpu_i8_latency_plan", "ce_gpu_debug_i8_latency_launches",
    "ce_gpu_gemm_mode_from_name",
    "ce_gpu_sessions_create_ex", "ce_gpu_sessions_stats",
    "ce_gpu_model_pad_widths", "ce_gpu_model_padded_widths",
    "ce_gpu_model_admit_row_ops", "ce_gpu_debug_rowop_chain",
    "ce_gpu_debug_rowop_chain_q", "ce_gpu_debug_i8_static_launches",
    "ce_gpu_bf16_latency_max_rows", "ce_gpu_debug_bf16_latency_launches",
    "ce_gpu_debug_fill_allocs", "ce_gpu_debug_fill_ctx", "ce_gpu_debug_fill_sessions",
    "ce_gpu_plan_create_reusable", "ce_gpu_plan_assign", "ce_gpu_plan_capacity", "ce_gpu_debug_plan_tables",
]

# ce_gpu_model_set_gemm modes
GEMM_MODES = {"fp32": 0, "bf16x6": 1, "f16x3": 2, "bf16x6p": 3, "bf16": 4}

_lib = None


class CatearsError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"{ERRORS.get(code, code)}: {msg}")
        self.code = code


def lib():
    """Load the HIP library; raises ImportError if it was not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} missing: build it with `make` (hipcc, gfx950)")
    L = ctypes.CDLL(LIB_PATH)
    vp, ci, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    pp = ctypes.POINTER(ctypes.c_void_p)
    pi, pi64 = ctypes.POINTER(ci), ctypes.POINTER(i64)
    pi32 = ctypes.POINTER(ctypes.c_int32)
    sig = {
        "ce_gpu_last_error": (ctypes.c_char_p, []),
        "ce_gpu_version": (ctypes.c_char_p, []),
        "ce_gpu_ctx_create": (ci, [ci, vp, pp]),
        "ce_gpu_ctx_destroy": (ci, [vp]),
        "ce_gpu_ctx_set_stream": (ci, [vp, vp]),
        "ce_gpu_ctx_synchronize": (ci, [vp]),
        "ce_gpu_ctx_profile": (ci, [vp, ci]),
        "ce_gpu_ctx_profile_classes": (ci, [vp, ctypes.c_uint]),
        "ce_gpu_ctx_profile_read": (ci, [vp, ci, ctypes.POINTER(ctypes.c_double), pi64]),
        "ce_gpu_model_load_config": (ci, [vp, ctypes.c_char_p, pp]),
        "ce_gpu_model_load": (ci, [vp, ctypes.c_char_p, ctypes.c_char_p, ci, ci, pp]),
        "ce_gpu_model_info": (ci, [vp, pi, pi, pi, pi, pi, pi64]),
        "ce_gpu_model_tid2pdf": (ci, [vp, ctypes.POINTER(ctypes.c_int32), ci, pi]),
        "ce_gpu_model_destroy": (ci, [vp]),
        "ce_gpu_fbank_num_frames": (i64, [i64]),
        "ce_gpu_plan_create": (ci, [vp, vp, pi64, ci, ci, pp]),
        "ce_gpu_plan_info": (ci, [vp, pi, pi64, pi64, pi, pi]),
        "ce_gpu_plan_frame_offsets": (ci, [vp, pi64]),
        "ce_gpu_plan_destroy": (ci, [vp]),
        "ce_gpu_fbank": (ci, [vp, vp, vp, vp, vp]),
        "ce_gpu_fbank_s16": (ci, [vp, vp, vp, vp, vp]),
        "ce_gpu_cmvn": (ci, [vp, vp, vp, vp, vp]),
        "ce_gpu_am_forward": (ci, [vp, vp, vp, vp, vp]),
        "ce_gpu_score": (ci, [vp, vp, vp, vp, vp, vp, vp]),
        "ce_gpu_score_s16": (ci, [vp, vp, vp, vp, vp, vp, vp]),
        "ce_gpu_sgemm": (ci, [vp, ci, ci, ci, vp, ci, vp, ci, vp, ci]),
        "ce_gpu_quantize": (ci, [vp, vp, i64, vp, vp]),
        "ce_gpu_gemm_u8u8f32": (ci, [vp, ci, ci, ci, vp, vp, vp, vp, vp]),
        "ce_gpu_gemm_u8u8i32": (ci, [vp, ci, ci, ci, vp, vp, vp, vp, vp]),
        "ce_gpu_profile_anchor": (ci, [ci, vp]),
        "ce_gpu_trace_mark": (ci, [ci, vp, ci]),
        "ce_gpu_nnet_check_mem": (ci, [vp, i64, pi, pi, pi]),
        "ce_gpu_model_quantize": (ci, [vp, vp]),
        "ce_gpu_nnet_propagate_blocks": (ci, [vp, vp, vp, ci, ctypes.POINTER(ctypes.c_int32), ci, ci, vp]),
        "ce_gpu_ctx_profile_intervals": (ci, [vp, ci, vp, vp, ci, pi]),
        "ce_gpu_model_load_mem": (ci, [vp, vp, i64, vp, ci, ci, ci, pp]),
        "ce_gpu_nnet_propagate": (ci, [vp, vp, vp, ci, ci, ci, vp]),
        "ce_gpu_linear": (ci, [vp, ci, ci, ci, vp, ci, vp, ci, vp, vp, ci]),
        "ce_gpu_splice": (ci, [vp, ci, ci, vp, ci, ctypes.POINTER(ctypes.c_int32), ci, vp]),
        "ce_gpu_rowwise": (ci, [vp, ci, ci, ci, vp, ci, vp, vp]),
        "ce_gpu_loglik_gather": (ci, [vp, vp, ci, ci, ci, vp, ci, vp, vp, ci, ctypes.c_float, vp]),
        "ce_gpu_loglik_columns": (ci, [vp, vp, ci, ci, ci, vp, ci, vp]),
        "ce_gpu_model_set_gemm": (ci, [vp, ci]),
        "ce_gpu_model_get_gemm": (ci, [vp, pi]),
        "ce_gpu_gemm_mode_from_name": (ci, [ctypes.c_char_p, pi]),
        "ce_gpu_ctx_overflow": (ci, [vp, pi]),
        "ce_gpu_ctx_set_latency": (ci, [vp, ci]),
        "ce_gpu_ctx_set_fbank": (ci, [vp, ci]),
        "ce_gpu_ctx_set_wide_tiles": (ci, [vp, ci]),
        "ce_gpu_sum_f64": (ci, [vp, vp, i64, vp, vp]),
        "ce_gpu_sum_f64_many": (ci, [vp, ci, ctypes.POINTER(vp), pi64, vp, vp]),
        "ce_gpu_debug_counters": (ci, [pi64, pi64]),
        "ce_gpu_sessions_create": (ci, [vp, vp, vp, ci, ci, pp]),
        "ce_gpu_sessions_create_ex": (ci, [vp, vp, vp, ci, ci, ctypes.c_uint, pp]),
        "ce_gpu_sessions_stats": (ci, [vp, pi, pi64, pi64, pi64]),
        "ce_gpu_sessions_destroy": (ci, [vp]),
        "ce_gpu_sessions_reset": (ci, [vp, ci]),
        "ce_gpu_sessions_push": (ci, [vp, ci, pi32, pi32, pi32, vp, vp, i64, pi32]),
        "ce_gpu_sessions_push_s16": (ci, [vp, ci, pi32, pi32, pi32, vp, vp, i64, pi32]),
        "ce_gpu_quant_params_from_range": (ci, [ctypes.c_float, ctypes.c_float, ctypes.POINTER(ctypes.c_float), pi32]),
        "ce_gpu_model_calibrate": (ci, [vp, vp, vp, vp, ci, vp]),
        "ce_gpu_model_quantize_static": (ci, [vp, vp, vp, ci]),
        "ce_gpu_model_quant_params": (ci, [vp, vp, vp, ci, pi]),
        "ce_gpu_i8_latency_plan": (ci, [ci, ci, ci, pi, pi]),
        "ce_gpu_debug_i8_latency_launches": (ci, [pi64]),
        "ce_gpu_model_pad_widths": (ci, [vp, vp]),
        "ce_gpu_model_admit_row_ops": (ci, [vp, vp]),
        "ce_gpu_debug_rowop_chain": (ci, [vp, ci, vp, ci, ci, vp, ci, vp, vp, vp, ci, ci]),
        "ce_gpu_model_padded_widths": (ci, [vp, vp, vp, ci, pi]),
        "ce_gpu_debug_rowop_chain_q": (ci, [vp, ci, vp, ci, ci, vp, ci, vp, vp, ctypes.c_float, ctypes.c_int32, vp, ci,
                                            vp, vp]),
        "ce_gpu_debug_i8_static_launches": (ci, [pi64, pi64, pi64]),
        "ce_gpu_bf16_latency_max_rows": (ci, [pi]),
        "ce_gpu_debug_bf16_latency_launches": (ci, [pi64]),
        "ce_gpu_debug_fill_allocs": (ci, [ci, ctypes.c_uint32]),
        "ce_gpu_debug_fill_ctx": (ci, [vp, ctypes.c_uint32, pi64]),
        "ce_gpu_debug_fill_sessions": (ci, [vp, ctypes.c_uint32, ci, pi32]),
        "ce_gpu_plan_create_reusable": (ci, [vp, vp, ci, i64, ci, pp]),
        "ce_gpu_plan_assign": (ci, [vp, pi64, ci]),
        "ce_gpu_plan_capacity": (ci, [ci, i64, ci, ci, ci, pi64, pi64, pi64]),
        "ce_gpu_debug_plan_tables": (ci, [vp, ci, vp, i64, pi64]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def check(rc):
    if rc != CE_GPU_OK:
        raise CatearsError(rc, lib().ce_gpu_last_error().decode())
    return rc


def _ptr(t):
    """Device pointer of a torch tensor (or None)."""
    if t is None:
        return None
    if not t.is_cuda or not t.is_contiguous():
        raise ValueError("expected a contiguous device tensor")
    return ctypes.c_void_p(t.data_ptr())


def _ptr_rows(t):
    """Device pointer of a matrix argument that travels with its leading
    dimension (t.stride(0)): a 2-D device tensor whose rows are dense
    (stride(1) == 1) and do not overlap (stride(0) >= shape[1]).  The view may
    start at any element of its storage: the C-ABI asks for no alignment."""
    if t is None:
        return None
    if not t.is_cuda or t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1) or t.stride(0) < t.shape[1]:
        raise ValueError("expected a 2-D device tensor with dense rows (stride(1) == 1, stride(0) >= shape[1])")
    return ctypes.c_void_p(t.data_ptr())


class Context:
    """One device + one stream (defaults to torch's current stream)."""

    def __init__(self, device=0, stream=None):
        import torch
        self.device = device
        self._torch_stream = stream if stream is not None else torch.cuda.current_stream(device)
        h = ctypes.c_void_p()
        check(lib().ce_gpu_ctx_create(device, ctypes.c_void_p(self._torch_stream.cuda_stream),
                                      ctypes.byref(h)))
        self.h = h

    def set_stream(self, stream):
        self._torch_stream = stream
        check(lib().ce_gpu_ctx_set_stream(self.h, ctypes.c_void_p(stream.cuda_stream)))

    def synchronize(self):
        check(lib().ce_gpu_ctx_synchronize(self.h))

    def set_latency(self, on=True):
        """Latency mode (ce_gpu_ctx_set_latency): split-K nnet GEMMs for small
        row blocks scored one at a time.  Static int8 models take their
        split-K pair up to the crossover of i8_latency_plan (the same bits as
        off); plain bf16 models run row blocks of up to bf16_latency_max_rows()
        rows on the latency kernel (no split-K: the same bits as off); dynamic
        int8 ignores the mode."""
        check(lib().ce_gpu_ctx_set_latency(self.h, int(bool(on))))

    FBANK_MODES = {"exact": 0, "fast": 1}

    def set_wide_tiles(self, on=True):
        """128 x 128 bf16x6 tiles for every layer (ce_gpu_ctx_set_wide_tiles):
        all CUs per launch, for a batch scored while no other is in flight.
        Same bits as the default tiles."""
        check(lib().ce_gpu_ctx_set_wide_tiles(self.h, int(bool(on))))

    def set_fbank(self, mode="exact"):
        """Fbank kernel of this context (ce_gpu_ctx_set_fbank): "exact" (the
        reference's operation order, bit-exact pre-log energies) or "fast"
        (the same lane program with FMA contraction, ~12 % faster; as close
        to the exact result as the reference's own fp32 order,
        tests/test_gpu_fbank_fast.py)."""
        check(lib().ce_gpu_ctx_set_fbank(self.h, self.FBANK_MODES[mode]))

    def overflow(self):
        """True if an f16x3 GEMM met an out-of-range activation since the
        last call (synchronizes; ce_gpu_ctx_overflow)."""
        v = ctypes.c_int()
        check(lib().ce_gpu_ctx_overflow(self.h, ctypes.byref(v)))
        return bool(v.value)

    PROF_GEMM, PROF_GEMM_GATHER, PROF_FBANK, PROF_CMVN, PROF_FINALIZE, PROF_QUANT = range(6)

    def profile(self, enable=True, classes=None):
        """Time launches (HIP events); `classes`: iterable of PROF_* to time
        (default all)."""
        mask = 0xffffffff if classes is None else sum(1 << c for c in classes)
        check(lib().ce_gpu_ctx_profile_classes(self.h, mask))
        check(lib().ce_gpu_ctx_profile(self.h, int(enable)))

    def profile_read(self, cls):
        """(total_ms, launches) of a kernel class since the last read."""
        ms, n = ctypes.c_double(), ctypes.c_int64()
        check(lib().ce_gpu_ctx_profile_read(self.h, cls, ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, n.value

    def profile_intervals(self, cls):
        """[(start_ms, end_ms)] after the last profile_anchor(), per launch of a class."""
        n = ctypes.c_int()
        rc = lib().ce_gpu_ctx_profile_intervals(self.h, cls, None, None, 0, ctypes.byref(n))
        if rc != CE_GPU_OK and n.value == 0:
            check(rc)
        a = np.zeros(max(n.value, 1), np.float64)
        b = np.zeros_like(a)
        check(lib().ce_gpu_ctx_profile_intervals(self.h, cls, a.ctypes.data_as(ctypes.c_void_p),
                                                 b.ctypes.data_as(ctypes.c_void_p), len(a), ctypes.byref(n)))
        return list(zip(a[:n.value], b[:n.value]))

    def close(self):
        if getattr(self, "h", None):
            lib().ce_gpu_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Model:
    """config_path | (nnet, prior, left, right) files | image= NN02 bytes
    (+ optional prior probabilities, left/right default to the network's)."""

    def __init__(self, ctx, config_path=None, nnet=None, prior=None, left=None, right=None, image=None):
        h = ctypes.c_void_p()
        if config_path is not None:
            check(lib().ce_gpu_model_load_config(ctx.h, config_path.encode(), ctypes.byref(h)))
        elif image is not None:
            pr = None if prior is None else np.ascontiguousarray(prior, np.float32)
            buf = ctypes.create_string_buffer(bytes(image), len(image))
            check(lib().ce_gpu_model_load_mem(
                ctx.h, buf, len(image), None if pr is None else pr.ctypes.data_as(ctypes.c_void_p),
                0 if pr is None else pr.size, -1 if left is None else left, -1 if right is None else right,
                ctypes.byref(h)))
        else:
            check(lib().ce_gpu_model_load(ctx.h, nnet.encode(), prior.encode(), left, right,
                                          ctypes.byref(h)))
        self.h = h
        v = [ctypes.c_int() for _ in range(5)]
        p = ctypes.c_int64()
        check(lib().ce_gpu_model_info(h, *[ctypes.byref(x) for x in v], ctypes.byref(p)))
        self.left, self.right, self.input_dim, self.num_pdfs, self.num_linear = [x.value for x in v]
        self.num_params = p.value

    def quantize(self, ctx):
        """Switch to the int8 path (ce_gpu_model_quantize)."""
        check(lib().ce_gpu_model_quantize(ctx.h, self.h))
        return self

    def calibrate(self, ctx, plan, feats, ranges=None):
        """Per-Linear input (min, max) over the plan's utterances
        (ce_gpu_model_calibrate) -> (num_linear, 2) float32.  `ranges`: an
        earlier result to fold into (a corpus fed batch by batch)."""
        r = np.zeros((self.num_linear, 2), np.float32) if ranges is None else \
            np.array(ranges, np.float32).reshape(self.num_linear, 2)
        check(lib().ce_gpu_model_calibrate(ctx.h, self.h, plan.h, _ptr(feats), int(ranges is not None),
                                           r.ctypes.data_as(ctypes.c_void_p)))
        return r

    def quantize_static(self, ctx, ranges):
        """Switch to static int8: frozen activation parameters from the
        calibrated ranges (ce_gpu_model_quantize_static)."""
        r = np.ascontiguousarray(ranges, np.float32)
        if r.ndim != 2 or r.shape[1] != 2:
            raise ValueError("ranges must be (num_linear, 2)")
        check(lib().ce_gpu_model_quantize_static(ctx.h, self.h, r.ctypes.data_as(ctypes.c_void_p), r.shape[0]))
        return self

    def quant_params(self):
        """(scale float32[n], zero_point int32[n]) of a static int8 model
        (n = 0 otherwise; ce_gpu_model_quant_params)."""
        n = ctypes.c_int()
        check(lib().ce_gpu_model_quant_params(self.h, None, None, 0, ctypes.byref(n)))
        s, z = np.zeros(n.value, np.float32), np.zeros(n.value, np.int32)
        check(lib().ce_gpu_model_quant_params(self.h, s.ctypes.data_as(ctypes.c_void_p),
                                              z.ctypes.data_as(ctypes.c_void_p), n.value, ctypes.byref(n)))
        return s, z

    def pad_widths(self, ctx):
        """Re-lay the model onto padded layer widths (hidden widths to
        multiples of 32, the last to a multiple of 4, zero weights in the
        pads) so that every GEMM mode, latency mode and wide tiles take a net
        of any width; the model then is in the mode it would have loaded in.
        Nothing changes for a model already inside the envelope
        (ce_gpu_model_pad_widths)."""
        check(lib().ce_gpu_model_pad_widths(ctx.h, self.h))
        return self

    def admit_row_ops(self, ctx):
        """Admit the model's row steps (Normalize, Softmax, a post chain too
        long to fuse) to the matrix-core programs: the model then takes the
        modes fp32, bf16x6 and bf16, latency mode and pad_widths, and is in
        the mode it would have loaded in.  Nothing changes for a model
        without a row step (ce_gpu_model_admit_row_ops)."""
        check(lib().ce_gpu_model_admit_row_ops(ctx.h, self.h))
        return self

    def padded_widths(self):
        """(true int32[n], padded int32[n]): each Linear's output width as the
        net has it and as the model runs it (ce_gpu_model_padded_widths)."""
        n = ctypes.c_int()
        check(lib().ce_gpu_model_padded_widths(self.h, None, None, 0, ctypes.byref(n)))
        t, p = np.zeros(n.value, np.int32), np.zeros(n.value, np.int32)
        check(lib().ce_gpu_model_padded_widths(self.h, t.ctypes.data_as(ctypes.c_void_p),
                                               p.ctypes.data_as(ctypes.c_void_p), n.value, ctypes.byref(n)))
        return t, p

    def set_gemm(self, mode):
        """Matrix-core form of the fp32 Linear layers: "fp32" (fp32 MFMA),
        "bf16x6" (three-plane bf16 split on the way into LDS, six products),
        "bf16x6p" (the same with the planes stored in HBM; bit-identical),
        "f16x3" (two scaled fp16 planes, three products) or "bf16" (both
        operands rounded to bf16 once, one product, hidden activations kept
        as bf16: not fp32-accurate, never a default);
        ce_gpu_model_set_gemm."""
        check(lib().ce_gpu_model_set_gemm(self.h, GEMM_MODES[mode]))
        return self

    @property
    def gemm(self):
        v = ctypes.c_int()
        check(lib().ce_gpu_model_get_gemm(self.h, ctypes.byref(v)))
        return {b: a for a, b in GEMM_MODES.items()}[v.value]

    def tid2pdf(self):
        n = ctypes.c_int()
        check(lib().ce_gpu_model_tid2pdf(self.h, None, 0, ctypes.byref(n)))
        out = np.zeros(n.value, np.int32)
        check(lib().ce_gpu_model_tid2pdf(self.h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                         n.value, ctypes.byref(n)))
        return out

    def close(self):
        if getattr(self, "h", None):
            lib().ce_gpu_model_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def gemm_mode_from_name(name):
    """The ce_gpu_model_set_gemm number of a mode name
    (ce_gpu_gemm_mode_from_name; needs no device).  `name`: bytes, str or
    None (NULL)."""
    v = ctypes.c_int(-1)
    check(lib().ce_gpu_gemm_mode_from_name(name.encode() if isinstance(name, str) else name, ctypes.byref(v)))
    return v.value


def quant_params_from_range(mn, mx):
    """(scale, zero_point) of the reference's Quantize for a tensor with these
    extremes (ce_gpu_quant_params_from_range; needs no device)."""
    s, z = ctypes.c_float(), ctypes.c_int32()
    check(lib().ce_gpu_quant_params_from_range(float(mn), float(mx), ctypes.byref(s), ctypes.byref(z)))
    return np.float32(s.value), int(z.value)


def profile_anchor(device, stream):
    """Record the time origin for Context.profile_intervals on `stream`."""
    check(lib().ce_gpu_profile_anchor(device, ctypes.c_void_p(stream.cuda_stream)))


def nnet_check(image):
    """ce_gpu_nnet_check_mem: parse an NN02 image without a device; returns
    (num_layers, left, right) or raises CatearsError with the reference's
    message."""
    buf = bytes(image)
    n, l, r = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    check(lib().ce_gpu_nnet_check_mem(buf, len(buf), ctypes.byref(n), ctypes.byref(l), ctypes.byref(r)))
    return n.value, l.value, r.value


def trace_mark(device, stream, tag):
    """Launch the empty window-marker kernel with `tag` workgroups on `stream`
    (tools/trace_summary.py --window cuts a rocprofv3 kernel trace at it)."""
    check(lib().ce_gpu_trace_mark(device, ctypes.c_void_p(stream.cuda_stream), tag))


def union_ms(intervals):
    """Wall time covered by a set of (start, end) intervals."""
    total, cur_a, cur_b = 0.0, None, None
    for a, b in sorted(intervals):
        if cur_b is None or a > cur_b:
            if cur_b is not None:
                total += cur_b - cur_a
            cur_a, cur_b = a, b
        else:
            cur_b = max(cur_b, b)
    if cur_b is not None:
        total += cur_b - cur_a
    return total


def num_frames(n_samples):
    return lib().ce_gpu_fbank_num_frames(int(n_samples))


def _plan_capacity_args(max_utts, max_total_samples, max_rows):
    """The capacity of Plan.reusable as ints; ValueError for what
    ce_gpu_plan_create_reusable would refuse whatever the model."""
    max_utts, max_total_samples, max_rows = int(max_utts), int(max_total_samples), int(max_rows)
    if max_utts <= 0 or max_utts >= 2 ** 31:
        raise ValueError(f"max_utts must be in 1 .. 2^31 - 1, got {max_utts}")
    if max_total_samples <= 0 or max_total_samples >= 2 ** 63:
        raise ValueError(f"max_total_samples must be positive (and fit int64), got {max_total_samples}")
    if max_rows >= 2 ** 31:
        raise ValueError(f"max_rows must fit an int, got {max_rows}")
    return max_utts, max_total_samples, max_rows


def _plan_lengths(num_samples, max_utts, max_total_samples):
    """The lengths of Plan.assign as a contiguous int64 vector; ValueError
    for what ce_gpu_plan_assign would refuse (a negative length, more than
    max_utts utterances or max_total_samples samples) and for lengths that
    are no whole numbers."""
    a = np.asarray(num_samples)
    if a.ndim != 1:
        raise ValueError("num_samples must be a 1-D sequence of sample counts")
    if a.size and a.dtype.kind not in "iu":
        raise ValueError(f"num_samples must be integers, got dtype {a.dtype}")
    ns = np.ascontiguousarray(a, np.int64)
    if len(ns) > max_utts:
        raise ValueError(f"{len(ns)} utterances, the plan's max_utts is {max_utts}")
    if len(ns) and int(ns.min()) < 0:
        raise ValueError("negative sample count")
    if sum(int(n) for n in ns) > max_total_samples:
        raise ValueError(f"more than the plan's max_total_samples ({max_total_samples}) samples")
    return ns


def plan_capacity(max_utts, max_total_samples, left, right, max_rows=4096):
    """ce_gpu_plan_capacity: (frames, segments, packed rows) a reusable plan
    of this capacity reserves for a model of context (left, right).  Needs no
    device."""
    f, s, r = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    check(lib().ce_gpu_plan_capacity(int(max_utts), int(max_total_samples), int(max_rows), int(left), int(right),
                                     ctypes.byref(f), ctypes.byref(s), ctypes.byref(r)))
    return f.value, s.value, r.value


class Plan:
    def __init__(self, ctx, num_samples, model=None, max_rows=4096):
        ns = np.ascontiguousarray(num_samples, np.int64)
        h = ctypes.c_void_p()
        check(lib().ce_gpu_plan_create(ctx.h, model.h if model else None,
                                       ns.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                       len(ns), max_rows, ctypes.byref(h)))
        self.h = h
        self.is_reusable = False
        self._refresh()

    def _refresh(self):
        h = self.h
        a, d, e = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        b, c = ctypes.c_int64(), ctypes.c_int64()
        check(lib().ce_gpu_plan_info(h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c),
                                     ctypes.byref(d), ctypes.byref(e)))
        self.n_utt, self.total_samples, self.total_frames = a.value, b.value, c.value
        self.n_chunks, self.max_chunk_rows = d.value, e.value
        off = np.zeros(self.n_utt + 1, np.int64)
        check(lib().ce_gpu_plan_frame_offsets(h, off.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
        self.frame_offsets = off

    @classmethod
    def reusable(cls, ctx, max_utts, max_total_samples, model=None, max_rows=4096):
        """ce_gpu_plan_create_reusable: a plan for any lengths of at most
        `max_utts` utterances and `max_total_samples` samples in all, empty
        until assign().  Keeps a reference to `ctx`, which it is bound to."""
        max_utts, max_total_samples, max_rows = _plan_capacity_args(max_utts, max_total_samples, max_rows)
        self = cls.__new__(cls)
        self.h = None
        h = ctypes.c_void_p()
        check(lib().ce_gpu_plan_create_reusable(ctx.h, model.h if model else None, max_utts, max_total_samples,
                                                max_rows, ctypes.byref(h)))
        self.h = h
        self.is_reusable = True
        self.max_utts, self.max_total_samples = max_utts, max_total_samples
        self._ctx = ctx
        self._refresh()
        return self

    def assign(self, num_samples):
        """ce_gpu_plan_assign: replaces the lengths (stream-ordered, no
        allocation) and refreshes n_utt, total_samples, total_frames,
        n_chunks, max_chunk_rows and frame_offsets."""
        if not getattr(self, "is_reusable", False):
            raise ValueError("assign needs a plan from Plan.reusable (this one is immutable)")
        ns = _plan_lengths(num_samples, self.max_utts, self.max_total_samples)
        check(lib().ce_gpu_plan_assign(self.h, ns.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), len(ns)))
        self._refresh()
        return self

    def close(self):
        if getattr(self, "h", None):
            lib().ce_gpu_plan_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def fbank(ctx, plan, pcm, feats=None, mel=None):
    """Fbank::Process over the plan's utterances; `pcm` is float32 at raw
    int16 scale (ce_gpu_fbank) or int16 (ce_gpu_fbank_s16)."""
    import torch
    if feats is None:
        feats = torch.empty((plan.total_frames, 40), dtype=torch.float32, device=pcm.device)
    fn = lib().ce_gpu_fbank_s16 if pcm.dtype == torch.int16 else lib().ce_gpu_fbank
    if pcm.dtype not in (torch.int16, torch.float32):
        raise TypeError("pcm must be float32 or int16")
    check(fn(ctx.h, plan.h, _ptr(pcm), _ptr(feats), _ptr(mel)))
    return feats


def cmvn(ctx, plan, global_stats, feats, out=None):
    import torch
    if out is None:
        out = torch.empty_like(feats)
    check(lib().ce_gpu_cmvn(ctx.h, plan.h, _ptr(global_stats), _ptr(feats), _ptr(out)))
    return out


def am_forward(ctx, model, plan, feats, out=None):
    import torch
    if out is None:
        out = torch.empty((plan.total_frames, model.num_pdfs), dtype=torch.float32, device=feats.device)
    check(lib().ce_gpu_am_forward(ctx.h, model.h, plan.h, _ptr(feats), _ptr(out)))
    return out


def score(ctx, model, plan, pcm, global_stats=None, ws=None, out=None):
    import torch
    if ws is None:
        ws = torch.empty((2 * plan.total_frames * 40 + 1,), dtype=torch.float32, device=pcm.device)
    if out is None:
        out = torch.empty((plan.total_frames, model.num_pdfs), dtype=torch.float32, device=pcm.device)
    if pcm.dtype not in (torch.int16, torch.float32):
        raise TypeError("pcm must be float32 or int16")
    fn = lib().ce_gpu_score_s16 if pcm.dtype == torch.int16 else lib().ce_gpu_score
    check(fn(ctx.h, model.h, plan.h, _ptr(pcm), _ptr(global_stats), _ptr(ws), _ptr(out)))
    return out


SESSION_EOS = 1  # CE_GPU_SESSION_EOS
SESSIONS_INCREMENTAL = 1  # CE_GPU_SESSIONS_INCREMENTAL


def debug_counters():
    """ce_gpu_debug_counters: (device allocations, device releases) the
    library has made in this process so far."""
    a, f = ctypes.c_int64(), ctypes.c_int64()
    check(lib().ce_gpu_debug_counters(ctypes.byref(a), ctypes.byref(f)))
    return a.value, f.value


def i8_latency_plan(kpad, n, rows):
    """ce_gpu_i8_latency_plan: (slices, k_steps_per_slice) of a static int8
    Linear (K padded to kpad bytes, n outputs) on `rows` rows in latency
    mode; slices == 0 means the throughput kernel.  Needs no device."""
    s, per = ctypes.c_int(), ctypes.c_int()
    check(lib().ce_gpu_i8_latency_plan(int(kpad), int(n), int(rows), ctypes.byref(s), ctypes.byref(per)))
    return s.value, per.value


def debug_i8_latency_launches():
    """ce_gpu_debug_i8_latency_launches: split-K int8 GEMM launches of this
    process so far."""
    n = ctypes.c_int64()
    check(lib().ce_gpu_debug_i8_latency_launches(ctypes.byref(n)))
    return n.value


def bf16_latency_max_rows():
    """ce_gpu_bf16_latency_max_rows: the largest row block a plain bf16 Linear
    runs on the latency kernel on a latency context.  Needs no device."""
    n = ctypes.c_int()
    check(lib().ce_gpu_bf16_latency_max_rows(ctypes.byref(n)))
    return n.value


def debug_bf16_latency_launches():
    """ce_gpu_debug_bf16_latency_launches: plain bf16 latency GEMM launches of
    this process so far."""
    n = ctypes.c_int64()
    check(lib().ce_gpu_debug_bf16_latency_launches(ctypes.byref(n)))
    return n.value


def debug_i8_static_launches():
    """ce_gpu_debug_i8_static_launches: (quantize passes, row-step launches,
    row-step launches that stored the next Linear's bytes) the static int8
    program has enqueued in this process so far."""
    q, r, rq = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    check(lib().ce_gpu_debug_i8_static_launches(ctypes.byref(q), ctypes.byref(r), ctypes.byref(rq)))
    return q.value, r.value, rq.value


def debug_fill_allocs(on, word=0):
    """ce_gpu_debug_fill_allocs: while on, every device allocation the
    library makes in this process is filled with the 32-bit `word` before it
    is used (debug only; off by default)."""
    check(lib().ce_gpu_debug_fill_allocs(int(bool(on)), int(word) & 0xffffffff))


def debug_fill_ctx(ctx, word):
    """ce_gpu_debug_fill_ctx: fills the context's call-scoped device buffers
    (workspace, scratch, latency partials, block maps) with `word` on its
    stream; returns the bytes filled.  Debug only."""
    n = ctypes.c_int64()
    check(lib().ce_gpu_debug_fill_ctx(ctx.h, int(word) & 0xffffffff, ctypes.byref(n)))
    return n.value


def debug_fill_sessions(sessions, word, slots=()):
    """ce_gpu_debug_fill_sessions: fills the set's per-push scratch and every
    device region of the listed slots with `word` (a live slot's later rows
    are then garbage).  Debug only."""
    sl = np.ascontiguousarray(list(slots), np.int32)
    check(lib().ce_gpu_debug_fill_sessions(sessions.h, int(word) & 0xffffffff, len(sl),
                                           sl.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))))


PLAN_TABLES = (("sample_off", np.int64), ("frame_off", np.int64), ("block_utt", np.int32),
               ("row_src", np.int32), ("row_dst", np.int32), ("row_edge", np.uint32))


def debug_plan_tables(plan):
    """ce_gpu_debug_plan_tables: the plan's six device tables as numpy
    arrays by name (PLAN_TABLES), each as long as the current assignment
    uses.  Synchronizes the plan's context.  Debug only."""
    out = {}
    for which, (name, dtype) in enumerate(PLAN_TABLES):
        n = ctypes.c_int64()
        check(lib().ce_gpu_debug_plan_tables(plan.h, which, None, 0, ctypes.byref(n)))  # the length alone
        a = np.empty(n.value // np.dtype(dtype).itemsize, dtype)
        if n.value:
            check(lib().ce_gpu_debug_plan_tables(plan.h, which, a.ctypes.data_as(ctypes.c_void_p), a.nbytes,
                                                 ctypes.byref(n)))
        out[name] = a
    return out


class Sessions:
    """ce_gpu_sessions: `n_slots` live audio streams scored incrementally,
    their state (sample tail, CMVN sums and window, nnet context) on the
    device.  `global_stats`: the 41-float device tensor of ce_gpu_cmvn, or
    None for no CMVN.  One per context.

    `incremental` (CE_GPU_SESSIONS_INCREMENTAL): the set caches every layer's
    context rows per slot, so a push packs k + H nnet rows per slot instead
    of k + L + R (`packed_rows`); the same rows, counts and order."""

    MAX_CHUNK_ROWS = 4096  # packed rows per launch sequence

    def __init__(self, ctx, model, n_slots, max_chunk_samples, global_stats=None, incremental=False):
        self.ctx, self.model = ctx, model
        self.n_slots, self.max_chunk_samples = int(n_slots), int(max_chunk_samples)
        self._gstats = global_stats  # the library keeps the pointer
        self._state = [(0, 0, False)] * self.n_slots  # (samples, rows emitted, ended) per slot
        self.incremental = bool(incremental)
        h = ctypes.c_void_p()
        if incremental:
            check(lib().ce_gpu_sessions_create_ex(ctx.h, model.h, _ptr(global_stats), self.n_slots,
                                                  self.max_chunk_samples, SESSIONS_INCREMENTAL, ctypes.byref(h)))
        else:
            check(lib().ce_gpu_sessions_create(ctx.h, model.h, _ptr(global_stats), self.n_slots,
                                               self.max_chunk_samples, ctypes.byref(h)))
        self.h = h

    def stats(self):
        """ce_gpu_sessions_stats: host counters since create, as a dict --
        lead_rows (H; 0 when not incremental), pushes, packed_rows, chunks."""
        lead, pushes, packed, chunks = ctypes.c_int(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        check(lib().ce_gpu_sessions_stats(self.h, ctypes.byref(lead), ctypes.byref(pushes), ctypes.byref(packed),
                                          ctypes.byref(chunks)))
        return {"lead_rows": lead.value, "pushes": pushes.value, "packed_rows": packed.value, "chunks": chunks.value}

    @staticmethod
    def packed_rows(L, R, H, sample_counts, eos_at, incremental):
        """The packed nnet rows each push of one slot costs (the schedule()
        arguments; a push's total is the sum over its slots).  Not
        incremental: a push that emits r rows packs them with L + R context
        rows, once per piece when they do not fit one chunk of 4096 rows.
        Incremental: a push feeds positions -- L copies of frame 0 with the
        slot's first frame, its new frames, R copies of the last frame at
        the end -- behind H lead rows per piece.  Pure arithmetic."""
        frames_out, rows_out = Sessions.schedule(L, R, sample_counts, eos_at)
        ctx = H if incremental else L + R
        room = Sessions.MAX_CHUNK_ROWS - ctx
        out, frames = [], 0
        for i, (f, r) in enumerate(zip(frames_out, rows_out)):
            if incremental:
                eos = eos_at is not None and i == eos_at
                k = f + (L if frames == 0 and f > 0 else 0) + (R if eos and frames + f > 0 else 0)
            else:
                k = r
            frames += f
            out.append(k + -(-k // room) * ctx)
        return out

    @staticmethod
    def _advance(right, samples, rows, count, eos):
        """One push of `count` samples to a slot that has `samples` samples
        and `rows` emitted rows: (samples, frames completed, rows emitted,
        rows total) after it."""
        before = 0 if samples < 400 else 1 + (samples - 400) // 160
        samples += count
        frames = 0 if samples < 400 else 1 + (samples - 400) // 160
        total = frames if eos else max(0, frames - right)
        return samples, frames - before, total - rows, total

    @staticmethod
    def schedule(L, R, sample_counts, eos_at):
        """What a slot's pushes produce: ([frames completed by push i],
        [rows emitted by push i]) for pushes of sample_counts[i] samples, the
        push of index `eos_at` (None: none) carrying the end of the
        utterance.  A push emits every row whose R rows of right context
        exist (all remaining rows at the end); the left context L delays
        nothing (it clamps to frame 0).  Pure arithmetic, no device."""
        samples = rows = 0
        frames_out, rows_out = [], []
        for i, c in enumerate(sample_counts):
            if eos_at is not None and i > eos_at:
                raise ValueError("push after the end of the utterance")
            samples, f, r, rows = Sessions._advance(R, samples, rows, int(c), eos_at is not None and i == eos_at)
            frames_out.append(f)
            rows_out.append(r)
        return frames_out, rows_out

    def push(self, slots, pcm, counts, eos=None, out=None):
        """Advance `slots` (distinct) by counts[i] new samples each, laid back
        to back in the device tensor `pcm` (float32 at raw int16 scale, or
        int16); eos[i] true ends slot i's utterance.  Returns (loglik, rows):
        the newly complete rows of push 0, then push 1, ... and the row
        count of each push.  `out`: a (>= rows, num_pdfs) device tensor to
        write into (a view of its first rows is returned)."""
        import torch
        n = len(slots)
        sl = np.ascontiguousarray(slots, np.int32)
        cn = np.ascontiguousarray(counts, np.int32)
        fl = np.zeros(n, np.int32) if eos is None else np.ascontiguousarray(
            [SESSION_EOS if e else 0 for e in eos], np.int32)
        assert len(cn) == n and len(fl) == n
        after, need = {}, 0
        for i in range(n):
            k = int(sl[i])
            if 0 <= k < self.n_slots and not self._state[k][2] and k not in after:
                s, _, r, total = self._advance(self.model.right, self._state[k][0], self._state[k][1], int(cn[i]),
                                               bool(fl[i]))
                after[k] = (s, total, bool(fl[i]))
                need += r
        if pcm is not None and pcm.dtype not in (torch.int16, torch.float32):
            raise TypeError("pcm must be float32 or int16")
        dev = pcm.device if pcm is not None else torch.device("cuda", self.ctx.device)
        if out is None:
            out = torch.empty((max(need, 1), self.model.num_pdfs), dtype=torch.float32, device=dev)
        rows = np.zeros(n, np.int32)
        fn = lib().ce_gpu_sessions_push_s16 if pcm is not None and pcm.dtype == torch.int16 else lib().ce_gpu_sessions_push
        p32 = ctypes.POINTER(ctypes.c_int32)
        check(fn(self.h, n, sl.ctypes.data_as(p32), cn.ctypes.data_as(p32), fl.ctypes.data_as(p32), _ptr(pcm),
                 _ptr(out), out.shape[0], rows.ctypes.data_as(p32)))
        for k, st in after.items():
            self._state[k] = st
        return out[:int(rows.sum())], rows

    def reset(self, slot):
        """The slot starts a new utterance."""
        check(lib().ce_gpu_sessions_reset(self.h, int(slot)))
        self._state[int(slot)] = (0, 0, False)

    def close(self):
        if getattr(self, "h", None):
            lib().ce_gpu_sessions_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def nnet_propagate(ctx, model, x, subtract_prior=False, out=None):
    """Nnet::Propagate on one padded block (+ the AM's prior subtraction)."""
    import torch
    net_l, net_r = model.left, model.right
    rows = x.shape[0]
    if out is None:
        out = torch.empty((max(rows - net_l - net_r, 0), model.num_pdfs), dtype=torch.float32, device=x.device)
    check(lib().ce_gpu_nnet_propagate(ctx.h, model.h, _ptr_rows(x), rows, x.stride(0), int(subtract_prior), _ptr(out)))
    return out


def nnet_propagate_blocks(ctx, model, x, block_rows, subtract_prior=False, out=None):
    """ce_gpu_nnet_propagate_blocks: independent padded blocks back to back."""
    import torch
    rows = np.ascontiguousarray(block_rows, np.int32)
    n_out = int(rows.sum()) - len(rows) * (model.left + model.right)
    if out is None:
        out = torch.empty((n_out, model.num_pdfs), dtype=torch.float32, device=x.device)
    check(lib().ce_gpu_nnet_propagate_blocks(ctx.h, model.h, _ptr_rows(x), x.stride(0),
                                             rows.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), len(rows),
                                             int(subtract_prior), _ptr(out)))
    return out


def loglik_gather(ctx, loglik, tid2pdf, rows, trans, am_scale=1.0, out=None):
    """ce_gpu_loglik_gather: am_scale * loglik[rows[i], tid2pdf[trans[i]]]
    (Decoder::LogLikelihood for n pairs); int32 device tensors."""
    import torch
    n = int(rows.numel())
    assert trans.numel() == n and rows.dtype == trans.dtype == tid2pdf.dtype == torch.int32
    if out is None:
        out = torch.empty((n,), dtype=torch.float32, device=loglik.device)
    check(lib().ce_gpu_loglik_gather(ctx.h, _ptr_rows(loglik), loglik.shape[0], loglik.stride(0), loglik.shape[1],
                                     _ptr(tid2pdf),
                                     int(tid2pdf.numel()), _ptr(rows), _ptr(trans), n, float(am_scale),
                                     _ptr(out)))
    return out


def loglik_columns(ctx, loglik, cols, out=None):
    """ce_gpu_loglik_columns: loglik[:, cols] compacted (int32 device cols)."""
    import torch
    assert cols.dtype == torch.int32
    if out is None:
        out = torch.empty((loglik.shape[0], int(cols.numel())), dtype=torch.float32, device=loglik.device)
    check(lib().ce_gpu_loglik_columns(ctx.h, _ptr_rows(loglik), loglik.shape[0], loglik.stride(0), loglik.shape[1],
                                      _ptr(cols), int(cols.numel()), _ptr(out)))
    return out


SUM_PARTS = 1024  # CE_GPU_SUM_PARTS


def sum_f64(x, acc, part):
    """ce_gpu_sum_f64 on torch's current stream: acc (a 0-d float64 device
    tensor) += the float64 sum of the contiguous float32 tensor x; part: a
    float64 device tensor of >= SUM_PARTS elements (scratch, stream-ordered)."""
    import torch
    assert x.dtype == torch.float32 and x.is_contiguous() and x.is_cuda
    assert acc.dtype == torch.float64 and acc.numel() == 1 and part.dtype == torch.float64
    assert part.numel() >= SUM_PARTS
    stream = torch.cuda.current_stream(x.device).cuda_stream
    check(lib().ce_gpu_sum_f64(stream, _ptr(x), x.numel(), _ptr(part), _ptr(acc)))
    return acc


SUM_MAX_BUFS = 16  # CE_GPU_SUM_MAX_BUFS


def sum_f64_many(xs, acc, part):
    """ce_gpu_sum_f64_many on torch's current stream: acc += the float64 sum
    of every contiguous float32 tensor in xs, SUM_MAX_BUFS at a time (one
    launch pair per group)."""
    import torch
    assert acc.dtype == torch.float64 and acc.numel() == 1 and part.dtype == torch.float64
    assert part.numel() >= SUM_PARTS
    stream = torch.cuda.current_stream(acc.device).cuda_stream
    for g in range(0, len(xs), SUM_MAX_BUFS):
        grp = xs[g:g + SUM_MAX_BUFS]
        for x in grp:
            assert x.dtype == torch.float32 and x.is_contiguous() and x.is_cuda
        ptrs = (ctypes.c_void_p * len(grp))(*[_ptr(x) for x in grp])
        ns = (ctypes.c_int64 * len(grp))(*[x.numel() for x in grp])
        check(lib().ce_gpu_sum_f64_many(stream, len(grp), ptrs, ns, _ptr(part), _ptr(acc)))
    return acc


def sgemm(ctx, a, b, c=None):
    import torch
    m, k = a.shape
    n = b.shape[1]
    if c is None:
        c = torch.empty((m, n), dtype=torch.float32, device=a.device)
    check(lib().ce_gpu_sgemm(ctx.h, m, n, k, _ptr_rows(a), a.stride(0), _ptr_rows(b), b.stride(0), _ptr_rows(c),
                             c.stride(0)))
    return c


ROW_OPS = {"relu": 0, "batchnorm": 1, "log_softmax": 2, "softmax": 3, "normalize": 4}  # CE_GPU_ROW_*


def linear(ctx, x, w, bias=None, out=None):
    """ce_gpu_linear: x (rows, in_dim) @ w (in_dim, out_dim) + bias, each
    matrix with its own leading dimension."""
    import torch
    rows, in_dim = x.shape
    out_dim = w.shape[1]
    assert w.shape[0] == in_dim
    if out is None:
        out = torch.empty((rows, out_dim), dtype=torch.float32, device=x.device)
    check(lib().ce_gpu_linear(ctx.h, rows, in_dim, out_dim, _ptr_rows(x), x.stride(0), _ptr_rows(w), w.stride(0),
                              _ptr(bias), _ptr_rows(out), out.stride(0)))
    return out


def splice(ctx, x, indices, out=None):
    """ce_gpu_splice: row r of the result is x[clamp(r + i)] for i in
    `indices`, side by side (the reference's clamped Splice); dense output."""
    import torch
    rows, dim = x.shape
    idx = np.ascontiguousarray(indices, np.int32)
    if out is None:
        out = torch.empty((rows, dim * len(idx)), dtype=torch.float32, device=x.device)
    check(lib().ce_gpu_splice(ctx.h, rows, dim, _ptr_rows(x), x.stride(0),
                              idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), len(idx), _ptr(out)))
    return out


def rowwise(ctx, op, x, scale=None, offset=None):
    """ce_gpu_rowwise in place on the rows of x; op: a ROW_OPS name."""
    check(lib().ce_gpu_rowwise(ctx.h, ROW_OPS[op], x.shape[0], x.shape[1], _ptr_rows(x), x.stride(0), _ptr(scale),
                               _ptr(offset)))
    return x


def rowop_chain(ctx, ops, x, dim=None, vectors=None, out16=None):
    """ce_gpu_debug_rowop_chain: the row ops `ops` (ROW_OPS names, at most 4)
    in one launch on the first `dim` columns of x's rows, in place;
    vectors[q] = (scale, offset) for a BatchNorm.  out16: an int16 / uint16 /
    bfloat16 device tensor of x's rows that takes the rows as bf16 instead
    (all its columns).  Returns out16 if given, else x."""
    dim = x.shape[1] if dim is None else dim
    n = len(ops)
    kinds = (ctypes.c_int * max(n, 1))(*[ROW_OPS[o] for o in ops])
    sc = (ctypes.c_void_p * max(n, 1))(*[_ptr(vectors[q][0]) if vectors and vectors[q] else None for q in range(n)])
    of = (ctypes.c_void_p * max(n, 1))(*[_ptr(vectors[q][1]) if vectors and vectors[q] else None for q in range(n)])
    o16, ld16, w16 = (None, 0, 0) if out16 is None else (_ptr_rows(out16), out16.stride(0), out16.shape[1])
    check(lib().ce_gpu_debug_rowop_chain(ctx.h, n, kinds, x.shape[0], dim, _ptr_rows(x), x.stride(0), sc, of, o16,
                                         ld16, w16))
    return x if out16 is None else out16


def debug_rowop_chain_q(ctx, ops, x, scale, zero_point, q, rowsum, zero, vectors=None):
    """ce_gpu_debug_rowop_chain_q: the row ops `ops` (ROW_OPS names, at most
    4; none: a pure quantize) on the rows of x, which then leave as the next
    Linear's shifted bytes under (scale, zero_point) in q (an int8 device
    tensor of x's rows, at least x's columns wide: the columns behind are
    written as 0), their sums in rowsum[r] with zero[r] cleared (int32 device
    vectors).  Returns q."""
    n = len(ops)
    kinds = (ctypes.c_int * max(n, 1))(*[ROW_OPS[o] for o in ops])
    sc = (ctypes.c_void_p * max(n, 1))(*[_ptr(vectors[i][0]) if vectors and vectors[i] else None for i in range(n)])
    of = (ctypes.c_void_p * max(n, 1))(*[_ptr(vectors[i][1]) if vectors and vectors[i] else None for i in range(n)])
    check(lib().ce_gpu_debug_rowop_chain_q(ctx.h, n, kinds, x.shape[0], x.shape[1], _ptr_rows(x), x.stride(0), sc, of,
                                           float(scale), int(zero_point), _ptr_rows(q), q.stride(0), _ptr(rowsum),
                                           _ptr(zero)))
    return q


def quantize(ctx, x, q=None):
    """Returns (uint8 tensor, 8-byte device params tensor {f32 scale, i32 zp});
    `q`: a contiguous uint8 device tensor of x's element count to write into."""
    import torch
    if q is None:
        q = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    assert q.dtype == torch.uint8 and q.numel() == x.numel()
    prm = torch.empty(2, dtype=torch.int32, device=x.device)
    check(lib().ce_gpu_quantize(ctx.h, _ptr(x), x.numel(), _ptr(q), _ptr(prm)))
    return q, prm


def params_host(prm):
    """(scale, zero_point) of a device params record."""
    raw = prm.cpu().numpy()
    return float(raw[:1].view(np.float32)[0]), int(raw[1])


def gemm_u8(ctx, a, pa, b, pb, out_int32=False):
    import torch
    m, k = a.shape
    n = b.shape[1]
    if out_int32:
        c = torch.empty((m, n), dtype=torch.int32, device=a.device)
        check(lib().ce_gpu_gemm_u8u8i32(ctx.h, m, n, k, _ptr(a), _ptr(pa), _ptr(b), _ptr(pb), _ptr(c)))
    else:
        c = torch.empty((m, n), dtype=torch.float32, device=a.device)
        check(lib().ce_gpu_gemm_u8u8f32(ctx.h, m, n, k, _ptr(a), _ptr(pa), _ptr(b), _ptr(pb), _ptr(c)))
    return c
