"""The weight images' host arithmetic (no GPU): csrc/weight_images.cc -- the
bf16 / fp16 conversions, the bf16 plane and fragment images, the fp16 planes,
the int8 image and ce_gpu_model_pad_widths' re-layout -- built alone under
AddressSanitizer + UndefinedBehaviorSanitizer as a stand-alone program
(tests/native/weight_images_test.cc, `make sanitize`) that checks them against
the formats' definitions and the layouts the kernel headers document."""
import os
import subprocess

from conftest import ROOT


def test_weight_images_under_sanitizers():
    exe = os.path.join(ROOT, "build", "bin", "weight_images_asan")
    subprocess.check_call(["make", "-C", ROOT, "-s", exe[len(ROOT) + 1:]], stdout=subprocess.DEVNULL)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "PASSED" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
