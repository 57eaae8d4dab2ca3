"""The configuration key gpu_int8_ranges on the host (no GPU): model_io.cc's
read_int8_ranges -- the configuration reader plus the VEC0 reader plus the
pair check, what ce_gpu_model_load_config runs before it touches the device
-- built alone under AddressSanitizer + UndefinedBehaviorSanitizer as a
stand-alone program (tests/native/ranges_fuzz.cc, `make sanitize`) and fed a
valid file, every truncation, odd and empty lists, oversized headers and
seeded random corruptions."""
import os
import subprocess

from conftest import ROOT


def test_ranges_key_parser_under_sanitizers(tmp_path):
    exe = os.path.join(ROOT, "build", "bin", "ranges_fuzz_asan")
    subprocess.check_call(["make", "-C", ROOT, "-s", exe[len(ROOT) + 1:]], stdout=subprocess.DEVNULL)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, str(tmp_path), "3000"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "PASSED" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
