"""AddressSanitizer + UBSan run of the grade's host-only code (csrc/rtm_lut.cpp: the .cube reader and the white balance
matrix; csrc/rtm_grade_index.h: the LUT's index arithmetic, the function the kernel compiles): a stand-alone program of its
own, no library and no device (sanitizers are for host code only).  It reads well-formed files, every malformed family, a
valid file cut at every byte of its first 200, and checks the index function on 0, -0, denormals, N - 1 +- 1 ulp, +-3.4e38,
+-inf and NaN for every N in 2..256."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lut_reader_and_index_under_asan_ubsan(tmp_path):
    d = os.path.join(ROOT, "raytracingmin_amd", "csrc")
    subprocess.check_call(["make", "-C", d, "lut_selftest_asan"], stdout=subprocess.DEVNULL)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([os.path.join(d, "lut_selftest_asan"), str(tmp_path)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "lut selftest ok" in r.stdout
