"""AddressSanitizer + UBSan run of the scene proofs and the host grid builder (csrc/rtm_scene_facts.cpp, with the loader
csrc/rtm_scene.cpp): a stand-alone program of the two units, no library and no device (sanitizers are for host code only)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scene_facts_under_asan_ubsan():
    d = os.path.join(ROOT, "raytracingmin_amd", "csrc")
    subprocess.check_call(["make", "-C", d, "scene_facts_selftest_asan"], stdout=subprocess.DEVNULL)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([os.path.join(d, "scene_facts_selftest_asan"), os.path.join(ROOT, "scenes")], capture_output=True,
                       text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "scene facts selftest ok" in r.stdout
