"""Round 11 took instructions out of the render loop's trip without touching its arithmetic (profiles/r11/trip_slots.md): the
tolerance unit's axis-signature kernels keep a sphere's centre, normal row and kd * 2^24 in ONE 64-byte LDS row
(csrc/rtm_path.h: SceneLdsRows), the tolerance row's sin / cos table is a variable of the code object, and the wall-pair proof
transfers a sign with one v_bitop3_b32.  Here: every table kernel's layout on all-sphere scenes of 1 .. 24 spheres — the exact-n
kernels, the generic n < 8 kernel, the chunked kernel with one full chunk, chunk plus tail and the largest LDS table —, variants
0, 2 and 18 against variant 1 (reference math, global scene) and the CPU oracle; and the Cornell box through the headline
instantiation itself (test_wall_pairs_gpu.py's shapes), variant 18 against variant 0 and the oracle with 0 differing pixels.

The sample split and the stealing knobs are read once per process, so those frames render in a child process per setting: this
file run as a script."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_VARIANT = 18
NORTH_STAR_TOL = 1e-4  # tests/test_tolerance_gpu.py
COUNTERS = ("samples", "casts", "bounces", "draws")
SPHERE_COUNTS = [1, 3, 7, 8, 9, 16, 24]


@pytest.fixture(scope="module")
def rtm():
    import raytracingmin_amd as m
    return m


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _sphere_scene(rtm, n):
    """n spheres with distinct colours (kd), radii and centres off every axis; sphere 0 encloses the others and the camera, glows
    and reflects (every ray hits something, a path bounces until the roulette ends it).  Seeded: the same scene in every process."""
    from raytracingmin_amd import Camera, Material, SettingData, SphereObject, vec3
    rng = np.random.default_rng(1100 + n)
    objs = [SphereObject(vec3(0.7, 1.5, 0.9), 30.0 + 0.01 * n, Material(vec3(0.55, 0.6, 0.65), vec3(0.5, 0.45, 0.4)))]
    for k in range(1, n):
        c = rng.uniform(-3.5, 3.5, 3)
        c = np.where(np.abs(c) < 0.05, 0.05, c)  # off-axis: no zero coordinate
        r = 0.45 + 0.9 * k / n + 0.001 * k       # distinct radii
        col = 0.25 + 0.7 * rng.random(3)         # distinct kd
        objs.append(SphereObject(vec3(*c), float(r), Material(vec3(*col), vec3(0, 0, 0))))
    cam = Camera(vec3(0.3, -0.4, -11.0), vec3(0.1, 0.2, 0.0), vec3(0, 1, 0), 1.2)
    return SettingData(width=16, height=16, samples=4, superSamples=2, camera=cam, object=objs)


def _render(rtm, data, mb, seed, variant):
    out, st = rtm.Renderer(data, mode="repaired", max_bounces=mb, seed=seed, variant=variant).render_rows_device(want=("f64",))
    return out["f64"].cpu().numpy(), st


def _oracle_frame(oracle, data, mb, seed):
    st_c, arr_c, n = data.to_c()
    ost, oarr = oracle.Settings.from_buffer_copy(bytes(st_c)), (oracle.Sphere * max(n, 1)).from_buffer_copy(bytes(arr_c))
    return oracle.render(ost, oarr, n, oracle.make_options(mode=oracle.MODE_REPAIRED, max_bounces=mb, seed=seed, row_begin=0,
                                                           row_end=data.height))


@pytest.mark.parametrize("mb", [8, -1])
@pytest.mark.parametrize("n", SPHERE_COUNTS)
def test_every_table_kernels_layout(rtm, oracle, n, mb):
    """16x16, S 4, SS 2: variants 0 and 2 are variant 1's and the oracle's frame bit for bit, variant 18 is within 1e-4 of both;
    casts, bounces and draws equal everywhere"""
    data = _sphere_scene(rtm, n)
    ref, cnt = _oracle_frame(oracle, data, mb, 0x5EED + n)
    img1, st1 = _render(rtm, data, mb, 0x5EED + n, 1)
    assert st1["variant"] == 1
    assert ref.max() > 0.0 and cnt["bounces"] > 0  # light arrives and paths bounce: the shading block's look-ups ran
    assert np.array_equal(_bits(img1), _bits(ref))
    for variant in (0, 2, TOL_VARIANT):
        img, st = _render(rtm, data, mb, 0x5EED + n, variant)
        assert variant == 0 or st["variant"] == variant
        differing = int((_bits(img) != _bits(img1)).any(axis=-1).sum())
        worst = max(float(np.max(np.abs(img - img1))), float(np.max(np.abs(img - ref))))
        print(f"n {n}, cap {mb}, variant {variant} (ran {st['variant']}): {differing} of 256 pixels differ from variant 1, "
              f"max |delta| {worst:.3e}, casts {st['casts']} / {st1['casts']} / oracle {cnt['casts']}")
        if variant == TOL_VARIANT:
            assert worst <= NORTH_STAR_TOL, (n, mb)
        else:
            assert differing == 0 and np.array_equal(_bits(img), _bits(ref)), (n, mb, variant)
        assert {k: st[k] for k in COUNTERS} == {k: st1[k] for k in COUNTERS} == {k: cnt[k] for k in COUNTERS}, (n, mb, variant)


# ---- the headline instantiation: Cornell box, depth-capped, with and without the split -------------------------------------------
def _cornell(rtm, w, h, s, ss):
    import _oracle
    data = rtm.LoadData(_oracle.scene_path("cornellBoxSetting.json")).data
    data.width, data.height, data.samples, data.superSamples = w, h, s, ss
    return data


def _check_frames(what, ref, cnt, img0, st0, img18, st18):
    differing0 = int((_bits(img0) != _bits(ref)).any(axis=-1).sum())
    differing18 = int((_bits(img18) != _bits(ref)).any(axis=-1).sum())
    differing = int((_bits(img18) != _bits(img0)).any(axis=-1).sum())
    print(f"{what}: variant 0 — {differing0} pixels differ from the oracle; variant 18 — {differing18} from the oracle, {differing} from "
          f"variant 0, of {ref.shape[0] * ref.shape[1]}; casts {st18['casts']} / {st0['casts']} / oracle {cnt['casts']}")
    assert differing0 == 0 and differing18 == 0 and differing == 0, what
    assert {k: st0[k] for k in COUNTERS} == {k: cnt[k] for k in COUNTERS} == {k: st18[k] for k in COUNTERS}, what


@pytest.mark.parametrize("mb", [8, 1])
def test_cornell_through_the_headline_kernel(rtm, oracle, mb):
    """40x24 (ragged tiles), S 4, SS 2, caps 8 and 1"""
    data = _cornell(rtm, 40, 24, 4, 2)
    ref, cnt = _oracle_frame(oracle, data, mb, 0x5EED)
    img0, st0 = _render(rtm, data, mb, 0x5EED, 0)
    img18, st18 = _render(rtm, data, mb, 0x5EED, TOL_VARIANT)
    assert st18["variant"] == TOL_VARIANT and ref.max() > 0.0
    _check_frames(f"Cornell 40x24, cap {mb}", ref, cnt, img0, st0, img18, st18)


SPLIT_FRAME = dict(w=64, h=16, s=16, ss=2, mb=8, seed=77)  # (tests/test_wall_pairs_gpu.py: 16 tiles, 64 samples per pixel)
SPLIT_SETTINGS = {
    "whole tiles, stealing": ({"RTM_DEBUG_TAIL": "0", "RTM_DEBUG_STEAL": "1"}, False),    # main loop + tail loop + steal_finalize
    "whole tiles, no stealing": ({"RTM_DEBUG_TAIL": "0", "RTM_DEBUG_STEAL": "0"}, False), # main loop to the end
    "8 whole + 8 split tiles": ({"RTM_DEBUG_TAIL": "8", "RTM_DEBUG_STEAL": "1"}, True),   # all three loops in one launch
    "every tile split 8 ways": ({"RTM_DEBUG_SPLIT": "8"}, True),                          # head waves + small waves of 8 samples
}


def _child(out_path):
    """(script mode) renders SPLIT_FRAME with variants 0 and 18 under this process's knobs."""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import raytracingmin_amd as m
    f = SPLIT_FRAME
    data = _cornell(m, f["w"], f["h"], f["s"], f["ss"])
    res = {}
    for variant in (0, TOL_VARIANT):
        img, st = _render(m, data, f["mb"], f["seed"], variant)
        res[f"img{variant}"] = img
        res[f"stats{variant}"] = np.array(json.dumps({k: st[k] for k in COUNTERS + ("variant", "split")}))
    np.savez(out_path, **res)


@pytest.fixture(scope="module")
def split_reference(oracle):
    f = SPLIT_FRAME
    st, arr, n = oracle.load_scene(oracle.scene_path("cornellBoxSetting.json"), width=f["w"], height=f["h"], samples=f["s"],
                                   super_samples=f["ss"])
    return oracle.render(st, arr, n, oracle.make_options(mode=1, max_bounces=f["mb"], seed=f["seed"], height=f["h"]))


@pytest.mark.parametrize("setting", list(SPLIT_SETTINGS))
def test_cornell_split_and_stealing_loops(split_reference, tmp_path, setting):
    ref, cnt = split_reference
    env = {k: v for k, v in os.environ.items() if not k.startswith("RTM_DEBUG_")}
    knobs, is_split = SPLIT_SETTINGS[setting]
    env.update(knobs)
    out_path = str(tmp_path / "frames.npz")
    subprocess.run([sys.executable, os.path.abspath(__file__), out_path], env=env, check=True, timeout=120, cwd=ROOT)
    z = np.load(out_path)
    st, ts = json.loads(str(z["stats0"])), json.loads(str(z["stats18"]))
    assert ts["variant"] == TOL_VARIANT
    for got in (st["split"], ts["split"]):  # the knobs took effect: rtm_stats.split is the launch's waves per split tile
        assert (got > 1) if is_split else (got == 1), setting
    _check_frames(setting, ref, cnt, z["img0"], st, z["img18"], ts)


if __name__ == "__main__":
    _child(sys.argv[1])
