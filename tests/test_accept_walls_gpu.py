"""Round 15 (profiles/r15/accept_walls.md) on the device: the acceptance of the tolerance row's wall-pair search without a far-root
sum for a pair's wall (csrc/rtm_path.h: accept_batch_lane's WALLS; variant 18's pairs kernels).

Probe ops 61 / 62 of rtm_debug_math_probe (op 55's search, a wave holds 8 rays): the acceptance as the render kernels run it against
the form with t2 for every candidate, on the ray families of tests/_accept_walls_model.py (65 536 rays each; the families that
exist as (b, sq, idx) records alone are tests/test_accept_walls_host.py's) and on tests/_wall_pairs_model.py's grazing, flat,
into-a-second-wall and non-finite sets, which bring NaN roots, zero direction components and small b to the device: distance and hit
id bit for bit, the same chain in every wave, the general chain only behind the second question.
Frames: variant 18 against variant 0 and the CPU oracle, every pixel within 1e-4 (expected and printed: 0 pixels differ), `casts`,
`bounces`, `draws` equal; each says which kernel it ran through the host's hooks (tests/_tol_frames.py).

The sample split and the stealing knobs are read once per process, so those frames render in a child process per setting: this
file run as a script."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _accept_walls_model as A
import _wall_pairs_model as W
import _tol_frames as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_VARIANT = 18
OP_WALLS, OP_T2 = 61, 62
N_RAYS = A.PER_FAMILY


@pytest.fixture(scope="module")
def rtm():
    import raytracingmin_amd as m
    return m


@pytest.fixture(scope="module")
def ray_sets():
    bx, fam = A.ray_families()
    more = W.ray_sets(N_RAYS // 6 * 6 + 6, 2015, bx["c"], bx["r2"], bx["cam"], bx["target"])
    for name in ("grazing", "flat", "into_a_second_wall", "non_finite"):
        fam[name] = (more[name][0][:N_RAYS], more[name][1][:N_RAYS])
    return bx, fam


def _probe(rtm, op, table, org, dir):
    m = org.shape[0]
    a = np.zeros((m, 8))
    a[:, 0:3], a[:, 3:6] = org, dir
    b = np.zeros(a.size)
    b[:table.size] = table
    a = np.ascontiguousarray(a)
    out = np.full_like(a, np.nan)
    rtm._lib.check(rtm.lib().rtm_debug_math_probe(op, a.ctypes.data, b.ctypes.data, a.size, out.ctypes.data), "probe")
    assert not out[:, 5:].any()
    return out[:, 0].copy(), out[:, 1].astype(np.int64), out[:, 2] != 0.0, out[:, 3] != 0.0, out[:, 4] != 0.0


SETS = ["bounce", "primary", "gap_1e-3", "gap_1e-6", "gap_0", "grazing", "flat", "into_a_second_wall", "non_finite"]


@pytest.mark.parametrize("name", SETS)
def test_both_acceptance_forms_agree_bit_for_bit(rtm, ray_sets, name):
    bx, fam = ray_sets
    org, dir = fam[name]
    assert org.shape == (N_RAYS, 3)
    dis_w, hit_w, gen_w, block_w, again_w = _probe(rtm, OP_WALLS, bx["table"], org, dir)
    dis_t, hit_t, gen_t, block_t, again_t = _probe(rtm, OP_T2, bx["table"], org, dir)
    dis_p, hit_p, block_p, _, _ = _probe(rtm, 55, bx["table"], org, dir)
    print(f"{name}: rays in a wave that took the seven-sphere block {int(block_w.sum())}, the general chain {int(gen_w.sum())}, asked "
          f"again {int(again_w.sum())} (for nothing: {int((again_w & ~gen_w).sum())}) of {N_RAYS}; ids {np.unique(hit_w).tolist()}")
    assert np.array_equal(A.bits(dis_w), A.bits(dis_t)) and np.array_equal(hit_w, hit_t), name
    assert np.array_equal(A.bits(dis_w), A.bits(dis_p)) and np.array_equal(hit_w, hit_p), name  # op 55 IS op 61's search
    assert np.array_equal(gen_w, gen_t) and np.array_equal(block_w, block_t) and np.array_equal(block_w, block_p), name
    assert not again_t.any(), name                     # the form with t2 has no second question
    assert bool((again_w | ~gen_w).all()), name        # the general chain only behind it
    assert not (block_w & (gen_w | again_w)).any(), name  # a wave in the block never reaches this acceptance
    for flag in (gen_w, block_w, again_w):             # every decision is the wave's
        waves = flag.reshape(-1, 8)
        assert bool((waves.all(axis=1) | ~waves.any(axis=1)).all()), name
    if name in ("bounce", "primary"):
        assert not (again_w & ~gen_w).any(), name      # tests/test_accept_walls_host.py: none in the model either
        # ... and the pairs acceptance did run: a wave of 8 shuffled rays gets there when all 8 prove their pairs
        proven = A.candidates(bx, org, dir)[3].mean()
        assert (~block_w).mean() > 0.5 * proven ** 8 > 0.1, (name, proven)
    if name in ("gap_1e-6", "gap_0"):
        assert gen_w[~block_w].all() and (~block_w).any(), name  # every ray starts on the wall it enters: a far root in every wave
    if name != "non_finite":
        assert np.unique(hit_w).size >= 3, name


# ---- frames ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mb", [8, 1])
def test_cornell_through_the_pairs_kernel(rtm, oracle, mb):
    """40x24 (ragged tiles), S 4, SS 2, caps 8 and 1: the depth-capped axis-signature kernel with the pairs"""
    data = F.cornell(rtm, 40, 24, 4, 2)
    assert F.through_the_pairs_kernels(rtm, data)
    ref, cnt = F.oracle_frame(oracle, data, mb, 0x5EED)
    img0, st0 = F.render(rtm, data, mb, 0x5EED, 0)
    img18, st18 = F.render(rtm, data, mb, 0x5EED, TOL_VARIANT)
    assert st18["variant"] == TOL_VARIANT and ref.max() > 0.0 and cnt["bounces"] > 0
    F.check_frames(f"Cornell 40x24, S 4, cap {mb}", ref, cnt, img0, st0, img18, st18)


def test_camera_a_hair_in_front_of_a_wall(rtm, oracle):
    """32x32 from a camera 5e-4 in front of the +x wall, looking along it: the rays that head for that wall reach it within 0.001
    where they are steep enough — far roots, the general chain —, the others start a hair from the wall behind them (the
    seven-sphere block); bounce rays go through the packed minimum"""
    from raytracingmin_amd import vec3
    data = F.cornell(rtm, 32, 32, 4, 1)
    data.camera.origin = vec3(10.0 - 5e-4, 0.5, -3.0)
    data.camera.target = vec3(10.0 - 5e-4, 0.5, 3.0)
    assert F.through_the_pairs_kernels(rtm, data)
    ref, cnt = F.oracle_frame(oracle, data, 8, 23)
    img0, st0 = F.render(rtm, data, 8, 23, 0)
    img18, st18 = F.render(rtm, data, 8, 23, TOL_VARIANT)
    assert st18["variant"] == TOL_VARIANT and ref.max() > 0.0
    F.check_frames("camera 5e-4 in front of the +x wall", ref, cnt, img0, st0, img18, st18)


def test_simple_setting_keeps_its_own_kernel(rtm, oracle):
    """simpleSetting1.json 32x32: five spheres, no shared K and no pairs — the axis-signature kernel `-6285`, whose acceptance is
    accept_batch's and whose code this round does not touch"""
    data = F.scene(rtm, "simpleSetting1.json", 32, 32, 4, 2)
    assert len(data.object) == 5 and not F.through_the_pairs_kernels(rtm, data) and F.axis_signature_launch(rtm, data, F.SIG_SIMPLE5)
    ref, cnt = F.oracle_frame(oracle, data, 8, 0x5EED)
    img0, st0 = F.render(rtm, data, 8, 0x5EED, 0)
    img18, st18 = F.render(rtm, data, 8, 0x5EED, TOL_VARIANT)
    assert st18["variant"] == TOL_VARIANT and cnt["bounces"] > 0
    F.check_frames("simpleSetting1.json 32x32", ref, cnt, img0, st0, img18, st18)


def test_off_axis_scene_keeps_the_exact_n_kernel(rtm, oracle):
    """seven spheres off every axis: no signature, the exact-n kernel `-107` (untouched)"""
    data = F.off_axis_scene(rtm, 7)
    assert len(data.object) == 7 and F.no_signature(rtm, data)
    ref, cnt = F.oracle_frame(oracle, data, 8, 0x5EED + 7)
    img0, st0 = F.render(rtm, data, 8, 0x5EED + 7, 0)
    img18, st18 = F.render(rtm, data, 8, 0x5EED + 7, TOL_VARIANT)
    assert st18["variant"] == TOL_VARIANT and cnt["bounces"] > cnt["samples"]
    F.check_frames("off-axis scene, cap 8", ref, cnt, img0, st0, img18, st18)


SPLIT_FRAME = F.SPLIT_FRAME  # 64x16, S 16, SS 2, cap 8
SPLIT_SETTINGS = {
    "split forced, stealing on": ({"RTM_DEBUG_SPLIT": "8", "RTM_DEBUG_STEAL": "1"}, True),   # head waves + small waves
    "split off, stealing on": ({"RTM_DEBUG_TAIL": "0", "RTM_DEBUG_STEAL": "1"}, False),      # main loop + tail loop
    "split off, stealing off": ({"RTM_DEBUG_TAIL": "0", "RTM_DEBUG_STEAL": "0"}, False),     # main loop to the end
    "8 whole + 8 split tiles": ({"RTM_DEBUG_TAIL": "8", "RTM_DEBUG_STEAL": "1"}, True),      # all three loops in one launch
}


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
    F.check_frames(setting, ref, cnt, z["img0"], st, z["img18"], ts)


if __name__ == "__main__":
    F.child(sys.argv[1])
