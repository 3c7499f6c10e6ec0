"""Round 13 (profiles/r13/merged_mix.md): in the deferred-fold loops of the tolerance unit's axis-signature kernels a lane whose
path ends opens its next sample's stream inside the mix32 pair of the bounce's two draws (csrc/rtm_device.h: rng_merged_mix;
csrc/rtm_path.h: path_shade_core_reopen), and the empty record word is a constant of those kernels.  No word of any stream, no
draw, no counter and no bit of a result changes.

Probe ops 57 / 58 of rtm_debug_math_probe (one lane per record): the merged helper against plain rng_next_mi / rng_next /
rng_open, 65 536 seeded lanes, with the two kinds of lane mixed inside every wave.  Frames: variant 18 against variant 0 and the
CPU oracle with equal counters.  THROUGH THE MERGED LOOPS (the axis-signature kernels, which only the Cornell box's geometry
selects here: _through_the_axis_kernels; and of those every shape but any depth with the sample split: _merged_shape, from
rtm_stats.split): the Cornell box at caps 8 and 1 and, at 12 samples a pixel so that no split is planned, unlimited; with the
sample split and the stealing forced and off, in two passes cut inside a sub-pixel, at a width that leaves lanes outside the
frame (0 pixels differ); and the merged pair's two extremes — the box at cap 0, where every path ends at its first cast and every
lane restarts in every trip, and the box with every reflectance at 0.99 (cap 8) and 0.9 (any depth, again 12 samples a pixel),
where almost every lane continues (within 1e-4).
THROUGH THE KERNELS THAT KEEP THE PARENT'S CODE (they must not have moved): the box with no cap at 16 samples a pixel (the
any-depth kernel with the split), the camera turned away from a lone small sphere (one sphere: the generic n < 8 kernel) and the
all-hit scene of tests/test_trip_slots_gpu.py (7 off-axis spheres: the exact-n kernel).

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
PHI = 0x9E3779B9


@pytest.fixture(scope="module")
def rtm():
    import raytracingmin_amd as m
    return m


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ---- the probe ops ------------------------------------------------------------------------------------------------------------------
LANES = 65536
PATTERNS = ["all continue", "all end", "one of each kind", "alternating"]


def _probe(rtm, op, a):
    out = np.full(a.shape, np.nan)
    rtm._lib.check(rtm.lib().rtm_debug_math_probe(op, a.ctypes.data, None, a.size, out.ctypes.data), "probe")
    return out


def _ended(pattern):
    lane, wave = np.arange(LANES) % 64, np.arange(LANES) // 64
    if pattern == "all continue":
        return np.zeros(LANES, bool)
    if pattern == "all end":
        return np.ones(LANES, bool)
    if pattern == "one of each kind":  # one ended lane among 63 continuing ones, and the other way round; the odd lane moves
        return (lane == wave % 64) ^ (wave % 2 == 1)
    return lane % 2 == 1


@pytest.fixture(scope="module")
def words():
    rng = np.random.default_rng(1302)
    w = rng.integers(0, 2 ** 32, (LANES, 4), dtype=np.uint64).astype(np.float64)  # p0, p1, ctr, k1
    n_next = rng.integers(0, 65536, LANES).astype(np.float64)
    n_next[:6] = [0, 1, 15, 16, 65535, 37]
    return w, n_next


@pytest.mark.parametrize("pattern", PATTERNS)
def test_merged_helper_is_the_plain_calls(rtm, words, pattern):
    w, n_next = words
    ended = _ended(pattern)
    a = np.zeros((LANES, 8))
    a[:, :4], a[:, 4], a[:, 5] = w, n_next, ended
    a = np.ascontiguousarray(a.reshape(-1))
    merged, plain = _probe(rtm, 57, a).reshape(LANES, 8), _probe(rtm, 58, a).reshape(LANES, 8)
    assert np.array_equal(merged.view(np.uint64), plain.view(np.uint64))
    # ... and what both hold is what the pattern asked for: draws for a continuing lane, none for an ended one, a moved stream
    assert np.all(merged[ended, :2] == 0.0) and np.all(merged[~ended, 0] % 2 == 1) and np.all(merged[~ended, 1] % 2 == 1)
    ctr3 = (w[:, 2].astype(np.uint64) + 3 * PHI) % 2 ** 32
    assert np.array_equal(merged[~ended, 2], ctr3[~ended].astype(np.float64)) and np.array_equal(merged[~ended, 3], w[~ended, 3])
    if ended.any():
        assert not np.array_equal(merged[ended, 3], w[ended, 3])
    assert np.all(merged[:, 4:] == 0.0)


# ---- frames ---------------------------------------------------------------------------------------------------------------------------
def _cornell(rtm, w, h, s, ss):
    import _oracle
    data = rtm.LoadData(_oracle.scene_path("cornellBoxSetting.json")).data
    data.width, data.height, data.samples, data.superSamples = w, h, s, ss
    return data


def _render(rtm, data, mb, seed, variant):
    out, st = rtm.Renderer(data, mode="repaired", max_bounces=mb, seed=seed, variant=variant).render_rows_device(want=("f64",))
    return out["f64"].cpu().numpy(), st


def _oracle_frame(oracle, data, mb, seed):
    st_c, arr_c, n = data.to_c()
    ost, oarr = oracle.Settings.from_buffer_copy(bytes(st_c)), (oracle.Sphere * max(n, 1)).from_buffer_copy(bytes(arr_c))
    return oracle.render(ost, oarr, n, oracle.make_options(mode=oracle.MODE_REPAIRED, max_bounces=mb, seed=seed, row_begin=0,
                                                           row_end=data.height))


def _through_the_axis_kernels(rtm, data):
    """What ties a frame to the kernels round 13 changed: variant 18 takes an axis-signature instantiation (UNROLL <= -1000, the only
    ones with the merged pair: csrc/rtm_render_kernel.h, kAxisTolShape) for a scene of the Cornell box's seven spheres — the
    signature, the shared K, the opposite pairs and the envelope of the expanded form are facts of the GEOMETRY, which the host
    grants as a whole in rtm_debug_wall_pairs — in repaired mode from a camera inside it (csrc/rtm_kernels_tol.hip: launch_n).  So:
    the box's own geometry and camera, whatever the materials, and the grant.  That is the UNROLL; the SHAPE decides too (_merged_shape)."""
    import ctypes as C
    box = _cornell(rtm, data.width, data.height, data.samples, data.superSamples)
    geometry = lambda d: [(tuple(o.m_position), o.m_size) for o in d.object] + [tuple(d.camera.origin), tuple(d.camera.target),
                                                                                 tuple(d.camera.upVec), d.camera.fov]
    _, arr, n = data.to_c()
    out = (C.c_uint64 * 2)()
    rtm._lib.check(rtm.lib().rtm_debug_wall_pairs(arr, n, out), "wall pairs")
    return n == 7 and geometry(data) == geometry(box) and int(out[0]) == 1


def _merged_shape(mb, st18):
    """... and of the axis-signature kernels the any-depth shape (no cap, or one above 8) WITH the sample split keeps the parent's
    loop (kAxisTolShape leaves kPackL | kSplit out).  A launch splits whenever the pass's samples per pixel admit shares of at least
    8 (csrc/rtm_kernels.hip: choose_split) — 16 do, 12 do not —; rtm_stats.split says what this launch did."""
    any_depth = mb < 0 or mb > 8
    return not (any_depth and st18["split"] > 1)


def _check_frames(what, ref, cnt, img0, st0, img18, st18):
    differing0 = int((_bits(img0) != _bits(ref)).any(axis=-1).sum())
    differing18 = int((_bits(img18) != _bits(ref)).any(axis=-1).sum())
    differing = int((_bits(img18) != _bits(img0)).any(axis=-1).sum())
    print(f"{what}: variant 0 — {differing0} pixels differ from the oracle; variant 18 — {differing18} from the oracle, {differing} from "
          f"variant 0, of {ref.shape[0] * ref.shape[1]}; casts {st18['casts']} / {st0['casts']} / oracle {cnt['casts']}")
    assert differing0 == 0 and differing18 == 0 and differing == 0, what
    assert {k: st0[k] for k in COUNTERS} == {k: cnt[k] for k in COUNTERS} == {k: st18[k] for k in COUNTERS}, what


@pytest.mark.parametrize("w,h,s,mb", [(40, 24, 4, 8), (40, 24, 4, 1), (40, 24, 3, -1), (43, 16, 4, 8)])
def test_cornell_through_the_merged_loops(rtm, oracle, w, h, s, mb):
    """SS 2: ragged tiles at 40x24, lanes outside the frame at 43x16 (W no multiple of 8); caps 8 and 1 at S 4 (the depth-capped
    kernel with the split), unlimited at S 3: 12 samples a pixel admit no split, so the launch is the any-depth axis kernel WITHOUT
    the split — the one any-depth shape that has the merged pair"""
    data = _cornell(rtm, w, h, s, 2)
    assert _through_the_axis_kernels(rtm, data)
    ref, cnt = _oracle_frame(oracle, data, mb, 0x5EED)
    img0, st0 = _render(rtm, data, mb, 0x5EED, 0)
    img18, st18 = _render(rtm, data, mb, 0x5EED, TOL_VARIANT)
    assert st18["variant"] == TOL_VARIANT and ref.max() > 0.0
    assert _merged_shape(mb, st18) and (mb >= 0 or st18["split"] == 1)
    _check_frames(f"Cornell {w}x{h}, S {s}, cap {mb}", ref, cnt, img0, st0, img18, st18)


def test_any_depth_with_the_sample_split_keeps_the_parents_loop(rtm, oracle):
    """40x24, S 4, SS 2, no cap: 16 samples a pixel are split in two, and the any-depth axis kernel with the split has neither of
    round 13's items (scratch: profiles/r13/merged_mix.md §4) — what this frame holds is that that kernel did not move"""
    data = _cornell(rtm, 40, 24, 4, 2)
    ref, cnt = _oracle_frame(oracle, data, -1, 0x5EED)
    img0, st0 = _render(rtm, data, -1, 0x5EED, 0)
    img18, st18 = _render(rtm, data, -1, 0x5EED, TOL_VARIANT)
    assert st18["variant"] == TOL_VARIANT and st18["split"] > 1 and not _merged_shape(-1, st18)
    _check_frames("Cornell 40x24, S 4, no cap (split)", ref, cnt, img0, st0, img18, st18)


def test_every_lane_restarts_in_every_trip_of_the_merged_loop(rtm, oracle):
    """the Cornell box at cap 0 through the headline instantiation: every path ends at its first cast (the depth cap: no draw), so
    in every trip all 64 lanes are `ended` lanes of the merged pair and take its words as their next sample's stream — 16 restarts
    a lane, across the sub-pixel changes"""
    data = _cornell(rtm, 40, 24, 4, 2)
    assert _through_the_axis_kernels(rtm, data)
    ref, cnt = _oracle_frame(oracle, data, 0, 0x5EED)
    assert cnt["bounces"] == 0 and cnt["draws"] == 0 and cnt["casts"] == cnt["samples"] and ref.max() > 0.0
    img0, st0 = _render(rtm, data, 0, 0x5EED, 0)
    img18, st18 = _render(rtm, data, 0, 0x5EED, TOL_VARIANT)
    assert st18["variant"] == TOL_VARIANT and _merged_shape(0, st18)
    _check_frames("Cornell 40x24, cap 0", ref, cnt, img0, st0, img18, st18)


@pytest.mark.parametrize("kd,mb,s", [(0.99, 8, 4), (0.9, -1, 3)])
def test_almost_every_lane_continues_in_the_merged_loop(rtm, oracle, kd, mb, s):
    """the Cornell box's geometry with every reflectance at kd (the light's too): at 0.99 under cap 8 a path all but always runs
    to the cap (the depth-capped axis kernel: 8 of 9 casts continue), at 0.9 with no cap paths go 9 deep on average and far past
    16 (the any-depth axis kernel, pooled stack included; S 3 — 12 samples a pixel — so that no split is planned and the launch is
    the shape with the merged pair) — nearly all lanes of a trip are `continuing` lanes of the pair.
    16x16, SS 2.  Within 1e-4 of variant 0 and of the oracle, counters equal."""
    from raytracingmin_amd import vec3
    data = _cornell(rtm, 16, 16, s, 2)
    for o in data.object:
        o.m_material.color = vec3(kd, kd, kd)
    assert _through_the_axis_kernels(rtm, data)
    ref, cnt = _oracle_frame(oracle, data, mb, 0x5EED)
    assert cnt["bounces"] > 0.85 * cnt["casts"] and ref.max() > 0.0
    img0, st0 = _render(rtm, data, mb, 0x5EED, 0)
    img18, st18 = _render(rtm, data, mb, 0x5EED, TOL_VARIANT)
    assert st18["variant"] == TOL_VARIANT
    assert _merged_shape(mb, st18) and (mb >= 0 or st18["split"] == 1)
    worst = max(float(np.max(np.abs(img18 - img0))), float(np.max(np.abs(img18 - ref))))
    print(f"reflectance {kd}, cap {mb}: max |delta| {worst:.3e}, {cnt['bounces'] / cnt['casts']:.3f} of the casts continue, "
          f"max depth {cnt['max_depth']}")
    assert np.array_equal(_bits(img0), _bits(ref))
    assert worst <= NORTH_STAR_TOL
    assert {k: st0[k] for k in COUNTERS} == {k: cnt[k] for k in COUNTERS} == {k: st18[k] for k in COUNTERS}


SPLIT_FRAME = dict(w=64, h=16, s=16, ss=2, mb=8, seed=77)  # (tests/test_trip_slots_gpu.py: 16 tiles, 64 samples per pixel)
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


def test_two_passes_cut_inside_a_sub_pixel(rtm, split_reference):
    """samples [0, 37) and [37, 64) of SPLIT_FRAME (S 16: the cut is inside the third sub-pixel; a lane past the first pass's end
    stays at n_end = 37): the accumulator after the second pass is the single pass's frame and the oracle's, counters summed"""
    import torch
    ref, cnt = split_reference
    f = SPLIT_FRAME
    data = _cornell(rtm, f["w"], f["h"], f["s"], f["ss"])
    r = rtm.Renderer(data, mode="repaired", max_bounces=f["mb"], seed=f["seed"], variant=TOL_VARIANT)
    single, st1 = r.render_rows_device(want=("f64",))
    accum = torch.empty((f["h"], f["w"], 3), dtype=torch.float64, device=single["f64"].device)
    total = {k: 0 for k in COUNTERS}
    for a, b in ((0, 37), (37, 64)):
        _, st = r.render_samples_device(a, b, accum, want=())
        assert st["variant"] == TOL_VARIANT
        for k in COUNTERS:
            total[k] += st[k]
    two = accum.cpu().numpy()
    assert np.array_equal(_bits(two), _bits(single["f64"].cpu().numpy()))
    assert np.array_equal(_bits(two), _bits(ref))
    assert total == {k: st1[k] for k in COUNTERS} == {k: cnt[k] for k in COUNTERS}


def test_every_path_ends_at_its_first_cast(rtm, oracle):
    """the camera turned away from a lone small glowing sphere: every cast misses, every lane restarts in every trip.  One sphere
    has no axis-signature kernel: this frame runs the generic n < 8 kernel, which keeps the parent's code (its restart still
    calls rng_open) — what it holds is that the kernels round 13 left alone did not move.  The same extreme through the merged
    loop: test_every_lane_restarts_in_every_trip_of_the_merged_loop."""
    from raytracingmin_amd import Camera, Material, SettingData, SphereObject, vec3
    objs = [SphereObject(vec3(0.0, 0.0, 5.0), 0.5, Material(vec3(0.7, 0.7, 0.7), vec3(1.0, 1.0, 1.0)))]
    cam = Camera(vec3(0.0, 0.0, 0.0), vec3(0.0, 0.0, -1.0), vec3(0, 1, 0), 1.0)
    data = SettingData(width=24, height=16, samples=4, superSamples=2, camera=cam, object=objs)
    assert not _through_the_axis_kernels(rtm, data)
    ref, cnt = _oracle_frame(oracle, data, 8, 0x5EED)
    assert cnt["bounces"] == 0 and cnt["draws"] == 0 and cnt["casts"] == cnt["samples"] and ref.max() == 0.0
    img0, st0 = _render(rtm, data, 8, 0x5EED, 0)
    img18, st18 = _render(rtm, data, 8, 0x5EED, TOL_VARIANT)
    assert st18["variant"] == TOL_VARIANT
    _check_frames("every path ends at its first cast", ref, cnt, img0, st0, img18, st18)


def _all_hit_scene(rtm):
    """tests/test_trip_slots_gpu.py's scene of 7 spheres: sphere 0 encloses the others and the camera, glows and reflects — every
    ray hits something and a path bounces until the roulette ends it"""
    from raytracingmin_amd import Camera, Material, SettingData, SphereObject, vec3
    n = 7
    rng = np.random.default_rng(1100 + n)
    objs = [SphereObject(vec3(0.7, 1.5, 0.9), 30.0 + 0.01 * n, Material(vec3(0.55, 0.6, 0.65), vec3(0.5, 0.45, 0.4)))]
    for k in range(1, n):
        c = rng.uniform(-3.5, 3.5, 3)
        c = np.where(np.abs(c) < 0.05, 0.05, c)
        r = 0.45 + 0.9 * k / n + 0.001 * k
        col = 0.25 + 0.7 * rng.random(3)
        objs.append(SphereObject(vec3(*c), float(r), Material(vec3(*col), vec3(0, 0, 0))))
    cam = Camera(vec3(0.3, -0.4, -11.0), vec3(0.1, 0.2, 0.0), vec3(0, 1, 0), 1.2)
    return SettingData(width=16, height=16, samples=4, superSamples=2, camera=cam, object=objs)


@pytest.mark.parametrize("mb", [8, -1])
def test_all_hit_scene_almost_every_lane_continues(rtm, oracle, mb):
    """(seven spheres off every axis: the exact-n kernel, which keeps the parent's code too — as above; through the merged loop:
    test_almost_every_lane_continues_in_the_merged_loop)"""
    data = _all_hit_scene(rtm)
    assert not _through_the_axis_kernels(rtm, data)
    ref, cnt = _oracle_frame(oracle, data, mb, 0x5EED + 7)
    img0, st0 = _render(rtm, data, mb, 0x5EED + 7, 0)
    img18, st18 = _render(rtm, data, mb, 0x5EED + 7, TOL_VARIANT)
    assert st18["variant"] == TOL_VARIANT and cnt["bounces"] > cnt["samples"]
    worst = max(float(np.max(np.abs(img18 - img0))), float(np.max(np.abs(img18 - ref))))
    print(f"all-hit scene, cap {mb}: max |delta| {worst:.3e}, bounces per sample {cnt['bounces'] / cnt['samples']:.2f}")
    assert np.array_equal(_bits(img0), _bits(ref))
    assert worst <= NORTH_STAR_TOL
    assert {k: st0[k] for k in COUNTERS} == {k: cnt[k] for k in COUNTERS} == {k: st18[k] for k in COUNTERS}


if __name__ == "__main__":
    _child(sys.argv[1])
