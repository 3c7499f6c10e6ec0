"""The bookkeeping of a trip of the deferred-fold render loops (csrc/rtm_render_kernel.h, round 6): the running sub-pixel
index that replaced n / S, lane masks formed by compares and combined as scalars, the two-instruction emitter test
(zero_term_queued) and the carry-in add of the sample counter.  None of it may move a bit or a counter: variant 0 is compared
with the CPU oracle BIT FOR BIT with equal counters, variant 18 (the tolerance row) with variant 0 of the same run under
north_star's bar of 1e-4 per pixel with equal counters.  Frames are 40x24 — ragged tiles — unless a test says otherwise.

The sample split and the stealing knobs (RTM_DEBUG_SPLIT / RTM_DEBUG_TAIL / RTM_DEBUG_STEAL) are read once per process, so
that test renders in a child process per setting: this file run as a script."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NORTH_STAR_TOL = 1e-4
TOL_VARIANT = 18
COUNTERS = ("samples", "casts", "bounces", "draws")
W, H = 40, 24


@pytest.fixture(scope="module")
def rtm():
    import raytracingmin_amd as m
    return m


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _cornell(rtm, w=W, h=H, s=4, ss=2):
    import _oracle
    data = rtm.LoadData(_oracle.scene_path("cornellBoxSetting.json")).data
    data.width, data.height, data.samples, data.superSamples = w, h, s, ss
    return data


def _oracle_view(oracle, data):
    st, arr, n = data.to_c()
    return oracle.Settings.from_buffer_copy(bytes(st)), (oracle.Sphere * max(n, 1)).from_buffer_copy(bytes(arr)), n


def _render(rtm, data, mode, mb, seed, variant=0, rows=None, band=None, skip=True):
    r = rtm.Renderer(data, mode=mode, max_bounces=mb, seed=seed, variant=variant)
    rb, re = rows if rows else (0, data.height)
    if not skip:
        os.environ["RTM_DEBUG_ZERO_SKIP"] = "0"
    try:
        out, st = r.render_rows_device(rb, re, want=("f64",), band=band)
    finally:
        os.environ.pop("RTM_DEBUG_ZERO_SKIP", None)
    assert st["variant"] == TOL_VARIANT or variant != TOL_VARIANT
    return out["f64"].cpu().numpy(), st


def _check_exact(what, img, st, ref, cnt):
    differing = int((_bits(img) != _bits(ref)).any(axis=-1).sum())
    print(f"{what}: variant 0 — {differing} pixels differ from the oracle; casts {st['casts']} vs {cnt['casts']}")
    assert differing == 0, what
    assert {k: st[k] for k in COUNTERS} == {k: cnt[k] for k in COUNTERS}, what


def _check_tol(what, tol, ts, img, st):
    differing = int((_bits(tol) != _bits(img)).any(axis=-1).sum())
    both_nan = np.isnan(tol) & np.isnan(img)
    worst = float(np.max(np.where(both_nan, 0.0, np.abs(tol - img)))) if tol.size else 0.0
    print(f"{what}: variant 18 — {differing} pixels differ from variant 0, max |difference| {worst:.3e}; casts {ts['casts']} vs {st['casts']}")
    assert worst <= NORTH_STAR_TOL, what
    assert np.array_equal(np.isnan(tol), np.isnan(img)), what
    assert {k: ts[k] for k in COUNTERS} == {k: st[k] for k in COUNTERS}, what


def _both(what, rtm, oracle, data, mode, mb, seed, rows=None, band=None, skip=True, tol=True):
    """variant 0 against the oracle, variant 18 against variant 0; returns variant 0's (image, stats)."""
    ost, oarr, n = _oracle_view(oracle, data)
    rb, re = rows if rows else (0, data.height)
    if band is not None:  # the image rows of the band: one 8-row band here, so a contiguous range the oracle renders as rows
        from raytracingmin_amd.distributed import band_row_index
        idx = list(band_row_index(rb, re, band[0], band[1]))
        assert idx == list(range(idx[0], idx[-1] + 1))
        rb, re = idx[0], idx[-1] + 1
    opt = oracle.make_options(mode=oracle.MODE_LITERAL if mode == "literal" else oracle.MODE_REPAIRED, max_bounces=mb, seed=seed,
                              row_begin=rb, row_end=re)
    ref, cnt = oracle.render(ost, oarr, n, opt)
    img, st = _render(rtm, data, mode, mb, seed, rows=rows, band=band, skip=skip)
    assert img.shape == ref.shape
    _check_exact(what, img, st, ref, cnt)
    if tol:
        timg, ts = _render(rtm, data, mode, mb, seed, variant=TOL_VARIANT, rows=rows, band=band, skip=skip)
        _check_tol(what, timg, ts, img, st)
    return img, st


# ---- sub-pixel stepping ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ss,s", [(1, 1), (2, 3), (3, 5), (4, 16)])
def test_sub_pixel_stepping(rtm, oracle, ss, s):
    """Every (SS, S): the whole frame, and rows 5:19 of it as band 1 of 3 (rtm_options' (count, index) = (3, 1)): a row range
    that starts inside a tile row, one band of it."""
    data = _cornell(rtm, s=s, ss=ss)
    _both(f"SS {ss} S {s} whole frame", rtm, oracle, data, "repaired", 8, 0x5EED)
    _both(f"SS {ss} S {s} rows 5:19 band 1 of 3", rtm, oracle, data, "repaired", 8, 0x5EED, rows=(5, 19), band=(3, 1))


@pytest.mark.parametrize("mb", [8, -1])
def test_passes_that_start_and_end_inside_a_sub_pixel(rtm, oracle, mb):
    """S = 5, SS = 3 (N = 45) in passes [0, 7), [7, 8), [8, 31), [31, 45): every pass but the first starts in the middle of a
    sub-pixel and every pass but the last ends in one.  The frame is the one-pass frame (the oracle's, for variant 0)."""
    import torch
    data = _cornell(rtm, s=5, ss=3)
    bounds = [(0, 7), (7, 8), (8, 31), (31, 45)]
    one, st = _both(f"S 5 SS 3 cap {mb}, one pass", rtm, oracle, data, "repaired", mb, 21)
    frames = {}
    for variant in (0, TOL_VARIANT):
        r = rtm.Renderer(data, mode="repaired", max_bounces=mb, seed=21, variant=variant)
        accum = torch.full((H, W, 3), float("nan"), dtype=torch.float64, device="cuda")
        sums = {k: 0 for k in COUNTERS}
        for a, b in bounds:
            _, ps = r.render_samples_device(a, b, accum, want=("f32",))
            for k in COUNTERS:
                sums[k] += ps[k]
        torch.cuda.synchronize()
        frames[variant] = (accum.cpu().numpy(), sums)
    got, sums = frames[0]
    print(f"passes, cap {mb}: {int((_bits(got) != _bits(one)).any(axis=-1).sum())} pixels differ from the one-pass frame")
    assert np.array_equal(_bits(got), _bits(one)) and sums == {k: st[k] for k in COUNTERS}
    tone, ts = _render(rtm, data, "repaired", mb, 21, variant=TOL_VARIANT)
    tgot, tsums = frames[TOL_VARIANT]
    assert np.array_equal(_bits(tgot), _bits(tone)) and tsums == {k: ts[k] for k in COUNTERS}  # the row's own one-pass frame
    _check_tol(f"passes, cap {mb}", tgot, tsums, got, sums)


# ---- sample split and stealing ----------------------------------------------------------------------------------------
SPLIT_FRAME = dict(w=64, h=16, s=16, ss=2, mb=8, seed=77)  # 16 tiles, 64 samples per pixel (16 is the floor for stealing)
# (environment, is the launch split?)  S = 16: a small wave's share of 8 samples starts in the middle of a sub-pixel every
# other time (samples 40 and 56 of the forced split: wave 0 keeps 32), which is where the running sub-pixel index of a small
# wave has to start right.
SPLIT_SETTINGS = {
    "whole tiles, stealing": ({"RTM_DEBUG_TAIL": "0", "RTM_DEBUG_STEAL": "1"}, False),    # main loop + tail loop + steal_finalize
    "whole tiles, no stealing": ({"RTM_DEBUG_TAIL": "0", "RTM_DEBUG_STEAL": "0"}, False), # main loop to the end
    "8 whole + 8 split tiles": ({"RTM_DEBUG_TAIL": "8", "RTM_DEBUG_STEAL": "1"}, True),   # all three loops in one launch
    "every tile split 8 ways": ({"RTM_DEBUG_SPLIT": "8"}, True),                          # head waves + small waves of 8 samples
}


def _child(out_path):
    """(script mode) renders SPLIT_FRAME with variants 0 and 18 under this process's knobs."""
    sys.path.insert(0, ROOT)
    import raytracingmin_amd as m
    f = SPLIT_FRAME
    data = _cornell(m, f["w"], f["h"], f["s"], f["ss"])
    res = {}
    for variant in (0, TOL_VARIANT):
        out, st = m.Renderer(data, mode="repaired", max_bounces=f["mb"], seed=f["seed"], variant=variant).render_rows_device(want=("f64",))
        res[f"img{variant}"] = out["f64"].cpu().numpy()
        res[f"stats{variant}"] = np.array(json.dumps({k: st[k] for k in COUNTERS + ("variant", "split")}))
    np.savez(out_path, **res)


@pytest.fixture(scope="module")
def split_reference(oracle):
    f = SPLIT_FRAME
    st, arr, n = oracle.load_scene(oracle.scene_path("cornellBoxSetting.json"), width=f["w"], height=f["h"], samples=f["s"],
                                   super_samples=f["ss"])
    return oracle.render(st, arr, n, oracle.make_options(mode=1, max_bounces=f["mb"], seed=f["seed"], height=f["h"]))


@pytest.mark.parametrize("setting", list(SPLIT_SETTINGS))
def test_split_and_stealing_loops(split_reference, tmp_path, setting):
    ref, cnt = split_reference
    env = {k: v for k, v in os.environ.items() if not k.startswith("RTM_DEBUG_")}
    knobs, is_split = SPLIT_SETTINGS[setting]
    env.update(knobs)
    out_path = str(tmp_path / "frames.npz")
    subprocess.run([sys.executable, os.path.abspath(__file__), out_path], env=env, check=True, timeout=120, cwd=ROOT)
    z = np.load(out_path)
    st, ts = json.loads(str(z["stats0"])), json.loads(str(z["stats18"]))
    assert ts["variant"] == TOL_VARIANT
    print(f"{setting}: split {st['split']} (variant 0), {ts['split']} (variant 18)")
    for got in (st["split"], ts["split"]):  # the knobs took effect: rtm_stats.split is the launch's waves per split tile
        assert (got > 1) if is_split else (got == 1), setting
    _check_exact(setting, z["img0"], st, ref, cnt)
    _check_tol(setting, z["img18"], ts, z["img0"], st)


# ---- the emitter test ---------------------------------------------------------------------------------------------------
def _emitter_scene(rtm, kind):
    from raytracingmin_amd import Material, SphereObject, vec3
    data = _cornell(rtm, s=4, ss=2)
    objs = list(data.object)
    n = len(objs)
    if kind == "no emitter":
        objs[0] = SphereObject(objs[0].m_position, objs[0].m_size, Material(vec3(0, 0, 0), vec3(0, 0, 0)))
    elif kind == "emitters at 0 and n - 1":  # the light, and the last wall made a second black light
        objs[n - 1] = SphereObject(objs[n - 1].m_position, objs[n - 1].m_size, Material(vec3(0, 0, 0), vec3(3, 2, 1)))
    elif kind == "one wall removed":  # the wall the camera looks at: primary rays and bounces miss
        del objs[5]
    elif kind == "diffuse emitter":  # a wall that reflects AND emits: the host proves nothing, every path end is queued
        objs[3] = SphereObject(objs[3].m_position, objs[3].m_size, Material(objs[3].m_material.color, vec3(0, .25, 0)))
    data.object = objs
    return data


@pytest.mark.parametrize("mb", [8, -1])
@pytest.mark.parametrize("kind", ["no emitter", "emitters at 0 and n - 1", "one wall removed", "diffuse emitter"])
def test_emitter_test_truth_table(rtm, oracle, kind, mb):
    data = _emitter_scene(rtm, kind)
    on, s_on = _both(f"{kind}, cap {mb}, skip on", rtm, oracle, data, "repaired", mb, 5)
    off, s_off = _both(f"{kind}, cap {mb}, RTM_DEBUG_ZERO_SKIP=0", rtm, oracle, data, "repaired", mb, 5, skip=False)
    assert np.array_equal(_bits(on), _bits(off)) and {k: s_on[k] for k in COUNTERS} == {k: s_off[k] for k in COUNTERS}
    assert on.any() == (kind != "no emitter")


# ---- the back edge ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mb", [0, 1, 2, 8, -1])
def test_depth_caps(rtm, oracle, mb):
    """Odd and even path lengths, a path that is its primary ray alone, and the any-depth kernel."""
    _both(f"depth cap {mb}", rtm, oracle, _cornell(rtm, s=6, ss=2), "repaired", mb, 0xBEEF)


@pytest.mark.parametrize("mb", [8, -1])
def test_literal_mode(rtm, oracle, mb):
    """Normal (0, 0, 0): the non-shortcut basis, and the speculative block's re-run with the compiler's math on every trip."""
    _both(f"literal mode, cap {mb}", rtm, oracle, _cornell(rtm, s=4, ss=2), "literal", mb, 3)


@pytest.mark.parametrize("mb", [8, -1])
def test_plane_room(rtm, oracle, mb):
    """scenes/planeRoom.json: plane normals with exact zeros (MathSpecZ).  Variant 0 only: the tolerance row serves spheres."""
    data = rtm.LoadData(oracle.scene_path("planeRoom.json")).data
    data.width, data.height, data.samples, data.superSamples = W, H, 4, 2
    arr, n = data.objects_c()
    oobj = (oracle.Object * max(n, 1)).from_buffer_copy(bytes(arr))
    ost = oracle.Settings.from_buffer_copy(bytes(data.settings_c()))
    ref, cnt = oracle.render_objects(ost, oobj, n, oracle.make_options(mode=1, max_bounces=mb, seed=9, height=H))
    img, st = _render(rtm, data, "repaired", mb, 9)
    _check_exact(f"planeRoom, cap {mb}", img, st, ref, cnt)
    assert ref.max() > 0.0


def test_nan_camera(rtm, oracle):
    """upVec parallel to the view direction: every primary direction is NaN, every ray misses, the frame is black."""
    data = _cornell(rtm, s=3, ss=2)
    data.camera = rtm.Camera(rtm.vec3(0, 0, -10), rtm.vec3(0, 0, 0), rtm.vec3(0, 0, 1), 2.0)
    for mode in ("repaired", "literal"):
        img, st = _both(f"NaN camera, {mode}", rtm, oracle, data, mode, 8, 1)
        assert not img.any() and st["casts"] == st["samples"] == W * H * 12


if __name__ == "__main__":
    _child(sys.argv[1])
