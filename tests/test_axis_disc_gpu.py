"""The tolerance row's expanded axis-sphere discriminant on the device (variant 18; csrc/rtm_path.h: sphere_disc under RTM_TOL,
round 9): rtm_debug_math_probe ops 53 / 54 (the new form, from the host's axis row; 54: a sphere of the shared-K group) against op 52 (the form of rounds 4 to 8, kept as
its reference) on seeded rays for every axis signature that has an instantiation, and small frames through every loop of the
kernel against the CPU oracle — variant 18 within north_star's 1e-4 per pixel with counters inside the bounds of
tests/test_tolerance_gpu.py, variant 0 the oracle's bits (the control that the exact unit did not move).

Bounds of the probe comparison, from the issue that asked for the change: |delta b| <= 8 ulp(|c_a| + |o|) — both forms round a
handful of terms of that size —, |delta D4| <= 1e-13 (b^2 + pp + r*r) — two orders under primary_tie_risk's margin of 1e-11 of
the same sum —, NaN and infinity exactly where the reference form has them.

The sample split and the stealing knobs are read once per process, so those frames render in a child process per setting: this
file run as a script."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _axis_disc_rays as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NORTH_STAR_TOL = 1e-4
TOL_VARIANT = 18
COUNTERS = ("samples", "casts", "bounces", "draws")
OP_DISC_REF, OP_DISC, OP_DISC_SHARED = 52, 53, 54
N_RAYS = 65536


@pytest.fixture(scope="module")
def rtm():
    import raytracingmin_amd as m
    return m


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ---- the probes -----------------------------------------------------------------------------------------------------------
def _probe(rtm, op, org, dir, axis, c, r2, row):
    m = org.shape[0]
    a = np.zeros((m, 8))
    a[:, 0:3], a[:, 3:6] = org, dir
    b = np.zeros((m, 8))
    b[:, 0], b[:, 1], b[:, 2], b[:, 3], b[:, 4] = axis, c, r2, row[1], row[2]
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    out = np.empty_like(a)
    rtm._lib.check(rtm.lib().rtm_debug_math_probe(op, a.ctypes.data, b.ctypes.data, a.size, out.ctypes.data), "probe")
    assert not out[:, 2:].any()
    return out[:, 0].copy(), out[:, 1].copy()


def _rays_with_edge_cases(scene, seed):
    """65 536 rays: bounces from points on the scene's spheres, camera rays, and among them directions along an axis, directions
    and origins with a zero component"""
    c, r2, org, dir = R.ray_set(scene, N_RAYS * 3 // 4, N_RAYS // 4, seed)
    org, dir = org[:N_RAYS].copy(), dir[:N_RAYS].copy()
    if org.shape[0] < N_RAYS:  # (the per-sphere share of the bounces was rounded down)
        extra = N_RAYS - org.shape[0]
        org, dir = np.concatenate([org, org[:extra]]), np.concatenate([dir, dir[::-1][:extra]])
    k = 0
    for axis in range(3):
        for sign in (1.0, -1.0):
            dir[k::97][:64] = 0.0
            dir[k::97, axis][:64] = sign  # along an axis, from points on spheres and from the camera (stride over the set)
            k += 1
    for axis in range(3):
        dir[k::89, axis][:256] = 0.0  # a zero component (the rest keeps its length: not unit, like nothing the kernel sees, still finite)
        k += 1
        org[k::83, axis][:256] = 0.0
        k += 1
    return c, r2, org, dir


@pytest.mark.parametrize("scene,seed", [("cornellBoxSetting.json", 52), ("simpleSetting1.json", 53), ("settingData.json", 54)])
def test_expanded_discriminant_against_the_form_it_replaces(rtm, scene, seed):
    c, r2, org, dir = _rays_with_edge_cases(scene, seed)
    assert org.shape == (N_RAYS, 3)
    rows, axis = R.host_rows(R.load_spheres(scene)[4]), R.axis_of(c)
    norm_o = np.sqrt(np.einsum("ij,ij->i", org, org))
    group = R.shared_k_group(rows, axis)
    assert axis.any()
    if scene == "cornellBoxSetting.json":
        assert group.tolist() == [False] + [True] * 6  # kAxisSigCornell7Walls: the launcher's extension of the signature
    for i in np.flatnonzero(axis):
        ca = float(c[i, axis[i] - 1])
        b_old, D_old = _probe(rtm, OP_DISC_REF, org, dir, axis[i], ca, r2[i], rows[i])
        b_np, D_np, scale = R.reference_form(c[i], r2[i], axis[i], org, dir)
        ulp = np.spacing(abs(ca) + norm_o)
        # the reference op ran the form it is meant to be: numpy's unfused restatement within the same bounds
        assert np.isfinite(b_old).all() and np.isfinite(D_old).all()  # finite rays of a compact scene
        assert np.all(np.abs(b_old - b_np) <= 8.0 * ulp) and np.all(np.abs(D_old - D_np) <= 1e-13 * scale), (scene, i)
        assert float(np.ptp(D_old)) > 0.0
        # every axis sphere through the form that adds its own K; a sphere of a shared-K group also through the form an extended
        # signature runs (o.o + K first)
        for op in (OP_DISC, OP_DISC_SHARED) if group[i] else (OP_DISC,):
            b_new, D_new = _probe(rtm, op, org, dir, axis[i], ca, r2[i], rows[i])
            db, dD = np.abs(b_new - b_old), np.abs(D_new - D_old)
            print(f"{scene} sphere {i} (axis {axis[i]}, c {ca:g}), op {op}: max |delta b| {float(np.max(db / ulp)):.2f} ulp(|c| + |o|), max "
                  f"|delta D4| {float(np.max(dD / scale)):.2e} of (b^2 + pp + r*r) [{float(np.max(dD)):.2e} absolute]; the reference op against "
                  f"numpy's unfused form: b {float(np.max(np.abs(b_old - b_np) / ulp)):.2f} ulp, D4 {float(np.max(np.abs(D_old - D_np) / scale)):.2e}")
            for old, new in ((b_old, b_new), (D_old, D_new)):
                assert np.array_equal(np.isnan(old), np.isnan(new)) and np.array_equal(np.isinf(old), np.isinf(new)), (scene, i, op)
            assert np.all(db <= 8.0 * ulp), (scene, i, op)
            assert np.all(dD <= 1e-13 * scale), (scene, i, op)


def test_overflowing_origin_gives_the_same_infinities(rtm):
    """An origin at 1e200 on the sphere's axis, direction along it: p p and o.o overflow alike, both forms give b = -1e200 and
    D4 = -inf — NaN and infinity where the reference form has them."""
    org = np.zeros((8, 3))
    dir = np.zeros((8, 3))
    for a in range(3):
        org[a, a], dir[a, a] = 1e200, 1.0
    for a in range(3):
        row = np.array([10010.0, -20020.0, 200100.0, 0.0])
        old = _probe(rtm, OP_DISC_REF, org, dir, a + 1, 10010.0, 1e8, row)
        for op in (OP_DISC, OP_DISC_SHARED):
            new = _probe(rtm, op, org, dir, a + 1, 10010.0, 1e8, row)
            print(f"axis {a + 1}: reference (b, D4) rows {list(zip(old[0][:3], old[1][:3]))}, op {op} {list(zip(new[0][:3], new[1][:3]))}")
            for o, n in zip(old, new):
                assert np.array_equal(np.isnan(o), np.isnan(n)) and np.array_equal(np.isinf(o), np.isinf(n))
        assert np.isinf(old[1][a]) and old[1][a] < 0.0


# ---- frames ---------------------------------------------------------------------------------------------------------------
def _scene(rtm, name, w, h, s, ss):
    import _oracle
    data = rtm.LoadData(_oracle.scene_path(name)).data
    data.width, data.height, data.samples, data.superSamples = w, h, s, ss
    return data


def _check_frames(what, ref, cnt, img0, st0, img18, st18, any_depth):
    differing0 = int((_bits(img0) != _bits(ref)).any(axis=-1).sum())
    both_nan = np.isnan(img18) & np.isnan(ref)
    worst = float(np.max(np.where(both_nan, 0.0, np.abs(img18 - ref))))
    differing18 = int((_bits(img18) != _bits(ref)).any(axis=-1).sum())
    print(f"{what}: variant 0 — {differing0} pixels differ from the oracle; variant 18 — {differing18} of {ref.shape[0] * ref.shape[1]} pixels "
          f"differ at all, max |delta| {worst:.3e}; casts {st18['casts']} / {st0['casts']} / oracle {cnt['casts']}")
    assert differing0 == 0, what  # the exact unit did not move
    assert {k: st0[k] for k in COUNTERS} == {k: cnt[k] for k in COUNTERS}, what
    assert worst <= NORTH_STAR_TOL, what
    assert np.array_equal(np.isnan(img18), np.isnan(ref)), what
    assert st18["samples"] == cnt["samples"], what
    # tests/test_tolerance_gpu.py: test_tolerance_row_small_frames_vs_oracle / test_tolerance_row_at_any_depth
    bound = 1e-4 * cnt["casts"] + 8 if any_depth else max(2, cnt["casts"] // 100000)
    assert abs(st18["casts"] - cnt["casts"]) <= bound, what


def _render(rtm, data, mode, mb, seed, variant):
    out, st = rtm.Renderer(data, mode=mode, max_bounces=mb, seed=seed, variant=variant).render_rows_device(want=("f64",))
    assert variant == 0 or st["variant"] == TOL_VARIANT
    return out["f64"].cpu().numpy(), st


def _against_oracle(what, rtm, oracle, data, mode, mb, seed):
    st_c, arr_c, n = data.to_c()
    ost, oarr = oracle.Settings.from_buffer_copy(bytes(st_c)), (oracle.Sphere * max(n, 1)).from_buffer_copy(bytes(arr_c))
    opt = oracle.make_options(mode=oracle.MODE_LITERAL if mode == "literal" else oracle.MODE_REPAIRED, max_bounces=mb, seed=seed,
                              row_begin=0, row_end=data.height)
    ref, cnt = oracle.render(ost, oarr, n, opt)
    img0, st0 = _render(rtm, data, mode, mb, seed, 0)
    img18, st18 = _render(rtm, data, mode, mb, seed, TOL_VARIANT)
    _check_frames(what, ref, cnt, img0, st0, img18, st18, mb < 0 or mb > 8)
    return ref


@pytest.mark.parametrize("mb", [8, 1, -1])
def test_cornell_depth_caps(rtm, oracle, mb):
    """40x24 (ragged tiles), S 4, SS 2: the depth-capped kernel, paths of one bounce, the any-depth kernel"""
    ref = _against_oracle(f"Cornell 40x24, cap {mb}", rtm, oracle, _scene(rtm, "cornellBoxSetting.json", 40, 24, 4, 2), "repaired", mb, 0x5EED)
    assert ref.max() > 0.0


def test_simple_setting(rtm, oracle):
    """kAxisSigSimple5: a general sphere at the origin next to four axis spheres"""
    ref = _against_oracle("simpleSetting1 80x48", rtm, oracle, _scene(rtm, "simpleSetting1.json", 80, 48, 16, 1), "repaired", 8, 11)
    assert ref.max() > 0.0


def test_setting_data(rtm, oracle):
    """kAxisSigSetting3"""
    _against_oracle("settingData 100x52", rtm, oracle, _scene(rtm, "settingData.json", 100, 52, 5, 2), "repaired", 8, 7)


def test_literal_mode(rtm, oracle):
    """(literal mode takes the plain exact-n kernels: the axis rows stay unread)"""
    _against_oracle("Cornell 40x24, literal mode", rtm, oracle, _scene(rtm, "cornellBoxSetting.json", 40, 24, 4, 2), "literal", 8, 3)


def test_small_sphere_far_out_takes_the_plain_kernels(rtm, oracle):
    """A scene of settingData.json's signature whose x-axis sphere is small and far out (radius 100 at 1e6, radius 1 at 1e5),
    filling the view of a camera next to it: compact, but outside the expanded form's envelope — in that form the sphere would
    hit itself on a share of its bounces (tests/test_axis_disc_host.py), and it emits, so each such hit is a wrong pixel.  The
    host refuses the scene and the launch takes the plain exact-n kernel: the oracle's frame within 1e-4, casts in bounds."""
    for cx, radius in ((1e6, 100.0), (1e5, 1.0)):
        ref = _against_oracle(f"sphere of radius {radius:g} at x = {cx:g}", rtm, oracle, R.far_sphere_scene(cx, radius), "repaired", 8, 5)
        assert ref.max() > 0.0


def test_scene_from_a_device_resident_array(rtm, oracle):
    """rtm_scene_create(on_device = 1): the geometry rows come back once and the axis rows are uploaded behind them — variant 18
    from such a scene object is the frame of the host-array scene object bit for bit, and the oracle's within 1e-4."""
    import ctypes as C
    import torch
    L = rtm.lib()
    w, h = 40, 24
    data = _scene(rtm, "cornellBoxSetting.json", w, h, 4, 2)
    st = data.settings_c()
    arr, n = data.spheres_c()
    ost, oarr, on = oracle.load_scene(oracle.scene_path("cornellBoxSetting.json"), width=w, height=h, samples=4, super_samples=2)
    ref, cnt = oracle.render(ost, oarr, on, oracle.make_options(mode=1, max_bounces=8, seed=3, height=h))
    opt = rtm.Renderer(data, mode="repaired", max_bounces=8, seed=3, variant=TOL_VARIANT)._options(0, h)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    d_arr = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()
    frames, casts = [], []
    for src, on_device in ((arr, 0), (C.c_void_p(d_arr.data_ptr()), 1)):
        handle = C.c_void_p()
        rtm._lib.check(L.rtm_scene_create(src, n, on_device, 0, C.byref(handle)), "rtm_scene_create")
        out = torch.empty((h, w, 3), dtype=torch.float64, device="cuda")
        stats = rtm._lib.rtm_stats()
        rtm._lib.check(L.rtm_render_scene(C.byref(st), handle, C.byref(opt), C.c_void_p(out.data_ptr()), None, None, stream, C.byref(stats)),
                       "rtm_render_scene")
        torch.cuda.synchronize()
        assert stats.variant == TOL_VARIANT
        frames.append(out.cpu().numpy())
        casts.append(int(stats.casts))
        assert L.rtm_scene_destroy(handle) == 0
    print(f"device-resident array: max |delta| from the oracle {float(np.max(np.abs(frames[1] - ref))):.3e}, casts {casts} / {cnt['casts']}")
    assert np.array_equal(_bits(frames[0]), _bits(frames[1])) and casts[0] == casts[1]
    assert float(np.max(np.abs(frames[1] - ref))) <= NORTH_STAR_TOL
    assert abs(casts[1] - cnt["casts"]) <= max(2, cnt["casts"] // 100000)


# ---- sample split and stealing: main, small-wave and tail loops -----------------------------------------------------------------
SPLIT_FRAME = dict(w=64, h=16, s=16, ss=2, mb=8, seed=77)  # (tests/test_loop_trims_gpu.py: 16 tiles, 64 samples per pixel)
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
    data = _scene(m, "cornellBoxSetting.json", f["w"], f["h"], f["s"], f["ss"])
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
    for got in (st["split"], ts["split"]):  # the knobs took effect: rtm_stats.split is the launch's waves per split tile
        assert (got > 1) if is_split else (got == 1), setting
    _check_frames(setting, ref, cnt, z["img0"], st, z["img18"], ts, False)


if __name__ == "__main__":
    _child(sys.argv[1])
