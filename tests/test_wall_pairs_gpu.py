"""The tolerance row's opposite-wall-pair search on the device (variant 18; csrc/rtm_path.h: sphere_chunk under kAxisPairsBit,
round 10).  rtm_debug_math_probe op 55 (the search with wall pairs) against op 56 (the seven-sphere block it replaces) on the
seeded ray sets of tests/_wall_pairs_model.py, 65 536 rays each: distance and hit id equal bit for bit on every ray — a wave
either proves that the walls it drops miss or runs the block itself —, and the fallback flag set on every ray the numpy model
says cannot prove it.  Then small frames through every loop of the kernel: variant 18 against variant 0 and the CPU oracle with
0 pixels that differ at all and equal counters, on the Cornell box (which gets the pair search), on a box whose x walls are not
symmetric (which does not), and from a camera a hair behind the corner of two walls (every primary ray takes the fallback).

The sample split and the stealing knobs are read once per process, so those frames render in a child process per setting: this
file run as a script."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _wall_pairs_model as W

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_VARIANT = 18
COUNTERS = ("samples", "casts", "bounces", "draws")
OP_PAIRS, OP_BLOCK = 55, 56
N_RAYS = 65536
SETS = ["bounce", "grazing", "behind_a_wall", "into_a_second_wall", "flat", "inside_a_wall", "camera", "non_finite"]


@pytest.fixture(scope="module")
def rtm():
    import raytracingmin_amd as m
    return m


@pytest.fixture(scope="module")
def box():
    c, r2, cam, target, data, rows, axis, group = W.cornell()
    sets = W.ray_sets(N_RAYS // 6 * 6 + 6, 2011, c, r2, cam, target)
    table = np.concatenate([np.concatenate([c, r2[:, None]], axis=1), rows]).reshape(-1)  # 7 geometry rows, 7 axis rows
    assert table.size == 56
    return dict(rows=rows, axis=axis, group=group, table=table, sets={k: (o[:N_RAYS], d[:N_RAYS]) for k, (o, d) in sets.items()})


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _probe(rtm, op, table, org, dir):
    m = org.shape[0]
    a = np.zeros((m, 8))
    a[:, 0:3], a[:, 3:6] = org, dir
    b = np.zeros(a.size)
    b[:table.size] = table
    a = np.ascontiguousarray(a)
    out = np.empty_like(a)
    rtm._lib.check(rtm.lib().rtm_debug_math_probe(op, a.ctypes.data, b.ctypes.data, a.size, out.ctypes.data), "probe")
    assert not out[:, 3:].any()
    return out[:, 0].copy(), out[:, 1].astype(np.int64), out[:, 2] != 0.0


@pytest.mark.parametrize("name", SETS)
def test_pair_search_is_the_seven_sphere_block_on_every_ray(rtm, box, name):
    org, dir = box["sets"][name]
    assert org.shape == (N_RAYS, 3)
    dis7, hit7, none = _probe(rtm, OP_BLOCK, box["table"], org, dir)
    dis4, hit4, fell_back = _probe(rtm, OP_PAIRS, box["table"], org, dir)
    _, m_hit, proven, _, _ = W.pair_path(box["rows"], box["axis"], box["group"], org, dir)
    _, m_hit7, _ = W.seven_block(box["rows"], box["axis"], box["group"], org, dir)
    waves = fell_back.reshape(-1, 8)  # a wave of the probe holds 8 rays
    print(f"{name}: {int(fell_back.sum())} of {N_RAYS} rays in a wave that took the block ({int((~proven).sum())} rays cannot prove it in numpy), "
          f"ids seen {np.unique(hit7).tolist()}; the block's ids differ from numpy's on {int((hit7 != m_hit7).sum())} rays")
    assert not none.any()
    assert np.array_equal(hit4, hit7), name
    assert np.array_equal(_bits(dis4), _bits(dis7)), name
    assert bool(fell_back[~proven].all()), name  # every ray the model says fails
    assert bool((waves.all(axis=1) | ~waves.any(axis=1)).all()), name  # ... and the decision is the wave's
    if name in ("bounce", "camera", "into_a_second_wall"):
        assert fell_back.mean() < 0.1, name  # the pair path did run
    if name != "non_finite":
        assert np.unique(hit7).size >= 3


# ---- frames ---------------------------------------------------------------------------------------------------------------
def _scene(rtm, w, h, s, ss):
    import _oracle
    data = rtm.LoadData(_oracle.scene_path("cornellBoxSetting.json")).data
    data.width, data.height, data.samples, data.superSamples = w, h, s, ss
    return data


def _check_frames(what, ref, cnt, img0, st0, img18, st18):
    differing0 = int((_bits(img0) != _bits(ref)).any(axis=-1).sum())
    differing18 = int((_bits(img18) != _bits(ref)).any(axis=-1).sum())
    print(f"{what}: variant 0 — {differing0} pixels differ from the oracle; variant 18 — {differing18} of {ref.shape[0] * ref.shape[1]} pixels "
          f"differ at all; casts {st18['casts']} / {st0['casts']} / oracle {cnt['casts']}")
    assert differing0 == 0 and differing18 == 0, what
    assert {k: st0[k] for k in COUNTERS} == {k: cnt[k] for k in COUNTERS} == {k: st18[k] for k in COUNTERS}, what


def _render(rtm, data, mb, seed, variant):
    out, st = rtm.Renderer(data, mode="repaired", max_bounces=mb, seed=seed, variant=variant).render_rows_device(want=("f64",))
    assert variant == 0 or st["variant"] == TOL_VARIANT
    return out["f64"].cpu().numpy(), st


def _against_oracle(what, rtm, oracle, data, mb, seed):
    st_c, arr_c, n = data.to_c()
    ost, oarr = oracle.Settings.from_buffer_copy(bytes(st_c)), (oracle.Sphere * max(n, 1)).from_buffer_copy(bytes(arr_c))
    ref, cnt = oracle.render(ost, oarr, n, oracle.make_options(mode=oracle.MODE_REPAIRED, max_bounces=mb, seed=seed, row_begin=0,
                                                                row_end=data.height))
    img0, st0 = _render(rtm, data, mb, seed, 0)
    img18, st18 = _render(rtm, data, mb, seed, TOL_VARIANT)
    _check_frames(what, ref, cnt, img0, st0, img18, st18)
    return ref


def _granted(rtm, data):
    import ctypes as C
    _, arr, n = data.to_c()
    out = (C.c_uint64 * 2)()
    rtm._lib.check(rtm.lib().rtm_debug_wall_pairs(arr, n, out), "wall pairs")
    return int(out[0])


@pytest.mark.parametrize("mb", [8, 1, -1])
def test_cornell_depth_caps(rtm, oracle, mb):
    """40x24 (ragged tiles), S 4, SS 2: the depth-capped kernel, paths of one bounce, the any-depth kernel"""
    data = _scene(rtm, 40, 24, 4, 2)
    assert _granted(rtm, data) == 1
    ref = _against_oracle(f"Cornell 40x24, cap {mb}", rtm, oracle, data, mb, 0x5EED)
    assert ref.max() > 0.0


def test_asymmetric_box_keeps_the_seven_sphere_kernels(rtm, oracle):
    """the -x wall at -10011: not the negative of +10010 (and another K), so no pair search — and the same frame"""
    from raytracingmin_amd import vec3
    data = _scene(rtm, 40, 24, 4, 2)
    data.object[2].m_position = vec3(-10011.0, 0.0, 0.0)
    assert _granted(rtm, data) == 0
    ref = _against_oracle("box with x walls at 10010 and -10011", rtm, oracle, data, 8, 0x5EED)
    assert ref.max() > 0.0


def test_camera_behind_the_corner_of_two_walls(rtm, oracle):
    """32x32 from a camera 4e-4 behind the +x and -y walls, looking into the room: every primary ray starts inside two wall
    spheres, whose far roots count — none of them can prove that the wall behind it misses, so their trips take the block"""
    from raytracingmin_amd import vec3
    data = _scene(rtm, 32, 32, 4, 1)
    data.camera.origin = vec3(10.0 + 4e-4, -10.0 - 4e-4, 0.0)
    assert _granted(rtm, data) == 1
    _against_oracle("camera behind the corner of two walls", rtm, oracle, data, 8, 21)


def test_scene_from_a_device_resident_array(rtm, oracle):
    """rtm_scene_create(on_device = 1): the host proves the pairs from the rows that come back — the frame of the host-array
    scene object bit for bit, and the oracle's"""
    import ctypes as C
    import torch
    L = rtm.lib()
    w, h = 40, 24
    data = _scene(rtm, w, h, 4, 2)
    st = data.settings_c()
    arr, n = data.spheres_c()
    ost, oarr, on = oracle.load_scene(oracle.scene_path("cornellBoxSetting.json"), width=w, height=h, samples=4, super_samples=2)
    ref, cnt = oracle.render(ost, oarr, on, oracle.make_options(mode=1, max_bounces=8, seed=3, height=h))
    opt = rtm.Renderer(data, mode="repaired", max_bounces=8, seed=3, variant=TOL_VARIANT)._options(0, h)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    d_arr = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()
    for src, on_device in ((arr, 0), (C.c_void_p(d_arr.data_ptr()), 1)):
        handle = C.c_void_p()
        rtm._lib.check(L.rtm_scene_create(src, n, on_device, 0, C.byref(handle)), "rtm_scene_create")
        out = torch.empty((h, w, 3), dtype=torch.float64, device="cuda")
        stats = rtm._lib.rtm_stats()
        rtm._lib.check(L.rtm_render_scene(C.byref(st), handle, C.byref(opt), C.c_void_p(out.data_ptr()), None, None, stream, C.byref(stats)),
                       "rtm_render_scene")
        torch.cuda.synchronize()
        assert stats.variant == TOL_VARIANT
        assert L.rtm_scene_destroy(handle) == 0
        assert np.array_equal(_bits(out.cpu().numpy()), _bits(ref)), on_device
        assert {k: int(getattr(stats, k)) for k in COUNTERS} == {k: cnt[k] for k in COUNTERS}, on_device


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
    data = _scene(m, f["w"], f["h"], f["s"], f["ss"])
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
    _check_frames(setting, ref, cnt, z["img0"], st, z["img18"], ts)


if __name__ == "__main__":
    _child(sys.argv[1])
