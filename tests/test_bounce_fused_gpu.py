"""Round 14 (profiles/r14/bounce_fused.md): the tolerance unit's shading block takes a bounce direction from ONE reciprocal root,
k = sqrt(r2) / y, without the reference's orthonormal basis (csrc/rtm_path.h: bounce_nd_fused; every kernel of the unit).

Probe ops 59 / 60 of rtm_debug_math_probe (one lane per record): the fused form against the form with the basis built and
against the long-double truth from the same y and the device's own sine and cosine (ops 42 / 43), 65 536 seeded records of the
families of tests/_bounce_model.py; per component within 2^-44 — two light roots at 2^-45 each (tests/test_bounce_fused_host.py
has the model's figures) —, no lane sets `bad`.
Frames: variant 18 against variant 0 and the CPU oracle, every pixel within 1e-4, `casts`, `bounces`, `draws` equal.  Each says
which kernel it ran, through the host's hooks: the Cornell box's own geometry selects its axis-signature kernels, simpleSetting1.json
and settingData.json theirs; seven spheres off every axis run the exact-n kernel.  All of them have the fused bounce: no shape of
the unit keeps the parent's bounce: none gained scratch or lost occupancy (profiles/r14/bounce_fused.md §5).

The sample split and the stealing knobs are read once per process, so those frames render in a child process per setting: this
file run as a script."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _bounce_model as bm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_VARIANT = 18
NORTH_STAR_TOL = 1e-4  # tests/test_tolerance_gpu.py
COUNTERS = ("samples", "casts", "bounces", "draws")
BOUND = 2.0 ** -44
PER_FAMILY = 16384  # x 4 families = 65 536 records


@pytest.fixture(scope="module")
def rtm():
    import raytracingmin_amd as m
    return m


def _probe(rtm, op, a):
    out = np.full(a.shape, np.nan)
    rtm._lib.check(rtm.lib().rtm_debug_math_probe(op, a.ctypes.data, None, a.size, out.ctypes.data), "probe")
    return out


@pytest.fixture(scope="module")
def probed(rtm):
    """every family through ops 59 and 60 once, with the device's sine and cosine of the same draws and the truth from them"""
    res = []
    for name, w, m1, m2 in bm.families(PER_FAMILY, 1403):
        n = len(m1)
        a = np.zeros((n, 8))
        a[:, :3], a[:, 3], a[:, 4] = w, m1, m2
        a = np.ascontiguousarray(a.reshape(-1))
        fused, basis = _probe(rtm, 59, a).reshape(n, 8), _probe(rtm, 60, a).reshape(n, 8)
        md = np.ascontiguousarray(m1.astype(np.float64))
        truth = bm.nd_truth(w, m1, m2, trig=(bm.LD(_probe(rtm, 42, md)), bm.LD(_probe(rtm, 43, md))))
        res.append((name, fused, basis, truth))
    return res


def test_fused_form_against_the_basis_form_and_the_truth(probed):
    worst = 0.0
    for name, fused, basis, truth in probed:
        ef = np.abs(bm.LD(fused[:, :3]) - truth).max(axis=0).astype(np.float64)
        eb = np.abs(bm.LD(basis[:, :3]) - truth).max(axis=0).astype(np.float64)
        d = np.abs(fused[:, :3] - basis[:, :3]).max(axis=0)
        print(f"{name}: max |fused - truth| per component {ef / 2.0 ** -45} x 2^-45, basis form {eb / 2.0 ** -45} x 2^-45, "
              f"|fused - basis| {d / 2.0 ** -45} x 2^-45; lanes with `bad`: {int(fused[:, 3].sum())} / {int(basis[:, 3].sum())}")
        worst = max(worst, float(ef.max()), float(d.max()))
    for name, fused, basis, truth in probed:
        assert np.all(np.isfinite(fused[:, :3])) and np.all(np.isfinite(basis[:, :3])), name
        assert np.all(fused[:, 3] == 0.0) and np.all(basis[:, 3] == 0.0), name  # no lane sets `bad` on these inputs
        assert np.all(fused[:, 4:] == 0.0) and np.all(basis[:, 4:] == 0.0), name
        assert np.all(np.abs(bm.LD(fused[:, :3]) - truth) <= BOUND), name
        assert np.all(np.abs(fused[:, :3] - basis[:, :3]) <= BOUND), name
    assert worst > 0.0  # (the two forms are different arithmetic: identical results would mean one op ran twice)


def test_directions_are_near_unit(probed):
    """what the near-unit Normalize table behind nd needs: |nd|^2 within the table's window of a few float ulps around 1, in both
    forms"""
    for name, fused, basis, _ in probed:
        for nd in (fused[:, :3], basis[:, :3]):
            assert np.all(np.abs((nd * nd).sum(axis=1) - 1.0) < 4e-7), name


# ---- frames ---------------------------------------------------------------------------------------------------------------------------
def _scene(rtm, name, w, h, s, ss):
    import _oracle
    data = rtm.LoadData(_oracle.scene_path(name)).data
    data.width, data.height, data.samples, data.superSamples = w, h, s, ss
    return data


def _cornell(rtm, w, h, s, ss):
    return _scene(rtm, "cornellBoxSetting.json", w, h, s, ss)


def _render(rtm, data, mb, seed, variant):
    out, st = rtm.Renderer(data, mode="repaired", max_bounces=mb, seed=seed, variant=variant).render_rows_device(want=("f64",))
    return out["f64"].cpu().numpy(), st


def _oracle_frame(oracle, data, mb, seed):
    st_c, arr_c, n = data.to_c()
    ost, oarr = oracle.Settings.from_buffer_copy(bytes(st_c)), (oracle.Sphere * max(n, 1)).from_buffer_copy(bytes(arr_c))
    return oracle.render(ost, oarr, n, oracle.make_options(mode=oracle.MODE_REPAIRED, max_bounces=mb, seed=seed, row_begin=0,
                                                           row_end=data.height))


def _through_the_axis_kernels(rtm, data):
    """variant 18 takes an axis-signature instantiation (UNROLL <= -1000)
    for a scene of the Cornell box's seven spheres — its signature, shared K, opposite pairs and the expanded form's envelope are
    facts of the GEOMETRY, granted as a whole by rtm_debug_wall_pairs — in repaired mode from a camera inside it
    (csrc/rtm_kernels_tol.hip: launch_n).  As tests/test_merged_mix_gpu.py ties its frames to them."""
    import ctypes as C
    box = _cornell(rtm, data.width, data.height, data.samples, data.superSamples)
    geometry = lambda d: [(tuple(o.m_position), o.m_size) for o in d.object] + [tuple(d.camera.origin), tuple(d.camera.target),
                                                                                 tuple(d.camera.upVec), d.camera.fov]
    _, arr, n = data.to_c()
    out = (C.c_uint64 * 2)()
    rtm._lib.check(rtm.lib().rtm_debug_wall_pairs(arr, n, out), "wall pairs")
    return n == 7 and geometry(data) == geometry(box) and int(out[0]) == 1


SIG_SIMPLE5 = (1 << 2) | (1 << 4) | (2 << 6) | (2 << 8)  # csrc/rtm_path.h: kAxisSigSimple5
SIG_SETTING3 = 2 | (1 << 4)                               # kAxisSigSetting3


def _axis_signature_launch(rtm, data, sig):
    """... and for the other two signatures with an instantiation (RTM_AXIS_SIGNATURES), what launch_n asks of the scene, through
    the host's hooks: the signature itself and the compact bit (rtm_debug_scene_facts), a reach of the expanded form that holds
    the camera (rtm_debug_axis_rows' fourth column), the camera within the compact extent"""
    import ctypes as C
    _, arr, n = data.to_c()
    facts = (C.c_uint64 * 2)()
    rtm._lib.check(rtm.lib().rtm_debug_scene_facts(arr, n, facts), "scene facts")
    rows = (C.c_double * (4 * n))()
    rtm._lib.check(rtm.lib().rtm_debug_axis_rows(arr, n, rows), "axis rows")
    reach = max(rows[3::4])
    cam = float(np.linalg.norm(np.array(tuple(data.camera.origin), dtype=np.float64)))
    return int(facts[0]) == sig and (int(facts[1]) & 2) != 0 and reach > 0.0 and cam <= reach and cam <= 1e7


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _check_frames(what, ref, cnt, img0, st0, img18, st18):
    differing0 = int((_bits(img0) != _bits(ref)).any(axis=-1).sum())
    differing = int((_bits(img18) != _bits(img0)).any(axis=-1).sum())
    worst = max(float(np.max(np.abs(img18 - img0))), float(np.max(np.abs(img18 - ref))))
    print(f"{what}: variant 0 — {differing0} pixels differ from the oracle; variant 18 — {differing} from variant 0 of "
          f"{ref.shape[0] * ref.shape[1]}, max |delta| {worst:.3e}; casts {st18['casts']} / {st0['casts']} / oracle {cnt['casts']}")
    assert differing0 == 0, what
    assert worst <= NORTH_STAR_TOL, what
    assert {k: st0[k] for k in COUNTERS} == {k: cnt[k] for k in COUNTERS} == {k: st18[k] for k in COUNTERS}, what


@pytest.mark.parametrize("w,h,s,mb", [(40, 24, 4, 8), (40, 24, 4, 1), (43, 16, 4, 8), (40, 24, 3, -1)])
def test_cornell_through_the_axis_kernels(rtm, oracle, w, h, s, mb):
    """SS 2: ragged tiles at 40x24, lanes outside the frame at 43x16; caps 8 and 1 at S 4 (the depth-capped kernel with the
    split); unlimited at S 3 — 12 samples a pixel admit no split: the any-depth axis kernel without it"""
    data = _cornell(rtm, w, h, s, 2)
    assert _through_the_axis_kernels(rtm, data)
    ref, cnt = _oracle_frame(oracle, data, mb, 0x5EED)
    img0, st0 = _render(rtm, data, mb, 0x5EED, 0)
    img18, st18 = _render(rtm, data, mb, 0x5EED, TOL_VARIANT)
    assert st18["variant"] == TOL_VARIANT and ref.max() > 0.0 and cnt["bounces"] > 0
    assert mb >= 0 or st18["split"] == 1
    _check_frames(f"Cornell {w}x{h}, S {s}, cap {mb}", ref, cnt, img0, st0, img18, st18)


def test_almost_every_path_bounces_to_the_cap(rtm, oracle):
    """the Cornell box's geometry with every reflectance at 0.99 under cap 8: 8 of 9 casts run the bounce block"""
    from raytracingmin_amd import vec3
    data = _cornell(rtm, 16, 16, 4, 2)
    for o in data.object:
        o.m_material.color = vec3(0.99, 0.99, 0.99)
    assert _through_the_axis_kernels(rtm, data)
    ref, cnt = _oracle_frame(oracle, data, 8, 0x5EED)
    assert cnt["bounces"] > 0.85 * cnt["casts"] and ref.max() > 0.0
    img0, st0 = _render(rtm, data, 8, 0x5EED, 0)
    img18, st18 = _render(rtm, data, 8, 0x5EED, TOL_VARIANT)
    assert st18["variant"] == TOL_VARIANT
    _check_frames("reflectance 0.99, cap 8", ref, cnt, img0, st0, img18, st18)


@pytest.mark.parametrize("name,n,sig", [("simpleSetting1.json", 5, SIG_SIMPLE5), ("settingData.json", 3, SIG_SETTING3)])
def test_shipped_scenes_through_their_axis_kernels(rtm, oracle, name, n, sig):
    """32x32, S 4, SS 2, cap 8: five and three spheres with signatures of their own (no shared K, no pairs) — the depth-capped
    axis-signature kernels `-6285` and `-1147`"""
    data = _scene(rtm, name, 32, 32, 4, 2)
    assert len(data.object) == n and not _through_the_axis_kernels(rtm, data) and _axis_signature_launch(rtm, data, sig)
    ref, cnt = _oracle_frame(oracle, data, 8, 0x5EED)
    assert cnt["bounces"] > 0 and ref.max() > 0.0
    img0, st0 = _render(rtm, data, 8, 0x5EED, 0)
    img18, st18 = _render(rtm, data, 8, 0x5EED, TOL_VARIANT)
    assert st18["variant"] == TOL_VARIANT
    _check_frames(f"{name} 32x32", ref, cnt, img0, st0, img18, st18)


def test_off_axis_scene_through_the_exact_n_kernel(rtm, oracle):
    """seven spheres off every axis, sphere 0 around the others and the camera (tests/test_trip_slots_gpu.py's all-hit scene): no
    signature, so the exact-n kernel `-107` with three LDS tables"""
    from raytracingmin_amd import Camera, Material, SettingData, SphereObject, vec3
    n = 7
    rng = np.random.default_rng(1100 + n)
    objs = [SphereObject(vec3(0.7, 1.5, 0.9), 30.0 + 0.01 * n, Material(vec3(0.55, 0.6, 0.65), vec3(0.5, 0.45, 0.4)))]
    for k in range(1, n):
        c = rng.uniform(-3.5, 3.5, 3)
        c = np.where(np.abs(c) < 0.05, 0.05, c)
        col = 0.25 + 0.7 * rng.random(3)
        objs.append(SphereObject(vec3(*c), float(0.45 + 0.9 * k / n + 0.001 * k), Material(vec3(*col), vec3(0, 0, 0))))
    cam = Camera(vec3(0.3, -0.4, -11.0), vec3(0.1, 0.2, 0.0), vec3(0, 1, 0), 1.2)
    data = SettingData(width=16, height=16, samples=4, superSamples=2, camera=cam, object=objs)
    import ctypes as C
    _, arr, cnt_n = data.to_c()
    facts = (C.c_uint64 * 2)()
    rtm._lib.check(rtm.lib().rtm_debug_scene_facts(arr, cnt_n, facts), "scene facts")
    assert cnt_n == 7 and int(facts[0]) == 0  # no sphere on an axis: no signature
    ref, cnt = _oracle_frame(oracle, data, 8, 0x5EED + 7)
    img0, st0 = _render(rtm, data, 8, 0x5EED + 7, 0)
    img18, st18 = _render(rtm, data, 8, 0x5EED + 7, TOL_VARIANT)
    assert st18["variant"] == TOL_VARIANT and cnt["bounces"] > cnt["samples"]
    _check_frames("off-axis scene, cap 8", ref, cnt, img0, st0, img18, st18)


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
    """64x16, S 16, SS 2, cap 8 (the Cornell box: the axis-signature kernels) with the split and the stealing forced and off"""
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
