"""The tolerance row's trip after round 8 (variant 18; csrc/rtm_path.h half_of_rsq, ShadeOut::dir_scale / shade_commit,
csrc/rtm_device.h sincos_turn24_tab_load): the half of a reciprocal root by an integer add on its exponent, the angle split
in integers, and the bounced ray committed as (vector, scale) with the RNG counter advanced in place.  None of it may move a
bit: the probe ops of the new forms are compared BIT FOR BIT with the forms they replace, kept as reference functions (ops 45
.. 47 of rtm_debug_math_probe); frames compare variant 0 with the CPU oracle bit for bit with equal counters and variant 18
with variant 0 under north_star's bar of 1e-4 per pixel with equal counters.

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
W, H = 40, 24  # ragged tiles
OP_LIGHT_ROOT, OP_LIGHT_ROOT_REF = 41, 45
OP_SIN, OP_COS, OP_SIN_REF, OP_COS_REF = 42, 43, 46, 47
OP_FULL_ROOT, OP_FULL_ROOT_REF = 32, 48
OP_ROW_MS, OP_ROW_RINV, OP_ROW_R2F = 49, 50, 51


@pytest.fixture(scope="module")
def rtm():
    import raytracingmin_amd as m
    return m


def _probe(rtm, op, a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    out = np.empty_like(a)
    rtm._lib.check(rtm.lib().rtm_debug_math_probe(op, a.ctypes.data, None, a.size, out.ctypes.data), "probe")
    return out


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ---- the probes -----------------------------------------------------------------------------------------------------------
def test_light_root_by_exponent_half_is_the_multiply_form(rtm):
    """Op 41 (h0 by the exponent) against op 45 (h0 = 0.5 * y): the powers of two, random values over the whole range, what
    the shading block's two roots see, and the operands whose reciprocal root is no normal number."""
    rng = np.random.default_rng(41)
    j = np.arange(4096, dtype=np.float64) * float((1 << 23) // 4096)
    r2 = (2.0 * j + 1.0) * 2.0 ** -24  # (tests/test_shade_trig_gpu.py: the unit-range values)
    special = np.array([0.0, -0.0, -1.0, 5e-324, np.inf, np.nan])
    x = np.concatenate([2.0 ** np.arange(-1000, 1001, dtype=np.float64), 10.0 ** rng.uniform(-300.0, 300.0, 65536), r2, 1.0 - r2, special])
    got, ref = _probe(rtm, OP_LIGHT_ROOT, x), _probe(rtm, OP_LIGHT_ROOT_REF, x)
    nan = np.isnan(ref)
    differing = int((_bits(got) != _bits(ref))[~nan].sum())
    print(f"light root: {x.size} operands, {differing} differ from the multiply form; {int(nan.sum())} NaN results (both forms: "
          f"{bool(np.array_equal(np.isnan(got), nan))}); specials {dict(zip(map(str, special), got[-special.size:]))}")
    assert np.array_equal(np.isnan(got), nan)  # NaN where the reference form is NaN (the payload may differ), nowhere else
    assert differing == 0
    # and the reference form is what it is meant to be: over the normal operands a root to the light bound (2^-45), NaN for a
    # zero, a negative, an infinite and a NaN operand (5e-324 is the instruction's own business: only the two forms' agreement)
    normal = (x >= 2.0 ** -1022) & np.isfinite(x)
    assert not nan[normal].any() and nan[~normal & (x != 5e-324)].all()
    assert np.max(np.abs(ref[normal] / np.sqrt(x[normal]) - 1.0)) < 2.0 ** -44


def test_full_root_by_exponent_half_is_the_multiply_form(rtm):
    """Op 32 (seq_sqrt, the root with its residual step: h0 enters twice) against op 48, the same sequence with h0 = 0.5 * y."""
    rng = np.random.default_rng(32)
    special = np.array([0.0, -0.0, -1.0, 5e-324, np.inf, np.nan])
    x = np.concatenate([2.0 ** np.arange(-1000, 1001, dtype=np.float64), 10.0 ** rng.uniform(-300.0, 300.0, 65536), special])
    got, ref = _probe(rtm, OP_FULL_ROOT, x), _probe(rtm, OP_FULL_ROOT_REF, x)
    nan = np.isnan(ref)
    differing = int((_bits(got) != _bits(ref))[~nan].sum())
    print(f"full root: {x.size} operands, {differing} differ from the multiply form; {int(nan.sum())} NaN results")
    assert np.array_equal(np.isnan(got), nan) and differing == 0
    normal = (x >= 2.0 ** -1022) & np.isfinite(x)
    assert not nan[normal].any() and nan[~normal & (x != 5e-324)].all()
    assert np.max(np.abs(ref[normal] / np.sqrt(x[normal]) - 1.0)) < 2.0 ** -51  # a root to about an ulp


def test_normal_table_row_holds_nan_where_the_reciprocal_is_nan(rtm):
    """fill_norm_row, as the render kernels' prologue calls it, on r * r as the geometry table holds it (a float product widened
    to double).  A finite positive r * r — the smallest float subnormal and 9e18, the walls of radius 3e9, included — gives a
    finite refined reciprocal and the float itself as r2f; r * r = 0 (radius 0, or a product that underflows), infinite (a
    product that overflows: radius above 1.8e19) or NaN gives NaN for both, which is what normalize_on_sphere's one compare
    relies on."""
    radii = np.array([1.0, 4.0, 0.25, 1e5, 3e9, 1e-3, 1e-19, 1.8e19, 1.401298464324817e-45 ** 0.5 * 1.0000001], dtype=np.float32)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        good = (radii * radii).astype(np.float64)
        bad = np.array([0.0, np.float32(0.0) * np.float32(0.0), np.float32(1e-23) * np.float32(1e-23),
                        np.float32(1e20) * np.float32(1e20), np.inf, np.nan], dtype=np.float64)
    assert np.all(np.isfinite(good) & (good > 0.0)) and bad[2] == 0.0 and np.isinf(bad[3])
    r2 = np.concatenate([good, np.array([float(np.float32(1.401298464324817e-45)), float(np.finfo(np.float32).max)]), bad])
    n_good = r2.size - bad.size
    ms, rinv, r2f = _probe(rtm, OP_ROW_MS, r2), _probe(rtm, OP_ROW_RINV, r2), _probe(rtm, OP_ROW_R2F, r2)
    print("normal table rows (r*r, ms, rinv, r2f):", list(zip(r2.tolist(), ms.tolist(), rinv.tolist(), r2f.tolist())))
    want_ms = np.sqrt(r2[:n_good].astype(np.float32)).astype(np.float64)  # (float sqrt, correctly rounded both sides)
    assert np.array_equal(_bits(ms[:n_good]), _bits(want_ms))
    assert np.all(np.isfinite(rinv[:n_good])) and np.max(np.abs(rinv[:n_good] * want_ms - 1.0)) < 4e-16
    assert np.array_equal(_bits(r2f[:n_good]), _bits(r2[:n_good]))  # the float r * r itself
    assert np.all(np.isnan(rinv[n_good:])) and np.all(np.isnan(r2f[n_good:]))


def test_integer_angle_split_is_the_double_split_over_every_draw(rtm):
    """Ops 42 / 43 (the split in integers) against ops 46 / 47 (in doubles), all 2^23 odd m below 2^24."""
    m_all = 2.0 * np.arange(1 << 23, dtype=np.float64) + 1.0
    for name, op, op_ref in (("sin", OP_SIN, OP_SIN_REF), ("cos", OP_COS, OP_COS_REF)):
        got, ref = _probe(rtm, op, m_all), _probe(rtm, op_ref, m_all)
        differing = int((_bits(got) != _bits(ref)).sum())
        print(f"{name} over all 2^23 draws: {differing} values differ between the integer and the double split")
        assert differing == 0
        assert np.all(np.abs(ref) <= 1.0) and float(np.ptp(ref)) > 1.99  # the reference op ran: a sine / cosine over the circle


# ---- frames ---------------------------------------------------------------------------------------------------------------
def _cornell(rtm, w=W, h=H, s=4, ss=2):
    import _oracle
    data = rtm.LoadData(_oracle.scene_path("cornellBoxSetting.json")).data
    data.width, data.height, data.samples, data.superSamples = w, h, s, ss
    return data


def _render(rtm, data, mode, mb, seed, variant=0):
    out, st = rtm.Renderer(data, mode=mode, max_bounces=mb, seed=seed, variant=variant).render_rows_device(want=("f64",))
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
    worst = float(np.max(np.where(both_nan, 0.0, np.abs(tol - img))))
    print(f"{what}: variant 18 — {differing} pixels differ from variant 0, max |difference| {worst:.3e}; casts {ts['casts']} vs {st['casts']}")
    assert worst <= NORTH_STAR_TOL, what
    assert np.array_equal(np.isnan(tol), np.isnan(img)), what
    assert {k: ts[k] for k in COUNTERS} == {k: st[k] for k in COUNTERS}, what


def _both(what, rtm, oracle, data, mode, mb, seed):
    """variant 0 against the oracle, variant 18 against variant 0; returns variant 0's (image, stats)."""
    st_c, arr_c, n = data.to_c()
    ost, oarr = oracle.Settings.from_buffer_copy(bytes(st_c)), (oracle.Sphere * max(n, 1)).from_buffer_copy(bytes(arr_c))
    opt = oracle.make_options(mode=oracle.MODE_LITERAL if mode == "literal" else oracle.MODE_REPAIRED, max_bounces=mb, seed=seed,
                              row_begin=0, row_end=data.height)
    ref, cnt = oracle.render(ost, oarr, n, opt)
    img, st = _render(rtm, data, mode, mb, seed)
    assert img.shape == ref.shape
    _check_exact(what, img, st, ref, cnt)
    timg, ts = _render(rtm, data, mode, mb, seed, variant=TOL_VARIANT)
    _check_tol(what, timg, ts, img, st)
    return img, st


@pytest.mark.parametrize("mb", [8, 1, -1])
def test_cornell_depth_caps(rtm, oracle, mb):
    """SS 2, S 4: the depth-capped kernel, a path of at most one bounce, and the any-depth kernel.  Cornell's diagonal seams
    give flagged primary rays, so the fallback commit (scale 1.0) runs in each of them next to the table's."""
    img, _ = _both(f"Cornell {W}x{H}, cap {mb}", rtm, oracle, _cornell(rtm), "repaired", mb, 0x5EED)
    assert img.max() > 0.0


def test_simple_setting(rtm, oracle):
    data = rtm.LoadData(oracle.scene_path("simpleSetting1.json")).data
    data.width, data.height, data.samples, data.superSamples = W, H, 4, 2
    img, _ = _both(f"simpleSetting1 {W}x{H}", rtm, oracle, data, "repaired", 8, 11)
    assert img.max() > 0.0


@pytest.mark.parametrize("mb", [8, -1])
def test_literal_mode(rtm, oracle, mb):
    """Normal (0, 0, 0): the basis takes its some_x_axis arm and the block is re-run with the compiler's math on every trip —
    every committed direction comes with scale 1.0."""
    _both(f"literal mode, cap {mb}", rtm, oracle, _cornell(rtm), "literal", mb, 3)


@pytest.mark.parametrize("mb", [8, -1])
def test_room_of_huge_walls(rtm, oracle, mb):
    """The room of tests/test_shade_trig_gpu.py (walls of radius 3e9): a non-compact scene, so the search keeps its full roots
    (seq_sqrt_batch with the residual step: h0 by the exponent enters twice), hits that are not canonical — |hit - centre|^2
    does not round to the float r * r at that size, the general Normalize runs — and bounces that trip the speculative block's
    check (the fallback commit with scale 1.0).  Its rows of the normal table are all valid: sqrtf(9e18) has a refined
    reciprocal."""
    from raytracingmin_amd import Camera, Material, SettingData, SphereObject, vec3
    R = 3e9
    objs = [SphereObject(vec3(0, 9, 0), 4.0, Material(vec3(0, 0, 0), vec3(5, 5, 5)))]
    cols = [(.8, .3, .3), (.3, .8, .3), (.3, .3, .8), (.7, .7, .7), (.8, .3, .8), (.3, .8, .8)]
    for k in range(6):
        pos = [0.0, 0.0, 0.0]
        pos[k // 2] = (R + 10.0) * (1 if k % 2 == 0 else -1)
        objs.append(SphereObject(vec3(*pos), R, Material(vec3(*cols[k]), vec3(0, 0, 0))))
    cam = Camera(vec3(0.5, -1.0, -8.0), vec3(0, 0, 0), vec3(0, 1, 0), 1.5)
    data = SettingData(width=W, height=H, samples=4, superSamples=2, camera=cam, object=objs)
    _both(f"walls of radius 3e9, cap {mb}", rtm, oracle, data, "repaired", mb, 7)


def test_scene_with_invalid_normal_rows(rtm, oracle):
    """A lit room inside a sphere of radius 1e20 (r * r overflows a float: +inf), with a sphere of radius 0 and one of radius
    1e-23 (r * r underflows: 0) in the middle of it: three rows of the normal table hold NaN for the reciprocal and, since
    round 8, for r2f (test_normal_table_row_holds_nan_where_the_reciprocal_is_nan checks the rows themselves).  The frame must be
    the oracle's whatever those rows hold, and it is the room's: the huge sphere never returns a hit (its discriminant is
    infinite: t is infinite or NaN, never below the running distance) and the point spheres are missed by every ray that does not
    go through their centre exactly.  What normalize_on_sphere's compare guards against — a hit ON such a sphere whose squared
    length equals the row's r * r, +inf or 0 — cannot be rendered: it needs a hit point that is the sphere's centre to 4e-23."""
    from raytracingmin_amd import Camera, Material, SettingData, SphereObject, vec3
    R = 1e3
    objs = [SphereObject(vec3(0, 9, 0), 4.0, Material(vec3(0, 0, 0), vec3(5, 5, 5)))]
    cols = [(.8, .3, .3), (.3, .8, .3), (.3, .3, .8), (.7, .7, .7), (.8, .3, .8), (.3, .8, .8)]
    for k in range(6):
        pos = [0.0, 0.0, 0.0]
        pos[k // 2] = (R + 10.0) * (1 if k % 2 == 0 else -1)
        objs.append(SphereObject(vec3(*pos), R, Material(vec3(*cols[k]), vec3(0, 0, 0))))
    objs.append(SphereObject(vec3(0, 0, 0), 1e20, Material(vec3(.5, .5, .5), vec3(1, 1, 1))))
    objs.append(SphereObject(vec3(0.5, -1.0, 2.0), 0.0, Material(vec3(.5, .5, .5), vec3(1, 1, 1))))
    objs.append(SphereObject(vec3(-1.0, 0.5, 1.0), 1e-23, Material(vec3(.5, .5, .5), vec3(1, 1, 1))))
    cam = Camera(vec3(0.5, -1.0, -8.0), vec3(0, 0, 0), vec3(0, 1, 0), 1.5)
    data = SettingData(width=W, height=H, samples=4, superSamples=2, camera=cam, object=objs)
    for mb in (8, -1):
        img, _ = _both(f"room with three invalid normal rows, cap {mb}", rtm, oracle, data, "repaired", mb, 7)
        assert np.isfinite(img).all() and img.max() > 0.0


# ---- sample split and stealing: all three loop copies -----------------------------------------------------------------------
SPLIT_FRAME = dict(w=64, h=16, s=16, ss=2, mb=8, seed=77)  # (tests/test_trip_trim_gpu.py: 16 tiles, 64 samples per pixel)
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


if __name__ == "__main__":
    _child(sys.argv[1])
