"""The tolerance row's shading block since round 7 (variant 18; csrc/rtm_device.h sincos_turn24_tab_load / _apply,
csrc/rtm_path.h MathSpecT::sqrt64_unit): the sine and cosine of a draw's angle 2 pi m 2^-24 from a table of 16 384 points
(host long double, rounded once) and two series terms, and the block's two unit-range roots without the residual step.

Bounds.  Ops 42 / 43 of rtm_debug_math_probe against numpy's long double sin / cos of m 2 pi_L / 2^24, ALL 2^23 odd m:
3e-16 absolute.  A numpy emulation of the sequence without fused operations gives 2.15e-16 for both over all draws (table
point rounded once: 0.5 ulp of a value below 1 = 5.6e-17, times |cos r| ~ 1; the remainder r = fl 2 pi / 16384 carries 2^-53
relative of 1.92e-4; the two products and the sum round at 1.1e-16 each and partly cancel); the margin covers the device's
fused forms.  Op 44 against the correctly rounded root: 256 ulps = 1.5 e^2 for a seed good to e = 2^-23, the bound
tests/test_tolerance_gpu.py holds op 41 — the same sequence — to.  Frames: north_star's 1e-4 per pixel against the ORACLE,
cast counts within the slack of test_tolerance_row_small_frames_vs_oracle."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NORTH_STAR_TOL = 1e-4
TOL_VARIANT = 18
TRIG_BOUND = 3e-16
UNIT_ROOT_ULPS = 256


@pytest.fixture(scope="module")
def rtm():
    import raytracingmin_amd as m
    return m


def _probe(rtm, op, a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    out = np.empty_like(a)
    rtm._lib.check(rtm.lib().rtm_debug_math_probe(op, a.ctypes.data, None, a.size, out.ctypes.data), "probe")
    return out


def test_table_sincos_over_every_draw(rtm):
    """Every odd m < 2^24 in one call per op (64 MB of inputs), against long double sin / cos of the exact angle."""
    assert np.finfo(np.longdouble).nmant >= 63, "the reference of this test is x87 long double"
    m_all = 2.0 * np.arange(1 << 23, dtype=np.float64) + 1.0
    got_s, got_c = _probe(rtm, 42, m_all), _probe(rtm, 43, m_all)
    two_pi_l = np.longdouble(2) * np.arctan2(np.longdouble(0), np.longdouble(-1))
    step = two_pi_l / np.longdouble(1 << 24)
    worst_s = worst_c = 0.0
    chunk = 1 << 20  # (the long double reference in pieces: 16 MB each instead of 128)
    for a in range(0, m_all.size, chunk):
        angle = m_all[a:a + chunk].astype(np.longdouble) * step
        worst_s = max(worst_s, float(np.max(np.abs(got_s[a:a + chunk].astype(np.longdouble) - np.sin(angle)))))
        worst_c = max(worst_c, float(np.max(np.abs(got_c[a:a + chunk].astype(np.longdouble) - np.cos(angle)))))
    print(f"table sin / cos over all 2^23 draws: max |error| sin {worst_s:.3e}, cos {worst_c:.3e} (bound {TRIG_BOUND:.1e})")
    assert worst_s <= TRIG_BOUND and worst_c <= TRIG_BOUND


def test_unit_root_is_within_the_light_bound(rtm):
    """The 4 096 values (2 j + 1) 2^-24, j spread evenly over [0, 2^23), and 1 - each: what the block's two roots see."""
    j = np.arange(4096, dtype=np.float64) * float((1 << 23) // 4096)
    r2 = (2.0 * j + 1.0) * 2.0 ** -24
    worst = {}
    for name, x in (("r2", r2), ("1 - r2", 1.0 - r2)):
        assert x.min() > 0.0 and x.max() < 1.0
        got, want = _probe(rtm, 44, x), np.sqrt(x)
        u = np.abs(got.view(np.int64) - want.view(np.int64))
        worst[name] = int(u.max())
        assert u.max() <= UNIT_ROOT_ULPS, (name, int(u.max()))
    print("shading block's unit-range root, worst ulp distance from the correctly rounded root:", worst)


_oracle_frames = {}


def _oracle_frame(oracle, scene, w, h, s, ss, mb, seed):
    key = (scene, w, h, s, ss, mb, seed)
    if key not in _oracle_frames:
        path = oracle.scene_path(scene)
        st, arr, n = oracle.load_scene(path, width=w, height=h, samples=s, super_samples=ss)
        _oracle_frames[key] = oracle.render(st, arr, n, oracle.make_options(mode=1, max_bounces=mb, seed=seed, height=h))
    return _oracle_frames[key]


@pytest.mark.parametrize("scene,mb", [("cornellBoxSetting.json", 8), ("cornellBoxSetting.json", -1), ("simpleSetting1.json", 8)])
def test_small_frames_vs_oracle_two_streams_and_the_exact_unit(rtm, oracle, scene, mb):
    """64x48, S = 4, SS = 2: the depth-capped and the any-depth kernel both run the new block.  The row against the oracle;
    the same render on a second stream of the process, bit for bit (the table is shared and read-only); and the exact
    kernel's frame of the scene still the oracle's bits (the new pointer in RenderParams does not disturb the other unit)."""
    import torch
    w, h, s, ss, seed = 64, 48, 4, 2, 7
    ref, cnt = _oracle_frame(oracle, scene, w, h, s, ss, mb, seed)
    data = rtm.LoadData(oracle.scene_path(scene)).data
    data.width, data.height, data.samples, data.superSamples = w, h, s, ss
    r = rtm.Renderer(data, mode="repaired", max_bounces=mb, seed=seed, variant=TOL_VARIANT)
    out, stats = r.render_rows_device(want=("f64",))
    img = out["f64"].cpu().numpy()
    assert stats["variant"] == TOL_VARIANT
    delta = float(np.max(np.abs(img - ref)))
    differing = int((img.view(np.uint64) != ref.view(np.uint64)).any(axis=-1).sum())
    print(f"{scene} {w}x{h} @ {s * ss * ss} spp, max_bounces {mb}: max |delta| {delta:.3e}, {differing} pixels differ from the "
          f"oracle at all; casts {stats['casts']} vs {cnt['casts']}")
    assert delta <= NORTH_STAR_TOL
    assert abs(stats["casts"] - cnt["casts"]) <= max(2, cnt["casts"] // 100000)
    side = torch.cuda.Stream(device=torch.device("cuda", 0))
    with torch.cuda.stream(side):
        again, stats2 = r.render_rows_device(want=("f64",))
    side.synchronize()
    assert np.array_equal(again["f64"].cpu().numpy().view(np.uint64), img.view(np.uint64))
    assert all(stats2[k] == stats[k] for k in ("samples", "casts", "bounces", "draws"))
    exact, es = rtm.Renderer(data, mode="repaired", max_bounces=mb, seed=seed).render_rows_device(want=("f64",))
    assert es["variant"] != TOL_VARIANT
    assert np.array_equal(exact["f64"].cpu().numpy().view(np.uint64), ref.view(np.uint64))
    assert es["casts"] == cnt["casts"] and es["draws"] == cnt["draws"]


def test_non_compact_scene_stays_within_tolerance(rtm):
    """The room of test_tolerance_row_keeps_full_roots_outside_compact_scenes (walls of radius 3e9): the search keeps its full
    roots there, the shading block's two unit-range roots are light here too — nothing of the scene enters their operands."""
    from raytracingmin_amd import Camera, Material, SettingData, SphereObject, vec3
    R = 3e9
    objs = [SphereObject(vec3(0, 9, 0), 4.0, Material(vec3(0, 0, 0), vec3(5, 5, 5)))]
    cols = [(.8, .3, .3), (.3, .8, .3), (.3, .3, .8), (.7, .7, .7), (.8, .3, .8), (.3, .8, .8)]
    for k in range(6):
        pos = [0.0, 0.0, 0.0]
        pos[k // 2] = (R + 10.0) * (1 if k % 2 == 0 else -1)
        objs.append(SphereObject(vec3(*pos), R, Material(vec3(*cols[k]), vec3(0, 0, 0))))
    cam = Camera(vec3(0.5, -1.0, -8.0), vec3(0, 0, 0), vec3(0, 1, 0), 1.5)
    data = SettingData(width=96, height=64, samples=8, superSamples=2, camera=cam, object=objs)
    for mb in (8, -1):
        exact, _ = rtm.Renderer(data, mode="repaired", max_bounces=mb, seed=7).render_rows_device(want=("f64",))
        tol, ts = rtm.Renderer(data, mode="repaired", max_bounces=mb, seed=7, variant=TOL_VARIANT).render_rows_device(want=("f64",))
        assert ts["variant"] == TOL_VARIANT
        a, b = exact["f64"].cpu().numpy(), tol["f64"].cpu().numpy()
        worst = float(np.nanmax(np.abs(a - b)))
        differing = int((a.view(np.uint64) != b.view(np.uint64)).any(axis=-1).sum())
        print(f"walls of radius 3e9, max_bounces {mb}: max |delta| {worst:.3e}, {differing} pixels differ from the exact frame")
        assert worst <= NORTH_STAR_TOL
