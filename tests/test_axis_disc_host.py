"""The tolerance row's expanded axis-sphere discriminant (csrc/rtm_path.h: sphere_disc under RTM_TOL; round 9) against the form
it replaces, in numpy on the CPU — no device.  For a sphere whose centre is c on axis a
    reference form:  p = c - o_a,  b = p d_a - (foreign o d),  D4 = b b - (p p + foreign o o) + r*r
    expanded form:   b = c d_a - o.d,  D4 = b b - ((-2 c) o_a + o.o + K),  K = c c - r*r from the host (rtm_debug_axis_rows)
both in plain float64 without FMA, against long double.  Asserted per sphere, on the same rays: the expanded form's max abs
error of b and of D4 is at most 2 x the reference form's (2: numpy rounds a product the device fuses; seen: 0.68 .. 0.95 x on the Cornell walls, up to 1.45 x on the unit-sized spheres), and
the nearest hit's id from the expanded form is the reference form's for every ray.  K is the exact rational value rounded once."""
from fractions import Fraction

import numpy as np
import pytest

import _axis_disc_rays as R

LD = np.longdouble
N_BOUNCE, N_CAMERA = 840_000, 210_000  # 1.05 M rays per scene


@pytest.fixture(scope="module")
def long_double_is_wider():
    assert np.finfo(LD).nmant >= 63, "this test needs numpy's long double to be wider than float64 (x87: 64 bits)"


@pytest.mark.parametrize("scene,seed,shared", [("cornellBoxSetting.json", 9, False), ("cornellBoxSetting.json", 9, True),
                                               ("simpleSetting1.json", 10, False), ("settingData.json", 11, False)])
def test_expanded_form_is_no_worse_and_picks_the_same_hits(long_double_is_wider, scene, seed, shared):
    """shared: the spheres of the scene's shared-K group (the Cornell box's six walls) form o.o + K first, as the kernel of the
    extended signature does; without it every axis sphere adds its own K last (any other scene)."""
    c, r2, org, dir = R.ray_set(scene, N_BOUNCE, N_CAMERA, seed)
    data = R.load_spheres(scene)[4]
    rows, axis = R.host_rows(data), R.axis_of(c)
    assert org.shape[0] >= 1_000_000 and axis.any()
    m = org.shape[0]
    dis_ref, hit_ref = np.full(m, np.finfo(np.float64).max), np.full(m, -1)
    dis_exp, hit_exp = dis_ref.copy(), hit_ref.copy()
    dis_true, hit_true = dis_ref.copy(), hit_ref.copy()
    group = R.shared_k_group(rows, axis) if shared else np.zeros(len(axis), dtype=bool)
    assert group.any() == shared
    for i in range(c.shape[0]):
        b_ref, D_ref, _ = R.reference_form(c[i], r2[i], axis[i], org, dir)
        b_exp, D_exp = R.expanded_form(rows[i], c[i], r2[i], axis[i], org, dir, shared=bool(group[i]))
        # truth: from (c, r*r) themselves in long double — nothing of the host's row, so neither form is charged with K's rounding
        b_true, D_true, _ = R.reference_form(c[i], r2[i], axis[i], org, dir, LD)
        eb_ref, eb_exp = float(np.max(np.abs(b_ref - b_true))), float(np.max(np.abs(b_exp - b_true)))
        eD_ref, eD_exp = float(np.max(np.abs(D_ref - D_true))), float(np.max(np.abs(D_exp - D_true)))
        print(f"{scene} sphere {i} (axis {axis[i]}{', shared K' if group[i] else ''}, c {c[i].tolist()}, r*r {r2[i]:g}): max abs error of b {eb_ref:.2e} reference / "
              f"{eb_exp:.2e} expanded, of D4 {eD_ref:.2e} / {eD_exp:.2e}")
        assert eb_exp <= 2.0 * eb_ref and eD_exp <= 2.0 * eD_ref, (scene, i)
        R.accept(b_ref, D_ref, dis_ref, hit_ref, i)
        R.accept(b_exp, D_exp, dis_exp, hit_exp, i)
        R.accept(b_true.astype(np.float64), D_true.astype(np.float64), dis_true, hit_true, i)
    differ = int((hit_exp != hit_ref).sum())
    found = hit_ref >= 0
    worst_t = float(np.max(np.abs(dis_exp[found] - dis_ref[found]))) if found.any() else 0.0
    same = found & (hit_ref == hit_true)
    err_ref, err_exp = (float(np.max(np.abs(d[same] - dis_true[same]))) if same.any() else 0.0 for d in (dis_ref, dis_exp))
    print(f"{scene}: {m} rays, {int(found.sum())} hit something; hit id differs expanded / reference on {differ}, reference / long double "
          f"on {int((hit_ref != hit_true).sum())}; accepted distances differ by at most {worst_t:.2e} (against long double: reference "
          f"{err_ref:.2e}, expanded {err_exp:.2e})")
    assert differ == 0
    assert np.unique(hit_ref[found]).size >= min(3, c.shape[0])  # the rays see more than one sphere


@pytest.mark.parametrize("scene", ["cornellBoxSetting.json", "simpleSetting1.json", "settingData.json"])
def test_host_rows_hold_k_rounded_once(scene):
    """rows = (c, -2 c, K, reach) for an axis sphere, zeros for any other; K = c c - r*r as the exact rational value of the row's own
    c and its stored float product r*r, rounded to double once.  The Cornell walls: 10010^2 - 1e8 = 200100 exactly."""
    c, r2, _, _, data = R.load_spheres(scene)
    rows, axis = R.host_rows(data), R.axis_of(c)
    for i in range(c.shape[0]):
        if axis[i] == 0:
            assert not rows[i].any(), (scene, i)
            continue
        ca = float(c[i, axis[i] - 1])
        want = float(Fraction(ca) * Fraction(ca) - Fraction(float(r2[i])))  # (a Fraction converts correctly rounded)
        assert rows[i, :3].tolist() == [ca, -2.0 * ca, want], (scene, i, rows[i].tolist(), want)
    # the fourth entry: the reach within which the host has proven the expanded form safe for the scene — a power of two that
    # covers every sphere and the shipped camera at (0, 0, -10)
    reach = set(rows[axis != 0, 3].tolist())
    extent = float(np.max(np.sqrt((c * c).sum(axis=1)) + np.sqrt(r2)))
    assert len(reach) == 1, (scene, rows[:, 3].tolist())
    r = max(reach)
    print(f"{scene}: extent {extent:g}, proven reach {r:g}")
    assert r >= max(extent, 10.0) and np.log2(r) == int(np.log2(r)), (scene, r)
    if scene == "cornellBoxSetting.json":
        assert axis.tolist() == [2, 1, 1, 2, 2, 3, 3] and set(rows[1:, 2].tolist()) == {200100.0}


@pytest.mark.parametrize("cx,radius,expanded_breaks", [(1e6, 100.0, True), (1e5, 1.0, True), (1e4, 1.0, False)])
def test_small_sphere_far_out_is_outside_the_envelope(cx, radius, expanded_breaks):
    """Why the launcher asks for the host's proof: on bounce rays LEAVING a small sphere far out on an axis the expanded q cancels
    three terms of size c^2 (error up to 2^-49 (|c| + r)^2) where the form of rounds 4 to 8 squared the exact c - o_a, and the
    far root t2 = err / (2 r cos) passes Intersect's 1e-5f: the sphere hits itself.  The old form never does.  The host must
    refuse every such scene (reach 0) — also (1e4, 1), where the bound says it could and these rays do not show it."""
    data = R.far_sphere_scene(cx, radius)
    rows = R.host_rows(data)
    assert rows[0, 3] == 0.0 and rows[2, 3] == 0.0 and rows[2, 0] == cx, rows.tolist()
    c = np.array([[0.0, 10.0, 0.0], [0.0, 0.0, 0.0], [cx, 0.0, 0.0]])
    r2 = np.array([25.0, 4.0, float(np.float32(radius) * np.float32(radius))])
    org, dir = R.bounce_rays(np.random.default_rng(7), c, r2, 200_000, [2], noise=0.0)  # (points on the sphere to their own rounding)
    self_hits = {}
    for name, (b, D4) in (("reference", R.reference_form(c[2], r2[2], 1, org, dir)[:2]),
                          ("expanded", R.expanded_form(rows[2], c[2], r2[2], 1, org, dir))):
        dis, hit = np.full(org.shape[0], np.finfo(np.float64).max), np.full(org.shape[0], -1)
        R.accept(b, D4, dis, hit, 2)
        self_hits[name] = int((hit == 2).sum())
    print(f"sphere of radius {radius:g} at x = {cx:g}: rays that leave it and hit it again, of 200 000: {self_hits}")
    assert self_hits["reference"] == 0
    assert (self_hits["expanded"] > 0) == expanded_breaks
