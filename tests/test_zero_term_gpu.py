"""The zero-term skip of the deferred-fold kernels (csrc/rtm_render_kernel.h: zero_term_queued; SceneView::emit_mask): a path
end whose term is provably (+0, +0, +0) is not queued, folded, stored or added.  Nothing of the image or of the counters may
move: variant 0 is compared with the oracle BIT FOR BIT (tolerance 0.0) through every shape the skip touches, variant 18
with variant 0 under the bar tests/test_tolerance_gpu.py sets (1e-4 per pixel), and the skip switched off
(RTM_DEBUG_ZERO_SKIP=0, read per call) must give the same bits and counters as switched on.

A launch of up to 1 536 tiles is split whole (small waves + split_finalize_kernel, no stealing); 400x328 is 2 050 tiles: 514
whole ones (the main loop, the STEAL tail loop at 16 samples per pixel or more, steal_finalize_kernel) and 1 536 split."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NORTH_STAR_TOL = 1e-4
TOL_VARIANT = 18
COUNTERS = ("samples", "casts", "bounces", "draws")


@pytest.fixture(scope="module")
def rtm():
    import raytracingmin_amd as m
    return m


def _bits(t):
    return t.cpu().numpy().view(np.uint64)


def _render(rtm, data, mb, seed, variant=None, skip=True):
    kw = {} if variant is None else {"variant": variant}
    r = rtm.Renderer(data, mode="repaired", max_bounces=mb, seed=seed, **kw)
    if not skip:
        os.environ["RTM_DEBUG_ZERO_SKIP"] = "0"
    try:
        out, stats = r.render_rows_device(want=("f64",))
    finally:
        os.environ.pop("RTM_DEBUG_ZERO_SKIP", None)
    return out["f64"], stats


def _cornell(rtm, oracle, w, h, s, ss):
    path = oracle.scene_path("cornellBoxSetting.json")
    data = rtm.LoadData(path).data
    data.width, data.height, data.samples, data.superSamples = w, h, s, ss
    st, arr, n = oracle.load_scene(path, width=w, height=h, samples=s, super_samples=ss)
    return data, st, arr, n


@pytest.mark.parametrize("w,h,s,ss,mb", [(96, 64, 4, 2, 8),      # split whole: small waves only
                                         (400, 328, 8, 2, 8),    # whole tiles with the STEAL tail + split tiles
                                         (400, 328, 3, 1, 8),    # whole tiles, fewer than 16 samples: no stealing
                                         (96, 64, 4, 2, -1),     # unlimited depth (kPackL), split whole
                                         (400, 328, 4, 2, -1),   # unlimited depth, whole + split tiles
                                         (400, 328, 4, 2, 20)])  # a cap above 8: the any-depth kernel too
def test_cornell_bit_for_bit_vs_oracle(rtm, oracle, w, h, s, ss, mb):
    data, st, arr, n = _cornell(rtm, oracle, w, h, s, ss)
    ref, cnt = oracle.render(st, arr, n, oracle.make_options(mode=1, max_bounces=mb, seed=0x5EED, height=h))
    img, stats = _render(rtm, data, mb, 0x5EED)
    differing = int((_bits(img) != ref.view(np.uint64)).any(axis=-1).sum())
    print(f"{w}x{h} @ {s * ss * ss} spp, max_bounces {mb}: {differing} pixels differ from the oracle; casts {stats['casts']} vs {cnt['casts']}")
    assert differing == 0
    assert all(stats[k] == cnt[k] for k in ("casts", "bounces", "draws"))
    # the skip off: same bits, same counters
    off, stats_off = _render(rtm, data, mb, 0x5EED, skip=False)
    assert np.array_equal(_bits(img), _bits(off)) and all(stats[k] == stats_off[k] for k in COUNTERS)
    # the tolerance row against the exact kernel, skip on; and against itself with the skip off: the same bits
    tol, ts = _render(rtm, data, mb, 0x5EED, variant=TOL_VARIANT)
    assert ts["variant"] == TOL_VARIANT
    assert float(np.max(np.abs(tol.cpu().numpy() - img.cpu().numpy()))) <= NORTH_STAR_TOL
    tol_off, ts_off = _render(rtm, data, mb, 0x5EED, variant=TOL_VARIANT, skip=False)
    assert np.array_equal(_bits(tol), _bits(tol_off)) and all(ts[k] == ts_off[k] for k in COUNTERS)


def test_progressive_four_passes_bit_for_bit(rtm, oracle):
    """A frame in four seeded passes (every pass continues from what out64 holds) ends on the oracle's bits, both variants'
    rule as above."""
    w, h, s, ss, mb = 400, 328, 16, 2, 8
    data, st, arr, n = _cornell(rtm, oracle, w, h, s, ss)
    ref, _ = oracle.render(st, arr, n, oracle.make_options(mode=1, max_bounces=mb, seed=7, height=h))
    r = rtm.Renderer(data, mode="repaired", max_bounces=mb, seed=7)
    last = None
    for _, out, _stats in r.progressive(passes=4, want=("f64",)):
        last = out["f64"]
    assert np.array_equal(_bits(last), ref.view(np.uint64))
    rt = rtm.Renderer(data, mode="repaired", max_bounces=mb, seed=7, variant=TOL_VARIANT)
    for _, out, _stats in rt.progressive(passes=4, want=("f64",)):
        last_t = out["f64"]
    assert float(np.max(np.abs(last_t.cpu().numpy() - ref))) <= NORTH_STAR_TOL


def _room(rtm, wall_col=(.7, .7, .7), wall_em=(0, 0, 0), light=True):
    """A closed room of six wall spheres with a light in it (the Cornell box's construction, other numbers)."""
    from raytracingmin_amd import Camera, Material, SettingData, SphereObject, vec3
    R = 1e4
    objs = [SphereObject(vec3(0, 9, 0), 4.0, Material(vec3(0, 0, 0), vec3(5, 5, 5)))] if light else []
    for k in range(6):
        pos = [0.0, 0.0, 0.0]
        pos[k // 2] = (R + 10.0) * (1 if k % 2 == 0 else -1)
        col, em = ((wall_col, wall_em) if k == 3 else ((.7, .7, .7), (0, 0, 0)))
        objs.append(SphereObject(vec3(*pos), R, Material(vec3(*col), vec3(*em))))
    cam = Camera(vec3(0.5, -1.0, -8.0), vec3(0, 0, 0), vec3(0, 1, 0), 1.5)
    return SettingData(width=400, height=328, samples=8, superSamples=2, camera=cam, object=objs)


@pytest.mark.parametrize("kind", ["diffuse emitter", "inf colour"])
@pytest.mark.parametrize("mb", [8, -1])
def test_scenes_that_must_not_take_the_skip(rtm, kind, mb):
    """One wall emits and reflects (its level adds something to every fold through it); one wall's colour has an inf component
    (0 x inf is NaN, not +0): the host proves nothing, every path end is queued, and the frame and the counters are the same
    with the skip on and off — and are NOT the frame of the same room with that wall plain, i.e. the wall's ends did count."""
    data = _room(rtm, wall_em=(0, .25, 0)) if kind == "diffuse emitter" else _room(rtm, wall_col=(.7, float("inf"), .7))
    for variant in (None, TOL_VARIANT):
        on, s_on = _render(rtm, data, mb, 5, variant=variant)
        off, s_off = _render(rtm, data, mb, 5, variant=variant, skip=False)
        assert np.array_equal(_bits(on), _bits(off)), (kind, variant)
        assert all(s_on[k] == s_off[k] for k in COUNTERS), (kind, variant)
        plain, _ = _render(rtm, _room(rtm), mb, 5, variant=variant)
        assert not np.array_equal(_bits(on), _bits(plain)), (kind, variant)


@pytest.mark.parametrize("mb", [8, -1])
def test_lightless_scene_is_all_plus_zero(rtm, mb):
    """Nothing emits: every path end is a zero end, no term is stored at all — the frame is +0 in every bit through whole
    tiles (steal_finalize_kernel with no exported term), split tiles (split_finalize_kernel with counts of 0), and a frame
    that is split whole; the counters are those of the skip switched off."""
    data = _room(rtm, light=False)
    for w, h in ((400, 328), (96, 64)):
        data.width, data.height = w, h
        for variant in (None, TOL_VARIANT):
            on, s_on = _render(rtm, data, mb, 9, variant=variant)
            assert not _bits(on).any(), (w, h, variant)
            off, s_off = _render(rtm, data, mb, 9, variant=variant, skip=False)
            assert not _bits(off).any() and all(s_on[k] == s_off[k] for k in COUNTERS), (w, h, variant)
            assert s_on["casts"] > s_on["samples"]  # (paths did bounce)
