"""Progressive rendering on a real MI355X (-m gpu): a frame rendered as passes [0, a), [a, b), ..., [., N) through
rtm_render_scene_samples leaves the bytes one rtm_render_scene call leaves, in f64, f32 and u8, and the passes' counters
add up to the one-shot frame's.  Pass boundaries fall inside sub-pixels on purpose."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "raytracingmin_amd", "rtm_cli")
COUNTS = ("casts", "bounces", "draws")


@pytest.fixture(scope="module")
def rtm():
    import raytracingmin_amd as m
    n = C.c_int()
    m._lib.check(m.lib().rtm_device_count(C.byref(n)), "rtm_device_count")
    assert n.value >= 1
    return m


def _bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else a
    return a.view(np.uint64) if a.dtype == np.float64 else (a.view(np.uint32) if a.dtype == np.float32 else a)


def _one_shot(r, **kw):
    out, st = r.render_rows_device(want=("f64", "f32", "u8"), **kw)
    return {k: v.cpu().numpy() for k, v in out.items()}, st


def _in_passes(r, bounds, rows=None, band=None, stats=True):
    import torch
    rb, re = rows if rows else (0, r.data.height)
    opt = r._options(rb, re, band)
    from raytracingmin_amd import lib
    n_rows = lib().rtm_output_rows(C.byref(opt))
    accum = torch.full((n_rows, r.data.width, 3), float("nan"), dtype=torch.float64, device="cuda")
    sums = {k: 0 for k in COUNTS + ("samples",)}
    out = None
    for a, b in bounds:
        out, st = r.render_samples_device(a, b, accum, want=("f32", "u8"), stats=stats, row_begin=rb, row_end=re, band=band)
        if stats:
            assert st["samples"] == n_rows * r.data.width * (b - a)
            for k in sums:
                sums[k] += st[k]
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}, sums


def _check(r, bounds, rows=None, band=None, stats=True):
    kw = {}
    if rows:
        kw.update(row_begin=rows[0], row_end=rows[1])
    if band:
        kw.update(band=band)
    ref, st = _one_shot(r, **kw)
    got, sums = _in_passes(r, bounds, rows=rows, band=band, stats=stats)
    for k in ("f64", "f32", "u8"):
        assert np.array_equal(_bits(got[k]), _bits(ref[k])), k
    if not stats:
        return ref, st
    assert {k: sums[k] for k in COUNTS} == {k: st[k] for k in COUNTS}
    assert sums["samples"] == st["samples"]
    return ref, st


def _data(rtm, scene, w, h, s, ss, literal=False):
    import _oracle
    data = rtm.LoadData(_oracle.scene_path(scene), literal_loader=literal).data
    data.width, data.height, data.samples, data.superSamples = w, h, s, ss
    return data


@pytest.mark.parametrize("mode", ["literal", "repaired"])
@pytest.mark.parametrize("mb", [8, -1])
def test_cornell_passes_equal_the_oracle_frame(rtm, oracle, mode, mb):
    data = _data(rtm, "cornellBoxSetting.json", 45, 27, 8, 3, literal=(mode == "literal"))  # N = 72
    r = rtm.Renderer(data, mode=mode, max_bounces=mb, seed=0x5EED)
    ref, st = _check(r, [(0, 5), (5, 37), (37, 72)])
    ost, arr, n = oracle.load_scene(oracle.scene_path("cornellBoxSetting.json"), literal_loader=(mode == "literal"),
                                    width=45, height=27, samples=8, super_samples=3)
    want, cnt = oracle.render(ost, arr, n, oracle.make_options(mode=0 if mode == "literal" else 1, max_bounces=mb,
                                                               seed=0x5EED, height=27))
    assert np.array_equal(_bits(ref["f64"]), _bits(want))
    assert st["casts"] == cnt["casts"] and st["draws"] == cnt["draws"]


@pytest.mark.parametrize("w,h,s,ss,mb", [(64, 40, 8, 2, 8), (45, 27, 8, 3, 8), (40, 24, 24, 1, -1), (33, 17, 5, 2, 12),
                                          (24, 16, 5, 3, 8), (16, 16, 256, 4, 8)])
def test_forced_split_in_passes(rtm, w, h, s, ss, mb):
    data = _data(rtm, "cornellBoxSetting.json", w, h, s, ss)
    n = s * ss * ss
    bounds = [(0, 5), (5, n // 2 + 1), (n // 2 + 1, n)] if n > 8 else [(0, 3), (3, n)]
    _check(rtm.Renderer(data, mode="repaired", max_bounces=mb, seed=99, variant=9), bounds)


def test_default_kernel_with_stealing_in_passes(rtm):
    data = _data(rtm, "cornellBoxSetting.json", 72, 40, 16, 2, )  # 64 samples, depth 8: stealing on
    r = rtm.Renderer(data, mode="repaired", max_bounces=8, seed=3)
    _check(r, [(0, 5), (5, 37), (37, 64)])
    _check(r, [(0, 20), (20, 40), (40, 64)])  # passes of 16 samples and more: each steals on its own


def test_tolerance_row_passes_equal_its_own_frame(rtm):
    data = _data(rtm, "cornellBoxSetting.json", 45, 27, 8, 3)
    for mb in (8, -1):
        r = rtm.Renderer(data, mode="repaired", max_bounces=mb, seed=11, variant=18)
        _, st = _check(r, [(0, 5), (5, 37), (37, 72)])
        assert st["variant"] == 18


def test_grid_and_exhaustive_pipeline_in_passes(rtm):
    data = rtm.make_stress_scene(n=300, seed=5)
    data.width, data.height, data.samples, data.superSamples = 40, 29, 3, 2  # N = 12
    _, st = _check(rtm.Renderer(data, mode="repaired", max_bounces=8, seed=7), [(0, 5), (5, 7), (7, 12)])
    assert st["variant"] == 17
    big = rtm.make_stress_scene(n=600, seed=6)
    big.width, big.height, big.samples, big.superSamples = 24, 16, 3, 2
    # a depth cap: stats-less passes enqueue every trip at once; passes with stats, a cap too deep for that budget and
    # unlimited depth take the host-followed path
    capped = rtm.Renderer(big, mode="repaired", max_bounces=4, seed=7, variant=12)
    _check(capped, [(0, 5), (5, 7), (7, 12)], stats=False)
    _, st = _check(capped, [(0, 5), (5, 7), (7, 12)])
    assert st["variant"] == 12
    _check(rtm.Renderer(big, mode="repaired", max_bounces=900, seed=7, variant=12), [(0, 5), (5, 12)], stats=False)
    _check(rtm.Renderer(big, mode="repaired", max_bounces=-1, seed=7, variant=12), [(0, 5), (5, 12)])


def test_planes_and_surface_sample_in_passes(rtm):
    data = _data(rtm, "planeRoom.json", 40, 24, 4, 2)  # N = 16
    for variant in (0, 1):
        _check(rtm.Renderer(data, mode="repaired", max_bounces=8, seed=5, variant=variant), [(0, 5), (5, 11), (11, 16)])
    for scene in ("cornellBoxSetting.json", "planeRoom.json"):
        d = _data(rtm, scene, 24, 16, 3, 2)
        r = rtm.Renderer(d, mode="repaired", max_bounces=6, seed=5, integrator="SurfaeSample")
        _, st = _check(r, [(0, 5), (5, 7), (7, 12)])
        assert st["variant"] == 19


def test_bands_and_row_strips_in_passes(rtm):
    data = _data(rtm, "cornellBoxSetting.json", 45, 40, 8, 3)
    r = rtm.Renderer(data, mode="repaired", max_bounces=8, seed=1)
    _check(r, [(0, 5), (5, 37), (37, 72)], band=(3, 1))
    _check(r, [(0, 5), (5, 37), (37, 72)], rows=(8, 40))


def test_preview_is_the_accumulator_scaled_to_the_frame(rtm, oracle):
    import torch
    data = _data(rtm, "cornellBoxSetting.json", 45, 27, 8, 3)
    r = rtm.Renderer(data, mode="repaired", max_bounces=8, seed=2)
    accum = torch.empty((27, 45, 3), dtype=torch.float64, device="cuda")
    n = 72
    for a, b in [(0, 5), (5, 37)]:
        out, _ = r.render_samples_device(a, b, accum, want=("f32", "u8"))
        acc = accum.cpu().numpy()
        scaled = acc * (n / b)
        assert np.array_equal(out["f32"].cpu().numpy().view(np.uint32), scaled.astype(np.float32).view(np.uint32))
        assert np.array_equal(out["u8"].cpu().numpy(), oracle.quantise(scaled))


def test_one_pass_matches_the_oracles_per_sample_fold(rtm, oracle):
    w, h, s, ss, k = 24, 16, 4, 2, 11  # samples [0, 11) of N = 16
    data = _data(rtm, "cornellBoxSetting.json", w, h, s, ss)
    r = rtm.Renderer(data, mode="repaired", max_bounces=8, seed=0x5EED)
    import torch
    accum = torch.empty((h, w, 3), dtype=torch.float64, device="cuda")
    r.render_samples_device(0, k, accum, want=())
    got = accum.cpu().numpy()
    st, arr, n = oracle.load_scene(oracle.scene_path("cornellBoxSetting.json"), width=w, height=h, samples=s,
                                   super_samples=ss)
    opt = oracle.make_options(mode=1, max_bounces=8, seed=0x5EED, height=h)
    L = oracle.lib()
    rng = np.random.default_rng(4)
    for x, y in zip(rng.integers(0, w, 20), rng.integers(0, h, 20)):
        acc = np.zeros(3)
        for i in range(k):
            sub, smp = divmod(i, s)
            rad = (C.c_double * 3)()
            cnt = oracle.Counters()
            L.rtmo_sample_radiance(C.byref(st), arr, n, C.byref(opt), int(x), int(y), sub // ss + 1, sub % ss + 1, smp,
                                   rad, C.byref(cnt))
            for c in range(3):
                v = ((rad[c] / ss) / ss) / s
                acc[c] = acc[c] + min(max(v, 0.0), 1.0)
        assert np.array_equal(got[y, x].view(np.uint64), acc.view(np.uint64)), (x, y)


def test_stats_less_passes_enqueued_back_to_back(rtm):
    data = _data(rtm, "cornellBoxSetting.json", 45, 27, 8, 3)
    r = rtm.Renderer(data, mode="repaired", max_bounces=8, seed=8)
    ref, _ = _one_shot(r)
    bounds = [(0, 5), (5, 14), (14, 23), (23, 37), (37, 45), (45, 50), (50, 61), (61, 72)]
    got, _ = _in_passes(r, bounds, stats=False)
    for k in ("f64", "f32", "u8"):
        assert np.array_equal(_bits(got[k]), _bits(ref[k])), k
    r.stream_status()


def test_refusals_and_empty_range(rtm):
    import torch
    data = _data(rtm, "cornellBoxSetting.json", 24, 16, 4, 2)  # N = 16
    sentinel = float.fromhex("0x1.5555p-3")
    for variant in (15, 16):
        r = rtm.Renderer(data, mode="repaired", max_bounces=8, seed=1, variant=variant)
        accum = torch.full((16, 24, 3), sentinel, dtype=torch.float64, device="cuda")
        with pytest.raises(rtm.RtmError) as e:
            r.render_samples_device(0, 5, accum, want=("f64",))
        assert e.value.status == -8
        torch.cuda.synchronize()
        assert bool((accum == sentinel).all())
        r.render_samples_device(0, 16, accum, want=())  # the whole frame is served
    r = rtm.Renderer(data, mode="repaired", max_bounces=8, seed=1)
    accum = torch.full((16, 24, 3), sentinel, dtype=torch.float64, device="cuda")
    with pytest.raises(rtm.RtmError) as e:
        r.render_samples_device(0, 17, accum)
    assert e.value.status == -1
    out, st = r.render_samples_device(6, 6, accum, want=("u8",))
    assert st["samples"] == 0 and st["casts"] == 0
    torch.cuda.synchronize()
    assert bool((accum == sentinel).all())


def test_progressive_and_render_in_passes_write_the_same_files(rtm, tmp_path):
    data = _data(rtm, "cornellBoxSetting.json", 45, 27, 8, 3)
    r = rtm.Renderer(data, mode="repaired", max_bounces=8, seed=0x5EED)
    ref, _ = _one_shot(r)
    seen = []
    for end, out, st in r.progressive(passes=4, want=("f32", "u8")):
        seen.append(end)
    assert seen == [18, 36, 54, 72]
    assert np.array_equal(_bits(out["f64"]), _bits(ref["f64"])) and np.array_equal(out["u8"].cpu().numpy(), ref["u8"])
    r.Render(str(tmp_path / "one"))
    one = r.image.copy()
    r.Render(str(tmp_path / "four"), passes=4)
    assert np.array_equal(_bits(r.image), _bits(one))
    for ext in (".bmp", ".jpg"):
        assert (tmp_path / ("one" + ext)).read_bytes() == (tmp_path / ("four" + ext)).read_bytes(), ext


def test_cli_passes(tmp_path, oracle):
    if not os.path.exists(CLI):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "raytracingmin_amd", "csrc")], stdout=subprocess.DEVNULL)
    scene = oracle.scene_path("cornellBoxSetting.json")
    args = [CLI, "-json", scene, "--width", "45", "--height", "27", "--samples", "8", "--superSamples", "3",
            "--max-bounces", "8", "--seed", "77"]
    one = subprocess.run(args + ["--out", str(tmp_path / "one")], capture_output=True, text=True, timeout=120)
    assert one.returncode == 0, one.stdout + one.stderr
    four = subprocess.run(args + ["--out", str(tmp_path / "four"), "--passes", "4"], capture_output=True, text=True,
                          timeout=120)
    assert four.returncode == 0, four.stdout + four.stderr
    lines = [ln for ln in four.stdout.splitlines() if ln.startswith("pass ")]
    assert [ln.split(":")[0] for ln in lines] == ["pass 1/4", "pass 2/4", "pass 3/4", "pass 4/4"]
    assert "samples [0, 18)" in lines[0] and "samples [54, 72)" in lines[3]
    assert (tmp_path / "one.bmp").read_bytes() == (tmp_path / "four.bmp").read_bytes()
    bad = subprocess.run(args + ["--passes", "2", "--gpus", "2"], capture_output=True, text=True, timeout=60)
    assert bad.returncode != 0 and "--passes" in bad.stderr
