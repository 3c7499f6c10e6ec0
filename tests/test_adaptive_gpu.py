"""Tile lists (rtm_render_scene_tiles) and tile-adaptive sampling (rtm_render_adaptive) on a real MI355X (-m gpu).

Listed tiles equal the progressive state of the same range bit for bit in f64, f32 and u8, unlisted tiles keep their fill,
on frames whose sizes are not multiples of 8, on row ranges and band parts, through every kernel that serves lists.  The
adaptive driver's per-tile sample counts equal _adaptive_ref run on the progressive accumulators of every checkpoint, and
every tile's bytes equal the progressive state at its own count."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _adaptive_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "raytracingmin_amd", "rtm_cli")
COUNTS = ("casts", "bounces", "draws")
U8_FILL = 0xA5
UNSUPPORTED = -8


@pytest.fixture(scope="module")
def rtm():
    import raytracingmin_amd as m
    n = C.c_int()
    m._lib.check(m.lib().rtm_device_count(C.byref(n)), "rtm_device_count")
    assert n.value >= 1
    return m


def _bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else (a.view(np.uint32) if a.dtype == np.float32 else a)


def _data(rtm, scene, w, h, s, ss):
    import _oracle
    data = rtm.LoadData(_oracle.scene_path(scene)).data
    data.width, data.height, data.samples, data.superSamples = w, h, s, ss
    return data


def _kw(rows, band):
    kw = {}
    if rows:
        kw.update(row_begin=rows[0], row_end=rows[1])
    if band:
        kw.update(band=band)
    return kw


def _state(r, a, b, rows=None, band=None):
    """The whole call's progressive state after [0, a) and then [a, b): numpy f64 / f32 / u8 and the second pass's stats."""
    import torch
    kw = _kw(rows, band)
    from raytracingmin_amd import lib
    rb, re = rows or (0, r.data.height)
    n_rows = lib().rtm_output_rows(C.byref(r._options(rb, re, band)))
    acc = torch.empty((n_rows, r.data.width, 3), dtype=torch.float64, device="cuda")
    if a > 0:
        r.render_samples_device(0, a, acc, want=(), **kw)
    out, st = r.render_samples_device(a, b, acc, want=("f32", "u8"), **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}, st


def _pixel_mask(n_rows, w, tiles_x, tiles):
    m = np.zeros((n_rows, w), bool)
    for t in tiles:
        ty, tx = divmod(int(t), tiles_x)
        m[ty * 8:ty * 8 + 8, tx * 8:tx * 8 + 8] = True
    return m


def _list_tensor(tiles):
    import torch
    return torch.tensor(np.asarray(tiles, dtype=np.int64).astype(np.uint32).view(np.int32), device="cuda")


def _check_list(r, a, b, tiles, rows=None, band=None):
    """Render `tiles` over [a, b) into buffers filled with NaN / a sentinel (the listed tiles' accumulator holding the state
    at a); the listed tiles must equal the progressive state, every other pixel its fill, and stats.samples follow the rule."""
    import torch
    kw = _kw(rows, band)
    ty, tx = r.tiles_shape(**kw)
    want, _ = _state(r, a, b, rows, band)
    n_rows, w = want["f64"].shape[:2]
    mask = _pixel_mask(n_rows, w, tx, [t for t in tiles if 0 <= t < tx * ty])
    start = _state(r, 0, a, rows, band)[0]["f64"] if a > 0 else np.zeros((n_rows, w, 3))
    acc0 = np.where(mask[..., None], start, np.nan)
    acc = torch.from_numpy(acc0.copy()).cuda()
    out = {"f32": torch.full((n_rows, w, 3), float("nan"), dtype=torch.float32, device="cuda"),
           "u8": torch.full((n_rows, w, 3), U8_FILL, dtype=torch.uint8, device="cuda")}
    res, st = r.render_tiles_device(_list_tensor(tiles), a, b, acc, out=out, **kw)
    torch.cuda.synchronize()
    got = {k: res[k].cpu().numpy() for k in ("f64", "f32", "u8")}
    for k in ("f64", "f32", "u8"):
        assert np.array_equal(_bits(got[k][mask]), _bits(want[k][mask])), k
    assert np.array_equal(_bits(got["f64"][~mask]), _bits(acc0[~mask]))
    assert np.isnan(got["f32"][~mask]).all() and (got["u8"][~mask] == U8_FILL).all()
    assert st["samples"] == int(mask.sum()) * (b - a)
    return st


def _some_tiles(n_tiles, k, seed):
    return [int(t) for t in np.random.default_rng(seed).permutation(n_tiles)[:k]]


def test_default_kernel_lists_with_split_and_stealing(rtm):
    # 51 x 42 = 2 142 tiles; a list of 1 800 of them: its last 1 536 are sample-split, the rest whole tiles that steal
    data = _data(rtm, "cornellBoxSetting.json", 403, 333, 16, 2)  # N = 64
    r = rtm.Renderer(data, mode="repaired", max_bounces=8, seed=3)
    tiles = _some_tiles(51 * 42, 1800, 1)
    st = _check_list(r, 0, 64, tiles)
    assert st["split"] > 1
    _check_list(r, 24, 64, tiles)
    _check_list(r, 0, 40, tiles[:300] + [51 * 42, 51 * 42 + 7])  # a preview; entries past the frame do nothing


@pytest.mark.parametrize("variant", [0, 1, 18])
def test_small_frame_lists_per_variant(rtm, variant):
    data = _data(rtm, "cornellBoxSetting.json", 45, 27, 8, 3)  # N = 72, 6 x 4 tiles
    for mb in (8, -1):
        r = rtm.Renderer(data, mode="repaired", max_bounces=mb, seed=11, variant=variant)
        st = _check_list(r, 5, 37, _some_tiles(24, 13, variant))
        assert st["variant"] == (variant if variant else 2)
        _check_list(r, 0, 72, _some_tiles(24, 7, variant + 1))


def test_rows_and_bands_lists(rtm):
    data = _data(rtm, "cornellBoxSetting.json", 45, 40, 8, 3)
    r = rtm.Renderer(data, mode="repaired", max_bounces=8, seed=1)
    _check_list(r, 5, 37, [4, 0, 11, 7], rows=(8, 37))
    _check_list(r, 5, 37, [5, 0, 3], band=(3, 1))


def test_plane_grid_and_surface_sample_lists(rtm):
    data = _data(rtm, "planeRoom.json", 40, 24, 4, 2)  # N = 16
    for variant in (0, 1):
        _check_list(rtm.Renderer(data, mode="repaired", max_bounces=8, seed=5, variant=variant), 5, 11, [14, 2, 9, 5, 0])
    stress = rtm.make_stress_scene(n=300, seed=5)
    stress.width, stress.height, stress.samples, stress.superSamples = 40, 29, 3, 2  # N = 12
    st = _check_list(rtm.Renderer(stress, mode="repaired", max_bounces=8, seed=7), 5, 12, [19, 3, 7, 0, 12, 16])
    assert st["variant"] == 17
    d = _data(rtm, "cornellBoxSetting.json", 27, 19, 3, 2)
    r = rtm.Renderer(d, mode="repaired", max_bounces=6, seed=5, integrator="SurfaeSample")
    st = _check_list(r, 5, 12, [8, 1, 4, 6])
    assert st["variant"] == 19


def test_full_list_in_passes_is_the_one_shot_frame(rtm):
    import torch
    data = _data(rtm, "cornellBoxSetting.json", 45, 27, 8, 3)
    r = rtm.Renderer(data, mode="repaired", max_bounces=8, seed=8)
    one, st1 = r.render_rows_device(want=("f64", "f32", "u8"))
    acc = torch.empty((27, 45, 3), dtype=torch.float64, device="cuda")
    sums = {k: 0 for k in COUNTS + ("samples",)}
    lst = _list_tensor(range(24))
    for a, b in [(0, 5), (5, 37), (37, 72)]:
        out, st = r.render_tiles_device(lst, a, b, acc, want=("f32", "u8"))
        for k in sums:
            sums[k] += st[k]
    torch.cuda.synchronize()
    for k in ("f64", "f32", "u8"):
        assert np.array_equal(_bits(out[k]), _bits(one[k])), k
    assert sums == {k: st1[k] for k in sums}


def test_refusals_write_nothing(rtm):
    import torch
    sentinel = float.fromhex("0x1.5555p-3")
    data = _data(rtm, "cornellBoxSetting.json", 24, 16, 4, 2)
    big = rtm.make_stress_scene(n=600, seed=6)
    big.width, big.height, big.samples, big.superSamples = 24, 16, 3, 2
    cases = [(data, v) for v in (7, 15, 16)] + [(big, 12)]
    for d, variant in cases:
        r = rtm.Renderer(d, mode="repaired", max_bounces=4, seed=1, variant=variant)
        acc = torch.full((16, 24, 3), sentinel, dtype=torch.float64, device="cuda")
        with pytest.raises(rtm.RtmError) as e:
            r.render_tiles_device([0, 3], 0, 4, acc, want=("f64",))
        assert e.value.status == UNSUPPORTED, variant
        ts = torch.full((2, 3), 77, dtype=torch.int32, device="cuda")
        work = torch.empty(4096 + 24 * 16 * 24, dtype=torch.uint8, device="cuda")
        st, opt = d.settings_c(), r._options(0, 16)
        prm = rtm._lib.rtm_adaptive_params(2, 0.1)
        rc = rtm.lib().rtm_render_adaptive(C.byref(st), r._scene_handle(), C.byref(opt), C.byref(prm),
                                           C.c_void_p(acc.data_ptr()), None, None, C.c_void_p(ts.data_ptr()),
                                           C.c_void_p(work.data_ptr()), None, None)
        assert rc == UNSUPPORTED, variant
        torch.cuda.synchronize()
        assert bool((acc == sentinel).all()) and bool((ts == 77).all()), variant
    # an empty list enqueues nothing
    r = rtm.Renderer(data, mode="repaired", max_bounces=8, seed=1)
    acc = torch.full((16, 24, 3), sentinel, dtype=torch.float64, device="cuda")
    _, st = r.render_tiles_device(torch.empty(0, dtype=torch.int32, device="cuda"), 0, 16, acc, want=())
    torch.cuda.synchronize()
    assert st["samples"] == 0 and bool((acc == sentinel).all())


def _cornell72(rtm, seed=0x5EED):
    return rtm.Renderer(_data(rtm, "cornellBoxSetting.json", 45, 27, 8, 3), mode="repaired", max_bounces=8, seed=seed)


def test_adaptive_negative_threshold_is_the_full_frame(rtm):
    r = _cornell72(rtm)
    one, st1 = r.render_rows_device(want=("f64", "f32", "u8"))
    for thr, m in ((-1.0, 5), (0.5, 100)):  # no tile stops; m >= N: one pass
        out, ts, st = r.adaptive(thr, min_samples=m, want=("f32", "u8"))
        for k in ("f64", "f32", "u8"):
            assert np.array_equal(_bits(out[k]), _bits(one[k])), (thr, k)
        assert (ts.cpu().numpy() == 72).all()
        assert {k: st[k] for k in COUNTS + ("samples",)} == {k: st1[k] for k in COUNTS + ("samples",)}
        assert st["variant"] == st1["variant"]


def test_adaptive_huge_threshold_stops_every_tile_at_b1(rtm):
    r = _cornell72(rtm)
    want, _ = _state(r, 5, 10)
    out, ts, st = r.adaptive(1e30, min_samples=5, want=("f32", "u8"))
    assert (ts.cpu().numpy() == 10).all()
    for k in ("f64", "f32", "u8"):
        assert np.array_equal(_bits(out[k]), _bits(want[k])), k
    assert st["samples"] == 45 * 27 * 10


def _progressive_states(r, ends):
    import torch
    acc = torch.empty((r.data.height, r.data.width, 3), dtype=torch.float64, device="cuda")
    states, a = {}, 0
    for b in ends:
        out, _ = r.render_samples_device(a, b, acc, want=("f32", "u8"))
        torch.cuda.synchronize()
        states[b] = {"f64": acc.cpu().numpy(), "f32": out["f32"].cpu().numpy(), "u8": out["u8"].cpu().numpy()}
        a = b
    return states


@pytest.mark.parametrize("scene,w,h,s,ss,m", [("cornellBoxSetting.json", 61, 45, 16, 2, 4),
                                              ("settingData.json", 99, 53, 64, 1, 4)])
def test_adaptive_mid_threshold_matches_the_reference(rtm, scene, w, h, s, ss, m):
    data = _data(rtm, scene, w, h, s, ss)
    r = rtm.Renderer(data, mode="repaired", max_bounces=8, seed=21)
    n = s * ss * ss
    ends = ref.schedule(n, m)
    states = _progressive_states(r, ends)
    ty, tx = (h + 7) // 8, (w + 7) // 8
    E = np.array([ref.tile_error(states[ends[1]]["f64"], states[ends[0]]["f64"], n, ends[0], ends[1], tx, t)
                  for t in range(tx * ty)])
    thr = float(np.float32(np.median(E[E > 0])))  # about half the lit tiles stop at the first checkpoint
    want_ts, trace = ref.run({b: v["f64"] for b, v in states.items()}, n, m, thr, tx, ty)
    out, ts, st = r.adaptive(thr, min_samples=m, want=("f32", "u8"))
    ts = ts.cpu().numpy()
    assert np.array_equal(ts, want_ts)
    assert len(np.unique(ts)) >= 2
    got = {k: v.cpu().numpy() for k, v in out.items()}
    pixels = 0
    for t in range(tx * ty):
        y0, x0 = (t // tx) * 8, (t % tx) * 8
        sl = (slice(y0, min(y0 + 8, h)), slice(x0, min(x0 + 8, w)))
        k = int(ts.flat[t])
        for key in ("f64", "f32", "u8"):
            assert np.array_equal(_bits(got[key][sl]), _bits(states[k][key][sl])), (t, k, key)
        pixels += (sl[0].stop - y0) * (sl[1].stop - x0) * k
    assert st["samples"] == pixels
    if scene == "settingData.json":  # the black sky: tiles that are zero at N stop at b_1 and are the full frame there
        sky = [t for t in range(tx * ty)
               if not states[n]["f64"][(t // tx) * 8:(t // tx) * 8 + 8, (t % tx) * 8:(t % tx) * 8 + 8].any()]
        assert sky
        for t in sky:
            assert ts.flat[t] == ends[1]


def test_adaptive_is_deterministic_across_streams(rtm):
    import torch
    r = _cornell72(rtm, seed=4)
    first = r.adaptive(0.05, min_samples=5, want=("f32", "u8"))
    for _ in range(2):
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            again = r.adaptive(0.05, min_samples=5, want=("f32", "u8"))
        s.synchronize()
        for k in ("f64", "f32", "u8"):
            assert np.array_equal(_bits(again[0][k]), _bits(first[0][k])), k
        assert torch.equal(again[1], first[1])


def _read_pfm(path):
    raw = open(path, "rb").read()
    kind, dims, scale, body = raw.split(b"\n", 3)
    w, h = (int(v) for v in dims.split())
    assert kind == b"Pf" and scale == b"-1.0"
    return np.frombuffer(body, dtype="<f4").reshape(h, w)[::-1]


def _read_bmp(path):
    raw = open(path, "rb").read()
    off = int.from_bytes(raw[10:14], "little")
    w, h = int.from_bytes(raw[18:22], "little"), int.from_bytes(raw[22:26], "little")
    stride = (w * 3 + 3) & ~3
    rows = [np.frombuffer(raw, np.uint8, w * 3, off + y * stride).reshape(w, 3)[:, ::-1] for y in range(h)]
    return np.stack(rows[::-1])


def test_render_and_cli_adaptive_write_the_same_files(rtm, tmp_path):
    import torch
    w, h = 45, 27
    data = _data(rtm, "cornellBoxSetting.json", w, h, 8, 3)
    r = rtm.Renderer(data, mode="repaired", max_bounces=8, seed=77)
    # a threshold that stops about half the tiles at the first checkpoint of the default schedule (16, 32, 64, 72)
    a, b = _state(r, 0, 16)[0]["f64"], _state(r, 16, 32)[0]["f64"]
    E = [ref.tile_error(b, a, 72, 16, 32, 6, t) for t in range(24)]
    thr = float(np.float32(np.median(E)))
    rgb8 = r.Render(str(tmp_path / "py"), adaptive=thr, denoise=True)
    out, ts, _ = r.adaptive(thr, want=("f32", "u8"))
    ts = ts.cpu().numpy()
    assert len(np.unique(ts)) >= 2  # (some tiles stopped early: the preview scale matters below)
    assert np.array_equal(rgb8, out["u8"].cpu().numpy())
    # self.image is the adaptive frame's preview: its f32 rounding is the device's f32 view
    assert np.array_equal(r.image.astype(np.float32).view(np.uint32), _bits(out["f32"]))
    spp = np.repeat(np.repeat(ts, 8, 0), 8, 1)[:h, :w].astype(np.float32)
    assert np.array_equal(_read_pfm(tmp_path / "py_spp.pfm"), spp)
    # the denoised files filter that preview
    den = rtm.denoise(out["f32"], r.render_aov(), want=("u8",))["u8"].cpu().numpy()
    torch.cuda.synchronize()
    assert np.array_equal(_read_bmp(tmp_path / "py_denoised.bmp"), den)
    scene = os.path.join(ROOT, "scenes", "cornellBoxSetting.json")
    args = [CLI, "-json", scene, "--width", str(w), "--height", str(h), "--samples", "8", "--superSamples", "3",
            "--max-bounces", "8", "--seed", "77"]
    run = subprocess.run(args + ["--out", str(tmp_path / "cli"), "--adaptive", repr(thr), "--aov", "--denoise"],
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "adaptive:" in run.stdout
    for ext in (".bmp", ".jpg", "_spp.pfm", "_denoised.bmp", "_denoised.jpg"):
        assert (tmp_path / ("cli" + ext)).read_bytes() == (tmp_path / ("py" + ext)).read_bytes(), ext
    assert (tmp_path / "cli_depth.pfm").exists()
    # --adaptive-min: the huge threshold stops every tile at 2 m
    run = subprocess.run(args + ["--out", str(tmp_path / "m"), "--adaptive", "1e30", "--adaptive-min", "9"],
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    assert (_read_pfm(tmp_path / "m_spp.pfm") == 18).all()
    for extra in (["--passes", "2"], ["--gpus", "2"], ["--virtual-strips", "2"], ["--force-rccl"]):
        bad = subprocess.run(args + ["--adaptive", "0.1"] + extra, capture_output=True, text=True, timeout=60, cwd=tmp_path)
        assert bad.returncode != 0 and "--adaptive" in bad.stderr, extra


def _rmse(a, b):
    a, b = np.clip(a.astype(np.float64), 0, 1), np.clip(b.astype(np.float64), 0, 1)
    return float(np.sqrt(np.mean((a - b) ** 2)))


# threshold, bar on RMSE(adaptive) / RMSE(uniform) at equal samples.  Measured on an MI355X: settingData.json 0.021 (42.4
# mean spp of 256), Cornell box 0.044 (247.0 of 256: the tiles that run to N are exact, those of the light stop early)
QUALITY = {"settingData.json": (0.05, 0.25), "cornellBoxSetting.json": (0.05, 0.5)}


@pytest.mark.parametrize("scene", ["settingData.json", "cornellBoxSetting.json"])
def test_adaptive_beats_uniform_at_equal_samples(rtm, scene):
    import torch
    w, h, s, ss, m = 192, 104, 256, 1, 16
    data = _data(rtm, scene, w, h, s, ss)
    r = rtm.Renderer(data, mode="repaired", max_bounces=8, seed=5)
    full, _ = r.render_rows_device(want=("f32",))
    full = full["f32"].cpu().numpy()
    thr, bar = QUALITY.get(scene, (0.05, None))
    out, ts, st = r.adaptive(thr, min_samples=m, want=("f32",))
    mean_spp = st["samples"] / (w * h)
    k = int(np.ceil(mean_spp))  # the uniform preview gets at least the adaptive frame's samples
    acc = torch.empty((h, w, 3), dtype=torch.float64, device="cuda")
    uni, _ = r.render_samples_device(0, k, acc, want=("f32",))
    ea, eu = _rmse(out["f32"].cpu().numpy(), full), _rmse(uni["f32"].cpu().numpy(), full)
    print(f"{scene} {w}x{h}, N = {s * ss * ss}, threshold {thr}: mean {mean_spp:.1f} spp, RMSE adaptive {ea:.5f}, "
          f"uniform at {k} spp {eu:.5f}, ratio {ea / eu:.3f}")
    if bar is not None:
        assert ea <= bar * eu
