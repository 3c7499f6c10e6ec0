"""Depth of field on a real MI355X (-m gpu): rtm_defocus against the NumPy float64 restatement (_defocus_ref) on synthetic
frames from one pixel to several ragged tiles, the pixels that do not count, the 8-bit store bit for bit, the consequences
the header states, a frame whose tiles take different paths, determinism across calls, streams, alignments and forms, and the
Render / rtm_cli outputs.  test_defocus_matches_the_reference prints the worst error of every frame; DESIGN.md records the
largest."""
import ctypes as C
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import _defocus_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "raytracingmin_amd", "rtm_cli")
SCENE = os.path.join(ROOT, "scenes", "cornellBoxSetting.json")
OPEN_SCENE = os.path.join(ROOT, "scenes", "settingData.json")
TOL = 1e-4  # include/rtm.h: |got - ref| <= 1e-4 max(1, |ref|), for out_f32 of counting pixels and for coc_out
# one pixel; a row and a column smaller than the window; one tile; 131 x 63: several 32 x 16 tiles, ragged in both axes, halos
# that cross tile seams at R = 16
FRAMES = [(1, 1), (1, 17), (17, 1), (7, 5), (37, 23), (64, 64), (131, 63)]
CASES = ((4.0, 0.0, 4), (4.0, 3.0, 4), (4.0, 12.0, 16), (1.0, 6.0, 8), (9.0, 40.0, 16), (4.0, 1.0, 1))  # (zf, A, R): every R class
ALL = ("f32", "u8", "coc")


@pytest.fixture(scope="module")
def rtm():
    import raytracingmin_amd as m
    n = C.c_int()
    m._lib.check(m.lib().rtm_device_count(C.byref(n)), "rtm_device_count")
    assert n.value >= 1
    return m


@functools.lru_cache(maxsize=None)
def _frame(w, h):
    color, depth = _defocus_ref.frame(w, h)
    color.setflags(write=False)
    depth.setflags(write=False)
    return color, depth


@functools.lru_cache(maxsize=None)
def _ref(w, h, zf, A, R):
    """The float64 reference of a frame and a case, computed once and shared."""
    out, s = _defocus_ref.defocus_ref(*_frame(w, h), zf, A, R)
    out.setflags(write=False)
    s.setflags(write=False)
    return out, s


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()  # (a copy: the cached frames are read-only)


def _host_quantise(rtm, f32):
    v = np.ascontiguousarray(f32, dtype=np.float64)
    out = np.zeros(v.shape, np.uint8)
    rtm._lib.check(rtm.lib().rtm_quantise(v.ctypes.data, v.size, out.ctypes.data), "rtm_quantise")
    return out


def _bits(out):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().copy() for k, v in out.items()}


def _same_bits(a, b):
    return set(a) == set(b) and all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in a)


def _words(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("w,h", FRAMES)
def test_defocus_matches_the_reference(rtm, w, h):
    color, depth = _frame(w, h)
    cd, zd = _dev(color), _dev(depth)
    ok = _defocus_ref.counts(color, depth)
    worst, worst_s = 0.0, 0.0
    for zf, A, R in CASES:
        ref, ref_s = _ref(w, h, zf, A, R)
        out = _bits(rtm.defocus(cd, zd, zf, A, R, want=ALL))
        err = _defocus_ref.tolerance_excess(out["f32"][ok], ref[ok])
        err_s = _defocus_ref.tolerance_excess(out["coc"], ref_s)
        print(f"{w}x{h} zf {zf} A {A} R {R}: out_f32 {err:.3e}, coc_out {err_s:.3e}")
        assert err <= TOL, ((zf, A, R), err)
        assert err_s <= TOL, ((zf, A, R), err_s)
        # a pixel that does not count keeps its words and has a circle of +0
        assert np.array_equal(_words(out["f32"])[~ok], _words(color)[~ok]), (zf, A, R)
        assert np.all(_words(out["coc"])[~ok] == 0), (zf, A, R)
        # the 8-bit store is rtm_quantise of the call's own out_f32: exact at every pixel, 0 where a component is NaN
        assert np.array_equal(out["u8"], _host_quantise(rtm, out["f32"])), (zf, A, R)
        assert np.all(out["u8"][np.isnan(out["f32"])] == 0), (zf, A, R)
        worst, worst_s = max(worst, err), max(worst_s, err_s)
    print(f"{w}x{h}: worst error against the float64 reference: out_f32 {worst:.3e}, coc_out {worst_s:.3e} (bar {TOL})")


def test_aperture_zero_returns_every_pixel_bit_for_bit(rtm):
    for w, h in FRAMES:
        color, depth = _frame(w, h)
        for R in (1, 4, 8, 16):
            out = _bits(rtm.defocus(_dev(color), _dev(depth), 4.0, 0.0, R, want=ALL))
            assert np.array_equal(_words(out["f32"]), _words(color)), (w, h, R)
            assert np.all(out["coc"] == 0.0), (w, h, R)
            assert np.array_equal(out["u8"], _host_quantise(rtm, color)), (w, h, R)


def test_a_constant_frame_stays_constant(rtm):
    c = np.array([0.25, 3.0, 0.0], np.float32)
    for w, h in ((1, 1), (37, 23), (131, 63)):
        depth = _frame(w, h)[1]
        color = np.broadcast_to(c, (h, w, 3)).copy()
        ok = _defocus_ref.counts(color, depth)
        for zf, A, R in CASES:
            out = _bits(rtm.defocus(_dev(color), _dev(depth), zf, A, R))
            err = _defocus_ref.tolerance_excess(out["f32"][ok], np.broadcast_to(c, (h, w, 3))[ok])
            assert err <= TOL, (w, h, zf, A, R, err)


def test_a_focused_foreground_keeps_its_words_and_a_focused_background_does_not(rtm):
    w = h = 64
    color, depth = _frame(w, h)
    cd, zd = _dev(color), _dev(depth)
    first = _defocus_ref.disc_mask(w, h, 0) & ~_defocus_ref.disc_mask(w, h, 1) & ~_defocus_ref.disc_mask(w, h, 2)
    out = _bits(rtm.defocus(cd, zd, 1.0, 6.0, 8, want=ALL))
    kept = np.all(_words(out["f32"]) == _words(color), axis=-1)
    assert first.sum() == 493 and kept[first].all()  # r_p = 0 and nothing nearer: however blurred what lies behind it
    assert np.all(out["coc"][first] == 0.0) and not kept[depth == 4.0].any()
    out = _bits(rtm.defocus(cd, zd, 9.0, 40.0, 16, want=ALL))
    far = depth == 9.0
    changed = np.all(_words(out["f32"]) != _words(color), axis=-1)
    assert far.sum() == 183 and changed[far].all()  # r_p = 0 too, but what is in front of it spills over it
    assert np.all(out["coc"][far] == 0.0)


def test_a_frame_whose_tiles_take_different_paths(rtm):
    """The left half lies exactly at the focus (its tiles pass their inputs through, away from the seam), the right half is
    far (the full window): one launch, three kinds of tiles."""
    w, h, zf, A, R = 160, 48, 4.0, 12.0, 8
    rng = np.random.default_rng(7)
    color = (8 * rng.random((h, w, 3)) ** 4).astype(np.float32)
    depth = np.full((h, w), zf, np.float32)
    depth[:, w // 2:] = np.inf
    ref, ref_s = _defocus_ref.defocus_ref(color, depth, zf, A, R)
    out = _bits(rtm.defocus(_dev(color), _dev(depth), zf, A, R, want=ALL))
    err, err_s = _defocus_ref.tolerance_excess(out["f32"], ref), _defocus_ref.tolerance_excess(out["coc"], ref_s)
    print(f"{w}x{h} split frame: out_f32 {err:.3e}, coc_out {err_s:.3e}")
    assert err <= TOL and err_s <= TOL
    kept = np.all(_words(out["f32"]) == _words(color), axis=-1)
    assert kept[:, : w // 2 - (R + 1)].all()  # further than R + 1 from the seam: the input's words
    assert not kept[:, w // 2:].any() and np.all(out["coc"][:, w // 2:] == R) and np.all(out["coc"][:, : w // 2] == 0.0)
    assert np.array_equal(out["u8"], _host_quantise(rtm, out["f32"]))


def test_the_same_inputs_give_the_same_bits(rtm):
    import torch
    w, h = 131, 63
    color, depth = _frame(w, h)
    cd, zd = _dev(color), _dev(depth)
    buf = torch.empty(w * h * 3 + 8, dtype=torch.float32, device="cuda")
    shifted = buf[1:1 + w * h * 3].view(h, w, 3)
    shifted.copy_(cd)
    assert cd.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    for zf, A, R in ((4.0, 3.0, 4), (4.0, 4.0, 8), (9.0, 40.0, 16)):
        first = _bits(rtm.defocus(cd, zd, zf, A, R, want=ALL))
        assert _same_bits(first, _bits(rtm.defocus(cd, zd, zf, A, R, want=ALL))), (zf, A, R)  # a second call
        assert _same_bits(first, _bits(rtm.defocus(shifted, zd, zf, A, R, want=ALL))), (zf, A, R)  # a 4-mod-16 address
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        third = rtm.defocus(cd, zd, zf, A, R, want=ALL, stream=side)
        fourth = rtm.defocus(cd, zd, zf, A, R, want=ALL)  # the current stream's, enqueued while the side stream may still run
        side.synchronize()
        assert _same_bits(first, _bits(third)) and _same_bits(first, _bits(fourth)), (zf, A, R)
        for want in (("f32",), ("u8",), ("coc",)):  # a single output
            out = rtm.defocus(cd, zd, zf, A, R, want=want)
            assert tuple(out) == want
            assert np.array_equal(_bits(out)[want[0]].view(np.uint8), first[want[0]].view(np.uint8)), (zf, A, R, want)
    # the inputs are left alone
    assert np.array_equal(_words(cd.cpu().numpy()), _words(color)) and np.array_equal(_words(zd.cpu().numpy()), _words(depth))


def test_the_window_bound_and_the_pass_through_change_no_bit(rtm):
    """rtm_debug_defocus_form: form 1 runs every block over the whole window; form 0 is the call."""
    import torch
    from raytracingmin_amd import _lib
    L = rtm.lib()
    w, h = 131, 63
    color, depth = _frame(w, h)
    cd, zd = _dev(color), _dev(depth)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for zf, A, R in CASES:
        call = _bits(rtm.defocus(cd, zd, zf, A, R, want=ALL))
        prm = _lib.rtm_defocus_params(zf, A, R)
        for form in (0, 1):
            out = {"f32": torch.empty((h, w, 3), dtype=torch.float32, device="cuda"),
                   "u8": torch.empty((h, w, 3), dtype=torch.uint8, device="cuda"),
                   "coc": torch.empty((h, w), dtype=torch.float32, device="cuda")}
            _lib.check(L.rtm_debug_defocus_form(form, C.byref(prm), w, h, 0, cd.data_ptr(), zd.data_ptr(), out["f32"].data_ptr(),
                                                out["u8"].data_ptr(), out["coc"].data_ptr(), stream), "rtm_debug_defocus_form")
            assert _same_bits(call, _bits(out)), (zf, A, R, form)
    assert L.rtm_debug_defocus_form(2, C.byref(_lib.rtm_defocus_params(4.0, 4.0, 8)), w, h, 0, cd.data_ptr(), zd.data_ptr(),
                                    None, None, zd.data_ptr(), stream) == -1


def _read_bmp(path):
    raw = open(path, "rb").read()
    off = int.from_bytes(raw[10:14], "little")
    w, h = int.from_bytes(raw[18:22], "little"), int.from_bytes(raw[22:26], "little")
    stride = (w * 3 + 3) & ~3
    rows = [np.frombuffer(raw, np.uint8, w * 3, off + y * stride).reshape(w, 3)[:, ::-1] for y in range(h)]
    return np.stack(rows[::-1])


def _read_pfm(path):
    raw = open(path, "rb").read()
    kind, dims, scale, body = raw.split(b"\n", 3)
    w, h = (int(v) for v in dims.split())
    assert kind == b"PF" and scale == b"-1.0"
    return np.frombuffer(body, dtype="<f4").reshape(h, w, 3)[::-1]


def test_render_and_cli_defocus_the_last_stage(rtm, tmp_path):
    import torch
    scene = json.load(open(SCENE))
    scene["00 width"], scene["00 height"], scene["00 samples"], scene["00 superSamples"] = 64, 48, 4, 1
    small = tmp_path / "small.json"
    small.write_text(json.dumps(scene))
    args = [CLI, "-json", str(small), "--max-bounces", "8"]

    def run(stem, *flags, status=0):
        p = subprocess.run(args + ["--out", stem] + list(flags), cwd=tmp_path, capture_output=True, text=True, timeout=300)
        assert p.returncode == status, p.stdout + p.stderr
        return p.stdout if status == 0 else p.stderr

    r = rtm.Renderer(rtm.LoadData(str(small)).data, mode="repaired", max_bounces=8)
    r.Render(str(tmp_path / "py"), dof=True, tonemap=True, bloom=True)
    f32 = torch.from_numpy(r.image).cuda().to(torch.float32)
    depth = r.render_aov(want=("depth",))["depth"]
    zf = r.focus_distance()
    assert zf == 10.0  # the Cornell camera looks from z = -10 at the origin
    want = rtm.defocus(f32, depth, zf, want=("f32", "u8"))
    assert not torch.equal(want["f32"], f32)  # the walls are not at the target distance
    assert np.array_equal(_read_bmp(tmp_path / "py_dof.bmp"), want["u8"].cpu().numpy())
    shown = rtm.tonemap(rtm.bloom(want["f32"])["f32"], want=("u8", "f32"))  # bloom is lens glare: after the lens
    assert np.array_equal(_read_bmp(tmp_path / "py_display.bmp"), shown["u8"].cpu().numpy())
    # rtm_cli: the same files, one line, and the defocused frame is the last stage's
    text = run("cli", "--dof", "--display", "--bloom", "--display-pfm", "--pfm")
    line = [l for l in text.splitlines() if l.startswith("dof:")]
    assert line == ["dof: focus 10, aperture 4, max radius 8"], text
    assert (tmp_path / "cli_dof.bmp").read_bytes() == (tmp_path / "py_dof.bmp").read_bytes()
    assert (tmp_path / "cli_dof.jpg").read_bytes() == (tmp_path / "py_dof.jpg").read_bytes()
    assert np.array_equal(_words(_read_pfm(tmp_path / "cli.pfm")), _words(want["f32"].cpu().numpy()))
    assert np.array_equal(_words(_read_pfm(tmp_path / "cli_display.pfm")), _words(shown["f32"].cpu().numpy()))
    assert (tmp_path / "cli_display.bmp").read_bytes() == (tmp_path / "py_display.bmp").read_bytes()
    # the flags reach the call; --focus-pixel reads the depth plane; a denoised frame is the one that is defocused
    x, y = 32, 40
    z_at = float(depth[y, x].item())
    assert np.isfinite(z_at) and r.focus_distance(pixel=(x, y)) == z_at
    text = run("cli2", "--dof", "6.5", "--dof-radius", "12", "--focus-pixel", f"{x},{y}", "--denoise", "--pfm")
    assert [l for l in text.splitlines() if l.startswith("dof:")] == [f"dof: focus {z_at:.6g}, aperture 6.5, max radius 12"], text
    den = rtm.denoise(f32, r.render_aov(), want=("f32",))["f32"]
    want2 = rtm.defocus(den, depth, z_at, 6.5, 12)["f32"].cpu().numpy()
    assert np.array_equal(_words(_read_pfm(tmp_path / "cli2.pfm")), _words(want2))
    r.Render(str(tmp_path / "py2"), denoise=True, dof=dict(focus_pixel=(x, y), aperture=6.5, max_radius=12))
    assert (tmp_path / "py2_dof.bmp").read_bytes() == (tmp_path / "cli2_dof.bmp").read_bytes()
    text = run("cli3", "--dof", "--focus", "7.25", "--pfm")
    assert [l for l in text.splitlines() if l.startswith("dof:")] == ["dof: focus 7.25, aperture 4, max radius 8"], text
    assert np.array_equal(_words(_read_pfm(tmp_path / "cli3.pfm")), _words(rtm.defocus(f32, depth, 7.25)["f32"].cpu().numpy()))
    # without --dof: the files rtm_cli wrote before, byte for byte, and no dof file
    run("off", "--display", "--bloom", "--display-pfm", "--pfm")
    r.Render(str(tmp_path / "pyoff"), tonemap=True, bloom=True)
    assert not (tmp_path / "off_dof.bmp").exists() and not (tmp_path / "pyoff_dof.bmp").exists()
    assert (tmp_path / "off.bmp").read_bytes() == (tmp_path / "cli.bmp").read_bytes() == (tmp_path / "py.bmp").read_bytes()
    assert np.array_equal(_words(_read_pfm(tmp_path / "off.pfm")), _words(f32.cpu().numpy()))
    plain = rtm.tonemap(rtm.bloom(f32)["f32"], want=("u8", "f32"))
    assert np.array_equal(_words(_read_pfm(tmp_path / "off_display.pfm")), _words(plain["f32"].cpu().numpy()))
    assert np.array_equal(_read_bmp(tmp_path / "pyoff_display.bmp"), plain["u8"].cpu().numpy())
    assert (tmp_path / "off_display.bmp").read_bytes() == (tmp_path / "pyoff_display.bmp").read_bytes()


def test_a_focus_pixel_on_a_miss_is_refused_before_anything_is_rendered(rtm, tmp_path):
    """scenes/settingData.json: three spheres in open space, so the frame's corners see the sky (the Cornell box is closed)."""
    import torch
    scene = json.load(open(OPEN_SCENE))
    scene["00 width"], scene["00 height"], scene["00 samples"], scene["00 superSamples"] = 64, 48, 4, 1
    small = tmp_path / "open.json"
    small.write_text(json.dumps(scene))
    r = rtm.Renderer(rtm.LoadData(str(small)).data, mode="repaired", max_bounces=8)
    depth = r.render_aov(want=("depth",))["depth"]
    miss, hit = torch.nonzero(torch.isinf(depth)), torch.nonzero(torch.isfinite(depth))
    assert len(miss) > 0 and len(hit) > 0 and bool(torch.isinf(depth[0, 0]))  # the case cannot skip itself
    for my, mx in ((0, 0), tuple(int(v) for v in miss[-1])):
        p = subprocess.run([CLI, "-json", str(small), "--max-bounces", "8", "--out", "x", "--dof", "--focus-pixel", f"{mx},{my}"],
                           cwd=tmp_path, capture_output=True, text=True, timeout=300)
        assert p.returncode == 2 and "miss" in p.stderr and f"{mx},{my}" in p.stderr, (p.returncode, p.stdout, p.stderr)
        assert not any((tmp_path / name).exists() for name in ("x.bmp", "x.jpg", "x_dof.bmp", "x_dof.jpg"))
        with pytest.raises(ValueError, match="miss"):
            r.focus_distance(pixel=(mx, my))
        with pytest.raises(ValueError, match="miss"):
            r.Render(str(tmp_path / "py"), dof={"focus_pixel": (mx, my)})
        with pytest.raises(ValueError, match="miss"):
            r.write_dof(str(tmp_path / "py"), focus_pixel=(mx, my))
        assert not any((tmp_path / name).exists() for name in ("py.bmp", "py.jpg", "py_dof.bmp", "py_dof.jpg"))
    # a pixel that hits is taken, by both
    hy, hx = (int(v) for v in hit[len(hit) // 2])
    z_at = float(depth[hy, hx].item())
    assert r.focus_distance(pixel=(hx, hy)) == z_at
    p = subprocess.run([CLI, "-json", str(small), "--max-bounces", "8", "--out", "y", "--dof", "--focus-pixel", f"{hx},{hy}"],
                       cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and f"dof: focus {z_at:.6g}, aperture 4, max radius 8" in p.stdout.splitlines(), p.stdout + p.stderr
    r.Render(str(tmp_path / "py"), dof={"focus_pixel": (hx, hy)})
    assert (tmp_path / "y_dof.bmp").read_bytes() == (tmp_path / "py_dof.bmp").read_bytes()


def test_a_quotient_that_overflows_counts_as_the_largest_float(rtm):
    """Step 2 with a depth tiny against the focus distance: zf / z = +inf.  aperture 0 still is the identity (s = -0, not
    NaN), any other aperture gives s = -R; the reference says the same."""
    w, h = 37, 23
    color, depth = (np.array(a) for a in _frame(w, h))
    tiny = np.zeros((h, w), bool)
    tiny[5:9, 10:20] = True
    tiny &= _defocus_ref.counts(color, depth)
    depth[tiny] = np.float32(1e-30)
    depth[6, 12] = np.float32(1e-45)  # a denormal depth
    ok = _defocus_ref.counts(color, depth)
    for zf, A, R in ((3e38, 0.0, 8), (4.0, 0.0, 16), (3e38, 4.0, 8), (1e10, 2.5, 4)):
        zf = float(np.float32(zf))
        ref, ref_s = _defocus_ref.defocus_ref(color, depth, zf, A, R)
        assert np.all(np.isfinite(ref[ok])) and np.all(np.isfinite(ref_s))
        out = _bits(rtm.defocus(_dev(color), _dev(depth), zf, A, R, want=ALL))
        assert _defocus_ref.tolerance_excess(out["f32"][ok], ref[ok]) <= TOL, (zf, A, R)
        assert _defocus_ref.tolerance_excess(out["coc"], ref_s) <= TOL, (zf, A, R)
        if A == 0.0:
            assert np.array_equal(_words(out["f32"]), _words(color)), (zf, R)
            assert np.all(out["coc"] == 0.0), (zf, R)
        else:
            assert np.all(out["coc"][tiny & (depth < 1e-20)] == -R), (zf, A, R)
