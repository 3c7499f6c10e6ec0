"""Bloom on a real MI355X (-m gpu): rtm_bloom against the NumPy float64 restatement (_bloom_ref) on synthetic HDR frames of
every halving case, the pixels that do not count, the 8-bit store bit for bit, the properties the definition implies, the
16-byte and the plain load path, in-place use, determinism across calls and streams, and the Render / rtm_cli outputs."""
import ctypes as C
import itertools
import json
import os
import subprocess

import numpy as np
import pytest

import _bloom_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "raytracingmin_amd", "rtm_cli")
SCENE = os.path.join(ROOT, "scenes", "cornellBoxSetting.json")
TOL = 1e-4  # include/rtm.h: |got - ref| <= 1e-4 max(1, |ref|), for out_f32 of counting pixels and for bloom_out
# one pixel; single rows and columns; every ceil-halving case; 131 x 63 and 258 x 66: a level-1 plane of more than one 32 x 8
# tile in both axes with ragged edges; at 8 levels every frame ends in levels that have collapsed to 1 x 1
FRAMES = [(1, 1), (1, 17), (17, 1), (2, 2), (7, 5), (37, 23), (64, 64), (131, 63), (258, 66)]
CASES = list(itertools.product((0.0, 1.0, 3.0), (0.0, 0.5, 1.0), (0.0, 0.7, 1.0), (1, 3, 8)))  # threshold, knee, scatter, levels
SUBSET = CASES[::10]  # nine of the 81, fixed: for 258 x 66
INTENSITY = 0.2


@pytest.fixture(scope="module")
def rtm():
    import raytracingmin_amd as m
    n = C.c_int()
    m._lib.check(m.lib().rtm_device_count(C.byref(n)), "rtm_device_count")
    assert n.value >= 1
    return m


def _frame(w, h):
    """test_tonemap_gpu's recipe: 8 u^4, a long dark tail and highlights above 1; 10 % exactly black; one negative component;
    beyond two pixels one NaN pixel and one +inf pixel."""
    rng = np.random.default_rng(w * 1000 + h)
    color = (8 * rng.random((h, w, 3)) ** 4).astype(np.float32)
    color[rng.random((h, w)) < 0.1] = 0.0
    flat = color.reshape(-1, 3)
    flat[0] = [0.75, -0.25, 1.5]
    if w * h > 2:
        flat[(w * h) // 2] = [np.nan, 0.5, 0.5]
        flat[w * h - 1] = [0.5, np.inf, 0.5]
    return color


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


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
    return all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in a) and set(a) == set(b)


ALL = ("f32", "u8", "bloom")


@pytest.mark.parametrize("w,h", FRAMES)
def test_bloom_matches_the_reference(rtm, w, h):
    color = _frame(w, h)
    cd = _dev(color)
    ok = _bloom_ref.counts(color)
    worst = 0.0
    for threshold, knee, scatter, levels in (SUBSET if (w, h) == (258, 66) else CASES):
        kw = dict(threshold=threshold, knee=knee, intensity=INTENSITY, scatter=scatter, levels=levels)
        ref, ref_b = _bloom_ref.bloom_ref(color, **kw)
        out = _bits(rtm.bloom(cd, want=ALL, **kw))
        err = _bloom_ref.tolerance_excess(out["f32"][ok], ref[ok])
        err_b = _bloom_ref.tolerance_excess(out["bloom"], ref_b)
        print(f"{w}x{h} threshold {threshold} knee {knee} scatter {scatter} levels {levels}: out_f32 {err:.3e}, bloom_out {err_b:.3e}")
        assert err <= TOL, (kw, err)
        assert err_b <= TOL, (kw, err_b)
        # a pixel that does not count keeps its words
        assert np.array_equal(out["f32"][~ok].view(np.uint32), color[~ok].view(np.uint32)), kw
        # the 8-bit store is rtm_quantise of the call's own out_f32, component by component: exact at every pixel, 0 where the
        # component is below the range or NaN (rtm_quantise takes +inf, like everything above 1, to 255)
        assert np.array_equal(out["u8"], _host_quantise(rtm, out["f32"])), kw
        with np.errstate(invalid="ignore"):
            outside = ~(out["f32"] >= 0.0)
        assert np.all(out["u8"][outside] == 0), kw
        if w * h > 2:
            assert outside[~ok].sum() == 1 and np.all(out["u8"][~ok][np.isposinf(out["f32"][~ok])] == 255), kw
        worst = max(worst, err, err_b)
    print(f"{w}x{h}: worst error against the float64 reference {worst:.3e} (bar {TOL})")


def test_zero_intensity_leaves_counting_pixels_equal_to_the_input(rtm):
    for w, h in ((7, 5), (131, 63)):
        color = _frame(w, h)
        out = _bits(rtm.bloom(_dev(color), threshold=0.5, intensity=0.0, want=ALL))
        assert np.array_equal(out["f32"].view(np.uint32), color.view(np.uint32))  # c + 0 B: the pixels that count, too
        assert np.any(out["bloom"] > 0)


def test_a_threshold_above_the_maximum_leaves_the_bloom_plus_zero(rtm):
    for w, h in ((1, 1), (37, 23), (131, 63)):
        color = _frame(w, h)
        ok = _bloom_ref.counts(color)
        y_max = float(np.max((_bloom_ref.bright_pass(color, 0.0, 0.0) @ np.array(_bloom_ref.LUM))))
        for knee, threshold in ((0.0, 1.00001 * y_max), (0.5, 2.0 * y_max + 1e-3)):  # every float Y at or below T - K
            for levels in (1, 4, 8):
                out = _bits(rtm.bloom(_dev(color), threshold=float(threshold), knee=knee, levels=levels, want=ALL))
                assert np.all(out["bloom"].view(np.uint32) == 0), (w, h, knee, levels)  # +0, not -0
                assert np.array_equal(out["f32"][ok].view(np.uint32), color[ok].view(np.uint32))


def test_a_constant_frame_blooms_to_itself(rtm):
    c = np.array([0.25, 3.0, 0.0], np.float32)
    for w, h in ((1, 1), (7, 5), (131, 63)):
        color = np.broadcast_to(c, (h, w, 3)).copy()
        for scatter, levels in ((0.0, 1), (0.7, 6), (1.0, 8)):
            out = _bits(rtm.bloom(_dev(color), threshold=0.0, intensity=0.5, scatter=scatter, levels=levels, want=ALL))
            assert _bloom_ref.tolerance_excess(out["bloom"], np.broadcast_to(c, (h, w, 3))) <= TOL, (w, h, levels)
            assert _bloom_ref.tolerance_excess(out["f32"], np.broadcast_to(1.5 * c, (h, w, 3))) <= TOL, (w, h, levels)


def test_a_nan_pixel_adds_the_light_of_a_black_one(rtm):
    w, h = 37, 23
    color = _frame(w, h)
    ok = _bloom_ref.counts(color)
    assert (~ok).sum() == 2
    black = color.copy()
    black[~ok] = 0.0
    for levels in (1, 6):
        a = _bits(rtm.bloom(_dev(color), threshold=0.5, levels=levels, want=ALL))
        b = _bits(rtm.bloom(_dev(black), threshold=0.5, levels=levels, want=ALL))
        assert np.array_equal(a["bloom"].view(np.uint32), b["bloom"].view(np.uint32))
        assert np.array_equal(a["f32"][ok].view(np.uint32), b["f32"][ok].view(np.uint32))
        assert np.array_equal(a["u8"][ok], b["u8"][ok])


def test_a_misaligned_colour_tensor_gives_the_aligned_bits(rtm):
    import torch
    w, h = 131, 63
    color = _frame(w, h)
    aligned = _dev(color)
    buf = torch.empty(w * h * 3 + 8, dtype=torch.float32, device="cuda")
    shifted = buf[1:1 + w * h * 3].view(h, w, 3)
    shifted.copy_(aligned)
    assert aligned.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    for kw in (dict(), dict(threshold=0.0, levels=1), dict(threshold=3.0, knee=1.0, scatter=1.0, levels=8)):
        assert _same_bits(_bits(rtm.bloom(aligned, want=ALL, **kw)), _bits(rtm.bloom(shifted, want=ALL, **kw))), kw


def test_in_place_gives_the_out_of_place_bits(rtm):
    color = _frame(131, 63)
    for kw in (dict(), dict(threshold=0.0, intensity=1.0, levels=1), dict(threshold=3.0, scatter=0.0, levels=8)):
        want = _bits(rtm.bloom(_dev(color), want=ALL, **kw))
        cd = _dev(color)
        got = rtm.bloom(cd, want=ALL, out_f32=cd, **kw)
        assert got["f32"].data_ptr() == cd.data_ptr()
        assert _same_bits(_bits(got), want), kw


def test_the_same_inputs_give_the_same_bits_on_every_call_and_stream(rtm):
    import torch
    cd = _dev(_frame(131, 63))
    first = _bits(rtm.bloom(cd, want=ALL))
    second = _bits(rtm.bloom(cd, want=ALL))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    third = rtm.bloom(cd, want=ALL, stream=side)  # its own work buffer
    fourth = rtm.bloom(cd, want=ALL)  # the current stream's, enqueued while the side stream may still run
    side.synchronize()
    assert _same_bits(first, second) and _same_bits(first, _bits(third)) and _same_bits(first, _bits(fourth))


def test_the_bloom_plane_alone(rtm):
    color = _frame(37, 23)
    cd = _dev(color)
    both = _bits(rtm.bloom(cd, want=ALL))
    for want in (("bloom",), ("u8",), ("f32",)):
        out = rtm.bloom(cd, want=want)
        assert tuple(out) == want
        out = _bits(out)
        assert np.array_equal(out[want[0]].view(np.uint8), both[want[0]].view(np.uint8)), want
    assert np.array_equal(cd.cpu().numpy().view(np.uint32), color.view(np.uint32))  # the input is left alone


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


def test_write_display_blooms_before_the_display_transform(rtm, tmp_path):
    color = _frame(64, 64)
    color[~_bloom_ref.counts(color)] = 4.0
    cd = _dev(color)
    data = rtm.LoadData(SCENE).data
    data.width, data.height, data.samples, data.superSamples = 64, 64, 4, 1
    r = rtm.Renderer(data, mode="repaired", max_bounces=8)
    plain = r.write_display(str(tmp_path / "plain"), frame=cd)
    for name, arg, kw in (("on", True, {}), ("prm", dict(threshold=0.5, intensity=0.6, levels=3), dict(threshold=0.5, intensity=0.6, levels=3))):
        shown = r.write_display(str(tmp_path / name), frame=cd, bloom=arg)
        want = rtm.tonemap(rtm.bloom(cd, **kw)["f32"], want=("u8",))["u8"].cpu().numpy()
        assert np.array_equal(shown, want) and np.array_equal(_read_bmp(tmp_path / (name + "_display.bmp")), want), name
        assert not np.array_equal(shown, plain), name
    assert np.array_equal(cd.cpu().numpy(), color)  # the caller's frame is not bloomed in place
    assert np.array_equal(r.write_display(str(tmp_path / "off"), frame=cd, bloom=False), plain)


def test_render_and_cli_bloom_the_displayed_frame(rtm, tmp_path):
    import torch
    scene = json.load(open(SCENE))
    scene["00 width"], scene["00 height"], scene["00 samples"], scene["00 superSamples"] = 64, 48, 4, 1
    small = tmp_path / "small.json"
    small.write_text(json.dumps(scene))
    args = [CLI, "-json", str(small), "--max-bounces", "8"]

    def run(stem, *flags):
        p = subprocess.run(args + ["--out", stem] + list(flags), cwd=tmp_path, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout + p.stderr
        return p.stdout

    r = rtm.Renderer(rtm.LoadData(str(small)).data, mode="repaired", max_bounces=8)
    r.Render(str(tmp_path / "py"), tonemap=True, bloom=True)
    f32 = torch.from_numpy(r.image).cuda().to(torch.float32)
    bloomed = rtm.bloom(f32)["f32"]
    assert not torch.equal(bloomed, f32)  # the Cornell light is above the threshold
    want = rtm.tonemap(bloomed, want=("u8", "f32"))
    assert np.array_equal(_read_bmp(tmp_path / "py_display.bmp"), want["u8"].cpu().numpy())
    text = run("cli", "--display", "--bloom", "--display-pfm")
    line = [l for l in text.splitlines() if l.startswith("bloom:")]
    assert len(line) == 1 and line[0] == "bloom: threshold 1, knee 0.5, intensity 0.2, scatter 0.7, levels 6", text
    shown = _read_pfm(tmp_path / "cli_display.pfm")
    assert np.array_equal(shown.view(np.uint32), want["f32"].cpu().numpy().view(np.uint32))
    assert (tmp_path / "cli_display.bmp").read_bytes() == (tmp_path / "py_display.bmp").read_bytes()
    # without --bloom: another display frame, and the files rtm_cli wrote before
    run("off", "--display", "--display-pfm")
    assert not np.array_equal(_read_pfm(tmp_path / "off_display.pfm"), shown)
    assert np.array_equal(_read_pfm(tmp_path / "off_display.pfm").view(np.uint32),
                          rtm.tonemap(f32, want=("f32",))["f32"].cpu().numpy().view(np.uint32))
    assert (tmp_path / "off.bmp").read_bytes() == (tmp_path / "cli.bmp").read_bytes() == (tmp_path / "py.bmp").read_bytes()
    # the flags reach the call
    run("cli2", "--display", "--bloom", "0.5", "--bloom-threshold", "0.25", "--bloom-levels", "3", "--display-pfm")
    want2 = rtm.tonemap(rtm.bloom(f32, intensity=0.5, threshold=0.25, levels=3)["f32"], want=("f32",))["f32"].cpu().numpy()
    assert np.array_equal(_read_pfm(tmp_path / "cli2_display.pfm").view(np.uint32), want2.view(np.uint32))
