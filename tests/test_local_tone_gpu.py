"""The local tone operator on a real MI355X (-m gpu): rtm_tonemap_local against the NumPy float64 restatement (_local_tone_ref)
on synthetic HDR frames of every halving case, the pixels that do not count, the 8-bit store bit for bit, the device statistics
as the anchor, the consequences the header states, the 16-byte and the plain load path, in-place use, determinism across calls
and streams, and the Render / rtm_cli outputs against the three C calls made by hand."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import _local_tone_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "raytracingmin_amd", "rtm_cli")
SCENE = os.path.join(ROOT, "scenes", "cornellBoxSetting.json")
TOL = 1e-4  # include/rtm.h: |got - ref| <= 1e-4 max(1, |ref|), for out_f32 and for fused_out
ALL = ("f32", "u8", "fused")


@pytest.fixture(scope="module")
def rtm():
    import raytracingmin_amd as m
    n = C.c_int()
    m._lib.check(m.lib().rtm_device_count(C.byref(n)), "rtm_device_count")
    assert n.value >= 1
    return m


def _frame(w, h):
    """test_bloom_gpu's recipe: 8 u^4, a long dark tail and highlights above 1; 10 % exactly black; one negative component;
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


def _kw(case):
    """A case of the product as tonemap_local's arguments; the float parameters as the floats the library receives."""
    anchor, shadows, highlights, sigma, levels = case
    return dict(anchor=anchor, shadows=shadows, highlights=highlights, sigma=float(np.float32(sigma)), levels=levels)


@pytest.mark.parametrize("w,h", ref.FRAMES)
def test_local_matches_the_reference(rtm, w, h):
    color = _frame(w, h)
    cd = _dev(color)
    ok = ref.counts(color)
    worst = 0.0
    for case in (ref.SUBSET9 if (w, h) == (258, 66) else ref.SUBSET):
        kw = _kw(case)
        want, want_f = ref.local_ref(color, **kw)
        out = _bits(rtm.tonemap_local(cd, want=ALL, **kw))
        err = ref.tolerance_excess(out["f32"], want)
        err_f = ref.tolerance_excess(out["fused"], want_f)
        print(f"{w}x{h} {kw}: out_f32 {err:.3e}, fused_out {err_f:.3e}")
        assert err <= TOL, (kw, err)
        assert err_f <= TOL, (kw, err_f)
        # a pixel that does not count is exactly zero
        assert np.all(out["f32"][~ok].view(np.uint32) == 0) and np.all(out["u8"][~ok] == 0), kw
        assert np.all(np.isfinite(out["f32"])) and np.all(out["fused"] >= 0.0) and np.all(out["fused"] <= 1.0), kw
        # the 8-bit store is rtm_quantise of the call's own out_f32, component by component
        assert np.array_equal(out["u8"], _host_quantise(rtm, out["f32"])), kw
        worst = max(worst, err, err_f)
    print(f"{w}x{h}: worst error against the float64 reference {worst:.3e} (bar {TOL})")


def test_device_statistics_give_the_bits_of_their_exposure_in_the_anchor(rtm):
    for w, h in ((7, 5), (131, 63)):
        cd = _dev(_frame(w, h))
        for key, levels in ((0.18, 5), (0.5, 0), (0.05, 8)):
            stats = rtm.tonemap(cd, key=key, want=("stats",))["stats"]  # on the device: nothing is read back for the call
            with_stats = _bits(rtm.tonemap_local(cd, stats=stats, levels=levels, want=ALL))
            E = rtm.tonemap_stats(stats)["exposure"]
            assert np.isfinite(E) and E > 0 and E != 1.0
            assert _same_bits(with_stats, _bits(rtm.tonemap_local(cd, anchor=E, levels=levels, want=ALL))), (w, h, key)
            assert not _same_bits(with_stats, _bits(rtm.tonemap_local(cd, levels=levels, want=ALL)))


def test_equal_exposures_give_simple_reinhard_at_every_level_count(rtm):
    # (a)
    for w, h in ((1, 1), (37, 23), (131, 63)):
        color = _frame(w, h)
        for anchor, sigma in ((0.25, 0.1), (16.0, 1.0)):
            _, x = ref.exposed(color, anchor)
            for levels in (0, 1, 3, 8):
                out = _bits(rtm.tonemap_local(_dev(color), anchor=anchor, shadows=0.0, highlights=0.0, sigma=sigma, levels=levels,
                                              want=("fused",)))
                assert ref.tolerance_excess(out["fused"], x / (1 + x)) <= TOL, (w, h, anchor, levels)


def test_a_constant_frame_gives_what_levels_zero_gives(rtm):
    # (b)
    c = np.array([0.25, 3.0, 0.0], np.float32)
    for w, h in ((1, 1), (7, 5), (131, 63)):
        cd = _dev(np.broadcast_to(c, (h, w, 3)).copy())
        for kw in (dict(), dict(anchor=0.01, shadows=4.0, highlights=0.0), dict(anchor=16.0, shadows=0.0, highlights=8.0)):
            flat = _bits(rtm.tonemap_local(cd, levels=0, want=ALL, **kw))
            for levels in (1, 5, 8):
                out = _bits(rtm.tonemap_local(cd, levels=levels, want=ALL, **kw))
                assert ref.tolerance_excess(out["fused"], flat["fused"].astype(np.float64)) <= TOL, (w, h, levels, kw)
                assert ref.tolerance_excess(out["f32"], flat["f32"].astype(np.float64)) <= TOL, (w, h, levels, kw)


def test_levels_zero_is_pointwise(rtm):
    # (c): the same pixels in another order give the same bits in that order
    w, h = 37, 23
    color = _frame(w, h)
    perm = np.random.default_rng(3).permutation(w * h)
    shuffled = color.reshape(-1, 3)[perm].reshape(h, w, 3)
    for kw in (dict(), dict(anchor=16.0, shadows=4.0, highlights=0.0, sigma=0.1)):
        a = _bits(rtm.tonemap_local(_dev(color), levels=0, want=ALL, **kw))
        b = _bits(rtm.tonemap_local(_dev(shuffled), levels=0, want=ALL, **kw))
        assert np.array_equal(a["f32"].reshape(-1, 3)[perm].view(np.uint32), b["f32"].reshape(-1, 3).view(np.uint32))
        assert np.array_equal(a["fused"].reshape(-1)[perm].view(np.uint32), b["fused"].reshape(-1).view(np.uint32))
        assert np.array_equal(a["u8"].reshape(-1, 3)[perm], b["u8"].reshape(-1, 3))


def test_a_misaligned_colour_tensor_gives_the_aligned_bits(rtm):
    import torch
    w, h = 131, 63
    color = _frame(w, h)
    aligned = _dev(color)
    buf = torch.empty(w * h * 3 + 8, dtype=torch.float32, device="cuda")
    shifted = buf[1:1 + w * h * 3].view(h, w, 3)
    shifted.copy_(aligned)
    assert aligned.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    for kw in (dict(), dict(levels=0), dict(levels=1), dict(anchor=16.0, shadows=4.0, sigma=0.1, levels=8)):
        assert _same_bits(_bits(rtm.tonemap_local(aligned, want=ALL, **kw)), _bits(rtm.tonemap_local(shifted, want=ALL, **kw))), kw


def test_in_place_gives_the_out_of_place_bits(rtm):
    color = _frame(131, 63)
    for kw in (dict(), dict(levels=0), dict(levels=1), dict(anchor=0.25, highlights=4.0, levels=8)):
        want = _bits(rtm.tonemap_local(_dev(color), want=ALL, **kw))
        cd = _dev(color)
        got = rtm.tonemap_local(cd, want=ALL, out_f32=cd, **kw)
        assert got["f32"].data_ptr() == cd.data_ptr()
        assert _same_bits(_bits(got), want), kw


def test_the_same_inputs_give_the_same_bits_on_every_call_and_stream(rtm):
    import torch
    cd = _dev(_frame(131, 63))
    first = _bits(rtm.tonemap_local(cd, want=ALL))
    second = _bits(rtm.tonemap_local(cd, want=ALL))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    third = rtm.tonemap_local(cd, want=ALL, stream=side)  # its own work buffer
    fourth = rtm.tonemap_local(cd, want=ALL)  # the current stream's, enqueued while the side stream may still run
    side.synchronize()
    assert _same_bits(first, second) and _same_bits(first, _bits(third)) and _same_bits(first, _bits(fourth))


def test_each_output_alone(rtm):
    color = _frame(37, 23)
    cd = _dev(color)
    every = _bits(rtm.tonemap_local(cd, want=ALL))
    for want in (("fused",), ("u8",), ("f32",)):
        out = rtm.tonemap_local(cd, want=want)
        assert tuple(out) == want
        out = _bits(out)
        assert np.array_equal(out[want[0]].view(np.uint8), every[want[0]].view(np.uint8)), want
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


def _by_hand(rtm, f32, local_prm, auto, ev, key=0.18):
    """The display path of --display local from the three C calls: (u8, f32) of the shown frame."""
    import torch
    _lib = rtm._lib
    L = rtm.lib()
    H, W = f32.shape[:2]
    dev = f32.device.index
    work = torch.empty(max(256, L.rtm_tonemap_work_bytes(W, H)), dtype=torch.uint8, device=f32.device)
    pyramid = torch.empty(max(256, L.rtm_tonemap_local_work_bytes(W, H, local_prm[4])), dtype=torch.uint8, device=f32.device)
    stats = torch.zeros(4, dtype=torch.int32, device=f32.device)
    fused = torch.empty_like(f32)
    shown32 = torch.empty_like(f32)
    shown8 = torch.empty((H, W, 3), dtype=torch.uint8, device=f32.device)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    curve = _lib.rtm_tonemap_params(_lib.TONEMAP_OPS["aces"], _lib.TRANSFERS["srgb"], int(auto), 1, 0.0 if auto else ev, key, 0.0)
    store = _lib.rtm_tonemap_params(_lib.TONEMAP_OPS["clamp"], _lib.TRANSFERS["srgb"], 0, 1, 0.0, key, 0.0)
    prm = _lib.rtm_tonemap_local_params(1.0 if auto else 2.0 ** ev, *local_prm[1:])
    if auto:
        _lib.check(L.rtm_tonemap(C.byref(curve), W, H, dev, f32.data_ptr(), work.data_ptr(), None, None, stats.data_ptr(), stream),
                   "rtm_tonemap")
    _lib.check(L.rtm_tonemap_local(C.byref(prm), W, H, dev, f32.data_ptr(), stats.data_ptr() if auto else None, pyramid.data_ptr(),
                                   fused.data_ptr(), None, None, stream), "rtm_tonemap_local")
    _lib.check(L.rtm_tonemap(C.byref(store), W, H, dev, fused.data_ptr(), work.data_ptr(), shown32.data_ptr(), shown8.data_ptr(),
                             None, stream), "rtm_tonemap")
    torch.cuda.synchronize()
    return shown8.cpu().numpy(), shown32.cpu().numpy()


def test_render_and_cli_show_the_frame_of_the_three_calls(rtm, tmp_path):
    import torch
    scene = json.load(open(SCENE))
    scene["00 width"], scene["00 height"], scene["00 samples"], scene["00 superSamples"] = 64, 64, 16, 1
    small = tmp_path / "small.json"
    small.write_text(json.dumps(scene))
    args = [CLI, "-json", str(small), "--max-bounces", "8"]

    def run(stem, *flags):
        p = subprocess.run(args + ["--out", stem] + list(flags), cwd=tmp_path, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout + p.stderr
        return p.stdout

    r = rtm.Renderer(rtm.LoadData(str(small)).data, mode="repaired", max_bounces=8)
    r.Render(str(tmp_path / "result"), tonemap=True, local=True)
    f32 = torch.from_numpy(r.image).cuda().to(torch.float32)
    u8, shown = _by_hand(rtm, f32, (1.0, 2.0, 2.0, 0.25, 5), True, 0.0)
    assert np.array_equal(_read_bmp(tmp_path / "result_display.bmp"), u8)
    text = run("cli", "--display", "local", "--display-pfm")
    line = [l for l in text.splitlines() if l.startswith("local:")]
    assert len(line) == 1 and line[0] == "local: shadows 2, highlights 2, sigma 0.25, levels 5", text
    assert np.array_equal(_read_pfm(tmp_path / "cli_display.pfm").view(np.uint32), shown.view(np.uint32))
    assert (tmp_path / "cli_display.bmp").read_bytes() == (tmp_path / "result_display.bmp").read_bytes()
    # another frame than the global curve's, and the plain files rtm_cli and Render wrote before
    global_u8 = rtm.tonemap(f32, want=("u8",))["u8"].cpu().numpy()
    assert not np.array_equal(u8, global_u8)
    assert (tmp_path / "cli.bmp").read_bytes() == (tmp_path / "result.bmp").read_bytes()
    # the flags and a fixed exposure reach the calls
    run("cli2", "--display", "local", "--exposure", "1", "--local-shadows", "3", "--local-highlights", "1", "--local-sigma", "0.5",
        "--local-levels", "2", "--display-pfm")
    u8_2, shown_2 = _by_hand(rtm, f32, (1.0, 3.0, 1.0, 0.5, 2), False, 1.0)
    assert np.array_equal(_read_pfm(tmp_path / "cli2_display.pfm").view(np.uint32), shown_2.view(np.uint32))
    assert np.array_equal(_read_bmp(tmp_path / "cli2_display.bmp"), u8_2)
    py2 = r.write_display(str(tmp_path / "py2"), frame=f32, exposure=1.0, local=dict(shadows=3.0, highlights=1.0, sigma=0.5, levels=2))
    assert np.array_equal(py2, u8_2)
