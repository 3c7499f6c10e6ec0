"""Resize on a real MI355X (-m gpu): rtm_resize against the NumPy float64 restatement (_resize_ref) on the smallest shapes at
which its kernels can go wrong — one pixel, equal sizes, both directions across a 64-lane block edge, a ratio of 32 whose
source span is staged in more than one chunk — for every filter and both channel counts; the 8-bit store bit for bit, the
consequences the header states, holes, determinism across calls, streams and alignments, and the Render / rtm_cli outputs.
test_resize_matches_the_reference prints the worst error of every shape; DESIGN.md records the largest per filter."""
import ctypes as C
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import _resize_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "raytracingmin_amd", "rtm_cli")
SCENE = os.path.join(ROOT, "scenes", "cornellBoxSetting.json")
TOL = 1e-4  # include/rtm.h: |got - ref| <= 1e-4 max(1, |ref|)
FILTERS = _resize_ref.FILTERS
# (w, h) -> (W, H): one pixel; equal size; both axes in opposite directions; two pixels across a 64-lane block edge, both
# ways; several blocks; ratio 32 (Tx = 193 for lanczos3: the 257-pixel span is staged in two chunks) and back
SHAPES = [((1, 1), (1, 1)), ((1, 1), (5, 3)), ((5, 3), (1, 1)), ((7, 5), (7, 5)), ((67, 35), (23, 51)), ((23, 51), (67, 35)),
          ((64, 9), (130, 9)), ((130, 9), (64, 9)), ((300, 70), (150, 35)), ((257, 3), (8, 3)), ((8, 3), (257, 3))]
HOLE_SIZES = [(16, 16), (8, 8), (32, 32), (5, 23), (48, 16)]  # (W, H); (23, 5) stays out: its D comes within 1.5e-3 of 1/16


@pytest.fixture(scope="module")
def rtm():
    import raytracingmin_amd as m
    n = C.c_int()
    m._lib.check(m.lib().rtm_device_count(C.byref(n)), "rtm_device_count")
    assert n.value >= 1
    return m


@functools.lru_cache(maxsize=None)
def _frame(w, h, channels):
    f = _resize_ref.frame(w, h, channels)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def _ref(w, h, W, H, channels, filter):
    """The float64 reference of a shape, computed once and shared."""
    out, D = _resize_ref.resize_ref(_frame(w, h, channels), (H, W), filter)
    out.setflags(write=False)
    return out


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


@pytest.mark.parametrize("src,dst", SHAPES, ids=[f"{a[0]}x{a[1]}-{b[0]}x{b[1]}" for a, b in SHAPES])
def test_resize_matches_the_reference(rtm, src, dst):
    (w, h), (W, H) = src, dst
    worst = dict.fromkeys(FILTERS, 0.0)
    for channels in (1, 3):
        frame = _frame(w, h, channels)
        assert int((frame == 12.0).reshape(h * w, -1).all(axis=1).sum()) == min(3, w * h)  # the light's emission
        cd = _dev(frame)
        for f in FILTERS:
            ref = _ref(w, h, W, H, channels, f)
            out = _bits(rtm.resize(cd, (H, W), f, want=("f32", "u8")))
            assert out["f32"].shape == ref.shape == ((H, W, 3) if channels == 3 else (H, W)) and out["u8"].shape == ref.shape
            assert np.all(np.isfinite(out["f32"])), (channels, f)
            err = _resize_ref.tolerance_excess(out["f32"], ref)
            print(f"{w}x{h} -> {W}x{H} C {channels} {f}: out_f32 {err:.3e}")
            assert err <= TOL, (channels, f, err)
            # the 8-bit store is rtm_quantise of the call's own out_f32: exact at every pixel
            assert np.array_equal(out["u8"], _host_quantise(rtm, out["f32"])), (channels, f)
            assert np.array_equal(out["u8"], _resize_ref.quantise_u8(out["f32"])), (channels, f)
            # a single output: the same bits
            only32, only8 = _bits(rtm.resize(cd, (H, W), f, want=("f32",))), _bits(rtm.resize(cd, (H, W), f, want=("u8",)))
            assert tuple(only32) == ("f32",) and tuple(only8) == ("u8",)
            assert np.array_equal(_words(only32["f32"]), _words(out["f32"])) and np.array_equal(only8["u8"], out["u8"]), (channels, f)
            worst[f] = max(worst[f], err)
        assert np.array_equal(_words(cd.cpu().numpy()), _words(frame))  # the input is left alone
    print(f"{w}x{h} -> {W}x{H}: worst error against the float64 reference: "
          + ", ".join(f"{f} {worst[f]:.3e}" for f in FILTERS) + f" (bar {TOL})")


def test_equal_size_box_and_triangle_return_every_pixel(rtm):
    for w, h in ((1, 1), (7, 5), (67, 35), (130, 9)):
        for channels in (1, 3):
            frame = _frame(w, h, channels)
            cd = _dev(frame)
            for f in ("box", "triangle"):
                out = _bits(rtm.resize(cd, (h, w), f))["f32"]
                assert np.array_equal(out, frame), (w, h, channels, f)  # ==: out is c / 1
            out = _bits(rtm.resize(cd, (h, w), "lanczos3"))["f32"]  # the input within the tolerance
            assert _resize_ref.tolerance_excess(out, frame) <= TOL, (w, h, channels)


def test_box_at_an_integer_ratio_is_the_block_mean(rtm):
    for fct in (2, 3):
        for channels in (1, 3):
            W, H = 67, 5
            frame = _frame(W * fct, H * fct, channels)
            out = _bits(rtm.resize(_dev(frame), (H, W), "box"))["f32"]
            mean = frame.astype(np.float64).reshape(H, fct, W, fct, -1).mean(axis=(1, 3)).reshape(out.shape)
            assert _resize_ref.tolerance_excess(out, mean) <= TOL, (fct, channels)


def test_a_constant_frame_stays_constant(rtm):
    for (w, h), (W, H) in SHAPES:
        for channels in (1, 3):
            value = np.float32([0.25, 3.0, 0.0])[:channels]
            frame = np.broadcast_to(value, (h, w, channels)).reshape((h, w, 3) if channels == 3 else (h, w)).copy()
            cd = _dev(frame)
            for f in FILTERS:
                out = _bits(rtm.resize(cd, (H, W), f))["f32"]
                want = np.broadcast_to(value.astype(np.float64), (H, W, channels)).reshape(out.shape)
                assert _resize_ref.tolerance_excess(out, want) <= TOL, (w, h, W, H, channels, f)


def test_holes_are_skipped_and_what_is_left_renormalised(rtm):
    for channels in (1, 3):
        frame = _resize_ref.holes_frame(channels)
        ok = _resize_ref.counts(frame)
        assert (~ok).sum() == 36 and np.array_equal(np.argwhere(~ok).min(axis=0), [3, 4]) and np.array_equal(np.argwhere(~ok).max(axis=0), [8, 9])
        if channels == 3:
            assert np.isposinf(frame[4, 5]).all() and np.isnan(frame[6, 7, 2]) and frame[6, 7, 0] == 1.5
        cd = _dev(frame)
        # the same frame with a constant where it counts: stays that constant around the holes
        flat = np.where(np.broadcast_to(ok.reshape(16, 16, *([1] * (frame.ndim - 2))), frame.shape), np.float32(2.75), frame)
        fd = _dev(flat.astype(np.float32))
        for W, H in HOLE_SIZES:
            for f in FILTERS:
                ref, D = _resize_ref.resize_ref(frame, (H, W), f)
                # on the reference first: no destination pixel sits at the threshold, so the mask is decided
                gap = float(np.min(np.abs(D - _resize_ref.MIN_WEIGHT)))
                assert gap >= 1e-3, (W, H, f, gap)
                mask = D < _resize_ref.MIN_WEIGHT
                out = _bits(rtm.resize(cd, (H, W), f, want=("f32", "u8")))
                got = out["f32"].reshape(H, W, -1)
                assert np.array_equal(np.isnan(got).all(axis=-1), mask) and np.array_equal(np.isnan(got).any(axis=-1), mask), (W, H, f)
                assert np.all(np.isfinite(got[~mask])), (W, H, f)  # no pixel outside the mask is non-finite
                assert _resize_ref.tolerance_excess(got[~mask], ref.reshape(H, W, -1)[~mask]) <= TOL, (W, H, f)
                assert np.array_equal(out["u8"], _host_quantise(rtm, out["f32"])) and np.all(out["u8"].reshape(H, W, -1)[mask] == 0)
                const = _bits(rtm.resize(fd, (H, W), f))["f32"].reshape(H, W, -1)
                assert np.array_equal(np.isnan(const).any(axis=-1), mask), (W, H, f)
                assert _resize_ref.tolerance_excess(const[~mask], np.full_like(const[~mask], 2.75, dtype=np.float64)) <= TOL, (W, H, f)
        if channels == 3 and (16, 16) in HOLE_SIZES:  # equal size, BOX: a hole stays exactly the hole
            out = _bits(rtm.resize(cd, (16, 16), "box"))["f32"]
            assert np.array_equal(np.isnan(out).all(axis=-1), ~ok) and np.array_equal(out[ok], frame[ok])


def _call(rtm, src_t, w, h, W, H, which, channels, work, out32, out8, stream):
    from raytracingmin_amd import _lib
    prm = _lib.rtm_resize_params(which, channels)
    _lib.check(rtm.lib().rtm_resize(C.byref(prm), w, h, W, H, 0, src_t.data_ptr(), work.data_ptr(),
                                    out32.data_ptr() if out32 is not None else None, out8.data_ptr() if out8 is not None else None,
                                    C.c_void_p(stream.cuda_stream)), "rtm_resize")


def test_the_same_inputs_give_the_same_bits(rtm):
    import torch
    L = rtm.lib()
    for (w, h), (W, H) in (((67, 35), (23, 51)), ((64, 9), (130, 9)), ((257, 3), (8, 3))):
        for channels in (1, 3):
            frame = _frame(w, h, channels)
            cd = _dev(frame)
            n_in, n_out = w * h * channels, W * H * channels
            shape = (H, W, 3) if channels == 3 else (H, W)
            for which, f in enumerate(FILTERS):
                first = _bits(rtm.resize(cd, (H, W), f, want=("f32", "u8")))
                assert _same_bits(first, _bits(rtm.resize(cd, (H, W), f, want=("f32", "u8")))), (w, h, channels, f)  # a second call
                work_bytes = L.rtm_resize_work_bytes(w, h, W, H, which, channels)
                cur = torch.cuda.current_stream()
                for words in (1, 2):  # src and out_f32 offset by 4 and by 8 bytes
                    sbuf = torch.empty(n_in + 8, dtype=torch.float32, device="cuda")
                    obuf = torch.empty(n_out + 8, dtype=torch.float32, device="cuda")
                    shifted, oshift = sbuf[words:words + n_in], obuf[words:words + n_out]
                    shifted.copy_(cd.reshape(-1))
                    assert cd.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 4 * words and oshift.data_ptr() % 16 == 4 * words
                    work = torch.empty(work_bytes, dtype=torch.uint8, device="cuda")
                    out8 = torch.empty(shape, dtype=torch.uint8, device="cuda")
                    _call(rtm, shifted, w, h, W, H, which, channels, work, oshift, out8, cur)
                    got = _bits({"f32": oshift.reshape(shape), "u8": out8})
                    assert _same_bits(first, got), (w, h, channels, f, words)
                # two calls on two streams with two work buffers
                side = torch.cuda.Stream()
                side.wait_stream(cur)
                third = rtm.resize(cd, (H, W), f, want=("f32", "u8"), stream=side)
                fourth = rtm.resize(cd, (H, W), f, want=("f32", "u8"))  # the current stream's, while the side stream may still run
                side.synchronize()
                assert _same_bits(first, _bits(third)) and _same_bits(first, _bits(fourth)), (w, h, channels, f)


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


def test_render_and_cli_resize_the_last_stage(rtm, tmp_path):
    import torch
    scene = json.load(open(SCENE))
    scene["00 width"], scene["00 height"], scene["00 samples"], scene["00 superSamples"] = 192, 108, 4, 1
    small = tmp_path / "small.json"
    small.write_text(json.dumps(scene))
    args = [CLI, "-json", str(small), "--max-bounces", "8"]

    def run(stem, *flags):
        p = subprocess.run(args + ["--out", stem] + list(flags), cwd=tmp_path, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout + p.stderr
        return p.stdout

    r = rtm.Renderer(rtm.LoadData(str(small)).data, mode="repaired", max_bounces=8)
    r.Render(str(tmp_path / "py"), resize=(96, 54), tonemap=True)
    f32 = torch.from_numpy(r.image).cuda().to(torch.float32)
    want = rtm.resize(f32, (54, 96), want=("f32", "u8"))  # Render's (W, H) is resize()'s (H, W); the default filter
    assert _read_bmp(tmp_path / "py.bmp").shape == (108, 192, 3)
    assert np.array_equal(_read_bmp(tmp_path / "py_resized.bmp"), want["u8"].cpu().numpy())
    assert (tmp_path / "py_resized.jpg").stat().st_size > 0
    shown = rtm.tonemap(want["f32"], want=("u8", "f32"))
    assert np.array_equal(_read_bmp(tmp_path / "py_display.bmp"), shown["u8"].cpu().numpy())  # 54 x 96: the resized frame's
    # write_resized alone, of self.image, with another filter
    back = r.write_resized(str(tmp_path / "w"), (27, 48), filter="lanczos3")
    assert tuple(back.shape) == (27, 48, 3)
    assert np.array_equal(_words(back.cpu().numpy()), _words(rtm.resize(f32, (27, 48), "lanczos3")["f32"].cpu().numpy()))
    assert _read_bmp(tmp_path / "w_resized.bmp").shape == (27, 48, 3)
    # rtm_cli: the same files, one line, and the resized frame is the last stage's
    text = run("cli", "--resize", "96x54", "--display", "--display-pfm", "--pfm")
    assert [l for l in text.splitlines() if l.startswith("resize:")] == ["resize: cli_resized.bmp, cli_resized.jpg (96 x 54)"], text
    assert (tmp_path / "cli_resized.bmp").read_bytes() == (tmp_path / "py_resized.bmp").read_bytes()
    assert (tmp_path / "cli_resized.jpg").read_bytes() == (tmp_path / "py_resized.jpg").read_bytes()
    assert (tmp_path / "cli.bmp").read_bytes() == (tmp_path / "py.bmp").read_bytes()
    assert np.array_equal(_words(_read_pfm(tmp_path / "cli.pfm")), _words(want["f32"].cpu().numpy()))
    assert np.array_equal(_words(_read_pfm(tmp_path / "cli_display.pfm")), _words(shown["f32"].cpu().numpy()))
    assert (tmp_path / "cli_display.bmp").read_bytes() == (tmp_path / "py_display.bmp").read_bytes()
    # the filter reaches the call; an enlargement in x with a reduction in y, of a denoised frame
    text = run("cli2", "--denoise", "--resize", "200x50", "--resize-filter", "triangle", "--pfm")
    den = rtm.denoise(f32, r.render_aov(), want=("f32",))["f32"]
    want2 = rtm.resize(den, (50, 200), "triangle")["f32"].cpu().numpy()
    assert np.array_equal(_words(_read_pfm(tmp_path / "cli2.pfm")), _words(want2))
    r.Render(str(tmp_path / "py2"), denoise=True, resize=(200, 50, "triangle"))
    assert (tmp_path / "py2_resized.bmp").read_bytes() == (tmp_path / "cli2_resized.bmp").read_bytes()
    # without --resize: no resized file, and the display file has the render's size
    run("off", "--display")
    r.Render(str(tmp_path / "pyoff"), tonemap=True)
    assert not (tmp_path / "off_resized.bmp").exists() and not (tmp_path / "pyoff_resized.bmp").exists()
    assert _read_bmp(tmp_path / "off_display.bmp").shape == (108, 192, 3)
    assert (tmp_path / "off_display.bmp").read_bytes() == (tmp_path / "pyoff_display.bmp").read_bytes()
