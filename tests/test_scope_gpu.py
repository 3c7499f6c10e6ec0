"""The frame scopes on a real MI355X (-m gpu): rtm_scopes against the NumPy restatement (_scope_ref), word for word, on frames
from one pixel to several blocks and strips, in both modes, at columns 1, the width and a count that divides nothing; constant
frames (every lane on one bin) and frames without a counting pixel; the count rules on the device's words; every subset of
the outputs; calls, streams and alignments; rtm_scope_draw's bytes; Renderer.scopes, Renderer.write_scopes and rtm_cli."""
import ctypes as C
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import _scope_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "raytracingmin_amd", "rtm_cli")
SCENE = os.path.join(ROOT, "scenes", "cornellBoxSetting.json")
# (width, height, a column count that divides nothing; None where the width leaves none)
# the last frame has more pixels than one launch of the histogram has lanes (256 blocks of 1024): its grid stride takes a
# second, partial trip
FRAMES = [(1, 1, None), (1, 9, None), (9, 1, 2), (7, 5, 3), (33, 17, 5), (64, 64, 5), (131, 63, 5), (257, 129, 100), (641, 411, 7)]
MODES = ("log2", "code")


@pytest.fixture(scope="module")
def rtm():
    import raytracingmin_amd as m
    n = C.c_int()
    m._lib.check(m.lib().rtm_device_count(C.byref(n)), "rtm_device_count")
    assert n.value >= 1
    return m


@functools.lru_cache(maxsize=None)
def _frame(w, h, mode):
    """The linear frame for LOG2, the display frame for CODE: computed once, shared, read-only."""
    f = ref.frame(w, h, 1000 * w + h, display=(mode == "code"))
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def _ref_hist(w, h, mode):
    return ref.words(ref.histogram(_frame(w, h, mode), ref.MODES[mode]))


@functools.lru_cache(maxsize=None)
def _ref_wave(w, h, mode, columns):
    return ref.waveform(_frame(w, h, mode), ref.MODES[mode], columns)


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()  # (a copy: the cached frames are read-only)


def _host(out):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().view(np.uint32).copy() for k, v in out.items()}


def _columns(w, odd):
    return sorted({1, w} | ({odd} if odd else set()))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("w,h,odd", FRAMES)
def test_histogram_and_waveform_equal_the_reference_word_for_word(rtm, w, h, odd, mode):
    cd = _dev(_frame(w, h, mode))
    want_hist = _ref_hist(w, h, mode)
    alone = _host(rtm.scopes(cd, mode=mode))["histogram"]
    assert np.array_equal(alone, want_hist), np.flatnonzero(alone != want_hist)[:8]
    for columns in _columns(w, odd):
        got = _host(rtm.scopes(cd, mode=mode, columns=columns, want=("histogram", "waveform")))
        want_wave = _ref_wave(w, h, mode, columns)
        assert got["waveform"].shape == (4, 256, columns)
        assert np.array_equal(got["waveform"], want_wave), (columns, np.argwhere(got["waveform"] != want_wave)[:8])
        assert np.array_equal(got["histogram"], want_hist), (columns, np.flatnonzero(got["histogram"] != want_hist)[:8])
        ref.invariants(ref.from_words(got["histogram"]), got["waveform"], w * h)  # the count rules, on the device's words
        only = _host(rtm.scopes(cd, mode=mode, columns=columns, want=("waveform",)))  # every subset gives the same words
        assert np.array_equal(only["waveform"], got["waveform"]), columns
    assert np.array_equal(cd.cpu().numpy().view(np.uint32), _frame(w, h, mode).view(np.uint32))  # the input is left alone


@pytest.mark.parametrize("w,h,columns", [(7, 5, 3), (64, 64, 64), (131, 63, 5), (257, 129, 100)])
def test_constant_frames_and_frames_without_a_counting_pixel(rtm, w, h, columns):
    import torch
    # every lane of every wave hits one bin per channel
    for mode, colour in (("log2", (0.18, 1.0, 65536.0)), ("log2", (0.0, -1.0, 1e-40)), ("code", (0.5, 1.0, 0.0)), ("code", (-0.5, 2.0, 0.25))):
        f = np.broadcast_to(np.array(colour, np.float32), (h, w, 3)).copy()
        got = _host(rtm.scopes(_dev(f), mode=mode, columns=columns, want=("histogram", "waveform")))
        assert np.array_equal(got["histogram"], ref.words(ref.histogram(f, ref.MODES[mode]))), (mode, colour)
        assert np.array_equal(got["waveform"], ref.waveform(f, ref.MODES[mode], columns)), (mode, colour)
        hist = ref.from_words(_host(rtm.scopes(_dev(f), mode=mode))["histogram"])
        assert hist["pixels"] == w * h and np.array_equal(ref.words(hist), got["histogram"])
        assert np.count_nonzero(ref.words(hist)[:1032]) == 4  # one bin, or below, or above, per channel
    # a constant frame with one other pixel in the middle of a wave, and one that does not count
    f = np.full((h, w, 3), 0.25, np.float32)
    f[h // 2, w // 2] = (3.0, 0.5, 1e-9)
    f[0, 0, 1] = np.nan
    for mode in MODES:
        got = _host(rtm.scopes(_dev(f), mode=mode, columns=columns, want=("histogram", "waveform")))
        assert np.array_equal(got["histogram"], ref.words(ref.histogram(f, ref.MODES[mode])))
        assert np.array_equal(got["waveform"], ref.waveform(f, ref.MODES[mode], columns))
        assert np.array_equal(_host(rtm.scopes(_dev(f), mode=mode))["histogram"], got["histogram"])
    # no pixel counts
    for bad in (np.nan, np.inf, -np.inf):
        f = np.full((h, w, 3), 0.5, np.float32)
        f[..., (w + h) % 3] = bad
        for want in (("histogram",), ("histogram", "waveform")):
            got = _host(rtm.scopes(_dev(f), columns=columns, want=want))
            hist = ref.from_words(got["histogram"])
            assert hist["pixels"] == 0 and hist["not_counting"] == w * h and not got["histogram"][:1032].any()
            assert "waveform" not in got or not got["waveform"].any()
            assert rtm.scope_percentile(got["histogram"], 50) == (1.0, -2)
    torch.cuda.synchronize()


def test_the_same_inputs_give_the_same_words(rtm):
    import torch
    w, h, columns = 131, 63, 5
    for mode in MODES:
        color = _frame(w, h, mode)
        cd = _dev(color)
        buf = torch.empty(w * h * 3 + 8, dtype=torch.float32, device="cuda")
        shifted = buf[1:1 + w * h * 3].view(h, w, 3)
        shifted.copy_(cd)
        assert cd.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
        both = ("histogram", "waveform")
        same = lambda a, b: set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in a)
        for want in (both, ("histogram",)):
            first = _host(rtm.scopes(cd, mode=mode, columns=columns, want=want))
            assert same(first, _host(rtm.scopes(cd, mode=mode, columns=columns, want=want)))  # a second call
            assert same(first, _host(rtm.scopes(shifted, mode=mode, columns=columns, want=want)))  # a 4-mod-16 address
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            third = rtm.scopes(cd, mode=mode, columns=columns, want=want, stream=side)
            fourth = rtm.scopes(cd, mode=mode, columns=columns, want=want)  # enqueued while the side stream may still run
            side.synchronize()
            assert same(first, _host(third)) and same(first, _host(fourth))
            assert np.array_equal(first["histogram"], _ref_hist(w, h, mode))


@pytest.mark.parametrize("columns", [1, 5, 131])
def test_draw_gives_the_reference_bytes(rtm, columns):
    import torch
    clean = _ref_wave(131, 63, "log2", columns)
    wave = clean.copy()
    wave[3, 255, 0] = 0xFFFFFFFF  # count * gain does not wrap
    wd = torch.from_numpy(wave.view(np.int32)).cuda()
    for layout in ("luma", "overlay", "parade"):
        for gain in (1, 7):
            got = rtm.scope_draw(wd, layout=layout, gain=gain)
            torch.cuda.synchronize()
            want = ref.draw(wave, ref.LAYOUTS[layout], gain)
            assert tuple(got.shape) == want.shape and np.array_equal(got.cpu().numpy(), want), (layout, gain)
    # the device's own waveform, through both calls
    own = rtm.scopes(_dev(_frame(131, 63, "log2")), columns=columns, want=("waveform",))["waveform"]
    assert np.array_equal(rtm.scope_draw(own, layout="parade", gain=3).cpu().numpy(), ref.draw(clean, ref.PARADE, 3))


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


def _document(rtm, frame, mode):
    """What rtm_cli and write_scopes say of one frame, from the module's functions."""
    import torch
    hist = rtm.scope_histogram(rtm.scopes(torch.from_numpy(np.ascontiguousarray(frame)).cuda(), mode=mode)["histogram"])
    doc = rtm.scope_summary(hist, mode)
    doc["histogram"] = {"bins": hist["bins"].tolist(), "below": hist["below"].tolist(), "above": hist["above"].tolist()}
    return doc, hist


def test_renderer_and_cli_measure_the_frames_they_write(rtm, tmp_path):
    import torch
    W, H = 64, 48
    scene = json.load(open(SCENE))
    scene["00 width"], scene["00 height"], scene["00 samples"], scene["00 superSamples"] = W, H, 4, 1
    small = tmp_path / "small.json"
    small.write_text(json.dumps(scene))
    r = rtm.Renderer(rtm.LoadData(str(small)).data, mode="repaired", max_bounces=8)
    r.Render(str(tmp_path / "py"))
    f32 = torch.from_numpy(r.image).cuda().to(torch.float32)
    # Renderer.scopes is the module function on the same frame
    mine = r.scopes(columns=7, want=("histogram", "waveform"))
    direct = rtm.scopes(f32, columns=7, want=("histogram", "waveform"))
    torch.cuda.synchronize()
    assert np.array_equal(ref.words({**mine["histogram"], "reserved": np.zeros(2, np.uint32)}),
                          direct["histogram"].cpu().numpy().view(np.uint32))
    assert np.array_equal(mine["waveform"], direct["waveform"].cpu().numpy().view(np.uint32))
    assert np.array_equal(direct["histogram"].cpu().numpy().view(np.uint32), ref.words(ref.histogram(f32.cpu().numpy(), ref.LOG2)))
    assert mine["histogram"]["pixels"] == W * H
    shown = rtm.tonemap(f32, want=("f32",))["f32"]
    code = r.scopes(frame=shown, mode="code")["histogram"]
    assert np.array_equal(code["bins"], ref.histogram(shown.cpu().numpy(), ref.CODE)["bins"])
    # write_scopes: the JSON and the picture
    doc = r.write_scopes(str(tmp_path / "py"), layout="parade")
    want_doc, _ = _document(rtm, f32.cpu().numpy(), "log2")
    assert doc == want_doc and json.load(open(tmp_path / "py_scopes.json")) == json.loads(json.dumps(want_doc))
    gain = max(1, 2040 // H)
    picture = rtm.scope_draw(rtm.scopes(f32, columns=W, want=("waveform",))["waveform"], layout="parade", gain=gain)
    assert np.array_equal(_read_bmp(tmp_path / "py_waveform.bmp"), picture.cpu().numpy())

    def run(stem, *flags):
        p = subprocess.run([CLI, "-json", str(small), "--max-bounces", "8", "--out", stem] + list(flags), cwd=tmp_path,
                           capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout + p.stderr
        lines = [l for l in p.stdout.splitlines() if l.startswith("scopes: ")]
        assert len(lines) == 1, p.stdout
        return json.loads(lines[0][len("scopes: "):])

    # rtm_cli --scopes --display: the linear frame in stops, the display frame in code values, the display frame's waveform
    line = run("cli", "--scopes", "--display", "--pfm", "--display-pfm")
    for name in ("cli_scopes.json", "cli_waveform.bmp", "cli.pfm", "cli_display.pfm", "cli_display.bmp"):
        assert (tmp_path / name).exists(), name
    lin, disp = _read_pfm(tmp_path / "cli.pfm"), _read_pfm(tmp_path / "cli_display.pfm")
    assert np.array_equal(lin.view(np.uint32), f32.cpu().numpy().view(np.uint32))
    want_lin, _ = _document(rtm, lin, "log2")
    want_disp, _ = _document(rtm, disp, "code")
    full = json.load(open(tmp_path / "cli_scopes.json"))
    assert {k: v for k, v in full.items() if k != "display"} == json.loads(json.dumps(want_lin))
    assert full["display"] == json.loads(json.dumps(want_disp))
    strip = lambda d: {k: v for k, v in d.items() if k != "histogram"}
    assert line == {**strip(json.loads(json.dumps(want_lin))), "display": strip(json.loads(json.dumps(want_disp)))}
    assert "exposure" not in line and line["display"]["mode"] == "code" and line["mode"] == "log2"
    dd = torch.from_numpy(np.ascontiguousarray(disp)).cuda()
    picture = rtm.scope_draw(rtm.scopes(dd, mode="code", columns=W, want=("waveform",))["waveform"], gain=gain)
    assert np.array_equal(_read_bmp(tmp_path / "cli_waveform.bmp"), picture.cpu().numpy())
    # without --display: the linear frame's waveform, with its own columns and layout
    line = run("lin", "--scopes", "--scopes-columns", "7", "--scopes-layout", "overlay")
    assert line == strip(json.loads(json.dumps(want_lin)))
    picture = rtm.scope_draw(rtm.scopes(f32, columns=7, want=("waveform",))["waveform"], layout="overlay", gain=gain)
    assert np.array_equal(_read_bmp(tmp_path / "lin_waveform.bmp"), picture.cpu().numpy())
    # --expose-percentile: the exposure is the host helper's of the frame the transform takes, and the transform runs at it
    line = run("exp", "--scopes", "--display", "--expose-percentile", "99,0.8", "--pfm", "--display-pfm")
    ev = rtm.scope_exposure(rtm.scopes(f32)["histogram"], 99, 0.8)
    assert np.float32(line["exposure"]) == np.float32(ev) and ev != 0.0
    want_shown = rtm.tonemap(f32, exposure=ev, want=("f32", "u8"))
    assert np.array_equal(_read_pfm(tmp_path / "exp_display.pfm").view(np.uint32), want_shown["f32"].cpu().numpy().view(np.uint32))
    assert np.array_equal(_read_bmp(tmp_path / "exp_display.bmp"), want_shown["u8"].cpu().numpy())
    assert line["display"] == strip(json.loads(json.dumps(_document(rtm, want_shown["f32"].cpu().numpy(), "code")[0])))
    # a width below the default columns, and columns past the width
    p = subprocess.run([CLI, "-json", str(small), "--max-bounces", "8", "--out", "bad", "--scopes", "--scopes-columns", str(W + 1)],
                       cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert p.returncode == 2 and "exceeds the frame's width" in p.stderr
