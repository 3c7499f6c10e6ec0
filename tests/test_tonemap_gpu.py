"""The display transform on a real MI355X (-m gpu): rtm_tonemap against the NumPy float64 restatement (_tonemap_ref) on
synthetic HDR frames, the 8-bit stores bit for bit, the 16-byte and the plain load path, empty and black frames, the
identity case, in-place use, the skipped statistics, determinism across calls and streams, the dither's block means, and
the Render / rtm_cli outputs."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import _tonemap_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "raytracingmin_amd", "rtm_cli")
SCENE = os.path.join(ROOT, "scenes", "cornellBoxSetting.json")
TOL = 1e-4  # include/rtm.h: |out - ref| <= 1e-4 max(1, |ref|), for out_f32 and the three float statistics
FRAMES = [(1, 1), (1, 17), (7, 5), (37, 23), (64, 64), (131, 63)]  # 64 x 64: one reduction block; 131 x 63: two and a ragged third
CASES = list(itertools.product(_tonemap_ref.OPS, _tonemap_ref.TRANSFERS, ("auto", -1.0), (0.0, 2.0)))
STAT_FLOATS = ("log_average", "max_luminance", "exposure")


@pytest.fixture(scope="module")
def rtm():
    import raytracingmin_amd as m
    n = C.c_int()
    m._lib.check(m.lib().rtm_device_count(C.byref(n)), "rtm_device_count")
    assert n.value >= 1
    return m


def _frame(w, h):
    """8 u^4: a long dark tail and highlights above 1; 10 % exactly black; one negative component; beyond two pixels one
    NaN pixel and one +inf pixel."""
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


@pytest.mark.parametrize("w,h", FRAMES)
def test_tonemap_matches_the_reference(rtm, w, h):
    color = _frame(w, h)
    cd = _dev(color)
    black = ~_tonemap_ref.counts(color)
    worst, worst_s = 0.0, 0.0
    for op, transfer, exposure, white in CASES:
        ref, ref_stats = _tonemap_ref.tonemap_ref(color, op=op, transfer=transfer, exposure=exposure, white=white)
        for dither in (False, True):
            out = _bits(rtm.tonemap(cd, op=op, transfer=transfer, exposure=exposure, white=white, dither=dither,
                                    want=("f32", "u8", "stats")))
            stats = rtm.tonemap_stats(out["stats"])
            err = _tonemap_ref.tolerance_excess(out["f32"], ref)
            err_s = max(_tonemap_ref.tolerance_excess(stats[k], ref_stats[k]) for k in STAT_FLOATS)
            print(f"{w}x{h} {op} {transfer} exposure {exposure} white {white} dither {dither}: error {err:.3e}, "
                  f"of the statistics {err_s:.3e}")
            case = (op, transfer, exposure, white, dither)
            assert err <= TOL, (case, err)
            assert err_s <= TOL, (case, err_s, stats, ref_stats)
            assert stats["pixels"] == ref_stats["pixels"] == w * h - int(black.sum()), case
            assert np.all(out["f32"][black] == 0.0) and np.all(out["u8"][black] == 0), case
            want = _tonemap_ref.dither_u8(out["f32"]) if dither else _host_quantise(rtm, out["f32"])
            assert np.array_equal(out["u8"], want), case
            worst, worst_s = max(worst, err), max(worst_s, err_s)
    print(f"{w}x{h}: worst error against the float64 reference {worst:.3e}, of the statistics {worst_s:.3e} (bar {TOL})")


def test_a_misaligned_colour_tensor_gives_the_aligned_bits(rtm):
    import torch
    w, h = 131, 63
    color = _frame(w, h)
    aligned = _dev(color)
    buf = torch.empty(w * h * 3 + 8, dtype=torch.float32, device="cuda")
    shifted = buf[1:1 + w * h * 3].view(h, w, 3)
    shifted.copy_(aligned)
    assert aligned.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    a = _bits(rtm.tonemap(aligned, want=("f32", "u8", "stats")))
    b = _bits(rtm.tonemap(shifted, want=("f32", "u8", "stats")))
    assert np.array_equal(a["stats"], b["stats"])
    assert np.array_equal(a["f32"].view(np.uint32), b["f32"].view(np.uint32)) and np.array_equal(a["u8"], b["u8"])


def test_an_all_nan_frame_has_the_empty_statistics_and_a_black_image(rtm):
    color = np.full((5, 7, 3), np.nan, np.float32)
    out = _bits(rtm.tonemap(_dev(color), exposure="auto", key=0.18, want=("f32", "u8", "stats")))
    assert rtm.tonemap_stats(out["stats"]) == {"log_average": 1.0, "max_luminance": 1.0, "exposure": float(np.float32(0.18)),
                                              "pixels": 0}
    assert np.all(out["f32"] == 0.0) and np.all(out["u8"] == 0)
    out = _bits(rtm.tonemap(_dev(color), exposure=3.0, want=("stats",)))
    assert rtm.tonemap_stats(out["stats"]) == {"log_average": 1.0, "max_luminance": 1.0, "exposure": 8.0, "pixels": 0}


def test_an_all_black_frame_stays_finite(rtm):
    color = np.zeros((5, 7, 3), np.float32)
    for op in _tonemap_ref.OPS:
        out = _bits(rtm.tonemap(_dev(color), op=op, exposure="auto", want=("f32", "u8", "stats")))
        stats = rtm.tonemap_stats(out["stats"])
        assert all(np.isfinite(stats[k]) for k in STAT_FLOATS) and stats["pixels"] == 35, (op, stats)
        assert _tonemap_ref.tolerance_excess(stats["log_average"], 1e-4) <= TOL and stats["max_luminance"] == 0.0
        assert abs(stats["log_average"] - 1e-4) <= 1e-8  # (and well inside the bar: a relative 1e-4 of it)
        assert np.all(np.isfinite(out["f32"])) and np.all(out["f32"] == 0.0), op
        assert np.all(out["u8"] == 0), op  # the dither's largest bias is 63.5 / 64 < 1


def _cornell(rtm, **kw):
    data = rtm.LoadData(SCENE).data
    data.width, data.height, data.samples, data.superSamples = 64, 64, 4, 1
    return rtm.Renderer(data, mode="repaired", max_bounces=8, **kw)


def test_the_identity_parameters_give_the_renders_bytes(rtm):
    r = _cornell(rtm)
    out, _ = r.render_rows_device(want=("f32", "u8"), stats=False)
    got = _bits(rtm.tonemap(out["f32"], op="clamp", transfer="linear", exposure=0.0, dither=False, want=("u8", "f32")))
    assert np.array_equal(got["u8"], out["u8"].cpu().numpy())
    assert np.array_equal(got["u8"], _host_quantise(rtm, out["f32"].cpu().numpy()))


def test_in_place_gives_the_out_of_place_bits(rtm):
    color = _frame(131, 63)
    for kw in (dict(), dict(op="reinhard", exposure=-1.0, white=0.0), dict(op="clamp", transfer="linear", exposure=1.0)):
        want = _bits(rtm.tonemap(_dev(color), want=("f32", "u8", "stats"), **kw))
        cd = _dev(color)
        got = rtm.tonemap(cd, want=("f32", "u8", "stats"), out_f32=cd, **kw)
        assert got["f32"].data_ptr() == cd.data_ptr()
        got = _bits(got)
        for k in ("f32", "u8", "stats"):
            assert np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), (kw, k)


def test_a_call_that_needs_no_statistics_leaves_the_work_buffer_alone(rtm):
    import torch
    from raytracingmin_amd import _lib
    w, h = 131, 63
    L = rtm.lib()
    cd = _dev(_frame(w, h))
    n = L.rtm_tonemap_work_bytes(w, h)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for op, white in ((0, 0.0), (2, 0.0), (1, 2.0)):  # REINHARD only with a white point of its own
        work = torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")
        out32 = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
        prm = _lib.rtm_tonemap_params(op, 1, 0, 1, -1.0, 0.18, white)
        _lib.check(L.rtm_tonemap(C.byref(prm), w, h, 0, cd.data_ptr(), work.data_ptr(), out32.data_ptr(), None, None, stream),
                   "rtm_tonemap")
        torch.cuda.synchronize()
        assert bool(torch.all(work == 0xA5)), (op, white)
        # and the frame is the one a call with statistics maps
        name = {v: k for k, v in _lib.TONEMAP_OPS.items()}[op]
        want = _bits(rtm.tonemap(cd, op=name, exposure=-1.0, white=white, want=("f32", "stats")))
        assert np.array_equal(out32.cpu().numpy().view(np.uint32), want["f32"].view(np.uint32)), (op, white)
    # REINHARD with white == 0 does need them
    work = torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")
    prm = _lib.rtm_tonemap_params(1, 1, 0, 1, -1.0, 0.18, 0.0)
    _lib.check(L.rtm_tonemap(C.byref(prm), w, h, 0, cd.data_ptr(), work.data_ptr(), out32.data_ptr(), None, None, stream), "rtm_tonemap")
    torch.cuda.synchronize()
    assert not bool(torch.all(work == 0xA5))


def test_the_same_inputs_give_the_same_bits_on_every_call_and_stream(rtm):
    import torch
    cd = _dev(_frame(131, 63))
    first = _bits(rtm.tonemap(cd, exposure="auto", want=("f32", "u8", "stats")))
    second = _bits(rtm.tonemap(cd, exposure="auto", want=("f32", "u8", "stats")))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    third = rtm.tonemap(cd, exposure="auto", want=("f32", "u8", "stats"), stream=side)  # its own work buffer
    side.synchronize()
    third = _bits(third)
    for other in (second, third):
        for k in ("f32", "u8", "stats"):
            assert np.array_equal(first[k].view(np.uint8), other[k].view(np.uint8)), k


def test_the_dither_keeps_the_mean_of_every_aligned_block(rtm):
    v = np.float32(100.5 / 255)
    cd = _dev(np.full((64, 64, 3), v, np.float32))
    kw = dict(op="clamp", transfer="linear", exposure=0.0, want=("u8",))
    assert np.all(_bits(rtm.tonemap(cd, dither=False, **kw))["u8"] == 100)
    d = _bits(rtm.tonemap(cd, dither=True, **kw))["u8"]
    assert set(np.unique(d).tolist()) == {100, 101}
    means = d.reshape(8, 8, 8, 8, 3).astype(np.float64).mean(axis=(1, 3))
    assert np.all(np.abs(means - 255.0 * float(v)) <= 1.0 / 64), means


def _read_bmp(path):
    raw = open(path, "rb").read()
    off = int.from_bytes(raw[10:14], "little")
    w, h = int.from_bytes(raw[18:22], "little"), int.from_bytes(raw[22:26], "little")
    stride = (w * 3 + 3) & ~3
    rows = [np.frombuffer(raw, np.uint8, w * 3, off + y * stride).reshape(w, 3)[:, ::-1] for y in range(h)]
    return np.stack(rows[::-1])


def test_render_writes_the_display_files(rtm, tmp_path):
    import torch
    r = _cornell(rtm)
    plain = r.Render(str(tmp_path / "plain"))
    rgb8 = r.Render(str(tmp_path / "shown"), tonemap=True)
    assert np.array_equal(rgb8, plain)
    assert (tmp_path / "shown.bmp").read_bytes() == (tmp_path / "plain.bmp").read_bytes()
    assert (tmp_path / "shown.jpg").read_bytes() == (tmp_path / "plain.jpg").read_bytes()
    assert not (tmp_path / "plain_display.bmp").exists() and (tmp_path / "shown_display.jpg").stat().st_size > 0
    f32 = torch.from_numpy(r.image).cuda().to(torch.float32)
    want = rtm.tonemap(f32, want=("u8",))["u8"].cpu().numpy()
    shown = _read_bmp(tmp_path / "shown_display.bmp")
    assert np.array_equal(shown, want)
    assert not np.array_equal(shown, plain)  # an sRGB-encoded, exposed frame: not the linear truncation
    # a dict of parameters reaches tonemap()
    prm = dict(op="reinhard", transfer="linear", exposure=-1.0, dither=False)
    r.Render(str(tmp_path / "dict"), tonemap=prm)
    assert np.array_equal(_read_bmp(tmp_path / "dict_display.bmp"), rtm.tonemap(f32, want=("u8",), **prm)["u8"].cpu().numpy())
    # the displayed frame is the last stage asked for
    for name, kind, fn in (("dn", True, rtm.denoise), ("dv", "variance", rtm.denoise_variance)):
        r.Render(str(tmp_path / name), denoise=kind, tonemap=True)
        filtered = fn(f32, r.render_aov(), want=("f32", "u8"))
        want = rtm.tonemap(filtered["f32"], want=("u8",))["u8"].cpu().numpy()
        assert np.array_equal(_read_bmp(tmp_path / (name + "_display.bmp")), want), name
        assert not np.array_equal(want, shown), name
        suffix = "_denoised.bmp" if kind is True else "_denoised_var.bmp"
        assert np.array_equal(_read_bmp(tmp_path / (name + suffix)), filtered["u8"].cpu().numpy()), name  # its own file: unchanged
        assert (tmp_path / (name + ".bmp")).read_bytes() == (tmp_path / "plain.bmp").read_bytes(), name


def test_cli_display_writes_the_python_paths_bytes(rtm, tmp_path):
    args = [CLI, "-json", SCENE, "--width", "64", "--height", "64", "--samples", "4", "--superSamples", "1", "--max-bounces", "8"]

    def run(stem, *flags):
        p = subprocess.run(args + ["--out", stem] + list(flags), cwd=tmp_path, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout + p.stderr
        return p.stdout

    r = _cornell(rtm)
    r.Render(str(tmp_path / "py"), tonemap=True)
    text = run("cli", "--display")
    line = [l for l in text.splitlines() if l.startswith("display:")]
    assert len(line) == 1 and "cli_display.bmp" in line[0] and "cli_display.jpg" in line[0] and "exposure" in line[0], text
    assert (tmp_path / "cli_display.bmp").read_bytes() == (tmp_path / "py_display.bmp").read_bytes()
    assert (tmp_path / "cli_display.jpg").read_bytes() == (tmp_path / "py_display.jpg").read_bytes()
    assert (tmp_path / "cli.bmp").read_bytes() == (tmp_path / "py.bmp").read_bytes()
    # the flags, and the chain rule: the denoised frame is the one displayed, its own file keeps its bytes
    r.Render(str(tmp_path / "py2"), denoise=True, tonemap=dict(op="reinhard", transfer="linear", exposure=-1.5, dither=False))
    run("cli2", "--denoise", "--display", "reinhard", "--exposure", "-1.5", "--linear", "--no-dither")
    assert (tmp_path / "cli2_display.bmp").read_bytes() == (tmp_path / "py2_display.bmp").read_bytes()
    assert (tmp_path / "cli2_denoised.bmp").read_bytes() == (tmp_path / "py2_denoised.bmp").read_bytes()
    # refused with more than one GPU
    p = subprocess.run(args + ["--out", "multi", "--display", "--gpus", "2"], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert p.returncode != 0 and "--display" in p.stderr and not (tmp_path / "multi_display.bmp").exists()
