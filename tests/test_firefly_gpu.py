"""The firefly clamp on a real MI355X (-m gpu): rtm_firefly against the NumPy restatement (_firefly_ref) on synthetic frames
from one pixel to several ragged 32 x 16 tiles: the mask and the thresholds bit for bit, the unchanged pixels' words, the
changed pixels within the header's bar, the 8-bit store bit for bit, every subset of the outputs, determinism across calls,
streams and alignments, all 24 instantiations, and what the stage does for the stages behind it: Render and rtm_cli.
test_firefly_matches_the_reference prints the worst error of every frame; DESIGN.md records the largest."""
import ctypes as C
import functools
import itertools
import json
import os
import subprocess

import numpy as np
import pytest

import _firefly_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "raytracingmin_amd", "rtm_cli")
SCENE = os.path.join(ROOT, "scenes", "cornellBoxSetting.json")
TOL = 1e-4  # include/rtm.h: |got - ref| <= 1e-4 max(1, |ref|), for every changed component
# one pixel; a row and a column thinner than any window; less than a tile; one tile and a pixel; several tiles, ragged in both
# axes, with halos across tile seams at radius 3
FRAMES = [(1, 1), (1, 9), (9, 1), (3, 3), (7, 5), (33, 17), (64, 64), (131, 63)]
# (radius, rank, k, floor, repair): every radius, ranks 1, 3 and 8, both repair values
CASES = ((1, 3, 4.0, 0.01, 1), (1, 1, 1.0, 0.0, 1), (2, 3, 4.0, 0.01, 0), (3, 8, 2.0, 0.5, 1), (3, 1, 1.5, 0.0, 0), (2, 8, 4.0, 0.01, 1))
ALL = ("f32", "u8", "mask", "threshold")


@pytest.fixture(scope="module")
def rtm():
    import raytracingmin_amd as m
    n = C.c_int()
    m._lib.check(m.lib().rtm_device_count(C.byref(n)), "rtm_device_count")
    assert n.value >= 1
    return m


@functools.lru_cache(maxsize=None)
def _frame(w, h):
    color, marks = _firefly_ref.frame(w, h)
    color.setflags(write=False)
    return color, marks


@functools.lru_cache(maxsize=None)
def _ref(w, h, case):
    """The reference of a frame and a case, computed once and shared."""
    radius, rank, k, floor, repair = case
    ref = _firefly_ref.firefly_ref(_frame(w, h)[0], radius, rank, k, floor, bool(repair))
    for v in ref.values():
        v.setflags(write=False)
    return ref


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


def _call(rtm, cd, case, want=ALL, **kw):
    radius, rank, k, floor, repair = case
    return rtm.firefly(cd, radius, rank, k, floor, bool(repair), want=want, **kw)


@pytest.mark.parametrize("w,h", FRAMES)
def test_firefly_matches_the_reference(rtm, w, h):
    color, _ = _frame(w, h)
    cd = _dev(color)
    worst = 0.0
    for case in CASES:
        ref = _ref(w, h, case)
        out = _bits(_call(rtm, cd, case))
        # the decisions are exact
        assert np.array_equal(out["mask"], ref["mask"]), case
        assert np.array_equal(out["threshold"].view(np.uint32), ref["threshold"].view(np.uint32)), case
        # an unchanged pixel keeps its words, NaN payloads included
        same = ref["mask"] == 0
        assert np.array_equal(_words(out["f32"])[same], _words(color)[same]), case
        # a changed one is within the bar of the float64 evaluation
        err = _firefly_ref.tolerance_excess(out["f32"][~same], ref["out"][~same])
        print(f"{w}x{h} {case}: {int((ref['mask'] == 1).sum())} clamped, {int((ref['mask'] == 2).sum())} repaired, out_f32 {err:.3e}")
        assert err <= TOL, (case, err)
        if case[4]:
            assert np.all(np.isfinite(out["f32"])), case
        # the 8-bit store is rtm_quantise of the call's own out_f32: exact at every pixel, 0 where a component is NaN
        assert np.array_equal(out["u8"], _host_quantise(rtm, out["f32"])), case
        assert np.all(out["u8"][np.isnan(out["f32"])] == 0), case
        worst = max(worst, err)
    print(f"{w}x{h}: worst error of a changed component against the float64 reference: {worst:.3e} (bar {TOL})")


def test_every_subset_of_the_outputs_gives_the_same_bits(rtm):
    w, h = 33, 17
    cd = _dev(_frame(w, h)[0])
    for case in (CASES[0], CASES[3], CASES[4]):
        full = _bits(_call(rtm, cd, case))
        for r in range(1, len(ALL)):
            for want in itertools.combinations(ALL, r):
                out = _call(rtm, cd, case, want=want)
                assert tuple(out) == want
                got = _bits(out)
                assert all(np.array_equal(got[k].view(np.uint8), full[k].view(np.uint8)) for k in want), (case, want)


def test_the_same_inputs_give_the_same_bits(rtm):
    import torch
    w, h = 131, 63
    color, _ = _frame(w, h)
    cd = _dev(color)
    buf = torch.empty(w * h * 3 + 8, dtype=torch.float32, device="cuda")
    shifted = buf[1:1 + w * h * 3].view(h, w, 3)
    shifted.copy_(cd)
    assert cd.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    for case in (CASES[0], CASES[3], CASES[5]):
        first = _bits(_call(rtm, cd, case))
        assert _same_bits(first, _bits(_call(rtm, cd, case))), case  # a second call
        assert _same_bits(first, _bits(_call(rtm, shifted, case))), case  # a 4-mod-16 address
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        third = _call(rtm, cd, case, stream=side)
        fourth = _call(rtm, cd, case)  # the current stream's, enqueued while the side stream may still run
        side.synchronize()
        assert _same_bits(first, _bits(third)) and _same_bits(first, _bits(fourth)), case
    assert np.array_equal(_words(cd.cpu().numpy()), _words(color))  # the input is left alone


def test_every_instantiation_once(rtm):
    """24 kernels, radius 1..3 times rank 1..8, each run once on a tiny frame against the reference's decisions."""
    w, h = 33, 17
    color, _ = _frame(w, h)
    cd = _dev(color)
    for radius in (1, 2, 3):
        for rank in range(1, 9):
            ref = _firefly_ref.firefly_ref(color, radius, rank, 2.0, 0.01, True)
            out = _bits(rtm.firefly(cd, radius, rank, 2.0, 0.01, True, want=ALL))
            assert np.array_equal(out["mask"], ref["mask"]), (radius, rank)
            assert np.array_equal(out["threshold"].view(np.uint32), ref["threshold"].view(np.uint32)), (radius, rank)
            changed = ref["mask"] != 0
            assert _firefly_ref.tolerance_excess(out["f32"][changed], ref["out"][changed]) <= TOL, (radius, rank)
            assert np.array_equal(_words(out["f32"])[~changed], _words(color)[~changed]), (radius, rank)


def test_the_consequences_the_header_states(rtm):
    # a constant frame, and a frame without outliers whose pixels all count, are copied bit for bit
    for w, h in ((1, 1), (33, 17), (131, 63)):
        flat = np.broadcast_to(np.float32([0.25, 3.0, 0.0]), (h, w, 3)).copy()
        rng = np.random.default_rng(w)
        mild = (0.5 + 0.1 * rng.random((h, w, 3))).astype(np.float32)
        for frame in (flat, mild):
            for case in (CASES[0], CASES[3]) + (((1, 1, 1.0, 0.0, 1),) if frame is flat else ()):
                out = _bits(_call(rtm, _dev(frame), case))
                assert np.array_equal(_words(out["f32"]), _words(frame)) and not out["mask"].any(), (w, h, case)
    # at the defaults: rectangles keep their words, spikes and clusters are clamped; the line goes at rank 3 and stays at rank 2
    w, h = 131, 63
    color, marks = _frame(w, h)
    cd = _dev(color)
    out = _bits(rtm.firefly(cd, want=ALL))
    kept = np.all(_words(out["f32"]) == _words(color), axis=-1)
    assert kept[marks["rect"]].all() and kept[marks["block"]].all()
    for name in ("spikes", "cluster2", "cluster3", "line"):
        assert np.all(out["mask"][marks[name]] == 1), name
    assert np.all(out["mask"][marks["nonfinite"]] == 2)
    out2 = _bits(rtm.firefly(cd, rank=2, want=ALL))
    kept2 = np.all(_words(out2["f32"]) == _words(color), axis=-1)
    assert not kept[marks["line_inner"]].any() and kept2[marks["line_inner"]].all() and not out2["mask"][marks["line_inner"]].any()
    # repair off: the words of a pixel that does not count are kept, and its mask is 0
    off = _bits(rtm.firefly(cd, repair=False, want=ALL))
    bad = marks["nonfinite"]
    assert np.array_equal(_words(off["f32"])[bad], _words(color)[bad]) and not off["mask"][bad].any()
    assert np.all(np.isposinf(off["threshold"][bad]))


def test_firefly_in_front_of_the_denoiser_keeps_a_nan_out_of_the_frame(rtm):
    import torch
    w, h = 64, 64
    color, marks = _frame(w, h)
    cd = _dev(color)
    guides = {"depth": torch.full((h, w), 5.0, device="cuda"), "normal": torch.zeros((h, w, 3), device="cuda"),
              "albedo": torch.ones((h, w, 3), device="cuda"), "object": torch.zeros((h, w), dtype=torch.int32, device="cuda")}
    guides["normal"][..., 2] = 1.0
    alone = rtm.denoise(cd, guides)["f32"]
    assert not bool(torch.isfinite(alone).all())  # the case cannot skip itself: the denoiser alone keeps or spreads them
    cleaned = rtm.firefly(cd)["f32"]
    assert bool(torch.isfinite(cleaned).all())
    assert bool(torch.isfinite(rtm.denoise(cleaned, guides)["f32"]).all())


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


def test_render_and_cli_clean_the_frame_before_the_denoiser(rtm, tmp_path):
    import torch
    scene = json.load(open(SCENE))
    scene["00 width"], scene["00 height"], scene["00 samples"], scene["00 superSamples"] = 64, 64, 4, 1
    small = tmp_path / "small.json"
    small.write_text(json.dumps(scene))
    r = rtm.Renderer(rtm.LoadData(str(small)).data, mode="repaired", max_bounces=8)
    r.Render(str(tmp_path / "py"), firefly=True, denoise=True)
    for name in ("py.bmp", "py.jpg", "py_firefly.bmp", "py_firefly.jpg", "py_denoised.bmp", "py_denoised.jpg"):
        assert (tmp_path / name).exists(), name
    f32 = torch.from_numpy(r.image).cuda().to(torch.float32)
    want = rtm.firefly(f32, want=ALL)
    mask = want["mask"].cpu().numpy()
    counts = {"clamped": int((mask == 1).sum()), "repaired": int((mask == 2).sum()), "pixels": 64 * 64}
    assert r.firefly_counts == counts
    assert np.array_equal(_read_bmp(tmp_path / "py_firefly.bmp"), want["u8"].cpu().numpy())
    guides = r.render_aov()
    den = rtm.denoise(want["f32"], guides, want=("u8", "f32"))
    assert np.array_equal(_read_bmp(tmp_path / "py_denoised.bmp"), den["u8"].cpu().numpy())  # the cleaned frame is denoised
    # without firefly: the plain files are the same; the denoised frame differs only if something was clamped or repaired
    r.Render(str(tmp_path / "off"), denoise=True)
    assert (tmp_path / "off.bmp").read_bytes() == (tmp_path / "py.bmp").read_bytes() and not (tmp_path / "off_firefly.bmp").exists()
    plain = rtm.denoise(f32, guides, want=("u8",))["u8"].cpu().numpy()
    assert np.array_equal(_read_bmp(tmp_path / "off_denoised.bmp"), plain)
    differs = (tmp_path / "off_denoised.bmp").read_bytes() != (tmp_path / "py_denoised.bmp").read_bytes()
    assert not differs or mask.any()
    if not mask.any():
        assert torch.equal(want["f32"], f32)
    # a dict reaches the call, and the later stages take the cleaned frame too
    prm = dict(radius=2, rank=1, k=1.0, floor=0.0)
    r.Render(str(tmp_path / "py2"), firefly=prm, tonemap=True)
    want2 = rtm.firefly(f32, want=("f32", "u8", "mask"), **prm)
    assert int((want2["mask"] == 1).sum()) > 0  # every strict local maximum of the window
    assert np.array_equal(_read_bmp(tmp_path / "py2_firefly.bmp"), want2["u8"].cpu().numpy())
    assert np.array_equal(_read_bmp(tmp_path / "py2_display.bmp"), rtm.tonemap(want2["f32"], want=("u8",))["u8"].cpu().numpy())

    # rtm_cli: the same files, one line whose counts are the mask's, and the cleaned frame is the later stages'
    def run(stem, *flags):
        p = subprocess.run([CLI, "-json", str(small), "--max-bounces", "8", "--out", stem] + list(flags), cwd=tmp_path,
                           capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout + p.stderr
        lines = [l for l in p.stdout.splitlines() if l.startswith("firefly: ")]
        assert len(lines) == 1, p.stdout
        return json.loads(lines[0][len("firefly: "):])

    assert run("cli", "--firefly", "--denoise", "--pfm") == counts
    assert (tmp_path / "cli_firefly.bmp").read_bytes() == (tmp_path / "py_firefly.bmp").read_bytes()
    assert (tmp_path / "cli_firefly.jpg").read_bytes() == (tmp_path / "py_firefly.jpg").read_bytes()
    assert (tmp_path / "cli_denoised.bmp").read_bytes() == (tmp_path / "py_denoised.bmp").read_bytes()
    assert (tmp_path / "cli.bmp").read_bytes() == (tmp_path / "py.bmp").read_bytes()
    assert np.array_equal(_words(_read_pfm(tmp_path / "cli.pfm")), _words(den["f32"].cpu().numpy()))
    got = run("cli2", "--firefly", "1", "--firefly-rank", "1", "--firefly-radius", "2", "--firefly-floor", "0", "--pfm", "--display")
    mask2 = want2["mask"].cpu().numpy()
    assert got == {"clamped": int((mask2 == 1).sum()), "repaired": int((mask2 == 2).sum()), "pixels": 64 * 64}
    assert np.array_equal(_words(_read_pfm(tmp_path / "cli2.pfm")), _words(want2["f32"].cpu().numpy()))
    assert (tmp_path / "cli2_display.bmp").read_bytes() == (tmp_path / "py2_display.bmp").read_bytes()
    assert run("cli3", "--firefly", "--firefly-keep-nonfinite")["repaired"] == 0
