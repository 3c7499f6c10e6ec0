"""The perceptual frame difference on a real MI355X (-m gpu): rtm_flip against the NumPy float64 restatement (_flip_ref) on
synthetic display-referred pairs at three viewing conditions and both transfers, the histogram's exactness given the call's
own map, identical frames, non-finite pixels, the record across the three forms of the call, determinism across calls and
streams, guard bytes around every buffer the call writes, a rendered frame, and the rtm_cli output."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import _flip_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "raytracingmin_amd", "rtm_cli")
SCENE = os.path.join(ROOT, "scenes", "cornellBoxSetting.json")
# include/rtm.h: mean, min, max and the map against a float64 evaluation.  max(1e-9, 100 D) with D = 9.3e-14, the largest
# disagreement of the restatement's direct and separable orders over every (frame, ppd, transfer) of _flip_ref.CASES
# (tests/test_flip_host.py measures it again on every run)
TOLERANCE = 1e-9
MAP_TOLERANCE = TOLERANCE + 2.0 ** -25  # the map is rounded to float: half an ulp of a value in [0.5, 1]


@pytest.fixture(scope="module")
def rtm():
    import raytracingmin_amd as m
    n = C.c_int()
    m._lib.check(m.lib().rtm_device_count(C.byref(n)), "rtm_device_count")
    assert n.value >= 1
    return m


_REFERENCE = {}


def _reference(w, h, ppd, transfer):
    """The pair and its float64 evaluation, computed once and shared."""
    key = (w, h, ppd, transfer)
    if key not in _REFERENCE:
        a, b = _flip_ref.pair(w, h)
        for v in (a, b):
            v.setflags(write=False)
        _REFERENCE[key] = (a, b) + _flip_ref.flip_ref(a, b, transfer, ppd)
    return _REFERENCE[key]


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()  # a copy: the shared reference frames are read-only


def _run(rtm, a, b, want=("result", "map"), **kw):
    """flip() on host arrays or device tensors; returns (decoded result or None, map or None, raw result words or None)."""
    import torch
    ad = a if isinstance(a, torch.Tensor) else _dev(a)
    bd = b if isinstance(b, torch.Tensor) else _dev(b)
    out = rtm.flip(ad, bd, want=want, **kw)
    torch.cuda.synchronize()
    raw = out["result"].cpu().numpy().copy() if "result" in out else None
    return (rtm.flip_result(raw) if raw is not None else None, out["map"].cpu().numpy() if "map" in out else None, raw)


def _check_against(res, got_map, ref, ref_map, label, need_argmax=True):
    assert res["pixels"] == ref["pixels"] and res["nonfinite"] == ref["nonfinite"], label
    for k in ("mean", "min", "max"):
        err = abs(res[k] - ref[k])
        print(f"{label}: {k} device {res[k]!r} reference {ref[k]!r} absolute error {err:.3e} (bar {TOLERANCE})")
        assert err <= TOLERANCE, (label, k, res[k], ref[k])
    top = np.sort(ref_map[~np.isnan(ref_map)].ravel())[-2:]
    separated = top.size < 2 or top[1] - top[0] > 2 * TOLERANCE
    if need_argmax:
        assert separated, (label, "the reference's two largest values are too close for the argmax to be checked", top)
    if separated:
        assert (res["argmax_x"], res["argmax_y"]) == (ref["argmax_x"], ref["argmax_y"]), label
    if got_map is not None:
        assert np.array_equal(np.isnan(got_map), np.isnan(ref_map)), label
        keep = ~np.isnan(ref_map)
        err = float(np.abs(got_map.astype(np.float64)[keep] - ref_map[keep]).max()) if keep.any() else 0.0
        print(f"{label}: map worst absolute error {err:.3e} (bar {MAP_TOLERANCE:.3e})")
        assert err <= MAP_TOLERANCE, (label, err)
        assert np.array_equal(np.array(res["hist"], np.uint32), _flip_ref.histogram(got_map)), label  # exact, given its own map


@pytest.mark.parametrize("transfer", ["srgb", "linear"])
@pytest.mark.parametrize("w,h,ppd", _flip_ref.CASES)
def test_flip_matches_the_reference(rtm, w, h, ppd, transfer):
    a, b, ref, ref_map = _reference(w, h, ppd, transfer)
    ad, bd = _dev(a), _dev(b)
    label = f"{w}x{h} ppd {ppd} {transfer}"
    res, got, raw = _run(rtm, ad, bd, transfer=transfer, pixels_per_degree=ppd)
    _check_against(res, got, ref, ref_map, label)
    assert sum(res["hist"]) == res["pixels"] == w * h
    # the record alone, and the map alone: the record's bytes and the map's bits do not depend on what else is asked for
    _, _, raw_alone = _run(rtm, ad, bd, want=("result",), transfer=transfer, pixels_per_degree=ppd)
    assert np.array_equal(raw_alone, raw), label
    _, map_alone, _ = _run(rtm, ad, bd, want=("map",), transfer=transfer, pixels_per_degree=ppd)
    assert np.array_equal(map_alone.view(np.uint32), got.view(np.uint32)), label


def test_identical_frames(rtm):
    for w, h in ((1, 1), (37, 23), (131, 63)):
        a, _ = _flip_ref.pair(w, h)
        ad = _dev(a)
        for bd in (ad, _dev(a)):  # the same buffer twice (a_dev == b_dev), and an equal copy
            for transfer in ("srgb", "linear"):
                res, got, _ = _run(rtm, ad, bd, transfer=transfer)
                assert np.array_equal(got.view(np.uint32), np.zeros((h, w), np.uint32))  # +0 everywhere
                assert res["hist"][0] == w * h == res["pixels"] and sum(res["hist"]) == w * h
                assert res["mean"] == 0.0 and res["max"] == 0.0 and res["min"] == 0.0
                assert (res["argmax_x"], res["argmax_y"]) == (0, 0) and res["nonfinite"] == 0


def test_non_finite_pixels(rtm):
    w, h = 37, 23
    a, b = (v.copy() for v in _flip_ref.pair(w, h))
    a[0, 0, 1] = np.nan                                     # a corner, one frame
    b[0, 36] = [np.inf, 0.5, 0.5]                           # a corner, the other frame
    a[22, 17], b[22, 17] = [np.nan, 1, 0], [np.nan, 1, 0]  # an edge, both frames
    a[11, 0, 2] = -np.inf                                   # an edge
    a[10, 20], b[10, 20] = [np.inf, 0, 0], [-np.inf, 0, 0]  # the interior, both frames
    b[12, 21, 0] = np.nan                                   # the interior, next to it
    holes = [(0, 0), (0, 36), (22, 17), (11, 0), (10, 20), (12, 21)]
    for transfer in ("srgb", "linear"):
        ref, ref_map = _flip_ref.flip_ref(a, b, transfer)
        res, got, _ = _run(rtm, a, b, transfer=transfer)
        assert res["nonfinite"] == len(holes) and res["pixels"] == w * h - len(holes) == sum(res["hist"])
        assert all(np.isnan(got[y, x]) for y, x in holes) and np.isnan(got).sum() == len(holes)
        _check_against(res, got, ref, ref_map, f"non-finite {transfer}", need_argmax=False)
        # the black-substitution rule: the neighbours' values are those of the frames with the holes black in both
        a0, b0 = a.copy(), b.copy()
        for y, x in holes:
            a0[y, x] = b0[y, x] = 0.0
        _, filled, _ = _run(rtm, a0, b0, transfer=transfer)
        keep = ~np.isnan(got)
        assert np.array_equal(got[keep].view(np.uint32), filled[keep].view(np.uint32))
    nan = np.full((h, w, 3), np.nan, np.float32)
    res, got, _ = _run(rtm, nan, b)
    assert res["pixels"] == 0 and res["nonfinite"] == w * h and sum(res["hist"]) == 0 and np.isnan(got).all()
    assert res["mean"] == 0.0 and res["max"] == 0.0 and res["min"] == 0.0 and (res["argmax_x"], res["argmax_y"]) == (-1, -1)


def test_the_same_inputs_give_the_same_bits_on_every_call_and_stream(rtm):
    import torch
    a, b = _flip_ref.pair(131, 63)
    ad, bd = _dev(a), _dev(b)
    _, map0, raw0 = _run(rtm, ad, bd)
    _, map1, raw1 = _run(rtm, ad, bd)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    out = rtm.flip(ad, bd, want=("result", "map"), stream=side)  # its own work buffer
    side.synchronize()
    raw2, map2 = out["result"].cpu().numpy(), out["map"].cpu().numpy()
    for raw, m in ((raw1, map1), (raw2, map2)):
        assert np.array_equal(raw0, raw) and np.array_equal(map0.view(np.uint32), m.view(np.uint32))


def test_guard_bytes_and_inputs_are_untouched(rtm):
    import torch
    from raytracingmin_amd import _lib
    L = rtm.lib()
    G = 256  # guard bytes on each side
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for (w, h), ppd in (((37, 23), 128.0), ((131, 63), 67.02), ((1, 23), 8.0)):
        a, b = _flip_ref.pair(w, h)
        ad, bd = _dev(a), _dev(b)
        sizes = {"work": L.rtm_flip_work_bytes(w, h), "result": C.sizeof(_lib.rtm_flip_result), "map": 4 * w * h}
        bufs = {k: torch.full((n + 2 * G,), 0xA5, dtype=torch.uint8, device="cuda") for k, n in sizes.items()}
        ptr = {k: v.data_ptr() + G for k, v in bufs.items()}
        assert ptr["work"] % 256 == 0
        prm = _lib.rtm_flip_params(1, ppd)
        _lib.check(L.rtm_flip(C.byref(prm), w, h, 0, ad.data_ptr(), bd.data_ptr(), ptr["work"], ptr["result"], ptr["map"], stream),
                   "rtm_flip")
        torch.cuda.synchronize()
        for k, v in bufs.items():
            host = v.cpu().numpy()
            assert np.all(host[:G] == 0xA5) and np.all(host[G + sizes[k]:] == 0xA5), (w, h, k)
        rec = bufs["result"].cpu().numpy()[G:G + sizes["result"]]
        assert rtm.flip_result(rec.view(np.int32))["pixels"] == w * h
        assert not np.any(bufs["map"].cpu().numpy()[G:G + 4 * w * h].view(np.uint32) == 0xA5A5A5A5)  # every pixel written
        assert np.array_equal(ad.cpu().numpy().view(np.uint8), a.view(np.uint8))
        assert np.array_equal(bd.cpu().numpy().view(np.uint8), b.view(np.uint8))


def test_a_rendered_frame_against_its_denoised_self(rtm):
    data = rtm.LoadData(SCENE).data
    data.width, data.height, data.samples, data.superSamples = 64, 64, 4, 1
    r = rtm.Renderer(data, mode="repaired", max_bounces=8)
    noisy, _ = r.render_rows_device(want=("f32",), stats=False)
    denoised = rtm.denoise(noisy["f32"], r.render_aov(), want=("f32",))["f32"]
    shown_a = rtm.tonemap(noisy["f32"], want=("f32",))["f32"]
    shown_b = rtm.tonemap(denoised, want=("f32",))["f32"]
    ref, ref_map = _flip_ref.flip_ref(shown_a.cpu().numpy(), shown_b.cpu().numpy())
    res, got, _ = _run(rtm, shown_a, shown_b)
    assert np.isfinite([res["mean"], res["max"], res["min"]]).all() and res["mean"] > 0 and res["pixels"] == 64 * 64
    _check_against(res, got, ref, ref_map, "Cornell 4 spp against denoised", need_argmax=False)
    assert 0.0 < res["weighted_first_quartile"] <= res["weighted_median"] <= res["weighted_third_quartile"] <= 1.0
    assert r.flip(shown_b, frame=shown_a) == res  # Renderer.flip: the same call, decoded


def _read_pfm(rtm, path):
    L = rtm.lib()
    w, h, comp = C.c_int(), C.c_int(), C.c_int()
    assert L.rtm_read_pfm(os.fsencode(str(path)), C.byref(w), C.byref(h), C.byref(comp), None, 0) == 1
    data = np.zeros((h.value, w.value, comp.value), np.float32)
    assert L.rtm_read_pfm(os.fsencode(str(path)), C.byref(w), C.byref(h), C.byref(comp), data.ctypes.data, data.size) == 1
    return data


def test_cli_display_flip(rtm, tmp_path):
    args = [CLI, "-json", SCENE, "--width", "64", "--height", "64", "--samples", "4", "--superSamples", "1", "--max-bounces", "8"]

    def run(stem, *flags):
        p = subprocess.run(args + ["--out", stem] + list(flags), cwd=tmp_path, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout + p.stderr
        lines = [l for l in p.stdout.splitlines() if l.startswith("flip: ")]
        return json.loads(lines[0][len("flip: "):]) if len(lines) == 1 else None

    assert run("ref", "--denoise", "--display", "--display-pfm") is None
    rec = run("got", "--display", "--display-pfm", "--flip", "ref_display.pfm", "--flip-map")
    assert tuple(rec) == ("mean", "max", "min", "pixels", "nonfinite", "argmax_x", "argmax_y", "weighted_median")
    frame, reference = _read_pfm(rtm, tmp_path / "got_display.pfm"), _read_pfm(rtm, tmp_path / "ref_display.pfm")
    res, got, _ = _run(rtm, frame, reference)
    assert rec == {k: res[k] for k in rec} and rec["mean"] > 0 and rec["pixels"] == 64 * 64
    written = _read_pfm(rtm, tmp_path / "got_flip.pfm")
    assert written.shape == (64, 64, 1) and np.array_equal(written[..., 0].view(np.uint32), got.view(np.uint32))
    # the frame against its own display file: zero; and --display-pfm changed no other file's bytes
    assert run("same", "--display", "--flip", "got_display.pfm")["max"] == 0
    assert (tmp_path / "same_display.bmp").read_bytes() == (tmp_path / "got_display.bmp").read_bytes()
    assert not (tmp_path / "same_display.pfm").exists() and not (tmp_path / "same_flip.pfm").exists()
