"""Frame comparison on a real MI355X (-m gpu): rtm_compare against the NumPy float64 restatement (_compare_ref) on synthetic
HDR frames in both dtypes and both maps, the strict tolerance, one ulp between two double frames, argmax ties inside a block
and across two, non-finite pixels, identical frames, the 16-byte and the plain load path, determinism across calls and
streams, guard bytes around every buffer the call writes, rendered frames, and the rtm_cli outputs."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import _compare_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "raytracingmin_amd", "rtm_cli")
SCENE = os.path.join(ROOT, "scenes", "cornellBoxSetting.json")
# (w, h): smaller than a window, a thin strip, ragged in one tile, exactly one window, a ragged second tile, 2 x 2 whole
# tiles, 5 x 2 tiles with a ragged last column and row
FRAMES = [(1, 1), (1, 17), (7, 5), (11, 11), (37, 23), (64, 64), (131, 63)]
DTYPES = [np.float32, np.float64]
REL = 1e-9       # include/rtm.h: mse, rel_mse, psnr within 1e-9 relative
SSIM_ABS = 1e-9  # ssim within 1e-9 absolute
MAP_ABS = 1e-7   # the MAP_SSIM map within 1e-7 absolute


@pytest.fixture(scope="module")
def rtm():
    import raytracingmin_amd as m
    n = C.c_int()
    m._lib.check(m.lib().rtm_device_count(C.byref(n)), "rtm_device_count")
    assert n.value >= 1
    return m


def _frame(w, h, dtype):
    """test_tonemap_gpu._frame's distribution: 8 u^4 (a long dark tail, highlights above 1), 10 % exactly black, one
    negative component."""
    rng = np.random.default_rng(w * 1000 + h)
    color = (8 * rng.random((h, w, 3)) ** 4).astype(dtype)
    color[rng.random((h, w)) < 0.1] = 0.0
    color.reshape(-1, 3)[0] = [0.75, -0.25, 1.5]
    return color


def _pair(w, h, dtype):
    a = _frame(w, h, dtype)
    rng = np.random.default_rng(w * 7 + h)
    b = (a + 0.05 * rng.standard_normal((h, w, 3)) * (rng.random((h, w, 1)) < 0.7)).astype(dtype)  # 30 % of the pixels equal
    return a, b


_REFERENCE = {}


def _reference(w, h, dtype):
    """The pair and its float64 evaluation, computed once and shared."""
    key = (w, h, np.dtype(dtype).name)
    if key not in _REFERENCE:
        a, b = _pair(w, h, dtype)
        for v in (a, b):
            v.setflags(write=False)
        _REFERENCE[key] = (a, b) + _compare_ref.compare_ref(a, b)
    return _REFERENCE[key]


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()  # a copy: the shared reference frames are read-only


def _run(rtm, a, b, want=("result",), **kw):
    """compare() on host arrays or device tensors; returns (decoded result or None, map or None, raw result bytes or None)."""
    import torch
    ad = a if isinstance(a, torch.Tensor) else _dev(a)
    bd = b if isinstance(b, torch.Tensor) else _dev(b)
    out = rtm.compare(ad, bd, want=want, **kw)
    torch.cuda.synchronize()
    raw = out["result"].cpu().numpy().copy() if "result" in out else None
    return (rtm.compare_result(raw) if raw is not None else None, out["map"].cpu().numpy() if "map" in out else None, raw)


def _rel(got, want):
    if want == got:
        return 0.0  # both +inf included
    return abs(got - want) / abs(want) if np.isfinite(want) and want != 0 else float("inf")


def _check_against(res, ref, label):
    for k in _compare_ref.EXACT:
        assert res[k] == ref[k], (label, k, res[k], ref[k])
    for k in ("mse", "rel_mse", "psnr"):
        err = _rel(res[k], ref[k])
        print(f"{label}: {k} device {res[k]!r} reference {ref[k]!r} relative error {err:.3e} (bar {REL})")
        assert err <= REL, (label, k, res[k], ref[k])
    err = abs(res["ssim"] - ref["ssim"])
    print(f"{label}: ssim device {res['ssim']!r} reference {ref['ssim']!r} absolute error {err:.3e} (bar {SSIM_ABS})")
    assert err <= SSIM_ABS, (label, res["ssim"], ref["ssim"])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("w,h", FRAMES)
def test_compare_matches_the_reference(rtm, w, h, dtype):
    a, b, ref, maps = _reference(w, h, dtype)
    ad, bd = _dev(a), _dev(b)
    label = f"{w}x{h} {np.dtype(dtype).name}"
    res, _, raw = _run(rtm, ad, bd)
    _check_against(res, ref, label)
    for kind in ("abs", "ssim"):
        res_m, got, raw_m = _run(rtm, ad, bd, want=("result", "map"), map=kind)
        assert np.array_equal(raw_m, raw), (label, kind)  # the record does not depend on the map asked for
        _, alone, _ = _run(rtm, ad, bd, want=("map",), map=kind)  # the map-only launch gives the same map
        assert np.array_equal(alone.view(np.uint32), got.view(np.uint32)), (label, kind)
        if kind == "abs":
            want = maps["abs"].astype(np.float32)
            assert np.array_equal(np.isnan(got), np.isnan(want)), label
            assert np.array_equal(got[~np.isnan(want)], want[~np.isnan(want)]), label
        else:
            err = float(np.abs(got.astype(np.float64) - maps["ssim"]).max())
            print(f"{label}: SSIM map worst absolute error {err:.3e} (bar {MAP_ABS})")
            assert err <= MAP_ABS, (label, err)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_the_tolerance_is_a_strict_inequality(rtm, dtype):
    w, h = 131, 63
    tol = float(dtype(1e-4))  # representable in the frames' own type, so that D_p can equal it exactly
    up, down = float(np.nextafter(dtype(tol), dtype(np.inf))), float(np.nextafter(dtype(tol), dtype(0)))
    b = np.zeros((h, w, 3), dtype)
    a = np.zeros((h, w, 3), dtype)
    rng = np.random.default_rng(5)
    picks = rng.choice(w * h, size=90, replace=False)
    flat = a.reshape(-1, 3)
    for i, p in enumerate(picks):
        flat[p, i % 3] = (tol, up, down)[i // 30]  # 30 pixels of each kind, spread over the tiles
    res, _, _ = _run(rtm, a, b, tolerance=tol)
    assert res["outside"] == 30 and res["max_abs"] == up and res["pixels"] == w * h
    first_up = int(min(picks[30:60]))
    assert (res["argmax_x"], res["argmax_y"]) == (first_up % w, first_up // w)
    ref, _ = _compare_ref.compare_ref(a, b, tolerance=tol)
    assert ref["outside"] == 30
    res0, _, _ = _run(rtm, a, b, tolerance=0.0)
    assert res0["outside"] == 90


def test_one_ulp_at_one_between_two_double_frames_is_seen(rtm):
    w, h = 131, 63
    a = _frame(w, h, np.float64)
    b = a.copy()
    x, y = 77, 41
    a[y, x, 1], b[y, x, 1] = 1.0 + 2.0 ** -52, 1.0  # one ulp at 1.0
    res, emap, _ = _run(rtm, a, b, tolerance=0.0, want=("result", "map"))
    assert res["max_abs"] == 2.0 ** -52 and res["outside"] == 1 and (res["argmax_x"], res["argmax_y"]) == (x, y)
    assert res["mse"] > 0 and np.isfinite(res["psnr"])
    assert emap[y, x] == np.float32(2.0 ** -52) and np.count_nonzero(emap) == 1


def test_argmax_ties_go_to_the_lower_row_major_index(rtm):
    w, h = 131, 63
    for dtype in DTYPES:
        # one tile; two tiles of one tile row (the later tile holds the lower index); two tile rows
        for (x1, y1), (x2, y2) in (((9, 20), (3, 21)), ((100, 3), (2, 4)), ((5, 40), (120, 10)), ((40, 7), (41, 7))):
            a = np.zeros((h, w, 3), dtype)
            b = np.zeros((h, w, 3), dtype)
            a[y1, x1, 0] = 0.5
            a[y2, x2, 2] = -0.5
            a[h - 1, w - 1, 1] = 0.25
            res, _, _ = _run(rtm, a, b)
            want = min((y1 * w + x1, y2 * w + x2))
            assert res["max_abs"] == 0.5 and (res["argmax_x"], res["argmax_y"]) == (want % w, want // w), ((x1, y1), (x2, y2))
            assert res["outside"] == 3


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_non_finite_pixels(rtm, dtype):
    w, h = 37, 23
    a, b = (v.copy() for v in _pair(w, h, dtype))
    a[2, 3], b[2, 3] = [np.nan, 1, 2], [np.nan, 1, 2]             # the same NaN
    a[4, 36], b[4, 36] = [np.inf, -np.inf, 2], [np.inf, -np.inf, 2]  # the same infinities
    a[22, 0], b[22, 0] = [1, np.nan, np.inf], [1, np.nan, np.inf]
    clean, _ = _compare_ref.compare_ref(a, b)
    res, emap, _ = _run(rtm, a, b, want=("result", "map"))
    assert res["nonfinite"] == 3 and res["nonfinite_mismatch"] == 0 and res["pixels"] == w * h - 3
    _check_against(res, clean, f"same non-finite {np.dtype(dtype).name}")
    assert np.isnan(emap[2, 3]) and np.isnan(emap[4, 36]) and np.isnan(emap[22, 0]) and np.isnan(emap).sum() == 3
    # the sums exclude them: the finite fields are those of the frames with those pixels made equal and finite... except SSIM,
    # where they are black in both images; the reference has the same rule, checked above
    a[10, 10, 0] = np.nan                                # NaN against a number
    a[11, 11], b[11, 11] = [np.inf, 0, 0], [-np.inf, 0, 0]  # +inf against -inf
    b[12, 12, 2] = np.inf                                # a number against +inf
    ref, _ = _compare_ref.compare_ref(a, b)
    res, _, _ = _run(rtm, a, b)
    assert res["nonfinite"] == 6 and res["nonfinite_mismatch"] == 3 == ref["nonfinite_mismatch"]
    _check_against(res, ref, f"mismatching non-finite {np.dtype(dtype).name}")
    # an all-NaN frame: n = 0 and the n = 0 value of every field
    nan = np.full((h, w, 3), np.nan, dtype)
    res, emap, _ = _run(rtm, nan, b, want=("result", "map"))
    ref, _ = _compare_ref.compare_ref(nan, b)
    assert res["pixels"] == 0 and res["nonfinite"] == w * h and res["nonfinite_mismatch"] == w * h
    assert res["max_abs"] == 0.0 and res["mse"] == 0.0 and res["rel_mse"] == 0.0 and res["psnr"] == float("inf")
    assert res["outside"] == 0 and (res["argmax_x"], res["argmax_y"]) == (-1, -1)
    assert abs(res["ssim"] - ref["ssim"]) <= SSIM_ABS and abs(res["ssim"] - 1.0) <= 1e-12  # both luminance planes are black
    assert np.isnan(emap).all()
    res, _, _ = _run(rtm, nan, nan)
    assert res["nonfinite_mismatch"] == 0 and res["pixels"] == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_identical_frames(rtm, dtype):
    for w, h in ((1, 1), (37, 23), (131, 63)):
        a = _frame(w, h, dtype)
        ad = _dev(a)
        for bd in (ad, _dev(a)):  # the same buffer twice (a_dev == b_dev), and an equal copy
            res, emap, _ = _run(rtm, ad, bd, want=("result", "map"), tolerance=0.0)
            assert res["max_abs"] == 0.0 and res["mse"] == 0.0 and res["rel_mse"] == 0.0 and res["outside"] == 0
            assert res["psnr"] == float("inf") and abs(res["ssim"] - 1.0) <= 1e-12, res["ssim"]
            assert res["pixels"] == w * h and res["nonfinite"] == 0 and res["nonfinite_mismatch"] == 0
            assert (res["argmax_x"], res["argmax_y"]) == (0, 0) and np.all(emap == 0.0)
            _, smap, _ = _run(rtm, ad, bd, want=("map",), map="ssim")
            assert np.all(np.abs(smap.astype(np.float64) - 1.0) <= 1e-7)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_a_misaligned_frame_gives_the_aligned_bits(rtm, dtype):
    import torch
    w, h = 131, 63
    a, b, _, _ = _reference(w, h, dtype)
    tdtype = torch.float32 if dtype is np.float32 else torch.float64
    item = np.dtype(dtype).itemsize
    aligned = (_dev(a), _dev(b))
    shifted = []
    for v in aligned:
        buf = torch.empty(w * h * 3 + 8, dtype=tdtype, device="cuda")
        s = buf[1:1 + w * h * 3].view(h, w, 3)  # one element past a 16-byte boundary
        s.copy_(v)
        assert v.data_ptr() % 16 == 0 and s.data_ptr() % 16 == item and s.is_contiguous()
        shifted.append(s)
    for kind in ("abs", "ssim"):
        _, map0, raw0 = _run(rtm, *aligned, want=("result", "map"), map=kind)
        for pair in (shifted, (aligned[0], shifted[1]), (shifted[0], aligned[1])):
            _, map1, raw1 = _run(rtm, *pair, want=("result", "map"), map=kind)
            assert np.array_equal(raw0, raw1), kind
            assert np.array_equal(map0.view(np.uint32), map1.view(np.uint32)), kind


def test_the_same_inputs_give_the_same_bits_on_every_call_and_stream(rtm):
    import torch
    for dtype in DTYPES:
        a, b, _, _ = _reference(131, 63, dtype)
        ad, bd = _dev(a), _dev(b)
        _, map0, raw0 = _run(rtm, ad, bd, want=("result", "map"), map="ssim")
        _, map1, raw1 = _run(rtm, ad, bd, want=("result", "map"), map="ssim")
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        out = rtm.compare(ad, bd, want=("result", "map"), map="ssim", stream=side)  # its own work buffer
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
    for w, h in ((37, 23), (131, 63)):
        for dtype, code in ((np.float32, 0), (np.float64, 1)):
            a, b = _pair(w, h, dtype)
            ad, bd = _dev(a), _dev(b)
            sizes = {"work": L.rtm_compare_work_bytes(w, h), "result": C.sizeof(_lib.rtm_compare_result), "map": 4 * w * h}
            for kind in (0, 1):
                bufs = {k: torch.full((n + 2 * G,), 0xA5, dtype=torch.uint8, device="cuda") for k, n in sizes.items()}
                ptr = {k: v.data_ptr() + G for k, v in bufs.items()}
                assert ptr["work"] % 256 == 0
                prm = _lib.rtm_compare_params(code, kind, 1e-4, 1.0, 1e-2)
                _lib.check(L.rtm_compare(C.byref(prm), w, h, 0, ad.data_ptr(), bd.data_ptr(), ptr["work"], ptr["result"], ptr["map"],
                                         stream), "rtm_compare")
                torch.cuda.synchronize()
                for k, v in bufs.items():
                    host = v.cpu().numpy()
                    assert np.all(host[:G] == 0xA5) and np.all(host[G + sizes[k]:] == 0xA5), (w, h, dtype, kind, k)
                # the record in the caller's buffer is the one the work buffer's last 256 bytes hold
                rec = bufs["result"].cpu().numpy()[G:G + sizes["result"]]
                assert np.array_equal(rec, bufs["work"].cpu().numpy()[G + sizes["work"] - 256:][:sizes["result"]])
                assert rtm.compare_result(rec.view(np.int32))["pixels"] == w * h
                assert not np.any(bufs["map"].cpu().numpy()[G:G + 4 * w * h].view(np.uint32) == 0xA5A5A5A5)  # every pixel written
            assert np.array_equal(ad.cpu().numpy().view(np.uint8), a.view(np.uint8))
            assert np.array_equal(bd.cpu().numpy().view(np.uint8), b.view(np.uint8))


def _cornell(rtm, samples):
    data = rtm.LoadData(SCENE).data
    data.width, data.height, data.samples, data.superSamples = 64, 64, samples, 1
    return rtm.Renderer(data, mode="repaired", max_bounces=8)


def test_rendered_frames_match_the_reference(rtm):
    noisy_r = _cornell(rtm, 16)
    noisy, _ = noisy_r.render_rows_device(want=("f32", "f64"), stats=False)
    denoised = rtm.denoise(noisy["f32"], noisy_r.render_aov(), want=("f32",))["f32"]
    converged, _ = _cornell(rtm, 256).render_rows_device(want=("f32", "f64"), stats=False)
    for label, a, b in (("16 spp f32", noisy["f32"], converged["f32"]), ("denoised f32", denoised, converged["f32"]),
                        ("16 spp f64", noisy["f64"], converged["f64"])):
        ref, maps = _compare_ref.compare_ref(a.cpu().numpy(), b.cpu().numpy())
        res, smap, _ = _run(rtm, a, b, want=("result", "map"), map="ssim")
        _check_against(res, ref, label)
        assert float(np.abs(smap.astype(np.float64) - maps["ssim"]).max()) <= MAP_ABS, label
        assert res["pixels"] == 64 * 64 and 0 < res["mse"] and np.isfinite(res["psnr"])
    # Renderer.compare: the last image against a reference, decoded
    noisy_r.image = noisy["f64"].cpu().numpy()
    got = noisy_r.compare(converged["f64"])
    want, _ = _compare_ref.compare_ref(noisy_r.image, converged["f64"].cpu().numpy())
    _check_against(got, want, "Renderer.compare")


def _read_pfm(rtm, path):
    L = rtm.lib()
    w, h, comp = C.c_int(), C.c_int(), C.c_int()
    assert L.rtm_read_pfm(os.fsencode(str(path)), C.byref(w), C.byref(h), C.byref(comp), None, 0) == 1
    data = np.zeros((h.value, w.value, comp.value), np.float32)
    assert L.rtm_read_pfm(os.fsencode(str(path)), C.byref(w), C.byref(h), C.byref(comp), data.ctypes.data, data.size) == 1
    return data


def test_cli_pfm_and_compare(rtm, tmp_path):
    args = [CLI, "-json", SCENE, "--width", "64", "--height", "64", "--samples", "4", "--superSamples", "1", "--max-bounces", "8"]

    def run(stem, *flags, code=0):
        p = subprocess.run(args + ["--out", stem] + list(flags), cwd=tmp_path, capture_output=True, text=True, timeout=300)
        assert p.returncode == code, p.stdout + p.stderr
        return p

    def record(p):
        lines = [l for l in p.stdout.splitlines() if l.startswith("compare: ")]
        assert len(lines) == 1, p.stdout
        rec = json.loads(lines[0][len("compare: "):])
        assert tuple(rec) == _compare_ref.FIELDS
        return rec

    run("plain")
    run("ref", "--pfm", "--dump-f32", "ref.f32")
    frame = np.fromfile(tmp_path / "ref.f32", np.float32).reshape(64, 64, 3)
    assert np.array_equal(_read_pfm(rtm, tmp_path / "ref.pfm").view(np.uint32), frame.view(np.uint32))
    assert (tmp_path / "ref.bmp").read_bytes() == (tmp_path / "plain.bmp").read_bytes()  # no existing file's bytes change
    assert (tmp_path / "ref.jpg").read_bytes() == (tmp_path / "plain.jpg").read_bytes()
    rec = record(run("again", "--compare", "ref.pfm"))
    assert rec["outside"] == 0 and rec["max_abs"] == 0 and rec["pixels"] == 64 * 64 and rec["psnr"] == float("inf")
    assert not (tmp_path / "again.pfm").exists()
    # the denoised frame is the last stage: its own .pfm compares clean, and against the plain frame it does not
    run("dn", "--denoise", "--pfm")
    assert record(run("dn2", "--denoise", "--compare", "dn.pfm"))["max_abs"] == 0
    rec = record(run("dn3", "--denoise", "--compare", "ref.pfm"))
    want, _ = _compare_ref.compare_ref(_read_pfm(rtm, tmp_path / "dn.pfm"), frame)
    _check_against(rec, want, "rtm_cli --denoise --compare")
    assert rec["max_abs"] > 0 and rec["outside"] > 0
    # another size: exit status 1
    other = run("small", "--pfm", "--width", "32")
    assert other.returncode == 0
    p = run("bad", "--compare", "small.pfm", code=1)
    assert "32 x 64" in p.stderr and not (tmp_path / "bad.bmp").exists()
