"""The perceptual frame difference (rtm_flip), the parts that need no GPU: the NumPy restatement against itself (its two
evaluation orders, symmetry, locality, the filters' sums), the bindings and struct layouts, rtm_flip_work_bytes, rtm_flip's
argument checks (all made before any device call), flip_result's pooling of the histogram, the Python entry points' argument
errors and the CLI's refusals."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import _flip_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "raytracingmin_amd", "rtm_cli")
SCENE = os.path.join(ROOT, "scenes", "cornellBoxSetting.json")
SIZE_MAX = C.c_size_t(-1).value
# include/rtm.h: mean, min, max and the map against a float64 evaluation.  max(1e-9, 100 D) with D = 9.3e-14, the largest
# disagreement of the restatement's direct and separable orders over every (frame, ppd, transfer) of _flip_ref.CASES
TOLERANCE = 1e-9
D_RECORDED = 9.4e-14  # D rounded up in its second digit: what the two orders are held to below


def _header():
    return open(os.path.join(ROOT, "include", "rtm.h")).read()


# ---- the restatement against itself -----------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,ppd", _flip_ref.CASES)
def test_the_direct_and_the_separable_order_agree(w, h, ppd):
    a, b = _flip_ref.pair(w, h)
    for transfer in ("srgb", "linear"):
        sep = _flip_ref.flip_map(a, b, transfer, ppd, "separable")
        direct = _flip_ref.flip_map(a, b, transfer, ppd, "direct")
        d = float(np.abs(sep - direct).max())
        print(f"{w}x{h} ppd {ppd} {transfer}: direct against separable {d:.3e} (recorded D {D_RECORDED})")
        assert d <= D_RECORDED, (transfer, d)
        assert max(1e-9, 100 * d) == TOLERANCE
        assert np.all((sep >= 0.0) & (sep <= 1.0)) and np.all((direct >= 0.0) & (direct <= 1.0))
        # the definition is symmetric in a and b
        assert np.array_equal(_flip_ref.flip_map(b, a, transfer, ppd, "separable"), sep)


def test_identical_frames_give_an_all_zero_map():
    a, _ = _flip_ref.pair(37, 23)
    for order in ("separable", "direct"):
        m = _flip_ref.flip_map(a, a, "srgb", 67.02, order)
        assert np.array_equal(m, np.zeros((23, 37))) and not np.signbit(m).any()
    res, _ = _flip_ref.flip_ref(a, a)
    assert res["mean"] == res["max"] == res["min"] == 0.0 and (res["argmax_x"], res["argmax_y"]) == (0, 0)
    assert res["hist"][0] == 37 * 23 == res["pixels"] and res["hist"].sum() == 37 * 23


def test_black_against_white_is_one_constant():
    black, white = np.zeros((30, 41, 3), np.float32), np.ones((30, 41, 3), np.float32)
    for transfer in ("srgb", "linear"):
        m = _flip_ref.flip_map(black, white, transfer)
        assert np.all(m == m[0, 0])
        assert abs(m[0, 0] - 0.9673797618941135) <= 1e-12  # DESIGN.md records it


def test_a_one_pixel_change_stays_within_the_larger_radius():
    for ppd in (67.02, 8.0):
        reach = max(_flip_ref.csf_radius(ppd), _flip_ref.feature_radius(ppd))
        h, w = 2 * reach + 9, 2 * reach + 11
        a, _ = _flip_ref.pair(w, h)
        b = a.copy()
        y0, x0 = reach + 3, reach + 5
        b[y0, x0] = [0.9, 0.1, 0.4]
        m = _flip_ref.flip_map(a, b, "srgb", ppd)
        yy, xx = np.mgrid[0:h, 0:w]
        far = (np.abs(yy - y0) > reach) | (np.abs(xx - x0) > reach)
        assert far.any() and np.all(m[far] == 0.0) and m[y0, x0] > 0.0


def test_the_filters_sum_as_the_header_says():
    assert _flip_ref.csf_radius(_flip_ref.DEFAULT_PPD) == 10 and _flip_ref.feature_radius(_flip_ref.DEFAULT_PPD) == 9
    assert (_flip_ref.csf_radius(8.0), _flip_ref.feature_radius(8.0)) == (2, 1)
    assert (_flip_ref.csf_radius(128.0), _flip_ref.feature_radius(128.0)) == (18, 16)
    assert abs(_flip_ref.cmax() - 41.27609841459544) <= 1e-12
    for ppd in _flip_ref.PPDS + [_flip_ref.DEFAULT_PPD, 33.3]:
        for name, f in _flip_ref.csf_filters_2d(ppd).items():
            assert abs(f.sum() - 1.0) <= 1e-14, (ppd, name)
        t = _flip_ref.csf_tables(ppd)
        assert abs(t["y"].sum() - 1.0) <= 1e-14 and abs(t["cx"].sum() - 1.0) <= 1e-14
        assert abs(t["cz1"].sum() ** 2 + t["cz2"].sum() ** 2 - 1.0) <= 1e-14
        # the separable tables are the 2-D filters (entries up to 1: a few roundings of 1.1e-16 each)
        f2 = _flip_ref.csf_filters_2d(ppd)
        assert np.abs(np.outer(t["y"], t["y"]) - f2["y"]).max() <= 1e-15
        assert np.abs(np.outer(t["cz1"], t["cz1"]) + np.outer(t["cz2"], t["cz2"]) - f2["cz"]).max() <= 1e-15
        ft, f2 = _flip_ref.feature_tables(ppd), _flip_ref.feature_filters_2d(ppd)
        assert abs(ft["g"].sum() - 1.0) <= 1e-14
        for name in ("d", "p"):
            v = ft[name]
            assert abs(v[v > 0].sum() - 1.0) <= 1e-14 and abs(v[v < 0].sum() + 1.0) <= 1e-14, (ppd, name)
        for name, tab in (("edge", "d"), ("point", "p")):
            f = f2[name]
            assert abs(f[f > 0].sum() - 1.0) <= 1e-14 and abs(f[f < 0].sum() + 1.0) <= 1e-14, (ppd, name)
            assert np.abs(np.outer(ft["g"], ft[tab]) - f).max() <= 1e-15, (ppd, name)


def test_non_counting_pixels_are_black_to_their_neighbours():
    a, b = _flip_ref.pair(21, 21)
    a, b = a.copy(), b.copy()
    a[5, 6, 1] = np.nan
    b[20, 20] = [np.inf, 0, 0]
    res, m = _flip_ref.flip_ref(a, b)
    assert np.isnan(m[5, 6]) and np.isnan(m[20, 20]) and np.isnan(m).sum() == 2 == res["nonfinite"]
    a2, b2 = a.copy(), b.copy()
    a2[5, 6] = b2[5, 6] = a2[20, 20] = b2[20, 20] = 0.0
    m2 = _flip_ref.flip_map(a2, b2)
    keep = ~np.isnan(m)
    assert np.array_equal(m[keep], m2[keep])
    nan = np.full((3, 4, 3), np.nan, np.float32)
    res, _ = _flip_ref.flip_ref(nan, nan)
    assert res["pixels"] == 0 and res["mean"] == res["max"] == res["min"] == 0.0 and (res["argmax_x"], res["argmax_y"]) == (-1, -1)


# ---- the library without a device -------------------------------------------------------------------------------------
def test_flip_is_bound_and_exported_and_the_structs_match_the_header():
    import raytracingmin_amd as rtm
    from raytracingmin_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    header = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in ("rtm_flip", "rtm_flip_work_bytes"):
        assert name in _lib.SIGNATURES and hasattr(raw, name), name
        assert re.search(r"\b%s\s*\(" % name, header), name
    ctype = {"int32_t": C.c_int32, "uint64_t": C.c_uint64, "double": C.c_double, "uint32_t": C.c_uint32}
    for name, cls, size in (("rtm_flip_params", _lib.rtm_flip_params, 16), ("rtm_flip_result", _lib.rtm_flip_result, 1072)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, flags=re.S).group(1)
        declared = []
        for decl in body.split(";"):
            if decl.strip():
                ty, names = decl.split(None, 1)
                for n in names.split(","):
                    arr = re.fullmatch(r"(\w+)\[(\d+)\]", n.strip())
                    declared.append((arr.group(1), ctype[ty] * int(arr.group(2))) if arr else (n.strip(), ctype[ty]))
        assert [f[0] for f in cls._fields_] == [d[0] for d in declared], name
        assert [C.sizeof(f[1]) for f in cls._fields_] == [C.sizeof(d[1]) for d in declared], name
        assert C.sizeof(cls) == size, name
    assert C.sizeof(_lib.rtm_flip_result) == sum(C.sizeof(f[1]) for f in _lib.rtm_flip_result._fields_)  # no padding
    assert tuple(f[0] for f in _lib.rtm_flip_result._fields_) == _flip_ref.FIELDS
    assert "1072 bytes, no padding" in _header() and "within 1e-9 absolute" in _header()
    macro = re.search(r"#define RTM_FLIP_DEFAULTS \{([^}]*)\}", header).group(1)
    assert [v.strip() for v in macro.split(",")] == ["RTM_TRANSFER_SRGB", "RTM_FLIP_DEFAULT_PPD"]
    expr = re.search(r"#define RTM_FLIP_DEFAULT_PPD \((.*)\)", header).group(1)
    assert eval(expr) == rtm.FLIP_DEFAULTS["pixels_per_degree"] == _flip_ref.DEFAULT_PPD == 0.7 * 3840 / 0.7 * np.pi / 180
    assert rtm.FLIP_DEFAULTS == _flip_ref.DEFAULTS and _lib.TRANSFERS["srgb"] == 1 and _lib.TRANSFERS["linear"] == 0
    for name in ("flip", "flip_result", "FLIP_DEFAULTS"):
        assert name in rtm.__all__ and hasattr(rtm, name), name
    params = inspect.signature(rtm.flip).parameters
    assert {k: params[k].default for k in rtm.FLIP_DEFAULTS} == rtm.FLIP_DEFAULTS
    assert params["want"].default == ("result",) and params["stream"].default is None
    assert list(inspect.signature(rtm.Renderer.flip).parameters)[:3] == ["self", "reference", "frame"]
    assert _lib.lib().rtm_abi_version() == 5  # added without a bump


def test_flip_work_bytes():
    from raytracingmin_amd import _lib
    L = _lib.lib()
    for w, h in ((0, 5), (5, 0), (-4, 5), (5, -4), (0, 0), (-(2**31), -(2**31))):
        assert L.rtm_flip_work_bytes(w, h) == 0, (w, h)

    def formula(w, h):
        r256 = lambda v: -(-v // 256) * 256
        return r256(112 * w * h) + r256(32 * (-(-w // 64) * -(-h // 16))) + 1024

    assert L.rtm_flip_work_bytes(1, 1) == formula(1, 1) == 256 + 256 + 1024
    for w, h in ((1, 23), (7, 5), (21, 21), (37, 23), (64, 64), (65, 17), (131, 63), (1920, 1080), (3840, 2160), (2**31 - 1, 1)):
        assert L.rtm_flip_work_bytes(w, h) == formula(w, h), (w, h)
    assert 112 * (2**31 - 1) ** 2 > SIZE_MAX
    assert L.rtm_flip_work_bytes(2**31 - 1, 2**31 - 1) == SIZE_MAX


def test_flip_rejects_invalid_arguments_without_a_gpu():
    from raytracingmin_amd import _lib
    L = _lib.lib()
    good = (1, _flip_ref.DEFAULT_PPD)
    a, b, work, result, emap = (C.c_void_p(0x1000), C.c_void_p(0x20000), C.c_void_p(0x300000), C.c_void_p(0x4000000),
                                C.c_void_p(0x50000000))
    # fake device pointers: never dereferenced, every call below fails its checks first

    def call(p=good, w=8, h=8, dev=0, fa=a, fb=b, wk=work, res=result, mp=emap):
        prm = None if p is None else C.byref(_lib.rtm_flip_params(*p))
        return L.rtm_flip(prm, w, h, dev, fa, fb, wk, res, mp, None)

    assert call(p=None) == -1
    assert b"null" in L.rtm_last_error_detail()
    assert call(fa=None) == -1 and call(fb=None) == -1 and call(wk=None) == -1
    assert call(res=None, mp=None) == -1
    assert b"output" in L.rtm_last_error_detail()
    for w, h in ((0, 8), (8, 0), (-1, 8), (8, -3)):
        assert call(w=w, h=h) == -1, (w, h)
    for v in (-1, 2, 1 << 30):
        assert call(p=(v, 67.0)) == -1, v
        assert b"transfer" in L.rtm_last_error_detail()
    for v in (float("nan"), float("inf"), float("-inf"), 0.0, -67.0, np.nextafter(8.0, 0.0), np.nextafter(128.0, 200.0)):
        assert call(p=(1, v)) == -1, v
        assert b"pixels_per_degree" in L.rtm_last_error_detail()
    for off in (1, 2, 3):
        assert call(fa=C.c_void_p(0x1000 + off)) == -1 and call(fb=C.c_void_p(0x20000 + off)) == -1, off
        assert b"aligned" in L.rtm_last_error_detail()
        assert call(mp=C.c_void_p(0x50000000 + off)) == -1
    assert call(res=C.c_void_p(0x4000004)) == -1
    for off in (8, 16, 64, 128):  # work_dev not 256-byte aligned
        assert call(wk=C.c_void_p(0x300000 + off)) == -1, off
        assert b"work_dev" in L.rtm_last_error_detail()
    aligned = C.c_void_p(0x70000)
    for frame in ("fa", "fb"):  # work_dev or either output equal to a frame
        for other in ("wk", "res", "mp"):
            assert call(**{frame: aligned, other: aligned}) == -1, (frame, other)
            assert b"aliases" in L.rtm_last_error_detail()
    assert call(mp=aligned, wk=aligned) == -1 and call(mp=aligned, res=aligned) == -1
    assert b"map_out_dev" in L.rtm_last_error_detail()
    assert call(res=aligned, wk=aligned) == -1
    assert call(dev=-1) == -1
    assert b"device" in L.rtm_last_error_detail()
    # what is allowed passes every check and is refused only for its device number: the same frame twice, one output, a frame
    # at a 4-byte address, both transfers, the ends of the ppd range
    for kw in (dict(fb=a), dict(res=None), dict(mp=None), dict(fa=C.c_void_p(0x1004)), dict(p=(0, 8.0)), dict(p=(1, 128.0))):
        assert call(dev=-1, **kw) == -1, kw
        assert b"device" in L.rtm_last_error_detail(), kw
    # 2^31 pixels or more: unsupported (after the argument checks, still before any device call)
    assert call(w=2**16, h=2**15) == -8
    assert L.rtm_strerror(-8) == b"unsupported" and b"too large" in L.rtm_last_error_detail()


def test_flip_result_decodes_a_record_and_pools_the_histogram():
    import raytracingmin_amd as rtm
    from raytracingmin_amd import _lib

    def decode(hist):
        rec = _lib.rtm_flip_result(0.5, 0.75, 0.25, 2**40 + 1, 3, -1, 7, (C.c_uint32 * 256)(*hist))
        words = np.frombuffer(bytes(rec), np.int32)
        assert words.size == 268
        return rtm.flip_result(words)

    centre = lambda i: (i + 0.5) / 256.0
    # one bin: every quantile is its centre
    hist = [0] * 256
    hist[10] = 7
    out = decode(hist)
    assert out["weighted_median"] == out["weighted_first_quartile"] == out["weighted_third_quartile"] == centre(10)
    assert (out["mean"], out["max"], out["min"], out["pixels"], out["nonfinite"], out["argmax_x"], out["argmax_y"]) == \
        (0.5, 0.75, 0.25, 2**40 + 1, 3, -1, 7) and out["hist"] == hist
    # two bins, equal counts: the weights are 0.5 * 1.5/256 and 0.5 * 200.5/256, so the upper bin holds more than three
    # quarters of the weight and every quartile falls in it (a plain median would be the lower one)
    hist = [0] * 256
    hist[1], hist[200] = 100, 100
    out = decode(hist)
    assert out["weighted_median"] == out["weighted_first_quartile"] == centre(200)
    # three bins with weights 3 c(0) = 1.5/256, 1 c(1) = 1.5/256, 1 c(4) = 4.5/256 (total 7.5/256): the running weight is
    # 0.2, 0.4, 1.0 of the total: the first quartile is bin 1, the median and the third quartile bin 4
    hist = [0] * 256
    hist[0], hist[1], hist[4] = 3, 1, 1
    out = decode(hist)
    assert out["weighted_first_quartile"] == centre(1) and out["weighted_median"] == centre(4) == out["weighted_third_quartile"]
    for q in (0.25, 0.5, 0.75):
        assert _flip_ref.weighted_quantile(hist, q) == rtm.renderer._flip_weighted_quantile(hist, q)
    # an empty histogram
    assert decode([0] * 256)["weighted_median"] == 0.0
    # the host histogram rule: the FLOAT value times 256, truncated, 1.0 in the last bin, NaN nowhere
    m = np.array([0.0, 1.0 / 256, np.nextafter(np.float32(1.0 / 256), np.float32(0)), 0.999, 1.0, np.nan], np.float32)
    h = _flip_ref.histogram(m)
    assert h[0] == 2 and h[1] == 1 and h[255] == 2 and h.sum() == 5


def test_python_shape_and_dtype_errors_raise_before_any_device_use():
    import raytracingmin_amd as rtm
    a = np.zeros((4, 5, 3), np.float32)  # not even tensors: a mismatch is reported before the library or the device is touched
    for b in (np.zeros((5, 4, 3), np.float32), np.zeros((4, 5), np.float32), np.zeros((4, 5, 4), np.float32),
              np.zeros((4, 5, 3), np.float64), np.zeros((4, 6, 3), np.float32)):
        with pytest.raises(ValueError):
            rtm.flip(a, b)
    for bad in (np.zeros((4, 5, 3), np.float16), np.zeros((4, 5, 3), np.float64), np.zeros((0, 5, 3), np.float32)):
        with pytest.raises(ValueError):
            rtm.flip(bad, bad)
    for kw in (dict(transfer="gamma"), dict(pixels_per_degree=7.9), dict(pixels_per_degree=128.5), dict(pixels_per_degree=float("nan")),
               dict(want=()), dict(want=("result", "hist"))):
        with pytest.raises(ValueError):
            rtm.flip(a, a, **kw)


def test_cli_usage_mentions_flip_and_refuses_bad_references_before_rendering(tmp_path):
    r = subprocess.run([CLI, "-?"], capture_output=True, text=True, timeout=60)
    for word in ("--flip REF.pfm", "--flip-ppd", "--flip-map", "--display-pfm", "STEM_flip.pfm", "STEM_display.pfm", "flip: {"):
        assert word in r.stdout + r.stderr, word
    args = [CLI, "-json", SCENE, "--width", "8", "--height", "8", "--out", "x"]
    run = lambda *flags: subprocess.run(args + list(flags), cwd=tmp_path, capture_output=True, text=True, timeout=60)
    p = run("--flip", "missing.pfm")
    assert p.returncode == 1 and "missing.pfm" in p.stderr and not (tmp_path / "x.bmp").exists()
    (tmp_path / "other.pfm").write_bytes(b"PF\n4 8\n-1.0\n" + bytes(4 * 8 * 12))
    p = run("--flip", "other.pfm")
    assert p.returncode == 1 and "4 x 8" in p.stderr and not (tmp_path / "x.bmp").exists()
    (tmp_path / "grey.pfm").write_bytes(b"Pf\n8 8\n-1.0\n" + bytes(8 * 8 * 4))
    assert run("--flip", "grey.pfm").returncode == 1 and not (tmp_path / "x.bmp").exists()
    (tmp_path / "ok.pfm").write_bytes(b"PF\n8 8\n-1.0\n" + bytes(8 * 8 * 12))
    p = run("--flip", "ok.pfm", "--preview", "2", "--preview-only")
    assert p.returncode == 2 and "--flip" in p.stderr
    for flags in (("--flip", "ok.pfm", "--flip-ppd", "4"), ("--flip", "ok.pfm", "--flip-ppd", "many"), ("--flip-map",),
                  ("--flip-ppd", "30"), ("--display-pfm",)):
        p = run(*flags)
        assert p.returncode == 2 and not (tmp_path / "x.bmp").exists(), flags
