"""The colour grade, the parts that need no GPU: the bindings and the struct layout, rtm_grade's argument checks (all made
before any device call), rtm_grade_white_balance against the NumPy restatement, the .cube reader (round trips, the accepted
spellings, every refusal with its line number), the Python entry points' argument errors, the CLI's refusals, and the margin
condition on the inputs of test_grade_gpu: on each of its cases plain float32 arithmetic lies within 2e-5 max(1, |ref|) of the
float64 reference, which leaves the device's fast forms a factor of five inside the 1e-4 contract."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import _grade_ref
import _resize_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "raytracingmin_amd", "rtm_cli")
SCENE = os.path.join(ROOT, "scenes", "cornellBoxSetting.json")
MARGIN = 2e-5  # the float32 evaluation against the float64 one, on the GPU test's inputs
NAN, INF = float("nan"), float("inf")


def _header():
    return open(os.path.join(ROOT, "include", "rtm.h")).read()


def _params(**kw):
    """An rtm_grade_params straight from the values, with no check of the package's in between."""
    from raytracingmin_amd import _lib
    prm = _lib.rtm_grade_params()
    vals = dict(matrix=np.eye(3).ravel(), exposure=0.0, contrast=1.0, pivot=0.18, slope=(1, 1, 1), offset=(0, 0, 0), power=(1, 1, 1),
                saturation=1.0, lut_size=0, lut_interp=1, lut_min=(0, 0, 0), lut_max=(1, 1, 1))
    assert set(kw) <= set(vals), kw
    vals.update(kw)
    for name, v in vals.items():
        if name in ("lut_size", "lut_interp"):
            setattr(prm, name, int(v))
        elif np.ndim(v) == 0:
            setattr(prm, name, float(v))
        else:
            words = np.ascontiguousarray(v, dtype=np.float32).ravel()
            C.memmove(getattr(prm, name), words.ctypes.data, words.nbytes)
    return prm


def test_grade_is_bound_and_exported_and_the_struct_matches_the_header():
    import raytracingmin_amd as rtm
    from raytracingmin_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("rtm_grade", "rtm_grade_white_balance", "rtm_lut_parse_cube", "rtm_lut_load_cube"):
        assert name in _lib.SIGNATURES and hasattr(raw, name)
    header = _header()
    body = re.search(r"typedef struct rtm_grade_params \{(.*?)\} rtm_grade_params;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = []
    for decl in body.split(";"):
        if decl.strip():
            ty, names = decl.split(None, 1)
            for n in names.split(","):
                m = re.fullmatch(r"(\w+)(?:\[(\d+)\])?", n.strip())
                base = {"float": C.c_float, "int32_t": C.c_int32}[ty]
                declared.append((m.group(1), base * int(m.group(2)) if m.group(2) else base))
    want = [("matrix", C.c_float * 9), ("exposure", C.c_float), ("contrast", C.c_float), ("pivot", C.c_float), ("slope", C.c_float * 3),
            ("offset", C.c_float * 3), ("power", C.c_float * 3), ("saturation", C.c_float), ("lut_size", C.c_int32),
            ("lut_interp", C.c_int32), ("lut_min", C.c_float * 3), ("lut_max", C.c_float * 3)]
    assert [(f[0], f[1]) for f in _lib.rtm_grade_params._fields_] == declared == want
    assert C.sizeof(_lib.rtm_grade_params) == 120
    res, args = _lib.SIGNATURES["rtm_grade"]
    assert res is C.c_int and len(args) == 9 and args[1:4] == [C.c_int32, C.c_int32, C.c_int]
    assert len(_lib.SIGNATURES["rtm_grade_white_balance"][1]) == 3 and len(_lib.SIGNATURES["rtm_lut_parse_cube"][1]) == 7
    assert len(_lib.SIGNATURES["rtm_lut_load_cube"][1]) == 6
    enum = re.search(r"enum \{ (RTM_GRADE_TRILINEAR[^}]*) \};", header).group(1)
    assert [e.strip() for e in enum.split(",")] == [f"RTM_GRADE_{n.upper()} = {i}" for i, n in enumerate(_grade_ref.INTERPS)]
    defaults = re.search(r"#define RTM_GRADE_DEFAULTS(.*?)\n(?!\s)", header, flags=re.S).group(1).replace("\\", " ")
    assert re.sub(r"\s+", "", defaults) == ("{{1.0f,0.0f,0.0f,0.0f,1.0f,0.0f,0.0f,0.0f,1.0f},0.0f,1.0f,0.18f,{1.0f,1.0f,1.0f},"
                                            "{0.0f,0.0f,0.0f},{1.0f,1.0f,1.0f},1.0f,0,RTM_GRADE_TETRAHEDRAL,{0.0f,0.0f,0.0f},{1.0f,1.0f,1.0f}}")
    assert rtm.GRADE_INTERPS == _lib.GRADE_INTERPS == _grade_ref.INTERPS == ("trilinear", "tetrahedral")
    assert rtm.GRADE_DEFAULTS == _lib.GRADE_DEFAULTS == {"matrix": None, "exposure": 0.0, "contrast": 1.0, "pivot": 0.18, "slope": 1.0,
                                                         "offset": 0.0, "power": 1.0, "saturation": 1.0}
    for name in ("grade", "white_balance", "load_cube", "GRADE_DEFAULTS", "GRADE_INTERPS"):
        assert name in rtm.__all__ and hasattr(rtm, name)
    params = inspect.signature(rtm.grade).parameters
    assert list(params) == ["color", "matrix", "exposure", "contrast", "pivot", "slope", "offset", "power", "saturation", "lut", "lut_domain",
                            "interp", "want", "stream", "out_f32"]
    assert {k: params[k].default for k in rtm.GRADE_DEFAULTS} == rtm.GRADE_DEFAULTS
    assert params["lut"].default is None and params["lut_domain"].default == ((0, 0, 0), (1, 1, 1)) and params["interp"].default == "tetrahedral"
    assert params["want"].default == ("f32",) and params["stream"].default is None and params["out_f32"].default is None
    assert list(inspect.signature(rtm.white_balance).parameters) == ["kelvin", "tint"]
    assert list(inspect.signature(rtm.load_cube).parameters) == ["path"]
    for fn in (rtm.Renderer.Render, rtm.Renderer.write_display):
        p = inspect.signature(fn).parameters
        assert p["grade"].default is None and p["lut"].default is None
    assert _lib.lib().rtm_abi_version() == 5  # added without a bump
    assert re.search(r"#define RTM_ABI_VERSION 5\b", header)


def test_grade_rejects_invalid_arguments_without_a_gpu():
    from raytracingmin_amd import _lib
    L = _lib.lib()
    src, out32, out8, lut = C.c_void_p(0x1000), C.c_void_p(0x300000), C.c_void_p(0x4000000), C.c_void_p(0x5000000)
    # fake device pointers: never dereferenced, every call below fails its checks first

    def call(p={}, w=8, h=6, dev=0, s=src, t=None, o32=out32, o8=out8):
        prm = None if p is None else C.byref(_params(**p))
        return L.rtm_grade(prm, w, h, dev, s, t, o32, o8, None)

    def detail():
        return L.rtm_last_error_detail()

    def past(v, towards):
        return float(np.nextafter(np.float32(v), np.float32(towards)))

    assert call(p=None) == -1 and b"params" in detail()
    assert call(s=None) == -1 and b"color_dev" in detail()
    assert call(o32=None, o8=None) == -1 and b"out_f32_dev" in detail() and b"out_u8_dev" in detail()
    for kw in (dict(w=0), dict(h=0), dict(w=-1), dict(h=-3)):
        assert call(**kw) == -1 and b"size" in detail(), kw
    # a NaN, an infinity, and just past either end of every range
    for k in range(9):
        for v in (NAN, INF, -INF):
            m = np.eye(3).ravel()
            m[k] = v
            assert call(p=dict(matrix=m)) == -1 and b"matrix" in detail(), (k, v)
    for name, bad in (("exposure", (NAN, INF, -INF, past(32, 99), past(-32, -99))),
                      ("contrast", (NAN, INF, -INF, past(0.25, 0), past(4, 9))),
                      ("pivot", (NAN, INF, -INF, 0.0, -0.18)),
                      ("saturation", (NAN, INF, -INF, past(0, -1), past(4, 9)))):
        for v in bad:
            assert call(p={name: v}) == -1 and name.encode() in detail(), (name, v)
    for name, bad in (("slope", (NAN, INF, -INF, past(0, -1))), ("offset", (NAN, INF, -INF)),
                      ("power", (NAN, INF, -INF, past(0.1, 0), past(10, 99), 0.0))):
        for v in bad:
            for c in range(3):
                three = [1.0 if name != "offset" else 0.0] * 3
                three[c] = v
                assert call(p={name: three}) == -1 and name.encode() in detail(), (name, v, c)
    for n in (1, -1, 257, 1 << 20):
        assert call(p=dict(lut_size=n), t=lut) == -1 and b"lut_size" in detail(), n
    for v in (-1, 2, 1 << 30):
        assert call(p=dict(lut_interp=v)) == -1 and b"lut_interp" in detail(), v
        assert call(p=dict(lut_size=17, lut_interp=v), t=lut) == -1 and b"lut_interp" in detail(), v
    assert call(p=dict(lut_size=17)) == -1 and b"lut_dev is null" in detail()
    assert call(t=lut) == -1 and b"lut_dev is not null" in detail()
    for c in range(3):
        for name in ("lut_min", "lut_max"):
            for v in (NAN, INF, -INF):
                three = [0.0 if name == "lut_min" else 1.0] * 3
                three[c] = v
                assert call(p={name: three, "lut_size": 2}, t=lut) == -1 and b"lut_m" in detail(), (name, v, c)
        lo, hi = [0.0] * 3, [1.0] * 3
        hi[c] = 0.0
        assert call(p=dict(lut_min=lo, lut_max=hi, lut_size=2), t=lut) == -1 and b"lut_max <= lut_min" in detail(), c
        lo[c] = 0.5
        assert call(p=dict(lut_min=lo, lut_max=hi, lut_size=2), t=lut) == -1 and b"lut_max <= lut_min" in detail(), c
    for name in ("s", "o32", "t"):  # a float pointer that is not 4-byte aligned
        for off in (1, 2, 3):
            kw = {"t": lut}
            kw[name] = C.c_void_p(0x600000 + off)
            assert call(p=dict(lut_size=2), **kw) == -1 and b"4-byte" in detail(), (name, off)
    assert call(p=dict(lut_size=2), t=out32) == -1 and b"lut_dev aliases" in detail()
    assert call(p=dict(lut_size=2), t=out8) == -1 and b"lut_dev aliases" in detail()
    assert call(o8=src) == -1 and b"out_u8_dev aliases color_dev" in detail()
    assert call(dev=-1) == -1 and b"device" in detail()
    # a frame of 2^31 pixels or more: RTM_ERR_UNSUPPORTED
    assert call(w=1 << 16, h=1 << 15) == -8 and b"2^31 pixels" in detail()
    assert call(w=1 << 30, h=2) == -8 and b"2^31 pixels" in detail()
    # the limits themselves, in place, single outputs, an odd u8 pointer, a LUT at both sizes' ends pass every check: what
    # refuses these is the device
    for kw in (dict(p=dict(exposure=32, contrast=4, pivot=1e-30, slope=(0, 0, 0), offset=(-3e38, 3e38, 0), power=(0.1, 10, 1), saturation=4)),
               dict(p=dict(exposure=-32, contrast=0.25, saturation=0, matrix=np.full(9, -3e38))),
               dict(p=dict(lut_size=2, lut_interp=0, lut_min=(-3e38,) * 3, lut_max=(3e38,) * 3), t=lut),
               dict(p=dict(lut_size=256, lut_min=(0, 0, 0), lut_max=(1e-45,) * 3), t=lut),
               dict(o32=src), dict(o32=src, o8=None), dict(o32=None), dict(o8=None), dict(o8=C.c_void_p(0x4000001)), dict(w=1, h=1),
               dict(w=(1 << 16) - 1, h=1 << 15), dict(w=1, h=(1 << 31) - 1), dict(s=C.c_void_p(0x1004), o32=C.c_void_p(0x300008)),
               dict(p=dict(lut_size=2), t=src)):
        assert call(dev=-1, **kw) == -1, kw
        assert b"device" in detail(), kw


KELVINS = (1667, 2222, 2856, 4000, 4001, 6504, 25000)
TINTS = (-0.05, 0, 0.03)


def test_white_balance_matches_the_restatement():
    import raytracingmin_amd as rtm
    # the published chromaticities of Kang's fit, as the header quotes them
    for kelvin, xy in ((2856, (0.4471, 0.4075)), (5000, (0.3450, 0.3516)), (6504, (0.3134, 0.3236))):
        assert np.allclose(_grade_ref.planckian_xy(kelvin), xy, atol=5e-5), kelvin
    for kelvin in KELVINS:
        for tint in TINTS:
            want, rgb = _grade_ref.white_balance_ref(kelvin, tint)
            got = rtm.white_balance(kelvin, tint)
            assert got.shape == (3, 3) and got.dtype == np.float32
            assert np.max(np.abs(got.astype(np.float64) - want)) <= 1e-6, (kelvin, tint)
            white = got.astype(np.float64) @ rgb  # the source white's linear RGB comes out neutral
            assert np.ptp(white) <= 1e-5 * np.max(np.abs(white)), (kelvin, tint, white)
    assert np.allclose(rtm.white_balance(6504), np.eye(3), atol=0.05)  # D65's own temperature: close to the identity
    warm = rtm.white_balance(3200)
    assert warm[2, 2] > 1.5 and warm[0, 0] < 1.0  # a tungsten source: blue is lifted against red


def test_white_balance_refusals():
    import raytracingmin_amd as rtm
    from raytracingmin_amd import _lib
    L = _lib.lib()
    m = (C.c_float * 9)()
    for kelvin in (1666.9, 25000.1, 0.0, -5000.0, NAN, INF, -INF):
        assert L.rtm_grade_white_balance(kelvin, 0.0, m) == -1 and b"kelvin" in L.rtm_last_error_detail(), kelvin
    for tint in (-0.0501, 0.0501, NAN, INF, -INF):
        assert L.rtm_grade_white_balance(5000.0, tint, m) == -1 and b"tint" in L.rtm_last_error_detail(), tint
    assert L.rtm_grade_white_balance(5000.0, 0.0, None) == -1 and b"matrix_out" in L.rtm_last_error_detail()
    for kelvin, tint in ((1667, -0.05), (25000, 0.05)):
        assert L.rtm_grade_white_balance(kelvin, tint, m) == 0
    for bad in (dict(kelvin=1000), dict(kelvin=30000), dict(kelvin=NAN), dict(kelvin="5000"), dict(kelvin=True), dict(kelvin=5000, tint=0.06),
                dict(kelvin=5000, tint=NAN), dict(kelvin=5000, tint="green")):
        with pytest.raises(ValueError):
            rtm.white_balance(**bad)


def _parse(text, capacity=None):
    """(status, detail, size, domain_min, domain_max, table): the size query when capacity is None, else a load."""
    from raytracingmin_amd import _lib
    L = _lib.lib()
    raw = text if isinstance(text, bytes) else text.encode("ascii")
    n = C.c_int32(-1)
    lo, hi = (C.c_float * 3)(), (C.c_float * 3)()
    table = None if capacity is None else np.full(capacity, -7.0, np.float32)
    rc = L.rtm_lut_parse_cube(raw, len(raw), C.byref(n), lo, hi, None if table is None else table.ctypes.data, capacity or 0)
    return rc, (L.rtm_last_error_detail() or b"").decode(), n.value, tuple(lo), tuple(hi), table


@pytest.mark.parametrize("n", (2, 3, 17))
def test_cube_round_trip_is_bit_for_bit(tmp_path, n):
    import raytracingmin_amd as rtm
    rng = np.random.default_rng(n)
    table = ((rng.random((n, n, n, 3)) - 0.25) * 3.0).astype(np.float32)
    table[0, 0, 0] = (0.0, -0.0, 1e-38)  # -0 and a denormal-sized entry keep their bits
    table[-1, -1, -1] = (3.4e38, -3.4e38, 1.0)
    plain, fancy = tmp_path / "plain.cube", tmp_path / "fancy.cube"
    _grade_ref.write_cube(plain, table)
    got = rtm.load_cube(str(plain))
    assert got["size"] == n and got["domain_min"] == (0.0, 0.0, 0.0) and got["domain_max"] == (1.0, 1.0, 1.0)
    assert got["table"].dtype == np.float32 and got["table"].shape == (n, n, n, 3)
    assert np.array_equal(got["table"].view(np.uint32), table.view(np.uint32))
    # comments, blank lines, CR LF, a title, DOMAIN_MIN / DOMAIN_MAX
    _grade_ref.write_cube(fancy, table, domain_min=(-0.25, 0, 0.5), domain_max=(4, 1, 1.5), eol="\r\n", title="a look # not a comment",
                          comments=True)
    got = rtm.load_cube(fancy)  # (a path object)
    assert got["size"] == n and got["domain_min"] == (-0.25, 0.0, 0.5) and got["domain_max"] == (4.0, 1.0, 1.5)
    assert np.array_equal(got["table"].view(np.uint32), table.view(np.uint32))
    # the other spelling of the domain sets all three channels
    _grade_ref.write_cube(fancy, table, input_range=(-1, 2.5))
    got = rtm.load_cube(str(fancy))
    assert got["domain_min"] == (-1.0,) * 3 and got["domain_max"] == (2.5,) * 3
    assert np.array_equal(got["table"].view(np.uint32), table.view(np.uint32))
    # the size query, then the load; a table one float short
    text = open(plain, "rb").read()
    rc, _, size, lo, hi, _ = _parse(text)
    assert (rc, size, lo, hi) == (0, n, (0.0,) * 3, (1.0,) * 3)
    rc, _, size, _, _, out = _parse(text, 3 * n ** 3 + 5)
    assert rc == 0 and np.array_equal(out[:3 * n ** 3].view(np.uint32), table.ravel().view(np.uint32)) and np.all(out[3 * n ** 3:] == -7.0)
    rc, detail, size, _, _, out = _parse(text, 3 * n ** 3 - 1)
    assert rc == -7 and size == n and "too small" in detail and np.all(out == -7.0)  # RTM_ERR_CAPACITY: nothing is written


ROWS8 = "0 0 0\n1 0 0\n0 1 0\n1 1 0\n0 0 1\n1 0 1\n0 1 1\n1 1 1\n"
BAD_CUBES = [
    ("an unknown keyword", "LUT_3D_SIZE 2\nLUT_3D_FOO 1\n" + ROWS8, -4, 2),
    ("a size under 2", "LUT_3D_SIZE 1\n0 0 0\n", -4, 1),
    ("a size over 256", "# c\n\nLUT_3D_SIZE 257\n", -4, 3),
    ("a size that is no whole number", "LUT_3D_SIZE 2.5\n" + ROWS8, -4, 1),
    ("a size given twice", "LUT_3D_SIZE 2\nTITLE \"t\"\nLUT_3D_SIZE 2\n" + ROWS8, -4, 3),
    ("too few rows", "LUT_3D_SIZE 2\n0 0 0\n1 0 0\n", -4, 3),
    ("too many rows", "LUT_3D_SIZE 2\n" + ROWS8 + "0 0 0\n", -4, 10),
    ("a non-number", "LUT_3D_SIZE 2\n0 0 0\n1 zero 0\n", -4, 3),
    ("a NaN", "LUT_3D_SIZE 2\n0 nan 0\n", -4, 2),
    ("an infinity", "LUT_3D_SIZE 2\r\n0 0 0\r\n0 0 inf\r\n", -4, 3),
    ("a number past float's range", "LUT_3D_SIZE 2\n0 0 1e39\n", -4, 2),
    ("two numbers in a row", "LUT_3D_SIZE 2\n0 0\n", -4, 2),
    ("four numbers in a row", "LUT_3D_SIZE 2\n0 0 0 0\n", -4, 2),
    ("max <= min", "LUT_3D_SIZE 2\nDOMAIN_MIN 0 0 0\nDOMAIN_MAX 1 0 1\n" + ROWS8, -4, 3),
    ("max <= min by the range", "LUT_3D_INPUT_RANGE 1 1\nLUT_3D_SIZE 2\n" + ROWS8, -4, 1),
    ("a domain that is not finite", "LUT_3D_SIZE 2\nDOMAIN_MAX 1 inf 1\n" + ROWS8, -4, 2),
    ("data before the size", "0 0 0\nLUT_3D_SIZE 2\n" + ROWS8, -4, 1),
    ("a keyword inside the table", "LUT_3D_SIZE 2\n0 0 0\nDOMAIN_MIN 0 0 0\n", -4, 3),
    ("no size", "# nothing\nTITLE \"x\"\n", -4, 2),
    ("a 1D LUT", "TITLE \"t\"\nLUT_1D_SIZE 16\n", -8, 2),
]


@pytest.mark.parametrize("name,text,status,line", BAD_CUBES, ids=[c[0] for c in BAD_CUBES])
def test_cube_refusals_name_the_line(tmp_path, name, text, status, line):
    import raytracingmin_amd as rtm
    rc, detail, *_ = _parse(text)
    assert rc == status and detail.startswith(f"line {line}: "), (name, rc, detail)
    rc, detail, *_ = _parse(text, 24)  # with a table too: the same refusal
    assert rc == status and detail.startswith(f"line {line}: "), (name, rc, detail)
    path = tmp_path / "bad.cube"
    path.write_bytes(text.encode("ascii"))
    with pytest.raises(rtm.RtmError, match=f"line {line}: ") as e:
        rtm.load_cube(str(path))
    assert e.value.status == status


def test_cube_io_and_null_arguments(tmp_path):
    import raytracingmin_amd as rtm
    from raytracingmin_amd import _lib
    L = _lib.lib()
    with pytest.raises(rtm.RtmError) as e:
        rtm.load_cube(str(tmp_path / "missing.cube"))
    assert e.value.status == -3 and "cannot open" in str(e.value)  # RTM_ERR_IO
    n = C.c_int32()
    lo, hi = (C.c_float * 3)(), (C.c_float * 3)()
    assert L.rtm_lut_load_cube(None, C.byref(n), lo, hi, None, 0) == -1
    assert L.rtm_lut_parse_cube(None, 5, C.byref(n), lo, hi, None, 0) == -1
    assert L.rtm_lut_parse_cube(b"x", 1, None, lo, hi, None, 0) == -1
    assert L.rtm_lut_parse_cube(b"x", 1, C.byref(n), None, hi, None, 0) == -1
    assert L.rtm_lut_parse_cube(b"x", 1, C.byref(n), lo, None, None, 0) == -1
    assert L.rtm_lut_parse_cube(b"x", 1, C.byref(n), lo, hi, None, 3) == -1
    assert L.rtm_lut_parse_cube(None, 0, C.byref(n), lo, hi, None, 0) == -4  # an empty text has no size


def test_python_argument_errors_raise_before_any_device_use(tmp_path):
    import raytracingmin_amd as rtm
    color = np.zeros((4, 4, 3), np.float32)  # not even a tensor: a bad parameter comes first
    for kw in (dict(matrix=np.eye(2)), dict(matrix=[1, 2, 3]), dict(matrix=np.full((3, 3), NAN)), dict(matrix="identity"),
               dict(exposure=33), dict(exposure=NAN), dict(exposure="1"), dict(exposure=True), dict(contrast=0.2), dict(contrast=5),
               dict(pivot=0), dict(pivot=-1), dict(pivot=INF), dict(slope=-0.1), dict(slope=(1, 1)), dict(slope=(1, NAN, 1)),
               dict(slope="1"), dict(offset=INF), dict(offset=(0, 0, 0, 0)), dict(power=0.05), dict(power=(1, 11, 1)), dict(power=NAN),
               dict(saturation=-0.1), dict(saturation=4.5), dict(interp="cubic"), dict(interp=1), dict(lut=np.zeros((2, 2, 2, 3), np.float32)),
               dict(lut_domain=((0, 0, 0), (0, 1, 1))), dict(lut_domain=(0, 1, 2)), dict(lut_domain=((0,) * 3, (INF,) * 3)),
               dict(want=()), dict(want=("f64",))):
        with pytest.raises(ValueError):
            rtm.grade(color, **kw)
    data = rtm.LoadData(SCENE).data
    data.width, data.height = 16, 12
    good = tmp_path / "good.cube"
    _grade_ref.write_cube(good, _grade_ref.identity_table(2))
    bad = tmp_path / "bad.cube"
    bad.write_text("LUT_3D_SIZE 2\n0 0 0\n")
    for kw in (dict(grade="warm"), dict(grade=1.5), dict(grade=dict(gamma=2.2)), dict(grade=dict(contrast=9)), dict(grade=dict(tint=0.01)),
               dict(grade=dict(temperature=500)), dict(grade=dict(temperature=5000, matrix=np.eye(3))), dict(grade=dict(temperature=5000, tint=1)),
               dict(lut=3), dict(lut=dict(size=2)), dict(lut=dict(table=np.zeros((2, 2, 2, 3)))), dict(lut=dict(table=np.zeros((2, 3, 2, 3), np.float32))),
               dict(lut=dict(table=np.zeros((2, 2, 2, 3), np.float32), size=3)), dict(lut=dict(table=np.zeros((2, 2, 2, 3), np.float32), interp="x")),
               dict(lut=dict(table=np.zeros((2, 2, 2, 3), np.float32), domain_min=(0, 0, 0), domain_max=(1, 0, 1))),
               dict(lut=dict(table=np.zeros((2, 2, 2, 3), np.float32), title="x"))):
        with pytest.raises(ValueError):
            rtm.Renderer(data).Render("unused", tonemap=True, **kw)
        with pytest.raises(ValueError):
            rtm.Renderer(data).write_display("unused", **kw)
        assert not os.path.exists("unused.bmp") and not os.path.exists("unused_display.bmp")
    for kw in (dict(lut=str(bad)), dict(lut=str(tmp_path / "missing.cube"))):  # a file that does not load: before anything is rendered
        with pytest.raises(rtm.RtmError):
            rtm.Renderer(data).Render("unused", tonemap=True, **kw)
        assert not os.path.exists("unused.bmp")
    for kw in (dict(grade=dict(exposure=1)), dict(lut=str(good))):  # both act inside the display path
        with pytest.raises(ValueError, match="tonemap"):
            rtm.Renderer(data).Render("unused", **kw)
        assert not os.path.exists("unused.bmp")


REFUSALS = [
    (["--grade-exposure", "1"], "requires --display"),
    (["--grade-temperature", "3200"], "requires --display"),
    (["--grade-saturation", "0.5", "--pfm"], "requires --display"),
    (["--lut", "look.cube"], "requires --display"),
    (["--display", "--lut-interp", "trilinear"], "--lut-interp requires --lut"),
    (["--display", "--grade-tint", "0.01"], "requires --grade-temperature"),
    (["--display", "--grade-exposure", "1", "--gpus", "2"], "one GPU"),
    (["--display", "--lut", "look.cube", "--virtual-strips", "2"], "one GPU"),
    (["--display", "--grade-contrast", "1.2", "--force-rccl"], "one GPU"),
    (["--display", "--grade-temperature", "1000"], "--grade-temperature takes"),
    (["--display", "--grade-temperature", "warm"], "--grade-temperature takes"),
    (["--display", "--grade-temperature"], "--grade-temperature takes"),
    (["--display", "--grade-temperature", "5000", "--grade-tint", "0.06"], "--grade-tint takes"),
    (["--display", "--grade-exposure", "33"], "--grade-exposure takes"),
    (["--display", "--grade-exposure", "nan"], "--grade-exposure takes"),
    (["--display", "--grade-contrast", "5"], "--grade-contrast takes"),
    (["--display", "--grade-contrast", "1.2,0"], "--grade-contrast takes"),
    (["--display", "--grade-contrast", "1.2,0.18,1"], "--grade-contrast takes"),
    (["--display", "--grade-slope", "1,2"], "--grade-slope takes"),
    (["--display", "--grade-slope", "-1"], "--grade-slope takes"),
    (["--display", "--grade-slope", "1,1,1,1"], "--grade-slope takes"),
    (["--display", "--grade-offset", "inf"], "--grade-offset takes"),
    (["--display", "--grade-offset", "0,,0"], "--grade-offset takes"),
    (["--display", "--grade-power", "0.05"], "--grade-power takes"),
    (["--display", "--grade-power", "1,11,1"], "--grade-power takes"),
    (["--display", "--grade-saturation", "4.5"], "--grade-saturation takes"),
    (["--display", "--grade-saturation", "1,1,1"], "--grade-saturation takes"),
    (["--display", "--grade-gamma", "2.2"], "unknown option --grade-gamma"),
    (["--display", "--lut", "look.cube", "--lut-interp", "cubic"], "--lut-interp takes"),
]


@pytest.mark.parametrize("flags,word", REFUSALS, ids=[" ".join(f) for f, _ in REFUSALS])
def test_cli_refuses_before_any_gpu(tmp_path, flags, word):
    r = subprocess.run([CLI, "-json", SCENE, "--width", "8", "--height", "8", "--out", "x"] + flags, cwd=tmp_path,
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 2, (flags, r.stdout, r.stderr)
    assert word in r.stderr and ("--grade-" in r.stderr or "--lut" in r.stderr) and len(r.stderr.strip().splitlines()) == 1, (flags, r.stderr)
    assert not (tmp_path / "x.bmp").exists() and not (tmp_path / "x_display.bmp").exists()


def test_cli_refuses_a_cube_that_does_not_load_before_it_renders(tmp_path):
    bad = tmp_path / "bad.cube"
    bad.write_text("LUT_3D_SIZE 2\n0 0 0\n1 1 x\n")
    for path, word in ((bad, "line 3: "), (tmp_path / "missing.cube", "cannot open")):
        r = subprocess.run([CLI, "-json", SCENE, "--width", "8", "--height", "8", "--out", "x", "--display", "--lut", str(path)], cwd=tmp_path,
                           capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "--lut" in r.stderr and word in r.stderr, (r.stdout, r.stderr)
        assert not (tmp_path / "x.bmp").exists() and not (tmp_path / "x_display.bmp").exists()


def test_cli_usage_mentions_grade():
    r = subprocess.run([CLI, "-?"], capture_output=True, text=True, timeout=60)
    words = ("--grade-temperature K", "--grade-tint T", "--grade-exposure EV", "--grade-contrast C[,PIVOT]", "--grade-slope R,G,B|S",
             "--grade-offset R,G,B|S", "--grade-power R,G,B|S", "--grade-saturation S", "--lut FILE.cube", "--lut-interp trilinear|tetrahedral")
    for word in words:
        assert word in r.stdout + r.stderr, word
    head = open(os.path.join(ROOT, "raytracingmin_amd", "csrc", "rtm_main.cpp")).read().split("#include", 1)[0]
    for word in words:
        assert "[" + word + "]" in head, word


# ---- the margin condition on the GPU test's inputs, and the restatement itself ----------------------------------------
def test_the_gpu_cases_leave_float32_a_margin():
    """Every case of test_grade_gpu's comparison, on its largest frame: the float32 NumPy evaluation within 2e-5 max(1, |ref|) of
    the float64 one.  A case that fails this is a badly chosen input, not a kernel bug."""
    w, h = _grade_ref.SIZES[-1]
    frame = _resize_ref.frame(w, h)
    worst = {}
    for name, kw in _grade_ref.gpu_cases():
        ref = _grade_ref.grade_ref(frame, **kw)
        f32 = _grade_ref.grade_ref(frame, dtype=np.float32, **kw)
        assert f32.dtype == np.float32 and np.all(np.isfinite(ref))
        worst[name] = _grade_ref.tolerance_excess(f32, ref)
    top = max(worst, key=worst.get)
    print(f"{len(worst)} cases, worst float32 margin {worst[top]:.3e} ({top}), bar {MARGIN}")
    assert worst[top] <= MARGIN, (top, worst[top])
    assert len(worst) == 7 + 4 * 2 * 2 * 3 + 2


def test_the_restatement_itself():
    frame = _resize_ref.frame(67, 35)
    # the defaults change nothing; saturation 0 makes every pixel grey; an affine table is reproduced by both interpolants
    assert np.array_equal(_grade_ref.grade_ref(frame), frame.astype(np.float64))
    grey = _grade_ref.grade_ref(frame, saturation=0)
    assert np.array_equal(grey[..., 0], grey[..., 1]) and np.array_equal(grey[..., 1], grey[..., 2])
    for n in (2, 3, 17):
        for dom in (((0, 0, 0), (1, 1, 1)), ((-0.25,) * 3, (4,) * 3)):
            clipped = np.clip(frame.astype(np.float64), dom[0][0], dom[1][0])
            for interp in _grade_ref.INTERPS:
                out = _grade_ref.grade_ref(frame, lut=_grade_ref.affine_table(n, dom), lut_domain=dom, interp=interp)
                assert _grade_ref.tolerance_excess(out, _grade_ref.affine_of(clipped)) <= 1e-6, (n, dom, interp)
                out = _grade_ref.grade_ref(frame, lut=_grade_ref.identity_table(n, dom), lut_domain=dom, interp=interp)
                assert _grade_ref.tolerance_excess(out, clipped) <= 1e-6, (n, dom, interp)
    # the index arithmetic on the values where it can go wrong
    for n in (2, 3, 17, 256):
        for dt in (np.float32, np.float64):
            s = np.array([0.0, -0.0, 1e-45, n - 1, np.nextafter(dt(n - 1), dt(0)), np.nextafter(dt(n - 1), dt(1e9)), 3.4e38, -3.4e38, INF,
                          -INF, NAN, 0.5, n - 2, n - 1.5], dtype=dt)
            i, f = _grade_ref.lut_index(s, n)
            assert np.all((i >= 0) & (i <= n - 2) & (f >= 0) & (f <= 1)), (n, dt)
    # a tie takes the earlier channel first: with f_r == f_g the path goes r, then g
    t = np.zeros((2, 2, 2, 3), np.float32)
    t[0, 0, 1] = 1.0   # (r=1, g=0, b=0)
    t[0, 1, 0] = 5.0   # (r=0, g=1, b=0)
    t[0, 1, 1] = 2.0
    t[1, 1, 1] = 3.0
    out = _grade_ref.grade_ref(np.float32([[[0.5, 0.5, 0.25]]]), lut=t)
    assert np.allclose(out, 0.5 * 0 + 0.0 * 1.0 + 0.25 * 2.0 + 0.25 * 3.0)
