"""The coverage AOVs (rtm_render_mattes, rtm_matte, rtm_composite, rtm_debug_matte_rank), the parts that need no GPU: the
NumPy restatement on hand-made lists, the bindings and struct layouts, every refusal of the four entry points (all made before
any device call, with fake device pointers), the Python entry points' argument errors and the CLI's usage and refusals."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import _matte_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "raytracingmin_amd", "rtm_cli")
SCENE = os.path.join(ROOT, "scenes", "cornellBoxSetting.json")


def _header(name="rtm.h"):
    return open(os.path.join(ROOT, "include", name)).read()


# ---- the restatement on hand-made lists ---------------------------------------------------------------------------------
def test_rank_all_misses_and_one_id():
    i, c, a = _matte_ref.rank([[-1] * 16, [5] * 16], 4)
    assert i[:, 0].tolist() == [-1, -1, -1, -1] and (c[:, 0].view(np.uint32) == 0).all() and a[0] == 0.0 and not np.signbit(a[0])
    assert i[:, 1].tolist() == [5, -1, -1, -1] and c[:, 1].tolist() == [1.0, 0.0, 0.0, 0.0] and a[1] == 1.0
    i, c, a = _matte_ref.rank([[-1, 5, -7, 5]], 4)  # any negative id is a miss
    assert i[:, 0].tolist() == [5, -1, -1, -1] and c[0, 0] == 0.5 and a[0] == 0.5


def test_rank_a_tie_resolves_to_the_lower_id_whatever_is_seen_first():
    high_first = [9] * 32 + [3] * 32
    mixed = [9, 3] * 32
    for ids in (high_first, mixed, high_first[::-1]):
        i, c, a = _matte_ref.rank([ids], 2)
        assert i[:, 0].tolist() == [3, 9] and c[:, 0].tolist() == [0.5, 0.5] and a[0] == 1.0


def test_rank_64_distinct_ids_keeps_the_eight_lowest():
    ids = list(range(1063, 999, -1))  # descending: 64 distinct ids, each once
    i, c, a = _matte_ref.rank([ids], 8)
    assert i[:, 0].tolist() == list(range(1000, 1008))
    assert np.all(c[:, 0] == np.float32(1 / 64)) and a[0] == 1.0
    assert np.float32(a[0]) - c[:, 0].astype(np.float64).sum() == 56 / 64  # what truncation dropped


def test_rank_ninths_are_rounded_from_double():
    ids = [4, 4, 4, 4, 2, 2, 2, -1, -1]  # SS = 3
    i, c, a = _matte_ref.rank([ids], 3)
    assert i[:, 0].tolist() == [4, 2, -1]
    assert c[0, 0] == np.float32(4.0 / 9.0) and c[1, 0] == np.float32(3.0 / 9.0) and a[0] == np.float32(7.0 / 9.0)
    assert c[2, 0].view(np.uint32) == 0


def test_matte_sums_selected_layers_and_clamps_at_one():
    lid = np.array([[[1, 1]], [[2, 2]], [[-1, 3]]], np.int32)  # (3 layers, 1, 2)
    cov = np.array([[[0.75, 0.75]], [[0.5, 0.25]], [[0.0, 0.25]]], np.float32)
    assert _matte_ref.matte(lid, cov, [1]).tolist() == [[0.75, 0.75]]
    assert _matte_ref.matte(lid, cov, [2, 1]).tolist() == [[1.0, 1.0]]  # 1.25 clamps, 1.0 stays
    assert _matte_ref.matte(lid, cov, [3, 3, 7]).tolist() == [[0.0, 0.25]]
    assert _matte_ref.matte(lid, cov, [-1]).tolist() == [[0.0, 0.0]]  # a negative entry selects nothing, not the empty layers
    assert _matte_ref.matte(lid, cov, [-1]).view(np.uint32).max() == 0


def test_composite_alpha_one_is_the_colour_and_alpha_zero_adds_the_background():
    rng = np.random.default_rng(5)
    color = rng.random((3, 4, 3), dtype=np.float32)
    bg = (0.25, 0.5, 2.0)
    f, u = _matte_ref.composite(color, np.ones((3, 4), np.float32), bg)
    assert np.array_equal(f.view(np.uint32), color.view(np.uint32)) and np.array_equal(u, _matte_ref.quantise(color))
    f, _ = _matte_ref.composite(color, np.zeros((3, 4), np.float32), bg)
    assert np.array_equal(f, color + np.asarray(bg, np.float32))
    image = np.broadcast_to(np.asarray(bg, np.float32), color.shape).copy()
    alpha = rng.random((3, 4), dtype=np.float32)
    assert np.array_equal(_matte_ref.composite(color, alpha, image)[0], _matte_ref.composite(color, alpha, bg)[0])
    assert _matte_ref.quantise(np.array([0.0, 0.5, 1.0, 1.5, -0.1, np.nan], np.float32)).tolist() == [0, 127, 255, 255, 0, 0]


# ---- the library without a device ---------------------------------------------------------------------------------------
def test_the_entry_points_are_bound_exported_and_match_the_headers():
    import raytracingmin_amd as rtm
    from raytracingmin_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    header = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    debug = re.sub(r"/\*.*?\*/", "", _header("rtm_debug.h"), flags=re.S)
    for name in ("rtm_render_mattes", "rtm_matte", "rtm_composite"):
        assert name in _lib.SIGNATURES and hasattr(raw, name), name
        assert re.search(r"\b%s\s*\(" % name, header), name
    assert "rtm_debug_matte_rank" in _lib.DEBUG_SIGNATURES and hasattr(raw, "rtm_debug_matte_rank")
    assert re.search(r"\brtm_debug_matte_rank\s*\(", debug)
    ctype = {"int32_t*": C.c_void_p, "float*": C.c_void_p, "float": C.c_float}
    for name, cls, size in (("rtm_matte_buffers", _lib.rtm_matte_buffers, 24), ("rtm_composite_params", _lib.rtm_composite_params, 12)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, flags=re.S).group(1)
        declared = []
        for decl in body.split(";"):
            if decl.strip():
                ty, field = decl.split()
                arr = re.fullmatch(r"(\w+)\[(\d+)\]", field)
                declared.append((arr.group(1), ctype[ty] * int(arr.group(2))) if arr else (field, ctype[ty]))
        assert [f[0] for f in cls._fields_] == [d[0] for d in declared], name
        assert [C.sizeof(f[1]) for f in cls._fields_] == [C.sizeof(d[1]) for d in declared], name
        assert C.sizeof(cls) == size, name
    # the argument counts of the ctypes signatures are the headers'
    for name, text in (("rtm_render_mattes", header), ("rtm_matte", header), ("rtm_composite", header), ("rtm_debug_matte_rank", debug)):
        args = re.search(r"\b%s\s*\((.*?)\);" % name, text, flags=re.S).group(1)
        sig = {**_lib.SIGNATURES, **_lib.DEBUG_SIGNATURES}[name]
        assert len(args.split(",")) == len(sig[1]) and sig[0] is C.c_int, name
    # one default, in the header, the package and the restatement
    layers = int(re.search(r"#define RTM_MATTE_DEFAULT_LAYERS (\d+)", header).group(1))
    assert rtm.MATTE_DEFAULTS == _matte_ref.DEFAULTS == {"layers": layers} == {"layers": 4}
    for name in ("matte", "composite", "MATTE_DEFAULTS"):
        assert name in rtm.__all__ and hasattr(rtm, name), name
    p = inspect.signature(rtm.Renderer.render_mattes).parameters
    assert list(p)[:5] == ["self", "layers", "row_begin", "row_end", "band"] and p["layers"].default == layers
    assert p["want"].default == ("id", "coverage", "alpha") and p["stream"].default is None
    assert inspect.signature(rtm.Renderer.write_mattes).parameters["layers"].default == layers
    p = inspect.signature(rtm.composite).parameters
    assert p["background"].default == (0, 0, 0) and p["want"].default == ("f32",) and p["stream"].default is None
    assert list(inspect.signature(rtm.matte).parameters) == ["layer_id", "layer_coverage", "ids", "stream"]
    assert inspect.signature(rtm.Renderer.Render).parameters["mattes"].default is None
    assert _lib.lib().rtm_abi_version() == 5 and "#define RTM_ABI_VERSION 5" in _header()  # added without a bump


def _settings(w=16, h=8, ss=2):
    from raytracingmin_amd import _lib
    st = _lib.rtm_settings()
    st.width, st.height, st.samples, st.super_samples = w, h, 1, ss
    return st


def _options(h=8, **kw):
    from raytracingmin_amd import _lib
    opt = _lib.rtm_options()
    opt.mode, opt.row_begin, opt.row_end = 1, 0, h
    for k, v in kw.items():
        setattr(opt, k, v)
    return opt


def test_render_mattes_refusals_come_before_the_scene_is_looked_at():
    from raytracingmin_amd import _lib
    L = _lib.lib()
    planes = _lib.rtm_matte_buffers(0x1000, 0x20000, 0x300000)  # fake device pointers: never dereferenced

    def call(st=_settings(), opt=_options(), layers=4, out=planes):
        ref = lambda v: None if v is None else C.byref(v)
        return L.rtm_render_mattes(ref(st), None, ref(opt), layers, ref(out), None)  # a null scene throughout

    for layers in (0, 9, -1, 1 << 20):
        assert call(layers=layers) == -1, layers
        assert b"layers" in L.rtm_last_error_detail()
    assert call(out=_lib.rtm_matte_buffers()) == -1
    assert b"plane" in L.rtm_last_error_detail()
    assert call(st=None) == -1 and call(opt=None) == -1 and call(out=None) == -1
    assert call(opt=_options(row_end=9)) == -1 and call(opt=_options(row_begin=5, row_end=3)) == -1
    assert b"row" in L.rtm_last_error_detail()
    assert call(opt=_options(band_count=3, band_index=3)) == -1 and call(opt=_options(band_count=-1)) == -1
    assert b"band" in L.rtm_last_error_detail()
    assert call(opt=_options(mode=7)) == -1
    assert b"mode" in L.rtm_last_error_detail()
    assert call(st=_settings(ss=9)) == -8
    assert b"superSamples" in L.rtm_last_error_detail() and L.rtm_strerror(-8) == b"unsupported"
    assert call(st=_settings(ss=9), layers=9) == -1  # an argument error wins
    # everything in order: only then the null scene is the complaint, for every plane set and both ends of both ranges
    for kw in (dict(), dict(layers=1), dict(layers=8), dict(st=_settings(ss=8)), dict(st=_settings(ss=1)),
               dict(out=_lib.rtm_matte_buffers(None, None, 0x1000)), dict(out=_lib.rtm_matte_buffers(0x1000, None, None))):
        assert call(**kw) == -1, kw
        assert b"scene" in L.rtm_last_error_detail(), kw


def test_matte_rank_hook_refusals():
    from raytracingmin_amd import _lib
    L = _lib.lib()
    ids, oid, cov, alpha = 0x1000, 0x20000, 0x300000, 0x4000000

    def call(ss=2, layers=4, dev=0, i=ids, n=64, a=oid, b=cov, c=alpha):
        return L.rtm_debug_matte_rank(ss, layers, dev, i, n, a, b, c, None)

    for layers in (0, 9, -3):
        assert call(layers=layers) == -1, layers
    assert call(ss=0) == -1 and call(ss=-2) == -1
    assert call(i=None) == -1 and call(a=None, b=None, c=None) == -1
    for kw in (dict(i=ids + 2), dict(a=oid + 1), dict(b=cov + 3), dict(c=alpha + 2)):
        assert call(**kw) == -1, kw
        assert b"aligned" in L.rtm_last_error_detail()
    assert call(dev=-1) == -1
    assert b"device" in L.rtm_last_error_detail()
    assert call(ss=9) == -8 and call(ss=9, layers=0) == -1
    assert call(n=0) == 0  # nothing to rank: nothing is enqueued
    for kw in (dict(a=None), dict(b=None, c=None), dict(ss=8, layers=8), dict(ss=1, layers=1)):  # allowed: refused for the device alone
        assert call(dev=-1, **kw) == -1, kw
        assert b"device" in L.rtm_last_error_detail(), kw


def test_matte_refusals():
    from raytracingmin_amd import _lib
    L = _lib.lib()
    lid, cov, sel, out = 0x1000, 0x20000, 0x300000, 0x4000000

    def call(w=8, h=8, layers=4, dev=0, a=lid, b=cov, s=sel, n=3, o=out):
        return L.rtm_matte(w, h, layers, dev, a, b, s, n, o, None)

    for layers in (0, 9, -1):
        assert call(layers=layers) == -1, layers
        assert b"layers" in L.rtm_last_error_detail()
    for n in (0, 65, -1):
        assert call(n=n) == -1, n
        assert b"n_ids" in L.rtm_last_error_detail()
    for kw in (dict(a=None), dict(b=None), dict(s=None), dict(o=None)):
        assert call(**kw) == -1, kw
        assert b"null" in L.rtm_last_error_detail()
    for w, h in ((0, 8), (8, 0), (-1, 8), (8, -3)):
        assert call(w=w, h=h) == -1, (w, h)
    for kw in (dict(a=lid + 1), dict(b=cov + 2), dict(s=sel + 3), dict(o=out + 2)):
        assert call(**kw) == -1, kw
        assert b"aligned" in L.rtm_last_error_detail()
    for kw in (dict(o=lid), dict(o=cov), dict(o=sel)):
        assert call(**kw) == -1, kw
        assert b"input" in L.rtm_last_error_detail()
    assert call(dev=-1) == -1
    assert b"device" in L.rtm_last_error_detail()
    for kw in (dict(layers=1, n=1), dict(layers=8, n=64), dict(b=lid)):  # allowed: refused for the device alone
        assert call(dev=-1, **kw) == -1, kw
        assert b"device" in L.rtm_last_error_detail(), kw
    assert call(w=2**16, h=2**15) == -8


def test_composite_refusals():
    from raytracingmin_amd import _lib
    L = _lib.lib()
    color, alpha, bg, o32, o8 = 0x1000, 0x20000, 0x300000, 0x4000000, 0x50000001  # (the u8 output needs no alignment)

    def call(p=(0.0, 0.5, 1.0), w=8, h=8, dev=0, c=color, a=alpha, b=bg, f=o32, u=o8):
        prm = None if p is None else C.byref(_lib.rtm_composite_params((C.c_float * 3)(*p)))
        return L.rtm_composite(prm, w, h, dev, c, a, b, f, u, None)

    assert call(p=None) == -1 and call(c=None) == -1 and call(a=None) == -1
    assert b"null" in L.rtm_last_error_detail()
    assert call(f=None, u=None) == -1
    assert b"output" in L.rtm_last_error_detail()
    for v in (float("nan"), float("inf"), float("-inf")):
        for k in range(3):
            p = [0.0, 0.0, 0.0]
            p[k] = v
            assert call(p=p) == -1 and call(p=p, b=None) == -1, (v, k)
            assert b"background" in L.rtm_last_error_detail()
    for w, h in ((0, 8), (8, 0), (-1, 8), (8, -3)):
        assert call(w=w, h=h) == -1, (w, h)
    for kw in (dict(c=color + 1), dict(a=alpha + 2), dict(b=bg + 3), dict(f=o32 + 2)):
        assert call(**kw) == -1, kw
        assert b"aligned" in L.rtm_last_error_detail()
    for kw in (dict(f=alpha), dict(u=alpha), dict(f=bg), dict(u=bg)):
        assert call(**kw) == -1, kw
        assert b"alpha_dev or background_dev" in L.rtm_last_error_detail()
    assert call(dev=-1) == -1
    assert b"device" in L.rtm_last_error_detail()
    # allowed: in place, one output, no background image — refused for the device alone
    for kw in (dict(f=color), dict(f=None), dict(u=None), dict(b=None), dict(b=None, f=color, u=None)):
        assert call(dev=-1, **kw) == -1, kw
        assert b"device" in L.rtm_last_error_detail(), kw
    assert call(w=2**16, h=2**15) == -8
    assert L.rtm_strerror(-8) == b"unsupported"


# ---- Python and the CLI -------------------------------------------------------------------------------------------------
def test_python_argument_errors_raise_before_any_device_use(tmp_path):
    import raytracingmin_amd as rtm
    data = rtm.LoadData(SCENE).data
    data.width, data.height, data.samples, data.superSamples = 8, 8, 1, 1
    r = rtm.Renderer(data)
    for layers in (0, 9, -1, 2.5, "4", None, True):
        with pytest.raises(ValueError):
            r.render_mattes(layers=layers)
        with pytest.raises(ValueError):
            r.write_mattes(str(tmp_path / "x"), layers=layers)
    for want in ((), ("alpha", "depth"), ("ids",)):
        with pytest.raises(ValueError):
            r.render_mattes(want=want)
    lid, cov = np.zeros((2, 4, 5), np.int32), np.zeros((2, 4, 5), np.float32)  # not even tensors
    for ids in ([], list(range(65)), [1.5], ["a"], [2**31], 7, None, [True]):
        with pytest.raises(ValueError):
            rtm.matte(lid, cov, ids)
        if ids is not None:  # (write_mattes' None: no matte is asked for)
            with pytest.raises(ValueError):
                r.write_mattes(str(tmp_path / "x"), ids=ids)
    with pytest.raises(ValueError):
        rtm.matte(lid, cov, [1, 2])  # the lists are fine; the layers are no CUDA tensors
    color, alpha = np.zeros((4, 5, 3), np.float32), np.zeros((4, 5), np.float32)
    for bg in ((0, 0), (0, 0, 0, 0), (0, float("nan"), 0), (float("inf"), 0, 0), "red", 3, None, ("a", "b", "c")):
        with pytest.raises(ValueError):
            rtm.composite(color, alpha, background=bg)
        if bg is not None:
            with pytest.raises(ValueError):
                r.write_mattes(str(tmp_path / "x"), background=bg)
    for want in ((), ("f64",), ("f32", "alpha")):
        with pytest.raises(ValueError):
            rtm.composite(color, alpha, want=want)
    with pytest.raises(ValueError):
        rtm.composite(color, alpha)  # no CUDA tensors
    for bad in (1, "yes", [4], dict(layer=4), dict(layers=0), dict(ids=[]), dict(background=(1, 2)), dict(ids=[0], layers=9)):
        with pytest.raises(ValueError):
            r.Render(str(tmp_path / "x"), mattes=bad)
    assert not list(tmp_path.iterdir())  # nothing was rendered or written


def test_cli_usage_lists_the_flags_and_refuses_before_any_gpu_use(tmp_path):
    r = subprocess.run([CLI, "-?"], capture_output=True, text=True, timeout=60)
    for word in ("--alpha", "--matte ID[,ID...]", "--matte-layers K", "--background R,G,B", "STEM_alpha.pfm", "STEM_matte.pfm",
                 "STEM_matte.bmp", "STEM_over.bmp", "STEM_over.jpg", "STEM_over_display.bmp", "--matte-layers requires", "--preview-only"):
        assert word in r.stdout + r.stderr, word
    args = [CLI, "-json", SCENE, "--width", "8", "--height", "8", "--out", "x"]
    run = lambda *flags: subprocess.run(args + list(flags), cwd=tmp_path, capture_output=True, text=True, timeout=60)
    for flags in (("--matte", "1,,2"), ("--matte", "a"), ("--matte", "1,2x"), ("--matte", ""), ("--matte", "1.5"), ("--matte",),
                  ("--matte", ",".join(str(i) for i in range(65))), ("--matte", "99999999999"),
                  ("--matte", "1", "--matte-layers", "0"), ("--matte", "1", "--matte-layers", "9"),
                  ("--matte", "1", "--matte-layers", "two"), ("--matte-layers", "4"),
                  ("--background", "1,2"), ("--background", "1,2,3,4"), ("--background", "0,nan,0"), ("--background", "red"),
                  ("--background", "1e60,0,0"), ("--background",),
                  ("--alpha", "--gpus", "2"), ("--matte", "1", "--virtual-strips", "2"), ("--background", "0,0,0", "--force-rccl"),
                  ("--alpha", "--preview", "2", "--preview-only"), ("--alpha", "--superSamples", "9"),
                  ("--background", "0,0,0", "--superSamples", "12")):
        p = run(*flags)
        assert p.returncode == 2 and p.stderr and not (tmp_path / "x.bmp").exists(), (flags, p.returncode, p.stderr)
