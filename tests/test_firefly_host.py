"""The firefly clamp, the parts that need no GPU: the bindings and the struct layout, rtm_firefly's argument checks (all made
before any device call), the Python entry points' argument errors, the CLI's refusals, and the properties include/rtm.h
states, shown on the NumPy reference."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import _firefly_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "raytracingmin_amd", "rtm_cli")
SCENE = os.path.join(ROOT, "scenes", "cornellBoxSetting.json")
FIELDS = ("radius", "rank", "k", "floor", "repair")
FRAMES = ((37, 23), (131, 63))


def _header():
    return open(os.path.join(ROOT, "include", "rtm.h")).read()


def _words(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_firefly_is_bound_and_exported_and_the_struct_matches_the_header():
    import raytracingmin_amd as rtm
    from raytracingmin_amd import _lib
    assert "rtm_firefly" in _lib.SIGNATURES
    assert hasattr(C.CDLL(_lib.LIB_PATH), "rtm_firefly")
    header = _header()
    ctype = {"int32_t": C.c_int32, "float": C.c_float}
    body = re.search(r"typedef struct rtm_firefly_params \{(.*?)\} rtm_firefly_params;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = []
    for decl in body.split(";"):
        if decl.strip():
            ty, names = decl.split(None, 1)
            declared += [(n.strip(), ctype[ty]) for n in names.split(",")]
    assert [(f[0], f[1]) for f in _lib.rtm_firefly_params._fields_] == declared
    assert tuple(f[0] for f in _lib.rtm_firefly_params._fields_) == FIELDS
    assert C.sizeof(_lib.rtm_firefly_params) == 20
    assert [getattr(_lib.rtm_firefly_params, f).offset for f in FIELDS] == [0, 4, 8, 12, 16]
    # the header, the package, the reference: one set of defaults
    macro = re.search(r"#define RTM_FIREFLY_DEFAULTS \{([^}]*)\}", header).group(1)
    values = [v.strip() for v in macro.split(",")]
    assert values == ["1", "3", "4.0f", "0.01f", "1"]
    from_header = {"radius": int(values[0]), "rank": int(values[1]), "k": float(values[2].rstrip("f")),
                   "floor": float(values[3].rstrip("f")), "repair": bool(int(values[4]))}
    assert rtm.FIREFLY_DEFAULTS == _lib.FIREFLY_DEFAULTS == _firefly_ref.DEFAULTS == from_header
    assert callable(rtm.firefly) and "firefly" in rtm.__all__ and "FIREFLY_DEFAULTS" in rtm.__all__
    params = inspect.signature(rtm.firefly).parameters
    assert list(params) == ["color", "radius", "rank", "k", "floor", "repair", "want", "stream"]
    assert {k: params[k].default for k in rtm.FIREFLY_DEFAULTS} == rtm.FIREFLY_DEFAULTS
    assert params["want"].default == ("f32",) and params["stream"].default is None
    assert inspect.signature(rtm.Renderer.Render).parameters["firefly"].default is None
    assert list(inspect.signature(rtm.Renderer.write_firefly).parameters)[:3] == ["self", "fileName", "frame"]
    assert _lib.lib().rtm_abi_version() == 5  # added without a bump
    assert re.search(r"#define RTM_ABI_VERSION 5\b", header)


def test_firefly_rejects_invalid_arguments_without_a_gpu():
    from raytracingmin_amd import _lib
    L = _lib.lib()
    good = (1, 3, 4.0, 0.01, 1)
    color, out32, out8, mask, thr = (C.c_void_p(0x1000), C.c_void_p(0x20000), C.c_void_p(0x300000), C.c_void_p(0x4000000),
                                     C.c_void_p(0x50000000))
    # fake device pointers: never dereferenced, every call below fails its checks first

    def call(p=good, w=8, h=8, dev=0, c=color, o32=out32, o8=out8, m=mask, t=thr):
        prm = None if p is None else C.byref(_lib.rtm_firefly_params(*p))
        return L.rtm_firefly(prm, w, h, dev, c, o32, o8, m, t, None)

    def with_(**kw):
        d = dict(zip(FIELDS, good))
        d.update(kw)
        return tuple(d[k] for k in FIELDS)

    def detail():
        return L.rtm_last_error_detail()

    assert call(p=None) == -1 and b"params" in detail()
    assert call(c=None) == -1 and b"color_dev" in detail()
    assert call(o32=None, o8=None, m=None, t=None) == -1 and b"output" in detail()
    for w, h in ((0, 8), (8, 0), (-1, 8), (8, -3)):
        assert call(w=w, h=h) == -1 and b"size" in detail(), (w, h)
    for v in (0, 4, -1, 1 << 30):
        assert call(p=with_(radius=v)) == -1 and b"radius" in detail(), v
    for v in (0, 9, -1, 1 << 30):
        assert call(p=with_(rank=v)) == -1 and b"rank" in detail(), v
    for v in (float("nan"), float("inf"), float("-inf"), 0.0, 0.5, -4.0, float(np.nextafter(np.float32(1), np.float32(0)))):
        assert call(p=with_(k=v)) == -1 and b"k is" in detail(), v
    for v in (float("nan"), float("inf"), float("-inf"), -1.0, -1e-30, -0.0):
        assert call(p=with_(floor=v)) == -1 and b"floor" in detail(), v
    for v in (2, -1, 1 << 20):
        assert call(p=with_(repair=v)) == -1 and b"repair" in detail(), v
    for name in ("c", "o32", "t"):  # a float pointer that is not 4-byte aligned
        for off in (1, 2, 3):
            assert call(**{name: C.c_void_p(0x600000 + off)}) == -1 and b"4-byte" in detail(), (name, off)
    for name in ("o32", "o8", "m", "t"):  # a gather cannot run in place
        assert call(**{name: color}) == -1 and b"color_dev" in detail() and b"in place" in detail(), name
    outs = {"o32": out32, "o8": out8, "m": mask, "t": thr}
    for a in outs:  # two outputs equal to each other
        for b in outs:
            if a < b:
                assert call(**{a: outs[b]}) == -1 and b"outputs alias" in detail(), (a, b)
    assert call(dev=-1) == -1 and b"device" in detail()
    # a frame of 2^31 pixels or more
    assert call(w=1 << 16, h=1 << 15) == -8  # RTM_ERR_UNSUPPORTED
    assert b"too large" in detail()
    # 2^23 tiles of 32 x 16 or more: a frame thinner than a tile reaches the launch's 2^32 lanes before 2^31 pixels
    for w, h in ((1, 1 << 27), (1 << 28, 1), (15, 1 << 27), (1 << 28, 7)):
        assert call(w=w, h=h) == -8 and b"too large" in detail() and b"tiles" in detail(), (w, h)
    # the limits themselves, single outputs and odd byte pointers pass every check: what refuses these is the device
    for kw in (dict(p=with_(radius=1, rank=1)), dict(p=with_(radius=3, rank=8)), dict(p=with_(k=1.0, floor=0.0)),
               dict(p=with_(k=3e38, floor=3e38)), dict(p=with_(repair=0)), dict(o32=None, o8=None, m=None),
               dict(o32=None, o8=None, t=None), dict(o8=None, m=None, t=None), dict(o32=None, m=None, t=None),
               dict(o8=C.c_void_p(0x4000001), m=C.c_void_p(0x4100003)), dict(w=(1 << 16) - 1, h=1 << 15), dict(w=1, h=1),
               dict(w=1, h=(1 << 27) - 16), dict(w=(1 << 28) - 32, h=1)):
        assert call(dev=-1, **kw) == -1, kw
        assert b"device" in detail(), kw


def test_python_argument_errors_raise_before_any_device_use():
    import raytracingmin_amd as rtm
    color = np.zeros((4, 4, 3), np.float32)  # not even a tensor: a bad parameter comes first
    bad_params = (dict(radius=0), dict(radius=4), dict(radius=1.0), dict(radius=True), dict(radius=None),
                  dict(rank=0), dict(rank=9), dict(rank=2.0), dict(rank=True), dict(rank="3"),
                  dict(k=0.5), dict(k=float("nan")), dict(k=float("inf")), dict(k=None), dict(k=True), dict(k=1e60), dict(k=-4),
                  dict(floor=-0.01), dict(floor=-0.0), dict(floor=float("nan")), dict(floor=float("inf")), dict(floor=None),
                  dict(floor=1e60), dict(repair=2), dict(repair=None), dict(repair="yes"), dict(repair=1.0))
    for kw in bad_params + (dict(want=()), dict(want=("f64",)), dict(want=("coc",))):
        with pytest.raises(ValueError):
            rtm.firefly(color, **kw)
    # the words rtm_cli uses at parse time
    for kw, words in ((dict(radius=4), "an integer in 1..3"), (dict(rank=9), "an integer in 1..8"),
                      (dict(k=0.5), "a finite number that is at least 1"),
                      (dict(floor=-1.0), "a finite number that is not negative (nor -0.0)")):
        with pytest.raises(ValueError, match=re.escape(words)):
            rtm.firefly(color, **kw)
    data = rtm.LoadData(SCENE).data
    data.width, data.height = 16, 12
    for bad in ("clamp", 1, 4.0, [1], dict(radii=3), dict(window=3)) + bad_params:
        with pytest.raises(ValueError):
            rtm.Renderer(data).Render("unused", firefly=bad)
        assert not os.path.exists("unused.bmp") and not os.path.exists("unused_firefly.bmp")
    for bad in bad_params:
        with pytest.raises(ValueError):
            rtm.Renderer(data).write_firefly("unused", **bad)
    assert not os.path.exists("unused_firefly.bmp")


REFUSALS = [
    (["--firefly", "--gpus", "2"], "--firefly runs on one GPU"),
    (["--firefly", "--virtual-strips", "2"], "--firefly runs on one GPU"),
    (["--firefly", "--force-rccl"], "--firefly runs on one GPU"),
    (["--firefly", "--preview", "2", "--preview-only"], "--preview-only skips the full render: it does not combine with --firefly"),
    (["--firefly-rank", "2"], "require --firefly"),
    (["--firefly-radius", "2"], "require --firefly"),
    (["--firefly-floor", "0.1"], "require --firefly"),
    (["--firefly-keep-nonfinite"], "require --firefly"),
    (["--firefly", "0.5"], "--firefly takes a finite number that is at least 1"),
    (["--firefly", "-4"], "--firefly takes a finite number that is at least 1"),
    (["--firefly", "nan"], "--firefly takes a finite number that is at least 1"),
    (["--firefly", "inf"], "--firefly takes a finite number that is at least 1"),
    (["--firefly", "1e60"], "--firefly takes a finite number that is at least 1"),
    (["--firefly", "--firefly-rank", "0"], "--firefly-rank takes an integer in 1..8"),
    (["--firefly", "--firefly-rank", "9"], "--firefly-rank takes an integer in 1..8"),
    (["--firefly", "--firefly-rank", "2.5"], "--firefly-rank takes an integer in 1..8"),
    (["--firefly", "--firefly-rank"], "--firefly-rank takes an integer in 1..8"),
    (["--firefly", "--firefly-radius", "0"], "--firefly-radius takes an integer in 1..3"),
    (["--firefly", "--firefly-radius", "4"], "--firefly-radius takes an integer in 1..3"),
    (["--firefly", "--firefly-radius", "x"], "--firefly-radius takes an integer in 1..3"),
    (["--firefly", "--firefly-floor", "-0.01"], "--firefly-floor takes a finite number that is not negative (nor -0.0)"),
    (["--firefly", "--firefly-floor", "-0.0"], "--firefly-floor takes a finite number that is not negative (nor -0.0)"),
    (["--firefly", "--firefly-floor", "inf"], "--firefly-floor takes a finite number that is not negative (nor -0.0)"),
    (["--firefly", "--firefly-floor"], "--firefly-floor takes a finite number that is not negative (nor -0.0)"),
]


@pytest.mark.parametrize("flags,word", REFUSALS, ids=[" ".join(f) for f, _ in REFUSALS])
def test_cli_refuses_before_any_gpu(tmp_path, flags, word):
    r = subprocess.run([CLI, "-json", SCENE, "--width", "8", "--height", "8", "--out", "x"] + flags, cwd=tmp_path,
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 2, (flags, r.stdout, r.stderr)
    assert word in r.stderr and len(r.stderr.strip().splitlines()) == 1, (flags, r.stderr)
    assert not (tmp_path / "x.bmp").exists() and not (tmp_path / "x_firefly.bmp").exists()


def test_cli_usage_mentions_firefly():
    r = subprocess.run([CLI, "-?"], capture_output=True, text=True, timeout=60)
    for word in ("--firefly [K]", "--firefly-rank N", "--firefly-radius R", "--firefly-floor F", "--firefly-keep-nonfinite",
                 "STEM_firefly.bmp"):
        assert word in r.stdout + r.stderr, word
    head = open(os.path.join(ROOT, "raytracingmin_amd", "csrc", "rtm_main.cpp")).read().split("#include", 1)[0]
    assert "[--firefly [K]] [--firefly-rank N] [--firefly-radius R] [--firefly-floor F] [--firefly-keep-nonfinite]" in head
    assert "--firefly" in open(os.path.join(ROOT, "README.md")).read()


# ---- the properties include/rtm.h states, on the NumPy reference ---------------------------------------------------------
def test_reference_frame_recipe():
    for w, h in FRAMES:
        color, marks = _firefly_ref.frame(w, h)
        blocks = len(_firefly_ref.block_origins(w, h))
        assert blocks == (1 if w < 64 else 2)
        assert marks["spikes"].sum() == 3 * blocks and marks["cluster2"].sum() == 2 * blocks and marks["cluster3"].sum() == 3 * blocks
        assert marks["block"].sum() == 4 * blocks and marks["rect"].sum() == 12 * blocks
        assert marks["line"].sum() == 8 * blocks and marks["line_inner"].sum() == 6 * blocks
        assert marks["nonfinite"].sum() == 4 * blocks + 1 and marks["nonfinite"][h - 1, w - 1] and marks["rect"][7, 0]
        assert np.array_equal(marks["nonfinite"], ~_firefly_ref.counts(color))
        y = _firefly_ref.luminance(color)
        assert len(np.unique(y[marks["ties"]])) == 4 and np.all(y[marks["zeros"]] == 0)
        assert np.any(y[marks["negative"]] == 0) and np.any(y[marks["negative"]] > 0) and np.all(color[marks["negative"]].min(axis=-1) < 0)
    for w, h in ((1, 1), (2, 1)):
        color, marks = _firefly_ref.frame(w, h)
        assert _firefly_ref.counts(color).all() and not any(m.any() for m in marks.values())
    for w, h in ((1, 9), (9, 1), (3, 3), (7, 5)):
        color, marks = _firefly_ref.frame(w, h)
        assert marks["spikes"].sum() == 1 and marks["nonfinite"][h - 1, w - 1]
        assert marks["nonfinite"].sum() == (3 if (w, h) == (7, 5) else 1)


def test_reference_constant_frame_keeps_its_words():
    for c in ((0.25, 3.0, 0.0), (0.0, 0.0, 0.0), (-1.0, 0.5, 2.0), (3e38, 3e38, 3e38)):
        for w, h in ((1, 1), (7, 5), (37, 23)):
            color = np.broadcast_to(np.float32(c), (h, w, 3)).copy()
            for radius, rank, k, floor in ((1, 3, 4.0, 0.01), (1, 1, 1.0, 0.0), (3, 8, 2.0, 0.5), (2, 1, 1.0, 0.0)):
                ref = _firefly_ref.firefly_ref(color, radius, rank, k, floor)
                assert not ref["mask"].any(), (c, w, h, radius, rank)
                assert np.array_equal(_words(ref["out"]), _words(color))


def test_reference_output_luminance_never_exceeds_the_input():
    for w, h in FRAMES:
        color, marks = _firefly_ref.frame(w, h)
        ok = ~marks["nonfinite"]
        for radius, rank, k, floor in ((1, 3, 4.0, 0.01), (1, 1, 1.0, 0.0), (2, 3, 4.0, 0.01), (3, 8, 2.0, 0.5), (3, 1, 1.5, 0.0)):
            ref = _firefly_ref.firefly_ref(color, radius, rank, k, floor)
            y_in = _firefly_ref.luminance(color).astype(np.float64)
            o = ref["out"]
            y_out = np.maximum(0.2126 * o[..., 0] + 0.7152 * o[..., 1] + 0.0722 * o[..., 2], 0.0)
            assert np.all(y_out[ok] <= y_in[ok] * (1 + 1e-6)), (w, h, radius, rank)
            clamped = ref["mask"] == 1
            assert clamped.any() and np.allclose(y_out[clamped], ref["threshold"][clamped], rtol=1e-5, atol=1e-7)
            unchanged = ref["mask"] == 0
            assert np.array_equal(_words(o)[unchanged & ok], _words(color)[unchanged & ok])


def test_reference_defaults_keep_rectangles_and_catch_clusters_and_spikes():
    for w, h in FRAMES:
        color, marks = _firefly_ref.frame(w, h)
        mask = _firefly_ref.firefly_ref(color)["mask"]
        assert not mask[marks["rect"]].any() and not mask[marks["block"]].any()  # a convex corner has three bright neighbours
        assert np.all(mask[marks["spikes"]] == 1) and np.all(mask[marks["cluster2"]] == 1) and np.all(mask[marks["cluster3"]] == 1)
        assert np.all(mask[marks["nonfinite"]] == 2)
        planted = np.zeros((h, w), bool)
        for m in marks.values():
            planted |= m
        assert not mask[~planted].any()  # the gradient and its noise are no fireflies
        # the line: clamped at rank 3; at rank 2 its inner pixels are kept (two bright neighbours) and its two ends go
        assert np.all(mask[marks["line"]] == 1)
        mask2 = _firefly_ref.firefly_ref(color, rank=2)["mask"]
        assert not mask2[marks["line_inner"]].any() and np.all(mask2[marks["line"] & ~marks["line_inner"]] == 1)
        assert np.all(mask2[marks["cluster3"]] == 0) and np.all(mask2[marks["cluster2"]] == 1)


def test_reference_pixels_with_fewer_neighbours_than_rank_are_unchanged():
    for w, h in ((1, 9), (9, 1), (1, 2), (2, 1), (1, 1)):
        color, marks = _firefly_ref.frame(w, h)
        for radius in (1, 2, 3):
            ref = _firefly_ref.firefly_ref(color, radius=radius, rank=2 * radius + 1)  # a row has 2 radius neighbours at most
            ok = ~marks["nonfinite"]
            assert not ref["mask"][ok].any() and np.all(np.isposinf(ref["threshold"])), (w, h, radius)
            assert np.array_equal(_words(ref["out"])[ok], _words(color)[ok])
    color, marks = _firefly_ref.frame(9, 1)
    assert _firefly_ref.firefly_ref(color, rank=2)["mask"][marks["spikes"]].all()  # rank 2: the spike has two neighbours


def test_reference_repair_on_and_off():
    for w, h in FRAMES + ((7, 5), (3, 3)):
        color, marks = _firefly_ref.frame(w, h)
        bad = marks["nonfinite"]
        for radius in (1, 2, 3):
            on = _firefly_ref.firefly_ref(color, radius=radius, repair=True)
            assert np.all(np.isfinite(on["out"])) and np.all(on["mask"][bad] == 2) and not np.any(on["mask"][~bad] == 2)
            off = _firefly_ref.firefly_ref(color, radius=radius, repair=False)
            assert not off["mask"][bad].any() and np.array_equal(_words(off["out"])[bad], _words(color)[bad])
            # the decisions of the pixels that count are the same either way
            assert np.array_equal(on["mask"][~bad], off["mask"][~bad])
            assert np.array_equal(on["threshold"].view(np.uint32), off["threshold"].view(np.uint32))
            assert np.all(np.isposinf(on["threshold"][bad]))
    # n = 0: a lone non-finite pixel, and one whose neighbours are all non-finite, become (+0, +0, +0)
    lone = np.full((1, 1, 3), np.nan, np.float32)
    out = _firefly_ref.firefly_ref(lone)
    assert out["mask"][0, 0] == 2 and np.all(_words(out["out"]) == 0)
    allbad = np.full((3, 3, 3), np.inf, np.float32)
    assert np.all(_words(_firefly_ref.firefly_ref(allbad)["out"]) == 0)
    # the mean is that of the counting taps alone: of an adjacent pair, each ignores the other
    color, marks = _firefly_ref.frame(37, 23)
    (xa, ya), (xb, yb) = _firefly_ref.NONFINITE[0][0], _firefly_ref.NONFINITE[1][0]
    assert abs(xa - xb) == 1 and ya == yb
    near = [color[ya + dy, xa + dx].astype(np.float64) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
            if (dy, dx) != (0, 0) and (xa + dx, ya + dy) != (xb, yb)]
    assert np.allclose(_firefly_ref.firefly_ref(color)["out"][ya, xa], np.mean(near, axis=0), rtol=1e-12)


def test_reference_a_nonfinite_pixel_only_leaves_its_neighbours_windows():
    for w, h in FRAMES:
        color, marks = _firefly_ref.frame(w, h)
        bad = marks["nonfinite"]
        for radius, rank in ((1, 3), (2, 3), (3, 8)):
            t = _firefly_ref.firefly_ref(color, radius=radius, rank=rank)["threshold"]
            # which non-finite value it holds does not matter
            other = color.copy()
            other[bad] = np.float32([-np.inf, np.nan, 1e30])
            t2 = _firefly_ref.firefly_ref(other, radius=radius, rank=rank)["threshold"]
            assert np.array_equal(t.view(np.uint32), t2.view(np.uint32))
            # and a pixel whose window holds none of them has the threshold of the frame with finite values in their place
            finite = color.copy()
            finite[bad] = np.float32(1e6)
            t3 = _firefly_ref.firefly_ref(finite, radius=radius, rank=rank)["threshold"]
            reach = np.zeros((h, w), bool)
            for dy, dx in _firefly_ref.taps(radius) + [(0, 0)]:
                reach |= _firefly_ref._shifted(bad, radius, dy, dx, False)
            assert np.array_equal(t[~reach].view(np.uint32), t3[~reach].view(np.uint32))
            assert not np.array_equal(t[reach & ~bad], t3[reach & ~bad])  # 1e6 in a window does move its statistic


def test_reference_selection_does_not_depend_on_the_order_of_ties():
    """The decision path again, by the kernel's insertion chain and with the taps visited in other orders: a selection with
    multiplicity gives the same float whatever the order, so the masks and thresholds are identical, ties included."""
    rng = np.random.default_rng(5)
    for w, h in FRAMES:
        color, marks = _firefly_ref.frame(w, h)
        for radius, rank, k, floor in ((1, 3, 4.0, 0.01), (1, 1, 1.0, 0.0), (2, 8, 4.0, 0.01), (3, 8, 2.0, 0.5), (3, 1, 1.5, 0.0)):
            first = _firefly_ref.firefly_ref(color, radius, rank, k, floor)
            n_taps = len(_firefly_ref.taps(radius))
            for how in (dict(select="chain"), dict(select="chain", order=rng.permutation(n_taps)),
                        dict(select="sort", order=rng.permutation(n_taps)), dict(select="chain", order=np.arange(n_taps)[::-1])):
                again = _firefly_ref.firefly_ref(color, radius, rank, k, floor, **how)
                assert np.array_equal(first["mask"], again["mask"]), (w, h, radius, rank, how)
                assert np.array_equal(first["threshold"].view(np.uint32), again["threshold"].view(np.uint32))
        # Y_p > T is strict: at rank 1, k 1, floor 0 a pixel that ties with its largest neighbour is kept
        tied = _firefly_ref.firefly_ref(color, 1, 1, 1.0, 0.0)
        inner = marks["ties"] & (tied["Y"] == tied["threshold"])
        assert inner.any() and not tied["mask"][inner].any()
