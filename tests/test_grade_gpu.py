"""The colour grade on a real MI355X (-m gpu): rtm_grade against the NumPy float64 restatement (_grade_ref) on the smallest
shapes at which its kernel can go wrong — one pixel, less than a block, odd sizes, several blocks — for each parametric step
alone, all of them, a LUT alone (N in 2, 3, 17, 33, both interpolations, two domains; random, affine and identity tables) and
everything followed by a LUT; the all-defaults copy and pixels that do not count word for word; lattice and domain-edge inputs;
the clamp that keeps every LUT read inside the table; in place; determinism across calls, streams and alignments; and the
Render / rtm_cli outputs.  test_grade_matches_the_reference prints the worst error per case; DESIGN.md records it.

test_grade_host checks on the CPU that every compared case leaves float32 arithmetic within 2e-5 of the reference, and
test_lut_asan checks the index arithmetic the kernel compiles (rtm_grade_index.h) on the CPU, under the sanitizers, on the
values the clamp test sends through it here."""
import ctypes as C
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import _grade_ref
import _resize_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "raytracingmin_amd", "rtm_cli")
SCENE = os.path.join(ROOT, "scenes", "cornellBoxSetting.json")
TOL = 1e-4  # include/rtm.h: |got - ref| <= 1e-4 max(1, |ref|)
SIZES = _grade_ref.SIZES
INTERPS = _grade_ref.INTERPS


@pytest.fixture(scope="module")
def rtm():
    import raytracingmin_amd as m
    n = C.c_int()
    m._lib.check(m.lib().rtm_device_count(C.byref(n)), "rtm_device_count")
    assert n.value >= 1
    return m


@functools.lru_cache(maxsize=None)
def _frame(w, h):
    f = _resize_ref.frame(w, h)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def _cases():
    return tuple(_grade_ref.gpu_cases())


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()  # (a copy: the cached arrays are read-only)


def _on_device(kw):
    """grade_ref's keyword arguments as grade()'s: the table on the device."""
    return {k: (_dev(v) if k == "lut" else v) for k, v in kw.items()}


def _host_quantise(rtm, f32):
    with np.errstate(invalid="ignore"):
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


def _quantised_table(n, seed=0):
    """A random table in [0, 1] on multiples of 2^-10: every difference and every blend at f = 0 or 1 is computed exactly."""
    return (np.random.default_rng(900 + n + seed).integers(0, 1025, (n, n, n, 3)) / 1024.0).astype(np.float32)


@pytest.mark.parametrize("size", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_grade_matches_the_reference(rtm, size):
    w, h = size
    frame = _frame(w, h)
    cd = _dev(frame)
    worst = ("", 0.0)
    got_of = {}
    for name, kw in _cases():
        ref = _grade_ref.grade_ref(frame, **kw)
        assert np.all(np.isfinite(ref)), name
        dkw = _on_device(kw)
        out = _bits(rtm.grade(cd, want=("f32", "u8"), **dkw))
        got = out["f32"]
        assert got.shape == frame.shape and got.dtype == np.float32 and out["u8"].shape == frame.shape and np.all(np.isfinite(got)), name
        err = _grade_ref.tolerance_excess(got, ref)
        print(f"{w}x{h} {name}: out_f32 {err:.3e}")
        assert err <= TOL, (name, err)
        # the 8-bit store is rtm_quantise of the call's own out_f32: exact at every pixel
        assert np.array_equal(out["u8"], _host_quantise(rtm, got)) and np.array_equal(out["u8"], _grade_ref.quantise_u8(got)), name
        # a single output: the same bits
        only32, only8 = _bits(rtm.grade(cd, want=("f32",), **dkw)), _bits(rtm.grade(cd, want=("u8",), **dkw))
        assert tuple(only32) == ("f32",) and tuple(only8) == ("u8",)
        assert np.array_equal(_words(only32["f32"]), _words(got)) and np.array_equal(only8["u8"], out["u8"]), name
        got_of[name] = got
        if err > worst[1]:
            worst = (name, err)
    assert np.array_equal(_words(cd.cpu().numpy()), _words(frame))  # the input is left alone
    # saturation 0: r = g = b (= L), exactly
    grey = got_of["saturation-0"]
    assert np.array_equal(grey[..., 0], grey[..., 1]) and np.array_equal(grey[..., 1], grey[..., 2])
    # an affine table is reproduced by both interpolants, which therefore agree; the identity table returns the input clipped
    # to the domain
    for n in (2, 3, 17, 33):
        for k, dom in enumerate(_grade_ref.DOMAINS):
            clipped = np.clip(frame.astype(np.float64), dom[0][0], dom[1][0])
            tri, tet = (got_of[f"lut-{n}-{i}-domain{k}-affine"] for i in INTERPS)
            assert _grade_ref.tolerance_excess(tri, _grade_ref.affine_of(clipped)) <= TOL, (n, k)
            assert _grade_ref.tolerance_excess(tet, _grade_ref.affine_of(clipped)) <= TOL, (n, k)
            assert _grade_ref.tolerance_excess(tri, tet) <= 2 * TOL, (n, k)
            for i in INTERPS:
                assert _grade_ref.tolerance_excess(got_of[f"lut-{n}-{i}-domain{k}-identity"], clipped) <= TOL, (n, k, i)
    print(f"{w}x{h}: {len(got_of)} cases, worst error against the float64 reference {worst[1]:.3e} ({worst[0]}) (bar {TOL})")


def _salted(w, h):
    """The frame with pixels that do not count (NaNs with payloads, +-inf, one bad component) and words that a careless copy
    would change (-0, a denormal); fewer on a frame of fewer pixels."""
    f = _frame(w, h).copy()
    flat = f.reshape(-1, 3).view(np.uint32)
    salt = [(0x7FC00001, 0x3F800000, 0x3F800000), (0x3F800000, 0xFF800000, 0x40000000), (0x7F800000, 0x7F800000, 0x7F800000),
            (0x7F800123, 0xFFC00000, 0xFFFFFFFF), (0x80000000, 0x00000001, 0x80000001), (0x80000000, 0x80000000, 0x80000000),
            (0x3F000000, 0x3F000000, 0x7FA00000)]
    n = w * h
    for k, words in enumerate(salt):
        flat[(k * 37 + (0 if n <= len(salt) else 5)) % n] = words
    return f


def test_the_defaults_copy_every_word(rtm):
    for w, h in SIZES:
        f = _salted(w, h)
        out = _bits(rtm.grade(_dev(f), want=("f32", "u8")))
        assert np.array_equal(_words(out["f32"]), _words(f)), (w, h)
        assert np.array_equal(out["u8"], _host_quantise(rtm, f)), (w, h)  # NaN and -inf -> 0, +inf -> 255
        # default values given explicitly, -0 for 0 among them, are the defaults
        m = np.eye(3)
        m[0, 1] = m[2, 0] = -0.0
        out = _bits(rtm.grade(_dev(f), matrix=m, exposure=-0.0, offset=(-0.0, 0.0, -0.0)))
        assert np.array_equal(_words(out["f32"]), _words(f)), (w, h)


def test_pixels_that_do_not_count_are_copied_word_for_word(rtm):
    table = _dev(_grade_ref.smooth_table(17))
    for w, h in SIZES[1:]:
        f = _salted(w, h)
        ok = _grade_ref.counts(f)
        assert (~ok).sum() >= 4 and ok.sum() >= 4
        for kw in (dict(_grade_ref.EVERYTHING), dict(lut=table), dict(_grade_ref.EVERYTHING, lut=table, interp="trilinear")):
            out = _bits(rtm.grade(_dev(f), want=("f32", "u8"), **kw))
            assert np.array_equal(_words(out["f32"])[~ok], _words(f)[~ok]), (w, h, sorted(kw))
            host = {k: (v.cpu().numpy() if k == "lut" else v) for k, v in kw.items()}
            ref = _grade_ref.grade_ref(f, **host)
            assert _grade_ref.tolerance_excess(out["f32"][ok], ref[ok]) <= TOL, (w, h, sorted(kw))
            assert np.array_equal(out["u8"], _host_quantise(rtm, out["f32"]))


def test_lattice_inputs_return_the_entries(rtm):
    n = 17
    table = _quantised_table(n)
    rng = np.random.default_rng(5)
    idx = rng.integers(0, n, (35, 67, 3))
    idx[0, 0], idx[0, 1], idx[0, 2], idx[0, 3] = (0, 0, 0), (16, 16, 16), (16, 0, 16), (0, 16, 3)
    frame = (idx / 16.0).astype(np.float32)  # k / 16: the lattice coordinate is k exactly
    want = table[idx[..., 2], idx[..., 1], idx[..., 0]]
    for interp in INTERPS:
        got = _bits(rtm.grade(_dev(frame), lut=_dev(table), interp=interp))["f32"]
        assert np.array_equal(got, want), interp


def test_inputs_at_and_beyond_the_domain_edges_land_on_the_edge_entries(rtm):
    for n in (2, 3, 17, 33):
        table = _quantised_table(n)
        for k, dom in enumerate(_grade_ref.DOMAINS):
            lo, hi = np.float32(dom[0][0]), np.float32(dom[1][0])
            below = [lo, np.nextafter(lo, np.float32(-9)), lo - np.float32(1), np.float32(-3e38)]
            above = [hi, np.nextafter(hi, np.float32(9)), hi + np.float32(5), np.float32(3e38)]
            pixels, want = [], []
            for cr in (0, 1):
                for cg in (0, 1):
                    for cb in (0, 1):
                        for j in range(4):
                            pixels.append([(above if c else below)[(j + s) % 4] for s, c in enumerate((cr, cg, cb))])
                            want.append(table[(n - 1) * cb, (n - 1) * cg, (n - 1) * cr])
            frame = np.float32(pixels).reshape(4, 8, 3)
            want = np.float32(want).reshape(4, 8, 3)
            for interp in INTERPS:
                got = _bits(rtm.grade(_dev(frame), lut=_dev(table), lut_domain=dom, interp=interp))["f32"]
                if k == 0:  # (y - 0) (N - 1) is exact at 0 and 1: the corner entry itself
                    assert np.array_equal(got, want), (n, interp)
                else:  # the scale is rounded: hi may land one rounding inside the last cell
                    assert _grade_ref.tolerance_excess(got, want) <= TOL, (n, interp)


def test_the_clamp_keeps_every_lut_read_inside_the_table(rtm):
    """Counting pixels up to +-3e38 through saturation 1.5 (whose L + s (y - L) overflows to +-inf and to the NaN of inf - inf)
    into a LUT: the call succeeds, pixels that do not count keep their words, and every output of a counting pixel is finite
    and inside the table's per-channel range — it is a table entry or a blend of entries.  A blend a + f (b - a) with f in
    [0, 1] can pass b by a rounding of each of its three operations, so the range is taken with a slack of 4 ulp of 1.
    (The index arithmetic itself is checked on the CPU first: tests/test_lut_asan.py, csrc/lut_selftest.cpp.)"""
    import torch
    rng = np.random.default_rng(11)
    w, h = 130, 9
    f = _salted(w, h)
    big = np.float32([3e38, -3e38, 1e38, -1e38, 3.4028235e38, -3.4028235e38, 1e30, -1e30, 0.0, 1.0])
    pick = rng.integers(0, len(big), (h, w, 3))
    extreme = rng.random((h, w)) < 0.5
    ok = _grade_ref.counts(f)
    f[extreme & ok] = big[pick][extreme & ok]
    ok = _grade_ref.counts(f)
    assert (~ok).sum() >= 4 and (extreme & ok).sum() > 100
    slack = 4 * np.finfo(np.float32).eps
    for n in (2, 17, 256):
        table = rng.random((n, n, n, 3), dtype=np.float32)  # (N = 256: the largest table, 3 * 2^24 floats)
        lo, hi = table.reshape(-1, 3).min(axis=0), table.reshape(-1, 3).max(axis=0)
        td = _dev(table)
        for dom in _grade_ref.DOMAINS + (((-3e38,) * 3, (3e38,) * 3), ((0, 0, 0), (1e-45,) * 3)):
            for interp in INTERPS:
                out = rtm.grade(_dev(f), saturation=1.5, lut=td, lut_domain=dom, interp=interp, want=("f32", "u8"))  # raises unless RTM_OK
                torch.cuda.synchronize()
                got = out["f32"].cpu().numpy()
                assert np.array_equal(_words(got)[~ok], _words(f)[~ok]), (n, dom, interp)
                g = got[ok]
                assert np.all(np.isfinite(g)), (n, dom, interp)
                assert np.all(g >= lo - slack) and np.all(g <= hi + slack), (n, dom, interp, g.min(axis=0), g.max(axis=0))
                assert np.array_equal(out["u8"].cpu().numpy(), _host_quantise(rtm, got))
    # and without a LUT the overflow is IEEE's: infinities and NaNs come out, nothing is repaired
    got = _bits(rtm.grade(_dev(f), saturation=1.5))["f32"]
    assert not np.all(np.isfinite(got[ok])) and np.array_equal(_words(got)[~ok], _words(f)[~ok])


def test_in_place_equals_out_of_place(rtm):
    table = _dev(_grade_ref.smooth_table(17))
    for w, h in ((67, 35), (300, 70)):
        f = _salted(w, h)
        for kw in (dict(), dict(_grade_ref.EVERYTHING), dict(lut=table, interp="trilinear"), dict(_grade_ref.EVERYTHING, lut=table)):
            apart = _bits(rtm.grade(_dev(f), **kw))["f32"]
            cd = _dev(f)
            out = rtm.grade(cd, out_f32=cd, want=("f32", "u8"), **kw)
            assert out["f32"] is cd
            both = _bits(out)
            assert np.array_equal(_words(both["f32"]), _words(apart)), (w, h, sorted(kw))
            assert np.array_equal(both["u8"], _host_quantise(rtm, apart)), (w, h, sorted(kw))


def _call(rtm, prm, src_t, lut_t, w, h, out32, out8, stream):
    from raytracingmin_amd import _lib
    _lib.check(rtm.lib().rtm_grade(C.byref(prm), w, h, 0, src_t.data_ptr(), lut_t.data_ptr() if lut_t is not None else None,
                                   out32.data_ptr() if out32 is not None else None, out8.data_ptr() if out8 is not None else None,
                                   C.c_void_p(stream.cuda_stream)), "rtm_grade")


def test_the_same_inputs_give_the_same_bits(rtm):
    import torch
    from raytracingmin_amd import renderer
    table = _grade_ref.smooth_table(17)
    for w, h in ((67, 35), (130, 9)):
        frame = _frame(w, h)
        cd = _dev(frame)
        n = w * h * 3
        for kw in (dict(_grade_ref.EVERYTHING), dict(lut=table, interp="trilinear"), dict(_grade_ref.EVERYTHING, lut=table)):
            dkw = _on_device(kw)
            first = _bits(rtm.grade(cd, want=("f32", "u8"), **dkw))
            assert _same_bits(first, _bits(rtm.grade(cd, want=("f32", "u8"), **dkw))), (w, h, sorted(kw))  # a second call
            cur = torch.cuda.current_stream()
            pkw = {k: v for k, v in kw.items() if k != "lut"}
            struct = renderer._grade_params(lut_size=17 if "lut" in kw else 0, **pkw)
            for words in (1, 2):  # color, out_f32 and the table offset by 4 and by 8 bytes
                sbuf = torch.empty(n + 8, dtype=torch.float32, device="cuda")
                obuf = torch.empty(n + 8, dtype=torch.float32, device="cuda")
                shifted, oshift = sbuf[words:words + n], obuf[words:words + n]
                shifted.copy_(cd.reshape(-1))
                lut_t = None
                if "lut" in kw:
                    tbuf = torch.empty(table.size + 8, dtype=torch.float32, device="cuda")
                    lut_t = tbuf[words:words + table.size]
                    lut_t.copy_(dkw["lut"].reshape(-1))
                assert cd.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 4 * words and oshift.data_ptr() % 16 == 4 * words
                out8 = torch.empty(frame.shape, dtype=torch.uint8, device="cuda")
                _call(rtm, struct, shifted, lut_t, w, h, oshift, out8, cur)
                got = _bits({"f32": oshift.reshape(frame.shape), "u8": out8})
                assert _same_bits(first, got), (w, h, sorted(kw), words)
            # two calls on two streams
            side = torch.cuda.Stream()
            side.wait_stream(cur)
            third = rtm.grade(cd, want=("f32", "u8"), stream=side, **dkw)
            fourth = rtm.grade(cd, want=("f32", "u8"), **dkw)  # the current stream's, while the side stream may still run
            side.synchronize()
            assert _same_bits(first, _bits(third)) and _same_bits(first, _bits(fourth)), (w, h, sorted(kw))


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


def test_render_and_cli_grade_the_display_frame(rtm, tmp_path):
    import torch
    scene = json.load(open(SCENE))
    scene["00 width"], scene["00 height"], scene["00 samples"], scene["00 superSamples"] = 192, 108, 4, 1
    small = tmp_path / "small.json"
    small.write_text(json.dumps(scene))
    args = [CLI, "-json", str(small), "--max-bounces", "8"]
    look = tmp_path / "look.cube"
    _grade_ref.write_cube(look, _grade_ref.smooth_table(17), title="smooth", comments=True)

    def run(stem, *flags, status=0):
        p = subprocess.run(args + ["--out", stem] + list(flags), cwd=tmp_path, capture_output=True, text=True, timeout=300)
        assert p.returncode == status, p.stdout + p.stderr
        return p.stdout if status == 0 else p.stderr

    def same_files(a, b):
        return all((tmp_path / (a + ext)).read_bytes() == (tmp_path / (b + ext)).read_bytes() for ext in (".bmp", ".jpg"))

    r = rtm.Renderer(rtm.LoadData(str(small)).data, mode="repaired", max_bounces=8)
    params = dict(temperature=4300, tint=0.01, exposure=0.5, contrast=1.2, pivot=0.2, slope=(1.1, 0.9, 1.05), offset=(0.01, -0.02, 0.0),
                  power=(0.8, 1.2, 1.0), saturation=1.3)
    flags = ["--grade-temperature", "4300", "--grade-tint", "0.01", "--grade-exposure", "0.5", "--grade-contrast", "1.2,0.2",
             "--grade-slope", "1.1,0.9,1.05", "--grade-offset", "0.01,-0.02,0", "--grade-power", "0.8,1.2,1", "--grade-saturation", "1.3"]
    # Render and rtm_cli write the same files, and they are what grade() and tonemap() called by hand give
    r.Render(str(tmp_path / "py"), tonemap=True, bloom=True, grade=params, lut=str(look))
    text = run("cli", "--display", "--bloom", *flags, "--lut", str(look), "--display-pfm")
    assert len([l for l in text.splitlines() if l.startswith("grade:")]) == 1 and len([l for l in text.splitlines() if l.startswith("lut:")]) == 1, text
    assert "temperature 4300" in text and "saturation 1.29999995" in text and "size 17, tetrahedral" in text, text
    assert same_files("cli_display", "py_display") and same_files("cli", "py")
    f32 = torch.from_numpy(r.image).cuda().to(torch.float32)
    by_hand = dict(params)
    by_hand["matrix"] = rtm.white_balance(by_hand.pop("temperature"), by_hand.pop("tint"))
    graded = rtm.grade(rtm.bloom(f32)["f32"], **by_hand)["f32"]
    cube = rtm.load_cube(str(look))
    assert np.array_equal(cube["table"], _grade_ref.smooth_table(17))
    shown = rtm.grade(rtm.tonemap(graded, want=("f32",))["f32"], lut=torch.from_numpy(cube["table"]).cuda())["f32"]
    last = rtm.tonemap(shown, op="clamp", transfer="linear", exposure=0.0, want=("f32", "u8"))
    assert np.array_equal(_read_bmp(tmp_path / "py_display.bmp"), last["u8"].cpu().numpy())
    assert np.array_equal(_words(_read_pfm(tmp_path / "cli_display.pfm")), _words(last["f32"].cpu().numpy()))
    # the parametric grade alone and the look alone (trilinear, as load_cube's dict), each against the call by hand
    r.Render(str(tmp_path / "py2"), tonemap=dict(op="reinhard", dither=False), grade=dict(saturation=0.0))
    run("cli2", "--display", "reinhard", "--no-dither", "--grade-saturation", "0")
    assert same_files("cli2_display", "py2_display")
    grey = rtm.tonemap(rtm.grade(f32, saturation=0.0)["f32"], op="reinhard", dither=False)["u8"].cpu().numpy()
    assert np.array_equal(_read_bmp(tmp_path / "py2_display.bmp"), grey)
    assert np.array_equal(grey[..., 0], grey[..., 1]) and np.array_equal(grey[..., 1], grey[..., 2])
    r.Render(str(tmp_path / "py3"), tonemap=dict(dither=False), lut=dict(cube, interp="trilinear"))
    text = run("cli3", "--display", "--no-dither", "--lut", str(look), "--lut-interp", "trilinear")
    assert "size 17, trilinear" in text and "grade:" not in text
    assert same_files("cli3_display", "py3_display")
    tri = rtm.grade(rtm.tonemap(f32, dither=False, want=("f32",))["f32"], lut=torch.from_numpy(cube["table"]).cuda(), interp="trilinear")["f32"]
    assert np.array_equal(_read_bmp(tmp_path / "py3_display.bmp"),
                          rtm.tonemap(tri, op="clamp", transfer="linear", exposure=0.0, dither=False)["u8"].cpu().numpy())
    # write_display alone, of self.image
    back = r.write_display(str(tmp_path / "w"), grade=dict(exposure=-1), lut=cube)
    assert back.shape == (108, 192, 3) and (tmp_path / "w_display.jpg").stat().st_size > 0
    # without the flags: no line, and every file is what it was (the stage is opt-in); with them the display files differ
    text = run("off", "--display", "--bloom", "--display-pfm")
    r.Render(str(tmp_path / "pyoff"), tonemap=True, bloom=True)
    assert "grade:" not in text and "lut:" not in text
    assert same_files("off_display", "pyoff_display") and same_files("off", "cli") and same_files("off", "py")
    plain = rtm.tonemap(rtm.bloom(f32)["f32"], want=("f32", "u8"))
    assert np.array_equal(_read_bmp(tmp_path / "off_display.bmp"), plain["u8"].cpu().numpy())
    assert np.array_equal(_words(_read_pfm(tmp_path / "off_display.pfm")), _words(plain["f32"].cpu().numpy()))
    assert not same_files("off_display", "cli_display")
    # a grade whose values are all the defaults is the ungraded run, byte for byte
    run("noop", "--display", "--bloom", "--grade-exposure", "0", "--grade-slope", "1,1,1")
    assert same_files("noop_display", "off_display")
