"""The variance-guided denoiser on a real MI355X (-m gpu): rtm_denoise_variance against the NumPy float64 restatement
(_denoise_var_ref) on synthetic frames, its agreement with rtm_denoise when both colour terms are off, hard object edges,
determinism across calls and streams, the quality bars on a Cornell frame that is half 4 spp and half 256 spp, and the
Render / rtm_cli outputs."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _denoise_var_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "raytracingmin_amd", "rtm_cli")
SCENE = os.path.join(ROOT, "scenes", "cornellBoxSetting.json")
TOL = 1e-4  # include/rtm.h: |out - ref| <= 1e-4 max(1, |ref|), for the output and for v0
SIGMAS = {"sigma_lum": 2.0, "sigma_normal": 16.0, "sigma_depth": 0.5}
GUIDE_SETS = [(), ("object",), ("depth", "normal", "albedo", "object")]
GUIDES = ("depth", "normal", "albedo", "object")


@pytest.fixture(scope="module")
def rtm():
    import raytracingmin_amd as m
    n = C.c_int()
    m._lib.check(m.lib().rtm_device_count(C.byref(n)), "rtm_device_count")
    assert n.value >= 1
    return m


def _frame(w, h, seed):
    """A noisy colour frame and guides with structure: three normal directions, objects, misses (+inf, -1), dark albedo."""
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((3, 3))
    base /= np.linalg.norm(base, axis=1, keepdims=True)
    region = rng.integers(0, 3, (h, w))
    n = base[region] + 0.1 * rng.standard_normal((h, w, 3))
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    depth = (1 + 2 * rng.random((h, w))).astype(np.float32)
    miss = rng.random((h, w)) < 0.1
    depth[miss] = np.inf
    obj = region.astype(np.int32)
    obj[miss] = -1
    albedo = rng.random((h, w, 3)).astype(np.float32)
    albedo[rng.random((h, w, 3)) < 0.05] = 0.0
    color = (1.5 * rng.random((h, w, 3))).astype(np.float32)
    return color, {"depth": depth, "normal": n.astype(np.float32), "albedo": albedo, "object": obj}


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ref(color, guides, **kw):
    return _denoise_var_ref.denoise_variance_ref(color, guides.get("depth"), guides.get("normal"), guides.get("albedo"),
                                                 guides.get("object"), **kw)


def _host_quantise(rtm, f32):
    v = np.ascontiguousarray(f32, dtype=np.float64)
    out = np.zeros(v.shape, np.uint8)
    rtm._lib.check(rtm.lib().rtm_quantise(v.ctypes.data, v.size, out.ctypes.data), "rtm_quantise")
    return out


@pytest.mark.parametrize("w,h", [(1, 1), (1, 17), (7, 5), (37, 23), (130, 70)])
def test_denoise_variance_matches_the_reference(rtm, w, h):
    import torch
    from raytracingmin_amd import _lib
    color, guides = _frame(w, h, w * 1000 + h)
    color[0, 0] = [1.5, -0.25, 7.0]  # out of [0, 1]: u8 clamps and zeroes like rtm_quantise
    cd = _dev(color)
    gd = {k: _dev(v) for k, v in guides.items()}
    worst, worst_v = 0.0, 0.0
    for names in GUIDE_SETS:
        sub = {k: guides[k] for k in names}
        for k in (0, 1, 3, 5):
            out = rtm.denoise_variance(cd, {n: gd[n] for n in names}, iterations=k, want=("f32", "u8", "var"), **SIGMAS)
            torch.cuda.synchronize()
            f32, u8, var = out["f32"].cpu().numpy(), out["u8"].cpu().numpy(), out["var"].cpu().numpy()
            if k == 0:
                assert np.array_equal(f32.view(np.uint32), color.view(np.uint32)), names
            ref, v0 = _ref(color, sub, iterations=k, **SIGMAS)
            err = _denoise_var_ref.tolerance_excess(f32, ref)
            err_v = _denoise_var_ref.tolerance_excess(var, v0)
            print(f"{w}x{h} {names} K={k}: error {err:.3e}, of v0 {err_v:.3e}")
            assert err <= TOL, (names, k, err)
            assert err_v <= TOL, (names, k, err_v)
            worst, worst_v = max(worst, err), max(worst_v, err_v)
            assert np.array_equal(u8, _host_quantise(rtm, f32)), (names, k)
        # every form of the variance kernel (direct, LDS tiles of 64 x 4 and 64 x 8) holds the same bar
        L = rtm.lib()
        prm = _lib.rtm_denoise_var_params(0, SIGMAS["sigma_lum"], SIGMAS["sigma_normal"], SIGMAS["sigma_depth"])
        bufs = _lib.rtm_aov_buffers()
        for n in names:
            setattr(bufs, n, gd[n].data_ptr())
        work = torch.empty(L.rtm_denoise_variance_work_bytes(w, h), dtype=torch.uint8, device="cuda")
        v_call = torch.empty((h, w), dtype=torch.float32, device="cuda")
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(L.rtm_denoise_variance(C.byref(prm), w, h, 0, cd.data_ptr(), C.byref(bufs), work.data_ptr(), None, None,
                                          v_call.data_ptr(), stream), "rtm_denoise_variance")
        _, v0 = _ref(color, sub, iterations=0, **SIGMAS)
        for form in (0, 1, 2):
            v_form = torch.full((h, w), -1.0, dtype=torch.float32, device="cuda")
            _lib.check(L.rtm_debug_denoise_variance_kernel(form, C.byref(prm), w, h, 0, C.byref(bufs), work.data_ptr(),
                                                           v_form.data_ptr(), stream), "rtm_debug_denoise_variance_kernel")
            torch.cuda.synchronize()
            err_v = _denoise_var_ref.tolerance_excess(v_form.cpu().numpy(), v0)
            assert err_v <= TOL, (names, form, err_v)
            worst_v = max(worst_v, err_v)
    print(f"{w}x{h}: worst error against the float64 reference {worst:.3e}, of v0 {worst_v:.3e} (bar {TOL})")


def test_without_the_luminance_term_it_is_rtm_denoise_without_its_colour_term(rtm):
    import torch
    w, h = 130, 70
    color, guides = _frame(w, h, 21)
    cd, gd = _dev(color), {k: _dev(v) for k, v in guides.items()}
    for k in (1, 4):
        a = rtm.denoise_variance(cd, gd, iterations=k, sigma_lum=0.0, sigma_normal=16.0, sigma_depth=0.5)["f32"]
        b = rtm.denoise(cd, gd, iterations=k, sigma_color=0.0, sigma_normal=16.0, sigma_depth=0.5)["f32"]
        torch.cuda.synchronize()
        err = _denoise_var_ref.tolerance_excess(a.cpu().numpy(), b.cpu().numpy())
        print(f"sigma_lum = 0 against rtm_denoise with sigma_color = 0, K = {k}: {err:.3e}")
        assert err <= TOL, k


def test_object_edges_are_hard(rtm):
    """No colour and no variance crosses an object edge: a tap of another object weighs exactly zero.  The one thing that
    looks across is the 3 x 3 prefilter of the variance, which has no geometry weight by contract, so the pixels next to the
    edge may weigh their own side's taps differently; the bitwise checks below stay clear of what that can reach."""
    import torch
    w, h = 48, 32
    half = w // 2
    color, guides = _frame(w, h, 7)
    guides["object"][:, :half] = 0
    guides["object"][:, half:] = 1
    gd = {k: _dev(v) for k, v in guides.items()}
    other = color.copy()
    other[:, half:] = 100 + np.random.default_rng(8).random((h, w - half, 3)).astype(np.float32) * 3
    bits = lambda t: t.cpu().numpy().view(np.uint32)
    # v0, and the filter without the luminance term: the left half does not see the right half at all
    a = rtm.denoise_variance(_dev(color), gd, iterations=5, sigma_lum=0.0, want=("f32", "var"))
    b = rtm.denoise_variance(_dev(other), gd, iterations=5, sigma_lum=0.0, want=("f32", "var"))
    torch.cuda.synchronize()
    for k in ("f32", "var"):
        assert np.array_equal(bits(a[k])[:, :half], bits(b[k])[:, :half]), k
        assert not np.array_equal(bits(a[k])[:, half:], bits(b[k])[:, half:]), k
    # one level at the defaults: only the column next to the edge has a prefilter tap on the other side
    a = rtm.denoise_variance(_dev(color), gd, iterations=1)["f32"]
    b = rtm.denoise_variance(_dev(other), gd, iterations=1)["f32"]
    torch.cuda.synchronize()
    assert np.array_equal(bits(a)[:, : half - 1], bits(b)[:, : half - 1])
    # five levels at the defaults, no albedo: every left pixel is a mean of left pixels, far below the right half's 100
    plain = {k: v for k, v in gd.items() if k != "albedo"}
    out = rtm.denoise_variance(_dev(other), plain, iterations=5)["f32"].cpu().numpy()
    left = other[:, :half]
    assert np.all(out[:, :half] >= left.min(axis=(0, 1)) - 1e-5) and np.all(out[:, :half] <= left.max(axis=(0, 1)) + 1e-5)
    assert np.all(out[:, half:] >= 100 - 1e-3)


def test_denoise_variance_is_deterministic_across_calls_and_streams(rtm):
    import torch
    color, guides = _frame(300, 170, 11)
    cd, gd = _dev(color), {k: _dev(v) for k, v in guides.items()}
    want = ("f32", "u8", "var")
    first = rtm.denoise_variance(cd, gd, want=want)
    second = rtm.denoise_variance(cd, gd, want=want)
    only = rtm.denoise_variance(cd, gd, want=("var",))  # the variance-only call
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    third = rtm.denoise_variance(cd, gd, want=want, stream=s)
    s.synchronize()
    raw = torch.cuda.Stream()
    raw.wait_stream(torch.cuda.current_stream())
    fourth = rtm.denoise_variance(cd, gd, want=want, stream=raw.cuda_stream)
    only_raw = rtm.denoise_variance(cd, gd, want=("var",), stream=raw.cuda_stream)
    raw.synchronize()
    ref = {k: v.cpu().numpy() for k, v in first.items()}
    assert set(only) == {"var"}
    for out in (second, third, fourth, only, only_raw):
        for k in out:
            assert np.array_equal(out[k].cpu().numpy().view(np.uint8), ref[k].view(np.uint8)), k
    assert float(ref["var"].max()) > 0.0


def _cornell(rtm, w, h, samples, ss):
    import torch
    data = rtm.LoadData(SCENE).data
    data.width, data.height, data.samples, data.superSamples = w, h, samples, ss
    r = rtm.Renderer(data, mode="repaired", max_bounces=8)
    out, _ = r.render_rows_device(want=("f32",), stats=False)
    aov = r.render_aov()
    torch.cuda.synchronize()
    return r, out["f32"], aov


def test_variance_guidance_keeps_the_converged_half_of_a_mixed_cornell_frame(rtm):
    """Columns [0, 128) at 4 spp, [128, 256) at 256 spp, against 4096 spp.  At the shipped defaults: (a) the left half's RMSE
    is at most half the raw frame's (the project's bar for a denoiser); (b) the right half's is at most rtm_denoise's at its
    own defaults on the same frame — the feature's claim, no margin."""
    import torch
    _, noisy, aov = _cornell(rtm, 256, 256, 1, 2)
    _, fine, _ = _cornell(rtm, 256, 256, 64, 2)
    _, truth, _ = _cornell(rtm, 256, 256, 1024, 2)
    mixed = torch.cat([noisy[:, :128], fine[:, 128:]], dim=1).contiguous()
    fixed = rtm.denoise(mixed, aov)["f32"]
    guided = rtm.denoise_variance(mixed, aov)["f32"]
    torch.cuda.synchronize()
    clip = lambda t: np.clip(t.cpu().numpy().astype(np.float64), 0.0, 1.0)
    rmse = lambda a, b: float(np.sqrt(np.mean((a - b) ** 2)))
    t = clip(truth)
    halves = {"left": np.s_[:, :128], "right": np.s_[:, 128:]}
    e = {name: {side: rmse(clip(img)[sl], t[sl]) for side, sl in halves.items()}
         for name, img in (("raw", mixed), ("fixed", fixed), ("variance", guided))}
    print("Cornell 256x256, 4 spp | 256 spp against 4096 spp, RMSE left / right: " +
          ", ".join(f"{name} {e[name]['left']:.5f} / {e[name]['right']:.5f}" for name in e))
    assert e["variance"]["left"] <= 0.5 * e["raw"]["left"]
    assert e["variance"]["right"] <= e["fixed"]["right"]


def _read_bmp(path):
    raw = open(path, "rb").read()
    off = int.from_bytes(raw[10:14], "little")
    w, h = int.from_bytes(raw[18:22], "little"), int.from_bytes(raw[22:26], "little")
    stride = (w * 3 + 3) & ~3
    rows = [np.frombuffer(raw, np.uint8, w * 3, off + y * stride).reshape(w, 3)[:, ::-1] for y in range(h)]
    return np.stack(rows[::-1])


def _read_pfm(path):
    raw = open(path, "rb").read()
    head = raw.split(b"\n", 3)
    assert head[0] == b"Pf"
    w, h = (int(v) for v in head[1].split())
    return np.frombuffer(head[3], dtype="<f4").reshape(h, w)[::-1]


def test_render_writes_the_variance_guided_files(rtm, tmp_path):
    import torch
    data = rtm.LoadData(os.path.join(ROOT, "scenes", "settingData.json")).data
    data.width, data.height, data.samples, data.superSamples = 192, 104, 64, 1
    r = rtm.Renderer(data, mode="repaired", max_bounces=8)
    for name, kw in (("uni", {}), ("two", {"passes": 2}), ("ada", {"adaptive": 0.05})):
        plain = r.Render(str(tmp_path / (name + "_plain")), **kw)
        rgb8 = r.Render(str(tmp_path / name), denoise="variance", **kw)
        assert np.array_equal(rgb8, plain), name
        assert (tmp_path / (name + ".bmp")).read_bytes() == (tmp_path / (name + "_plain.bmp")).read_bytes(), name
        # the frame denoised is the one just rendered (the adaptive preview under adaptive=T), rounded to float
        f32 = torch.from_numpy(r.image).cuda().to(torch.float32)
        want = rtm.denoise_variance(f32, r.render_aov(), want=("u8", "var"))
        assert np.array_equal(_read_bmp(tmp_path / (name + "_denoised_var.bmp")), want["u8"].cpu().numpy()), name
        assert np.array_equal(_read_pfm(tmp_path / (name + "_variance.pfm")), want["var"].cpu().numpy()), name
        assert (tmp_path / (name + "_denoised_var.jpg")).stat().st_size > 0
        assert not (tmp_path / (name + "_denoised.bmp")).exists() and not (tmp_path / (name + "_plain_variance.pfm")).exists()
    assert (tmp_path / "uni.bmp").read_bytes() == (tmp_path / "two.bmp").read_bytes()
    assert (tmp_path / "uni_denoised_var.bmp").read_bytes() == (tmp_path / "two_denoised_var.bmp").read_bytes()
    assert (tmp_path / "ada_spp.pfm").exists()
    # denoise=True still writes what it wrote
    r.Render(str(tmp_path / "old"), denoise=True)
    f32 = torch.from_numpy(r.image).cuda().to(torch.float32)
    assert np.array_equal(_read_bmp(tmp_path / "old_denoised.bmp"), rtm.denoise(f32, r.render_aov(), want=("u8",))["u8"].cpu().numpy())
    assert not (tmp_path / "old_denoised_var.bmp").exists()


def test_cli_writes_the_variance_guided_files(rtm, tmp_path):
    import torch
    w, h = 64, 40
    args = [CLI, "-json", SCENE, "--width", str(w), "--height", str(h), "--samples", "16", "--superSamples", "2",
            "--max-bounces", "8"]

    def run(stem, *flags):
        p = subprocess.run(args + ["--out", stem] + list(flags), cwd=tmp_path, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout + p.stderr
        return p.stdout

    run("plain")
    assert "denoise-variance:" in run("var", "--denoise-variance")
    assert (tmp_path / "var.bmp").read_bytes() == (tmp_path / "plain.bmp").read_bytes()
    assert (tmp_path / "var_denoised_var.jpg").stat().st_size > 0 and not (tmp_path / "var_denoised.bmp").exists()
    data = rtm.LoadData(SCENE).data
    data.width, data.height, data.samples, data.superSamples = w, h, 16, 2
    r = rtm.Renderer(data, mode="repaired", max_bounces=8)
    f32 = r.render_rows_device(want=("f32",), stats=False)[0]["f32"]
    want = rtm.denoise_variance(f32, r.render_aov(), want=("u8", "var"))
    torch.cuda.synchronize()
    assert np.array_equal(_read_bmp(tmp_path / "var_denoised_var.bmp"), want["u8"].cpu().numpy())
    assert np.array_equal(_read_pfm(tmp_path / "var_variance.pfm"), want["var"].cpu().numpy())
    # with --adaptive and --denoise: the plain and fixed-filter files are those of a run without the new flag
    run("ref", "--adaptive", "0.05", "--denoise")
    run("all", "--adaptive", "0.05", "--denoise", "--denoise-variance")
    for ext in (".bmp", "_denoised.bmp", "_spp.pfm"):
        assert (tmp_path / ("all" + ext)).read_bytes() == (tmp_path / ("ref" + ext)).read_bytes(), ext
    assert not (tmp_path / "ref_denoised_var.bmp").exists()
    out, _, _ = r.adaptive(0.05, want=("f32",))
    want = rtm.denoise_variance(out["f32"], r.render_aov(), want=("u8",))["u8"].cpu().numpy()
    assert np.array_equal(_read_bmp(tmp_path / "all_denoised_var.bmp"), want)
    assert (tmp_path / "all_variance.pfm").exists()
    # with --aov and --passes: the same denoised frame as the one-pass run
    run("both", "--denoise-variance", "--aov", "--passes", "2")
    assert (tmp_path / "both_normal.pfm").exists()
    assert (tmp_path / "both_denoised_var.bmp").read_bytes() == (tmp_path / "var_denoised_var.bmp").read_bytes()
    assert (tmp_path / "both_variance.pfm").read_bytes() == (tmp_path / "var_variance.pfm").read_bytes()
