"""The à-trous denoiser on a real MI355X (-m gpu): rtm_denoise against the NumPy float64 restatement (_denoise_ref) on
synthetic frames and a Cornell render, hard object edges, determinism across calls and streams, the quality bar on the
Cornell box, and the Render / rtm_cli outputs."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _denoise_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "raytracingmin_amd", "rtm_cli")
SCENE = os.path.join(ROOT, "scenes", "cornellBoxSetting.json")
TOL = 1e-4  # include/rtm.h: |out - ref| <= 1e-4 max(1, |ref|)
SIGMAS = {"sigma_color": 1.0, "sigma_normal": 16.0, "sigma_depth": 0.5}
GUIDE_SETS = [(), ("depth",), ("normal",), ("albedo",), ("object",), ("depth", "normal", "albedo", "object")]


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
    return _denoise_ref.denoise_ref(color, guides.get("depth"), guides.get("normal"), guides.get("albedo"),
                                    guides.get("object"), **kw)


def _host_quantise(rtm, f32):
    v = np.ascontiguousarray(f32, dtype=np.float64)
    out = np.zeros(v.shape, np.uint8)
    rtm._lib.check(rtm.lib().rtm_quantise(v.ctypes.data, v.size, out.ctypes.data), "rtm_quantise")
    return out


@pytest.mark.parametrize("w,h", [(1, 1), (1, 17), (37, 23), (64, 64), (130, 70)])
def test_denoise_matches_the_reference(rtm, w, h):
    import torch
    color, guides = _frame(w, h, w * 1000 + h)
    color[0, 0] = [1.5, -0.25, 7.0]  # out of [0, 1]: u8 clamps and zeroes like rtm_quantise
    cd = _dev(color)
    gd = {k: _dev(v) for k, v in guides.items()}
    worst = 0.0
    for names in GUIDE_SETS:
        sub = {k: guides[k] for k in names}
        for k in (0, 1, 3, 5, 10):
            out = rtm.denoise(cd, {n: gd[n] for n in names}, iterations=k, want=("f32", "u8"), **SIGMAS)
            torch.cuda.synchronize()
            f32, u8 = out["f32"].cpu().numpy(), out["u8"].cpu().numpy()
            if k == 0:
                assert np.array_equal(f32.view(np.uint32), color.view(np.uint32)), names
            err = _denoise_ref.tolerance_excess(f32, _ref(color, sub, iterations=k, **SIGMAS))
            assert err <= TOL, (names, k, err)
            worst = max(worst, err)
            assert np.array_equal(u8, _host_quantise(rtm, f32)), (names, k)
    print(f"{w}x{h}: worst error against the float64 reference {worst:.3e} (bar {TOL})")


def test_object_edges_are_hard(rtm):
    import torch
    w, h = 48, 32
    color, guides = _frame(w, h, 7)
    guides["object"][:, : w // 2] = 0
    guides["object"][:, w // 2:] = 1
    gd = {k: _dev(v) for k, v in guides.items()}
    other = color.copy()
    other[:, w // 2:] = np.random.default_rng(8).random((h, w - w // 2, 3)).astype(np.float32) * 3
    a = rtm.denoise(_dev(color), gd, iterations=5)["f32"]
    b = rtm.denoise(_dev(other), gd, iterations=5)["f32"]
    torch.cuda.synchronize()
    a, b = a.cpu().numpy(), b.cpu().numpy()
    assert np.array_equal(a[:, : w // 2].view(np.uint32), b[:, : w // 2].view(np.uint32))
    assert not np.array_equal(a[:, w // 2:], b[:, w // 2:])


def test_denoise_is_deterministic_across_calls_and_streams(rtm):
    import torch
    color, guides = _frame(300, 170, 11)
    cd, gd = _dev(color), {k: _dev(v) for k, v in guides.items()}
    first = rtm.denoise(cd, gd, want=("f32", "u8"))
    second = rtm.denoise(cd, gd, want=("f32", "u8"))
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    third = rtm.denoise(cd, gd, want=("f32", "u8"), stream=s)
    s.synchronize()
    raw = torch.cuda.Stream()
    raw.wait_stream(torch.cuda.current_stream())
    fourth = rtm.denoise(cd, gd, want=("f32", "u8"), stream=raw.cuda_stream)
    raw.synchronize()
    ref = {k: v.cpu().numpy() for k, v in first.items()}
    for out in (second, third, fourth):
        assert np.array_equal(out["f32"].cpu().numpy().view(np.uint32), ref["f32"].view(np.uint32))
        assert np.array_equal(out["u8"].cpu().numpy(), ref["u8"])


def _cornell(rtm, w, h, samples, ss):
    import torch
    data = rtm.LoadData(SCENE).data
    data.width, data.height, data.samples, data.superSamples = w, h, samples, ss
    r = rtm.Renderer(data, mode="repaired", max_bounces=8)
    out, _ = r.render_rows_device(want=("f32",), stats=False)
    aov = r.render_aov()
    torch.cuda.synchronize()
    return r, out["f32"], aov


def test_cornell_frame_matches_the_reference(rtm):
    import torch
    _, f32, aov = _cornell(rtm, 128, 96, 4, 2)
    got = rtm.denoise(f32, aov, want=("f32",))["f32"]
    torch.cuda.synchronize()
    host = {k: v.cpu().numpy() for k, v in aov.items()}
    ref = _ref(f32.cpu().numpy(), host, **_denoise_ref.DEFAULTS)
    err = _denoise_ref.tolerance_excess(got.cpu().numpy(), ref)
    print(f"Cornell 128x96 at the defaults: worst error against the float64 reference {err:.3e}")
    assert err <= TOL


def test_denoise_halves_the_error_of_a_4spp_cornell_frame(rtm):
    import torch
    _, noisy, aov = _cornell(rtm, 256, 256, 1, 2)
    _, ref, _ = _cornell(rtm, 256, 256, 256, 2)
    den = rtm.denoise(noisy, aov)["f32"]
    torch.cuda.synchronize()
    clip = lambda t: np.clip(t.cpu().numpy().astype(np.float64), 0.0, 1.0)
    rmse = lambda a, b: float(np.sqrt(np.mean((a - b) ** 2)))
    raw_err, den_err = rmse(clip(noisy), clip(ref)), rmse(clip(den), clip(ref))
    print(f"Cornell 256x256: RMSE 4 spp {raw_err:.5f}, denoised {den_err:.5f}, ratio {den_err / raw_err:.3f} (bar 0.5)")
    assert den_err <= 0.5 * raw_err


def _read_bmp(path):
    raw = open(path, "rb").read()
    off = int.from_bytes(raw[10:14], "little")
    w, h = int.from_bytes(raw[18:22], "little"), int.from_bytes(raw[22:26], "little")
    stride = (w * 3 + 3) & ~3
    rows = [np.frombuffer(raw, np.uint8, w * 3, off + y * stride).reshape(w, 3)[:, ::-1] for y in range(h)]
    return np.stack(rows[::-1])


def test_render_and_cli_write_the_denoised_frame(rtm, tmp_path):
    import torch
    w, h = 64, 40
    data = rtm.LoadData(SCENE).data
    data.width, data.height, data.samples, data.superSamples = w, h, 4, 2
    r = rtm.Renderer(data, mode="repaired", max_bounces=8)
    plain = r.Render(str(tmp_path / "plain"))
    image = r.image.copy()
    rgb8 = r.Render(str(tmp_path / "py"), denoise=True)
    assert np.array_equal(rgb8, plain) and np.array_equal(r.image, image)
    assert (tmp_path / "py.bmp").read_bytes() == (tmp_path / "plain.bmp").read_bytes()
    for k in ("py_denoised.jpg", "py_denoised.bmp"):
        assert (tmp_path / k).stat().st_size > 0, k
    assert not (tmp_path / "plain_denoised.bmp").exists()
    # the Python path's quantised denoise of the frame, computed directly
    f32 = torch.from_numpy(image).cuda().to(torch.float32)
    want = rtm.denoise(f32, r.render_aov(), want=("u8",))["u8"].cpu().numpy()
    assert np.array_equal(_read_bmp(tmp_path / "py_denoised.bmp"), want)
    args = ["-json", SCENE, "--width", str(w), "--height", str(h), "--samples", "4", "--superSamples", "2",
            "--max-bounces", "8", "--out", "cli", "--denoise"]
    run = subprocess.run([CLI] + args, cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    assert (tmp_path / "cli.bmp").read_bytes() == (tmp_path / "plain.bmp").read_bytes()
    assert (tmp_path / "cli_denoised.jpg").stat().st_size > 0
    assert np.array_equal(_read_bmp(tmp_path / "cli_denoised.bmp"), want)
    # combined with --passes and --aov: the same denoised frame
    run = subprocess.run([CLI] + args[:-3] + ["--out", "both", "--denoise", "--aov", "--passes", "2"], cwd=tmp_path,
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    assert (tmp_path / "both_normal.pfm").exists()
    assert (tmp_path / "both_denoised.bmp").read_bytes() == (tmp_path / "cli_denoised.bmp").read_bytes()
