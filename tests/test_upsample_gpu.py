"""The AOV-guided upsampler on a real MI355X (-m gpu): rtm_upsample against the NumPy float64 restatement (_upsample_ref) on
synthetic frames, its properties on the device (constant signal, hard edges, the thin-feature fallback, determinism), the
bytes around its buffers, the quality of a Cornell preview, and the Render / rtm_cli outputs."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _upsample_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "raytracingmin_amd", "rtm_cli")
SCENE = os.path.join(ROOT, "scenes", "cornellBoxSetting.json")
TOL = 1e-4  # include/rtm.h: |out - ref| <= 1e-4 max(1, |ref|)
PLANES = ("depth", "normal", "albedo", "object")
GUIDE_SETS = [(), ("depth",), ("normal",), ("albedo",), ("object",), PLANES]
# (33, 9, 2) and (17, 5, 8) cross a 64-wide block boundary; (40, 3, 5) is 200 wide: a ragged last block, three row blocks
CASES = [(1, 1, 2), (3, 2, 3), (5, 7, 4), (33, 9, 2), (17, 5, 8), (40, 3, 5)]
# RMSE(preview at f = 2) / RMSE(the full frame at the same path count, denoised) on the Cornell box, 256 x 256: the measured
# ratio ("AOV-guided upsampling") plus 25 % against run-to-run seed and box differences
QUALITY_RATIO_BAR = 0.835  # 0.668 (RMSE 0.05217 / 0.07807, measured on an MI355X) x 1.25


@pytest.fixture(scope="module")
def rtm():
    import raytracingmin_amd as m
    n = C.c_int()
    m._lib.check(m.lib().rtm_device_count(C.byref(n)), "rtm_device_count")
    assert n.value >= 1
    return m


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _sub(d, names):
    return {k: d[k] for k in names}


def _host_quantise(rtm, f32):
    v = np.ascontiguousarray(f32, dtype=np.float64)
    out = np.zeros(v.shape, np.uint8)
    rtm._lib.check(rtm.lib().rtm_quantise(v.ctypes.data, v.size, out.ctypes.data), "rtm_quantise")
    return out


def _run(rtm, color, low, high, **kw):
    import torch
    out = rtm.upsample(_dev(color), {k: _dev(v) for k, v in low.items()}, {k: _dev(v) for k, v in high.items()}, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("w,h,f", CASES)
def test_upsample_matches_the_reference(rtm, w, h, f):
    color, low, high, _ = ref.synthetic_case(w, h, f, 1000 * w + 10 * h + f)
    color[0, 0] = [1.5, -0.25, 7.0]  # out of [0, 1]: u8 clamps and zeroes like rtm_quantise
    runs = [(names, {}) for names in GUIDE_SETS] + [(PLANES, {"sigma_normal": 0.0, "sigma_depth": 0.0}),
                                                    (PLANES, {"sigma_spatial": 1.0, "sigma_normal": 8.0, "sigma_depth": 0.5})]
    worst = 0.0
    for names, sig in runs:
        got = _run(rtm, color, _sub(low, names), _sub(high, names), factor=f, want=("f32", "u8"), **sig)
        assert got["f32"].shape == (f * h, f * w, 3)
        want = ref.upsample_ref(color, _sub(low, names), _sub(high, names), factor=f, **sig)
        err = ref.tolerance_excess(got["f32"], want)
        print(f"{w}x{h} x{f} {names or 'no guides'} {sig or 'defaults'}: error {err:.3e}")
        assert err <= TOL, (names, sig, err)
        worst = max(worst, err)
        assert np.array_equal(got["u8"], _host_quantise(rtm, got["f32"])), (names, sig)
    print(f"{w}x{h} x{f}: worst error against the float64 reference {worst:.3e} (bar {TOL})")


def test_constant_demodulated_signal_comes_back_at_full_resolution(rtm):
    w, h, f, k = 21, 6, 4, 0.75
    _, low, high, _ = ref.synthetic_case(w, h, f, 5)
    a_low = np.where(low["albedo"] > np.float32(1e-3), low["albedo"], np.float32(1.0))
    a_high = np.where(high["albedo"] > np.float32(1e-3), high["albedo"], np.float32(1.0)).astype(np.float64)
    got = _run(rtm, (np.float32(k) * a_low).astype(np.float32), low, high, factor=f)["f32"]
    assert ref.tolerance_excess(got, k * a_high) <= TOL


@pytest.mark.parametrize("f", (2, 4))
def test_object_edges_are_hard(rtm, f):
    """Two objects at 0 and 1 that meet on a low pixel boundary, no albedo (the bound: test_upsample_host's docstring)."""
    h, w = 6, 40  # 80 / 160 columns: the edge lies in the second block
    obj = np.zeros((h * f, w * f), np.int32)
    obj[:, (w // 2 + 3) * f:] = 1
    high = {"object": obj}
    low = {"object": ref.sample_low(obj, f)}
    color = np.repeat(low["object"].astype(np.float32)[..., None], 3, axis=2)
    _, matched, _ = ref.upsample_ref(color, low, high, factor=f, return_weights=True)
    got = _run(rtm, color, low, high, factor=f)["f32"]
    assert matched.all()
    assert np.max(np.abs(got.astype(np.float64) - obj[..., None])[matched]) <= 1e-5


def test_thin_feature_gets_the_spatial_average(rtm):
    w, h, f = 33, 9, 2
    color, low, high, thin = ref.synthetic_case(w, h, f, 6)
    guided = _run(rtm, color, _sub(low, ("object",)), _sub(high, ("object",)), factor=f)["f32"]
    plain = _run(rtm, color, {}, {}, factor=f)["f32"]
    assert thin.any()
    assert ref.tolerance_excess(guided[thin], plain[thin].astype(np.float64)) <= TOL
    assert not np.allclose(guided[~thin], plain[~thin], rtol=1e-3, atol=0)


def test_outputs_and_streams_give_the_same_bits(rtm):
    import torch
    w, h, f = 70, 11, 3
    color, low, high, _ = ref.synthetic_case(w, h, f, 7)
    cd, ld, hd = _dev(color), {k: _dev(v) for k, v in low.items()}, {k: _dev(v) for k, v in high.items()}
    both = rtm.upsample(cd, ld, hd, factor=f, want=("f32", "u8"))
    only32 = rtm.upsample(cd, ld, hd, factor=f, want=("f32",))
    only8 = rtm.upsample(cd, ld, hd, factor=f, want=("u8",))
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    a = rtm.upsample(cd, ld, hd, factor=f, want=("f32", "u8"), stream=s1)  # each call allocates its own work buffer
    b = rtm.upsample(cd, ld, hd, factor=f, want=("f32", "u8"), stream=s2.cuda_stream)
    s1.synchronize()
    s2.synchronize()
    bits = both["f32"].cpu().numpy().view(np.uint32)
    u8 = both["u8"].cpu().numpy()
    assert set(only32) == {"f32"} and set(only8) == {"u8"}
    assert np.array_equal(only32["f32"].cpu().numpy().view(np.uint32), bits)
    assert np.array_equal(only8["u8"].cpu().numpy(), u8)
    for out in (a, b):
        assert np.array_equal(out["f32"].cpu().numpy().view(np.uint32), bits)
        assert np.array_equal(out["u8"].cpu().numpy(), u8)


def test_bytes_around_the_buffers_are_untouched(rtm):
    import torch
    from raytracingmin_amd import _lib
    L = rtm.lib()
    w, h, f = 33, 9, 2  # 66 x 18: a ragged second block column and a ragged last block row
    color, low, high, _ = ref.synthetic_case(w, h, f, 8)
    cd, ld, hd = _dev(color), {k: _dev(v) for k, v in low.items()}, {k: _dev(v) for k, v in high.items()}
    n_out, n_work, pad = f * h * f * w * 3 * 4, L.rtm_upsample_work_bytes(w, h), 4096
    assert n_work == 32 * w * h
    arena = torch.full((pad + n_out + pad + n_work + pad,), 0xA5, dtype=torch.uint8, device="cuda")
    out_off, work_off = pad, pad + n_out + pad
    assert (arena.data_ptr() + work_off) % 16 == 0
    glo, ghi = _lib.rtm_aov_buffers(), _lib.rtm_aov_buffers()
    for k in PLANES:
        setattr(glo, k, ld[k].data_ptr())
        setattr(ghi, k, hd[k].data_ptr())
    prm = _lib.rtm_upsample_params(f, 0.5, 64.0, 0.05)
    _lib.check(L.rtm_upsample(C.byref(prm), w, h, 0, cd.data_ptr(), C.byref(glo), C.byref(ghi), arena.data_ptr() + work_off,
                              arena.data_ptr() + out_off, None, C.c_void_p(torch.cuda.current_stream().cuda_stream)),
               "rtm_upsample")
    torch.cuda.synchronize()
    host = arena.cpu().numpy()
    for a, b in ((0, out_off), (out_off + n_out, work_off), (work_off + n_work, host.size)):
        assert np.all(host[a:b] == 0xA5), (a, b)
    got = host[out_off:out_off + n_out].view(np.float32).reshape(f * h, f * w, 3)
    assert ref.tolerance_excess(got, ref.upsample_ref(color, low, high, factor=f)) <= TOL


# ---- end to end -----------------------------------------------------------------------------------------------------
def _read_bmp(path):
    raw = open(path, "rb").read()
    off = int.from_bytes(raw[10:14], "little")
    w, h = int.from_bytes(raw[18:22], "little"), int.from_bytes(raw[22:26], "little")
    stride = (w * 3 + 3) & ~3
    rows = [np.frombuffer(raw, np.uint8, w * 3, off + y * stride).reshape(w, 3)[:, ::-1] for y in range(h)]
    return np.stack(rows[::-1])


def test_render_and_cli_write_the_preview(rtm, tmp_path):
    import torch
    w = h = 64
    data = rtm.LoadData(SCENE).data
    data.width, data.height, data.samples, data.superSamples = w, h, 4, 2
    r = rtm.Renderer(data, mode="repaired", max_bounces=8)
    plain = r.Render(str(tmp_path / "plain"))
    image = r.image.copy()
    rgb8 = r.Render(str(tmp_path / "py"), preview=2, tonemap=True)
    assert np.array_equal(rgb8, plain) and np.array_equal(r.image, image)
    assert (tmp_path / "py.bmp").read_bytes() == (tmp_path / "plain.bmp").read_bytes()
    for k in ("py_preview.jpg", "py_preview.bmp", "py_display.bmp", "py_preview_display.bmp", "py_preview_display.jpg"):
        assert (tmp_path / k).stat().st_size > 0, k
    assert not (tmp_path / "plain_preview.bmp").exists()
    out = r.preview(2, want=("u8", "f32"))
    torch.cuda.synchronize()
    want = out["u8"].cpu().numpy()
    assert want.shape == (h, w, 3)
    assert np.array_equal(_read_bmp(tmp_path / "py_preview.bmp"), want)
    shown = rtm.tonemap(out["f32"], want=("u8",))["u8"].cpu().numpy()
    assert np.array_equal(_read_bmp(tmp_path / "py_preview_display.bmp"), shown)
    # the preview is the denoised low frame, upsampled: denoise=False is another image
    raw = r.preview(2, denoise=False, want=("u8",))["u8"].cpu().numpy()
    assert not np.array_equal(raw, want)
    args = ["-json", SCENE, "--width", str(w), "--height", str(h), "--samples", "4", "--superSamples", "2", "--max-bounces", "8"]
    run = subprocess.run([CLI] + args + ["--out", "cli", "--preview", "2"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    assert (tmp_path / "cli.bmp").read_bytes() == (tmp_path / "plain.bmp").read_bytes()
    assert (tmp_path / "cli_preview.jpg").stat().st_size > 0
    assert np.array_equal(_read_bmp(tmp_path / "cli_preview.bmp"), want)
    run = subprocess.run([CLI] + args + ["--out", "only", "--preview", "2", "--preview-only"], cwd=tmp_path, capture_output=True,
                         text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    assert not (tmp_path / "only.bmp").exists() and not (tmp_path / "only.jpg").exists()
    assert (tmp_path / "only_preview.bmp").read_bytes() == (tmp_path / "cli_preview.bmp").read_bytes()
    assert (tmp_path / "only_preview.jpg").stat().st_size > 0


# ---- quality on the Cornell box -------------------------------------------------------------------------------------
def _cornell(rtm, w, h, samples, ss):
    import torch
    data = rtm.LoadData(SCENE).data
    data.width, data.height, data.samples, data.superSamples = w, h, samples, ss
    r = rtm.Renderer(data, mode="repaired", max_bounces=8)
    out, _ = r.render_rows_device(want=("f32",), stats=False)
    aov = r.render_aov()
    torch.cuda.synchronize()
    return r, out["f32"], aov


def test_cornell_preview_beats_replication_and_the_unguided_filter(rtm):
    import torch
    _, truth, aov_high = _cornell(rtm, 256, 256, 256, 2)
    _, low, aov_low = _cornell(rtm, 128, 128, 4, 2)
    _, full1, _ = _cornell(rtm, 256, 256, 1, 2)  # the same number of paths as the low frame
    low_dn = rtm.denoise(low, aov_low)["f32"]
    route_a = rtm.denoise(full1, aov_high)["f32"]
    route_b = rtm.upsample(low_dn, aov_low, aov_high, factor=2)["f32"]
    route_c = low_dn.repeat_interleave(2, dim=0).repeat_interleave(2, dim=1)
    route_d = rtm.upsample(low_dn, factor=2)["f32"]
    torch.cuda.synchronize()
    clip = lambda t: np.clip(t.cpu().numpy().astype(np.float64), 0.0, 1.0)
    t = clip(truth)
    rmse = {k: float(np.sqrt(np.mean((clip(v) - t) ** 2))) for k, v in
            (("A", route_a), ("B", route_b), ("C", route_c), ("D", route_d))}
    ratio = rmse["B"] / rmse["A"]
    print(f"Cornell 256x256: RMSE A (full, 4 paths, denoised) {rmse['A']:.5f}, B (preview f=2) {rmse['B']:.5f}, "
          f"C (replicated) {rmse['C']:.5f}, D (no guides) {rmse['D']:.5f}; B / A = {ratio:.3f} (bar {QUALITY_RATIO_BAR})")
    assert rmse["B"] < rmse["C"]
    assert rmse["B"] < rmse["D"]
    if QUALITY_RATIO_BAR is not None:  # (None: no hardware run has measured the ratio yet; the bar follows the first)
        assert ratio <= QUALITY_RATIO_BAR
