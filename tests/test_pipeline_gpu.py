"""The whole post-process chain on a real MI355X (-m gpu).  The order of the stages is written down in two places, rtm_cli
(rtm_main.cpp with rtm_node.cpp, host vectors uploaded per stage) and Renderer.Render (device tensors handed on); every other
test runs a stage alone or with one neighbour.  Each test here is one long chain on a 100 x 60 frame (no multiple of 64, of
the adaptive tile's 8 in neither axis; even, for --preview 2), resized where it resizes to 67 x 35 (odd, below the 256 default
scope columns), and checks three things: (a) every file and every line rtm_cli writes equals the tensors and records of the
module's stage functions called in the documented order ("The stage order, as tested"); (b) Renderer.Render with
the same options writes the same bytes; (c) every stage call of (a), on the input the device took, is within its own test's
bar of its float64 restatement (tests/_pipeline.py: STAGES), so the restatements see rendered frames: fireflies next to the
emitter, albedo edges, AOV guides, and in the open scene inf depth, zero coverage and black sky."""
import ctypes as C
import json

import numpy as np
import pytest

import _grade_ref
import _pipeline as pl
from _pipeline import cli, lines_of, read_bmp, read_pfm, record_of, words

pytestmark = pytest.mark.gpu

W, H, SAMPLES, SS = 100, 60, 4, 1
RW, RH = 67, 35
BACKGROUND = (0.2, 0.4, 0.8)


@pytest.fixture(scope="module")
def rtm():
    import raytracingmin_amd as m
    n = C.c_int()
    m._lib.check(m.lib().rtm_device_count(C.byref(n)), "rtm_device_count")
    assert n.value >= 1
    return m


def _renderer(rtm, scene):
    return rtm.Renderer(rtm.LoadData(scene).data, mode="repaired", max_bounces=8)


def _frame(r):
    """The plain render as out_f32 gives it: the float64 frame rounded to float."""
    out, _ = r.render_rows_device(want=("f64", "f32"), stats=False)
    assert np.array_equal(words(out["f32"].cpu().numpy()), words(out["f64"].cpu().numpy().astype(np.float32)))
    return out["f32"]


def _is_pfm(path, tensor):
    """The file's words are the tensor's, and so is its size."""
    got, want = read_pfm(path), tensor.cpu().numpy() if hasattr(tensor, "cpu") else np.asarray(tensor)
    assert got.shape == want.shape, (path.name, got.shape, want.shape)
    assert np.array_equal(words(got), words(want)), (path.name, int((words(got) != words(want)).sum()))


def _is_bmp(path, tensor):
    got, want = read_bmp(path), tensor.cpu().numpy() if hasattr(tensor, "cpu") else np.asarray(tensor)
    assert got.shape == want.shape, (path.name, got.shape, want.shape)
    assert np.array_equal(got, want), (path.name, int((got != want).any(axis=-1).sum()))


def _same_files(tmp_path, a, b, suffixes):
    """Stem a's files are stem b's, byte for byte."""
    for s in suffixes:
        fa, fb = tmp_path / (a + s), tmp_path / (b + s)
        assert fa.exists() and fb.exists(), s
        assert fa.read_bytes() == fb.read_bytes(), (a, b, s)


def _num(v):
    """A double as rtm_cli prints it: 17 significant digits, which read back to the same double."""
    return "%.17g" % v


def _pair(suffix):
    return [suffix + ".bmp", suffix + ".jpg"]


def _scope_document(rtm, hist_tensor, mode):
    """What rtm_cli says of one frame's histogram: (the line's object, the document's)."""
    hist = rtm.scope_histogram(hist_tensor)
    line = rtm.scope_summary(hist, mode)
    doc = dict(line, histogram={"bins": hist["bins"].tolist(), "below": hist["below"].tolist(), "above": hist["above"].tolist()})
    return pl.as_json(line), pl.as_json(doc)


def _check_scopes(rtm, tmp_path, stem, stdout, lin, disp, picture, exposure=None):
    """The scopes: line, STEM_scopes.json, the waveform: line and STEM_waveform.bmp against the two scopes calls and the picture."""
    lin_line, lin_doc = _scope_document(rtm, lin["histogram"], "log2")
    disp_line, disp_doc = _scope_document(rtm, disp["histogram"], "code")
    extra = {} if exposure is None else {"exposure": exposure}
    line = record_of(stdout, "scopes: ")
    assert line == {**lin_line, "display": disp_line, **extra}
    assert json.load(open(tmp_path / f"{stem}_scopes.json")) == {**lin_doc, "display": disp_doc, **extra}
    _is_bmp(tmp_path / f"{stem}_waveform.bmp", picture)
    return line


def _display_line(stdout, stem, stats_words):
    """The display: line of the frame itself carries the first tonemap's statistics."""
    s = pl.tonemap_stats(stats_words.cpu().numpy())
    want = (f"{stem}_display.bmp, {stem}_display.jpg (log-average {s['log_average']:.6g}, max luminance {s['max_luminance']:.6g}, "
            f"exposure {s['exposure']:.6g}, {s['pixels']} pixels)")
    assert want in lines_of(stdout, "display: "), (want, lines_of(stdout, "display: "))


# ---- Chain A: everything linear, closed scene ---------------------------------------------------------------------------
LENS = dict(k1=-0.2, k2=0.03, chroma=0.004, vignette=0.4)
BLOOM_A = dict(intensity=0.3, threshold=1.5)
GRADE_A = dict(temperature=4300, contrast=1.15, saturation=1.2)
FLAGS_A = ["--aov", "--firefly", "--denoise", "--dof", "6", "--focus-pixel", "50,42", "--lens", "-0.2,0.03", "--lens-ca", "0.004",
           "--lens-vignette", "0.4", "--lens-zoom", "auto", "--resize", f"{RW}x{RH}", "--resize-filter", "lanczos3", "--display",
           "--bloom", "0.3", "--bloom-threshold", "1.5", "--grade-temperature", "4300", "--grade-contrast", "1.15",
           "--grade-saturation", "1.2", "--lut", "look.cube"]


def test_chain_a_everything_linear_in_the_closed_scene(rtm, tmp_path):
    import torch
    scene = pl.small_scene(tmp_path, pl.CORNELL, W, H, SAMPLES, SS)
    _grade_ref.write_cube(tmp_path / "look.cube", _grade_ref.smooth_table(9))
    stdout = cli(tmp_path, scene, "A", *FLAGS_A, "--scopes", "--scopes-layout", "parade", "--expose-percentile", "99,0.8", "--pfm",
                 "--display-pfm")

    # (a) the stage calls, in the documented order
    r = _renderer(rtm, scene)
    chain = pl.Chain(rtm, "chain A")
    frame = _frame(r)
    aov = r.render_aov()
    _is_bmp(tmp_path / "A.bmp", r.render_rows_device(want=("u8",), stats=False)[0]["u8"])
    ff = chain("firefly", color=frame)
    mask = ff["mask"].cpu().numpy()
    assert record_of(stdout, "firefly: ") == {"clamped": int((mask == 1).sum()), "repaired": int((mask == 2).sum()), "pixels": W * H}
    _is_bmp(tmp_path / "A_firefly.bmp", ff["u8"])
    dn = chain("denoise", color=ff["f32"], **aov)
    _is_bmp(tmp_path / "A_denoised.bmp", dn["u8"])
    zf = float(aov["depth"][42, 50].item())  # the focus: the depth plane at --focus-pixel 50,42
    assert np.isfinite(zf) and zf > 0 and zf == r.focus_distance((50, 42))
    assert lines_of(stdout, "dof: ") == [f"focus {zf:.6g}, aperture 6, max radius 8"]
    df = chain("defocus", dict(focus_distance=zf, aperture=6.0, max_radius=8), color=dn["f32"], depth=aov["depth"])
    _is_bmp(tmp_path / "A_dof.bmp", df["u8"])
    zoom = rtm.lens_fit_zoom(W, H, **LENS)  # at the render's size: the lens runs before the resize
    assert zoom != rtm.lens_fit_zoom(RW, RH, **LENS)
    assert lines_of(stdout, "lens: ") == [f"A_lens.bmp, A_lens.jpg (zoom {zoom:.9g})"]
    ln = chain("lens", dict(LENS, zoom=zoom), color=df["f32"])
    _is_bmp(tmp_path / "A_lens.bmp", ln["u8"])
    rs = chain("resize", dict(size=(RH, RW), filter="lanczos3"), color=ln["f32"])
    assert lines_of(stdout, "resize: ") == [f"A_resized.bmp, A_resized.jpg ({RW} x {RH})"]
    _is_bmp(tmp_path / "A_resized.bmp", rs["u8"])
    _is_pfm(tmp_path / "A.pfm", rs["f32"])  # the last linear frame
    assert read_pfm(tmp_path / "A.pfm").shape == (RH, RW, 3)
    # the display path, all of it at the resized size: bloom, grade, the exposure from their frame, the curve, the look
    bl = chain("bloom", BLOOM_A, color=rs["f32"])
    gr = chain("grade", dict(matrix=rtm.white_balance(4300), contrast=1.15, saturation=1.2), color=bl["f32"])
    exposed = chain("scopes", dict(mode="log2", columns=RW), color=gr["f32"])
    ev = rtm.scope_exposure(exposed["histogram"], 99, 0.8)
    assert ev != 0.0 and ev != rtm.scope_exposure(rtm.scopes(rs["f32"])["histogram"], 99, 0.8)  # the bloom and the grade count
    assert lines_of(stdout, "expose-percentile: ") == [f"A at 99 percent to {_num(0.8)}, exposure {_num(ev)}"]
    tm = chain("tonemap", dict(exposure=ev), color=gr["f32"])
    _display_line(stdout, "A", tm["stats"])
    cube = rtm.load_cube(str(tmp_path / "look.cube"))
    look = chain("grade", dict(lut_domain=(cube["domain_min"], cube["domain_max"]), interp="tetrahedral"), color=tm["f32"],
                 lut=torch.from_numpy(cube["table"]).cuda())
    shown = chain("tonemap", dict(op="clamp", transfer="linear", exposure=0.0), color=look["f32"])
    _is_pfm(tmp_path / "A_display.pfm", shown["f32"])
    _is_bmp(tmp_path / "A_display.bmp", shown["u8"])
    assert read_pfm(tmp_path / "A_display.pfm").shape == (RH, RW, 3) and read_bmp(tmp_path / "A_display.bmp").shape == (RH, RW, 3)
    # the scopes: the last linear frame in stops, the display frame after the look in code values, over the resized width
    lin = chain("scopes", dict(mode="log2", columns=RW), color=rs["f32"])
    disp = chain("scopes", dict(mode="code", columns=RW), color=shown["f32"])
    gain = max(1, 2040 // RH)
    picture = chain("scope_draw", dict(layout="parade", gain=gain), waveform=disp["waveform"])["u8"]
    line = _check_scopes(rtm, tmp_path, "A", stdout, lin, disp, picture, exposure=ev)
    assert np.float32(line["exposure"]) == np.float32(ev)
    assert read_bmp(tmp_path / "A_waveform.bmp").shape == (256, 3 * RW, 3)  # 201 x 256: the parade over 67 columns
    assert lines_of(stdout, "waveform: ") == [f"A_waveform.bmp ({3 * RW} x 256, gain {gain}), A_scopes.json"]
    assert line["pixels"] == line["display"]["pixels"] == RW * RH
    # the AOV planes: the render's size, no stage touches them
    for name in ("depth", "normal", "albedo"):
        _is_pfm(tmp_path / f"A_{name}.pfm", aov[name])
        assert read_pfm(tmp_path / f"A_{name}.pfm").shape[:2] == (H, W)

    # (b) Renderer.Render writes rtm_cli's bytes (no counterpart for --scopes and --expose-percentile: a run without them)
    cli(tmp_path, scene, "A2", *FLAGS_A)
    _renderer(rtm, scene).Render(str(tmp_path / "Apy"), aov=True, firefly=True, denoise=True, dof=dict(aperture=6.0, focus_pixel=(50, 42)),
                                 lens=dict(LENS, zoom="auto"), resize=(RW, RH, "lanczos3"), tonemap=True, bloom=BLOOM_A, grade=GRADE_A,
                                 lut=str(tmp_path / "look.cube"))
    files = _pair("") + _pair("_firefly") + _pair("_denoised") + _pair("_dof") + _pair("_lens") + _pair("_resized") + _pair("_display")
    files += ["_depth.pfm", "_normal.pfm", "_albedo.pfm", "_normal.bmp", "_albedo.bmp"]
    _same_files(tmp_path, "Apy", "A2", files)
    _same_files(tmp_path, "A", "A2", [f for f in files if "_display" not in f])  # the exposure is all the two runs differ in
    assert read_bmp(tmp_path / "A2_display.bmp").shape == (RH, RW, 3)

    # (c) every call above against its float64 restatement, on the input the device took
    worst = chain.teacher_force()
    assert set(worst) == {"firefly", "denoise", "defocus", "lens", "resize", "bloom", "grade", "scopes", "tonemap", "scope_draw"}


# ---- Chain B: open scene, coverage, local tone, adaptive ---------------------------------------------------------------------
FLAGS_B = ["--adaptive", "0.05", "--firefly", "--denoise-variance", "--dof", "--display", "local", "--local-shadows", "3", "--bloom",
           "--alpha", "--matte", "0,2", "--background", "0.2,0.4,0.8"]


def _local_display(chain, frame):
    """write_display's local path at automatic exposure: bloom, the statistics, the operator at their E, the clamp and store."""
    bl = chain("bloom", color=frame)
    stats = chain("tonemap", color=bl["f32"])["stats"]
    fused = chain("tonemap_local", dict(anchor=1.0, shadows=3.0), color=bl["f32"], stats=stats)
    return chain("tonemap", dict(op="clamp", transfer="srgb", exposure=0.0), color=fused["f32"]), stats


def test_chain_b_open_scene_coverage_local_tone_adaptive(rtm, tmp_path):
    scene = pl.small_scene(tmp_path, pl.OPEN_SCENE, W, H, SAMPLES, SS)
    stdout = cli(tmp_path, scene, "B", *FLAGS_B, "--scopes", "--pfm", "--display-pfm")

    r = _renderer(rtm, scene)
    chain = pl.Chain(rtm, "chain B")
    out, tiles, _ = r.adaptive(0.05, want=("f32", "u8"))
    aov = r.render_aov()
    planes = r.render_mattes(4)
    depth, alpha = aov["depth"].cpu().numpy(), planes["alpha"].cpu().numpy()
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):  # the corners miss: the case is about frames that hold misses
        assert np.isposinf(depth[y, x]) and alpha[y, x] == 0.0 and aov["object"][y, x].item() == -1
    assert 0 < np.isposinf(depth).sum() < W * H and (alpha == 1.0).any()
    _is_bmp(tmp_path / "B.bmp", out["u8"])
    spp = np.repeat(np.repeat(tiles.cpu().numpy(), 8, axis=0), 8, axis=1)[:H, :W].astype(np.float32)
    _is_pfm(tmp_path / "B_spp.pfm", spp)
    ff = chain("firefly", color=out["f32"])
    mask = ff["mask"].cpu().numpy()
    assert record_of(stdout, "firefly: ") == {"clamped": int((mask == 1).sum()), "repaired": int((mask == 2).sum()), "pixels": W * H}
    _is_bmp(tmp_path / "B_firefly.bmp", ff["u8"])
    dv = chain("denoise_variance", color=ff["f32"], **aov)
    _is_bmp(tmp_path / "B_denoised_var.bmp", dv["u8"])
    _is_pfm(tmp_path / "B_variance.pfm", dv["var"])
    zf = r.focus_distance()  # the camera's target distance
    assert lines_of(stdout, "dof: ") == [f"focus {zf:.6g}, aperture 4, max radius 8"]
    df = chain("defocus", dict(focus_distance=zf), color=dv["f32"], depth=aov["depth"])
    _is_bmp(tmp_path / "B_dof.bmp", df["u8"])
    _is_pfm(tmp_path / "B.pfm", df["f32"])
    shown, stats = _local_display(chain, df["f32"])
    _display_line(stdout, "B", stats)
    _is_pfm(tmp_path / "B_display.pfm", shown["f32"])
    _is_bmp(tmp_path / "B_display.bmp", shown["u8"])
    lin = chain("scopes", dict(mode="log2", columns=W), color=df["f32"])
    disp = chain("scopes", dict(mode="code", columns=W), color=shown["f32"])
    gain = max(1, 2040 // H)
    picture = chain("scope_draw", dict(layout="luma", gain=gain), waveform=disp["waveform"])["u8"]
    line = _check_scopes(rtm, tmp_path, "B", stdout, lin, disp, picture)
    assert "exposure" not in line and read_bmp(tmp_path / "B_waveform.bmp").shape == (256, W, 3)
    assert lines_of(stdout, "waveform: ") == [f"B_waveform.bmp ({W} x 256, gain {gain}), B_scopes.json"]
    # the coverage planes: the defocused frame over the background, with the alpha of the frame as traced
    _is_pfm(tmp_path / "B_alpha.pfm", planes["alpha"])
    matte = chain("matte", dict(ids=[0, 2]), id=planes["id"], coverage=planes["coverage"])["f32"]
    _is_pfm(tmp_path / "B_matte.pfm", matte)
    assert float(matte.max().item()) > 0.0
    over = chain("composite", dict(background=BACKGROUND), color=df["f32"], alpha=planes["alpha"])
    _is_bmp(tmp_path / "B_over.bmp", over["u8"])
    undefocused = rtm.composite(dv["f32"], planes["alpha"], BACKGROUND, want=("u8",))["u8"]
    assert not np.array_equal(undefocused.cpu().numpy(), over["u8"].cpu().numpy())  # the dof does reach the composite
    over_shown, _ = _local_display(chain, over["f32"])
    _is_bmp(tmp_path / "B_over_display.bmp", over_shown["u8"])
    for name in ("B.bmp", "B_dof.bmp", "B_display.bmp", "B_over.bmp", "B_over_display.bmp", "B_matte.bmp"):
        assert read_bmp(tmp_path / name).shape == (H, W, 3), name

    # (b) Renderer.Render writes rtm_cli's bytes (no counterpart for --scopes: a run without it)
    cli(tmp_path, scene, "B2", *FLAGS_B)
    _renderer(rtm, scene).Render(str(tmp_path / "Bpy"), adaptive=0.05, firefly=True, denoise="variance", dof=True, tonemap=True,
                                 local=dict(shadows=3.0), bloom=True, mattes=dict(ids=[0, 2], background=BACKGROUND))
    files = _pair("") + _pair("_firefly") + _pair("_denoised_var") + _pair("_dof") + _pair("_display") + _pair("_over")
    files += _pair("_over_display") + ["_spp.pfm", "_variance.pfm", "_alpha.pfm", "_matte.pfm", "_matte.bmp"]
    _same_files(tmp_path, "Bpy", "B2", files)
    _same_files(tmp_path, "B", "B2", files)

    # the known difference, pinned: rtm_cli refuses --resize with any coverage flag, Render only with mattes' background
    cli(tmp_path, scene, "B3", "--resize", f"{RW}x{RH}", "--matte", "0,2", status=2)
    _renderer(rtm, scene).Render(str(tmp_path / "Bres"), resize=(RW, RH), mattes=dict(ids=[0, 2]))
    assert read_pfm(tmp_path / "Bres_matte.pfm").shape == (H, W) and read_bmp(tmp_path / "Bres_resized.bmp").shape == (RH, RW, 3)
    _is_pfm(tmp_path / "Bres_matte.pfm", matte)

    # (c) the restatements on frames that hold misses: inf depth, guides missing at the sky, zero alpha
    worst = chain.teacher_force()
    assert set(worst) == {"firefly", "denoise_variance", "defocus", "bloom", "tonemap", "tonemap_local", "scopes", "scope_draw",
                          "matte", "composite"}


# ---- Chain C: both denoisers, passes, the measuring stages -------------------------------------------------------------------
def test_chain_c_both_denoisers_passes_and_the_measuring_stages(rtm, tmp_path):
    scene = pl.small_scene(tmp_path, pl.CORNELL, W, H, SAMPLES, SS)
    cli(tmp_path, scene, "ref", "--denoise-variance", "--display", "--pfm", "--display-pfm")
    cli(tmp_path, scene, "den", "--denoise", "--display", "--pfm", "--display-pfm")
    both = ["--passes", "3", "--denoise", "--denoise-variance", "--display"]
    same = cli(tmp_path, scene, "same", *both, "--compare", "ref.pfm", "--flip", "ref_display.pfm", "--flip-map")
    # in passes the bits are the one-pass frame's through the whole chain, and of the two denoisers the variance-guided frame
    # is the last stage
    rec = record_of(same, "compare: ")
    assert rec["max_abs"] == 0 and rec["outside"] == 0 and rec["pixels"] == W * H
    assert record_of(same, "flip: ")["max"] == 0
    diff = cli(tmp_path, scene, "diff", *both, "--compare", "den.pfm", "--flip", "den_display.pfm", "--flip-map")

    r = _renderer(rtm, scene)
    chain = pl.Chain(rtm, "chain C")
    frame = _frame(r)
    last = None
    for _, out, _ in r.progressive(passes=3, want=("f32",)):
        last = out
    assert np.array_equal(words(last["f32"].cpu().numpy()), words(frame.cpu().numpy()))
    aov = r.render_aov()
    dn = chain("denoise", color=frame, **aov)
    dv = chain("denoise_variance", color=frame, **aov)
    shown_dn, shown_dv = chain("tonemap", color=dn["f32"]), chain("tonemap", color=dv["f32"])
    for stem, lin, shown in (("ref", dv, shown_dv), ("den", dn, shown_dn)):
        _is_pfm(tmp_path / f"{stem}.pfm", lin["f32"])
        _is_pfm(tmp_path / f"{stem}_display.pfm", shown["f32"])
        _is_bmp(tmp_path / f"{stem}_display.bmp", shown["u8"])
    for stem in ("same", "diff"):  # every intermediate file of the run with both
        _is_bmp(tmp_path / f"{stem}_denoised.bmp", dn["u8"])
        _is_bmp(tmp_path / f"{stem}_denoised_var.bmp", dv["u8"])
        _is_pfm(tmp_path / f"{stem}_variance.pfm", dv["var"])
        _is_bmp(tmp_path / f"{stem}_display.bmp", shown_dv["u8"])
    # the measuring stages: the line's fields are the records' of the two Python-side frames
    cmp_out = chain("compare", a=dv["f32"], b=dn["f32"])
    rec = record_of(diff, "compare: ")
    assert tuple(rec) == pl._compare_ref.FIELDS
    pl.compare_fields_agree(rec, pl.compare_record(cmp_out["result"].cpu().numpy()), "rtm_cli --compare")
    assert rec["max_abs"] > 0 and rec["outside"] > 0
    flip_out = chain("flip", a=shown_dv["f32"], b=shown_dn["f32"])
    res = pl.flip_record(flip_out["result"].cpu().numpy())
    rec = record_of(diff, "flip: ")
    assert tuple(rec) == ("mean", "max", "min", "pixels", "nonfinite", "argmax_x", "argmax_y", "weighted_median")
    assert rec == {k: res[k] for k in rec} and rec["mean"] > 0 and rec["pixels"] == W * H
    _is_pfm(tmp_path / "diff_flip.pfm", flip_out["map"])
    assert not np.any(read_pfm(tmp_path / "same_flip.pfm"))

    # (b) Renderer.Render: the frame in passes with the variance-guided denoiser, and with the plain one
    _renderer(rtm, scene).Render(str(tmp_path / "Cvar"), passes=3, denoise="variance", tonemap=True)
    _same_files(tmp_path, "Cvar", "ref", _pair("") + _pair("_denoised_var") + _pair("_display") + ["_variance.pfm"])
    _same_files(tmp_path, "Cvar", "same", _pair("") + _pair("_denoised_var") + _pair("_display") + ["_variance.pfm"])
    _renderer(rtm, scene).Render(str(tmp_path / "Cden"), denoise=True, tonemap=True)
    _same_files(tmp_path, "Cden", "den", _pair("") + _pair("_denoised") + _pair("_display"))
    _same_files(tmp_path, "den", "same", _pair("_denoised"))

    worst = chain.teacher_force()
    assert set(worst) == {"denoise", "denoise_variance", "tonemap", "compare", "flip"}


# ---- Chain D: preview under the display path ------------------------------------------------------------------------------------
FLAGS_D = ["--preview", "2", "--display", "--bloom", "--grade-exposure", "0.5"]


def test_chain_d_preview_under_the_display_path(rtm, tmp_path):
    scene = pl.small_scene(tmp_path, pl.CORNELL, W, H, SAMPLES, SS)
    stdout = cli(tmp_path, scene, "D", *FLAGS_D, "--expose-percentile", "50", "--scopes")

    r = _renderer(rtm, scene)
    chain = pl.Chain(rtm, "chain D")

    def display(frame):
        """bloom, grade, the frame's own percentile exposure, the curve."""
        gr = chain("grade", dict(exposure=0.5), color=chain("bloom", color=frame)["f32"])
        ev = rtm.scope_exposure(chain("scopes", dict(mode="log2", columns=W), color=gr["f32"])["histogram"], 50, 0.18)
        return chain("tonemap", dict(exposure=ev), color=gr["f32"]), ev

    preview = r.preview(2, want=("f32", "u8"))
    _is_bmp(tmp_path / "D_preview.bmp", preview["u8"])
    shown_p, ev_p = display(preview["f32"])
    _is_bmp(tmp_path / "D_preview_display.bmp", shown_p["u8"])
    frame = _frame(r)
    shown_f, ev_f = display(frame)
    _is_bmp(tmp_path / "D_display.bmp", shown_f["u8"])
    assert read_bmp(tmp_path / "D_preview_display.bmp").shape == read_bmp(tmp_path / "D_display.bmp").shape == (H, W, 3)
    # two lines, each stem with its own exposure, the preview's first
    assert ev_p != ev_f and ev_p != 0.0 and ev_f != 0.0
    assert lines_of(stdout, "expose-percentile: ") == [f"D_preview at 50 percent to {_num(0.18)}, exposure {_num(ev_p)}",
                                                       f"D at 50 percent to {_num(0.18)}, exposure {_num(ev_f)}"]
    lin = chain("scopes", dict(mode="log2", columns=W), color=frame)
    disp = chain("scopes", dict(mode="code", columns=W), color=shown_f["f32"])
    picture = chain("scope_draw", dict(layout="luma", gain=max(1, 2040 // H)), waveform=disp["waveform"])["u8"]
    line = _check_scopes(rtm, tmp_path, "D", stdout, lin, disp, picture, exposure=ev_f)  # the frame's exposure, not the preview's
    assert np.float32(line["exposure"]) == np.float32(ev_f) != np.float32(ev_p)

    # (b) Renderer.Render writes rtm_cli's bytes (no counterpart for --expose-percentile and --scopes: a run without them)
    cli(tmp_path, scene, "D2", *FLAGS_D)
    _renderer(rtm, scene).Render(str(tmp_path / "Dpy"), preview=2, tonemap=True, bloom=True, grade=dict(exposure=0.5))
    _same_files(tmp_path, "Dpy", "D2", _pair("") + _pair("_preview") + _pair("_preview_display") + _pair("_display"))
    _same_files(tmp_path, "D", "D2", _pair("") + _pair("_preview"))
    assert (tmp_path / "D_display.bmp").read_bytes() != (tmp_path / "D2_display.bmp").read_bytes()

    worst = chain.teacher_force()
    assert set(worst) == {"bloom", "grade", "scopes", "tonemap", "scope_draw"}
