"""What test_pipeline_gpu.py shares: the readers of the files rtm_cli and Renderer.Render write, the small scene and the CLI
launch, and STAGES, one row per stage of the post-process chain: the device call of raytracingmin_amd, the float64 NumPy
restatement of the same operation (tests/_*_ref.py) and the comparison with the bar of that stage's own GPU test.  A Chain
records every stage call it makes, inputs and outputs read back, so that each restatement can be run on the very input the
device received (teacher forcing: stage k's reference takes the device's output of stage k - 1, errors do not compound)."""
import collections
import json
import os
import subprocess

import numpy as np

import _compare_ref
import _defocus_ref
import _denoise_ref
import _denoise_var_ref
import _firefly_ref
import _flip_ref
import _grade_ref
import _lens_ref
import _local_tone_ref
import _bloom_ref
import _matte_ref
import _resize_ref
import _scope_ref
import _tonemap_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "raytracingmin_amd", "rtm_cli")
CORNELL = os.path.join(ROOT, "scenes", "cornellBoxSetting.json")
OPEN_SCENE = os.path.join(ROOT, "scenes", "settingData.json")

TOL = 1e-4  # include/rtm.h: |got - ref| <= 1e-4 max(1, |ref|), the bar of every stage's float outputs
# tests/test_compare_gpu.py: mse, rel_mse and psnr within 1e-9 relative, ssim within 1e-9 absolute
COMPARE_REL, COMPARE_SSIM_ABS = 1e-9, 1e-9
# tests/test_flip_gpu.py: mean, min and max within 1e-9 absolute; the map, rounded to float, half an ulp of [0.5, 1] more
FLIP_ABS = 1e-9
FLIP_MAP_ABS = FLIP_ABS + 2.0 ** -25
AOV_PLANES = ("depth", "normal", "albedo", "object")


# ---- files ----------------------------------------------------------------------------------------------------------------
def read_bmp(path):
    """The (H, W, 3) uint8 pixels of a 24-bit .bmp, top row first, RGB."""
    raw = open(path, "rb").read()
    off = int.from_bytes(raw[10:14], "little")
    w, h = int.from_bytes(raw[18:22], "little"), int.from_bytes(raw[22:26], "little")
    stride = (w * 3 + 3) & ~3
    rows = [np.frombuffer(raw, np.uint8, w * 3, off + y * stride).reshape(w, 3)[:, ::-1] for y in range(h)]
    return np.stack(rows[::-1])


def read_pfm(path):
    """The float32 words of a .pfm, top row first: (H, W, 3) of a "PF" file, (H, W) of a "Pf" one."""
    raw = open(path, "rb").read()
    kind, dims, scale, body = raw.split(b"\n", 3)
    w, h = (int(v) for v in dims.split())
    assert kind in (b"PF", b"Pf") and scale == b"-1.0", (kind, scale)
    shape = (h, w, 3) if kind == b"PF" else (h, w)
    assert len(body) == 4 * int(np.prod(shape)), (path, len(body), shape)
    return np.frombuffer(body, dtype="<f4").reshape(shape)[::-1]


def words(a):
    """The 32-bit words of a float32 array (or of what rounds to one): equal words are equal bits, NaN payloads included."""
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- the scene and the CLI ------------------------------------------------------------------------------------------------
def small_scene(tmp_path, scene_json, w, h, samples, ss):
    """`scene_json` with its size and sample counts rewritten, as tmp_path/small.json; returns the path."""
    scene = json.load(open(scene_json))
    scene["00 width"], scene["00 height"], scene["00 samples"], scene["00 superSamples"] = w, h, samples, ss
    small = tmp_path / "small.json"
    small.write_text(json.dumps(scene))
    return str(small)


def cli(tmp_path, scene, stem, *flags, status=0):
    """One fresh rtm_cli process in tmp_path; checks the exit status and returns stdout."""
    p = subprocess.run([CLI, "-json", scene, "--max-bounces", "8", "--out", stem] + [str(f) for f in flags], cwd=tmp_path,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == status, (p.returncode, p.stdout, p.stderr)
    return p.stdout


def lines_of(stdout, prefix):
    """The texts behind `prefix` of the lines of stdout that start with it, in order."""
    return [l[len(prefix):] for l in stdout.splitlines() if l.startswith(prefix)]


def record_of(stdout, prefix):
    """The JSON object of the one line of stdout that starts with `prefix`."""
    found = lines_of(stdout, prefix)
    assert len(found) == 1, (prefix, stdout)
    return json.loads(found[0])


def as_json(doc):
    """`doc` as json.load gives it back: tuples as lists, NumPy numbers as Python's."""
    return json.loads(json.dumps(doc))


# ---- the rows' helpers ----------------------------------------------------------------------------------------------------
def _excess(got, ref):
    return _denoise_ref.tolerance_excess(got, ref)


def _quantised(out):
    """The 8-bit store is rtm_quantise of the call's own out_f32, bit for bit."""
    assert np.array_equal(out["u8"], _tonemap_ref.quantise_u8(out["f32"]))


def _guides(i):
    return {k: i[k] for k in AOV_PLANES if k in i}


def _guide_args(i):
    return i.get("depth"), i.get("normal"), i.get("albedo"), i.get("object")


def _firefly_check(i, out, ref, p):
    assert np.array_equal(out["mask"], ref["mask"])  # the decisions are exact
    assert np.array_equal(words(out["threshold"]), words(ref["threshold"]))
    same = ref["mask"] == 0
    assert np.array_equal(words(out["f32"])[same], words(i["color"])[same])  # an unchanged pixel keeps its words
    _quantised(out)
    return _excess(out["f32"][~same], ref["out"][~same])


def _denoise_check(i, out, ref, p):
    _quantised(out)
    return _excess(out["f32"], ref)


def _denoise_var_check(i, out, ref, p):
    _quantised(out)
    return max(_excess(out["f32"], ref[0]), _excess(out["var"], ref[1]))


def _defocus_check(i, out, ref, p):
    ok = _defocus_ref.counts(i["color"], i["depth"])
    assert np.array_equal(words(out["f32"])[~ok], words(i["color"])[~ok])  # a pixel that does not count keeps its words
    assert np.all(words(out["coc"])[~ok] == 0)
    _quantised(out)
    return max(_excess(out["f32"][ok], ref[0][ok]), _excess(out["coc"], ref[1]))


def _lens_check(i, out, ref, p):
    inside = ref["inside"].reshape(out["f32"].shape)
    border = np.broadcast_to(_lens_ref.border_words(_lens_ref.with_defaults(p)["border"]), out["f32"].shape)
    assert np.array_equal(words(out["f32"])[~inside], words(border)[~inside])  # the inside mask is exact
    hole = np.isnan(ref["out"])
    assert np.array_equal(np.isnan(out["f32"]), hole)
    _quantised(out)
    return _excess(out["f32"][inside & ~hole], ref["out"][inside & ~hole])


def _resize_check(i, out, ref, p):
    hole = np.isnan(ref[0])
    assert np.array_equal(np.isnan(out["f32"]), hole)
    _quantised(out)
    return _excess(out["f32"][~hole], ref[0][~hole])


def _bloom_check(i, out, ref, p):
    ok = _bloom_ref.counts(i["color"])
    assert np.array_equal(words(out["f32"])[~ok], words(i["color"])[~ok])
    _quantised(out)
    return max(_excess(out["f32"][ok], ref[0][ok]), _excess(out["bloom"], ref[1]))


def _grade_reference(i, p):
    p = dict(p)
    if "lut" in i:
        p["lut"] = i["lut"]
    return _grade_ref.grade_ref(i["color"], **p)


def _grade_check(i, out, ref, p):
    ok = _grade_ref.counts(i["color"])
    assert np.array_equal(words(out["f32"])[~ok], words(i["color"])[~ok])
    assert np.array_equal(out["u8"], _grade_ref.quantise_u8(out["f32"]))
    return _excess(out["f32"][ok], ref[ok])


def tonemap_stats(stat_words):
    """rtm_tonemap_stats from the four words of tonemap()'s "stats"."""
    raw = np.ascontiguousarray(stat_words).view(np.uint32)
    f = raw.view(np.float32)
    return {"log_average": float(f[0]), "max_luminance": float(f[1]), "exposure": float(f[2]), "pixels": int(raw[3])}


def _tonemap_reference(i, p):
    kw = {k: v for k, v in p.items() if k != "dither"}
    return _tonemap_ref.tonemap_ref(i["color"], **kw)


def _tonemap_check(i, out, ref, p):
    stats = tonemap_stats(out["stats"])
    assert stats["pixels"] == ref[1]["pixels"]
    black = ~_tonemap_ref.counts(i["color"])
    assert np.all(out["f32"][black] == 0.0) and np.all(out["u8"][black] == 0)
    store = _tonemap_ref.dither_u8 if p.get("dither", True) else _tonemap_ref.quantise_u8
    assert np.array_equal(out["u8"], store(out["f32"]))  # the 8-bit store of the call's own out_f32, bit for bit
    return max([_excess(out["f32"], ref[0])] + [_excess(stats[k], ref[1][k]) for k in ("log_average", "max_luminance", "exposure")])


def _local_reference(i, p):
    exposure = tonemap_stats(i["stats"])["exposure"] if "stats" in i else None  # the device's own E, by stream order
    return _local_tone_ref.local_ref(i["color"], exposure=exposure, **p)


def _local_check(i, out, ref, p):
    ok = _local_tone_ref.counts(i["color"])
    assert np.all(words(out["f32"])[~ok] == 0)
    _quantised(out)
    return max(_excess(out["f32"], ref[0]), _excess(out["fused"], ref[1]))


def _scopes_reference(i, p):
    mode = _scope_ref.MODES[p.get("mode", "log2")]
    return _scope_ref.histogram(i["color"], mode), _scope_ref.waveform(i["color"], mode, p["columns"])


def _scopes_check(i, out, ref, p):
    assert np.array_equal(out["histogram"].view(np.uint32), _scope_ref.words(ref[0]))  # integer counts: exact words
    assert np.array_equal(out["waveform"].view(np.uint32), ref[1])
    return 0.0


def _draw_check(i, out, ref, p):
    assert out["u8"].shape == ref.shape and np.array_equal(out["u8"], ref)
    return 0.0


def _matte_check(i, out, ref, p):
    assert np.array_equal(words(out["f32"]), words(ref))
    return 0.0


def _composite_check(i, out, ref, p):
    assert np.array_equal(words(out["f32"]), words(ref[0])) and np.array_equal(out["u8"], ref[1])  # float32 in order: bit for bit
    return 0.0


def compare_record(result_words):
    import raytracingmin_amd as rtm
    return rtm.compare_result(np.ascontiguousarray(result_words))


def flip_record(result_words):
    import raytracingmin_amd as rtm
    return rtm.flip_result(np.ascontiguousarray(result_words))


def _rel(got, want):
    if want == got:
        return 0.0  # both +inf included
    return abs(got - want) / abs(want) if np.isfinite(want) and want != 0 else float("inf")


def compare_fields_agree(got, want, label):
    """tests/test_compare_gpu.py's rule for a compare record: the integer fields and max_abs exact, mse, rel_mse and psnr
    within 1e-9 relative, ssim within 1e-9 absolute."""
    for k in _compare_ref.EXACT:
        assert got[k] == want[k], (label, k, got[k], want[k])
    for k in ("mse", "rel_mse", "psnr"):
        assert _rel(got[k], want[k]) <= COMPARE_REL, (label, k, got[k], want[k])
    assert abs(got["ssim"] - want["ssim"]) <= COMPARE_SSIM_ABS, (label, got["ssim"], want["ssim"])


def _compare_check(i, out, ref, p):
    compare_fields_agree(compare_record(out["result"]), ref[0], "compare")
    return 0.0


def _flip_check(i, out, ref, p):
    res, (want, want_map) = flip_record(out["result"]), ref
    assert res["pixels"] == want["pixels"] and res["nonfinite"] == want["nonfinite"]
    for k in ("mean", "min", "max"):
        assert abs(res[k] - want[k]) <= FLIP_ABS, (k, res[k], want[k])
    top = np.sort(want_map[~np.isnan(want_map)].ravel())[-2:]
    if top.size < 2 or top[1] - top[0] > 2 * FLIP_ABS:  # else the reference's two largest are too close to name one
        assert (res["argmax_x"], res["argmax_y"]) == (want["argmax_x"], want["argmax_y"])
    assert np.array_equal(np.isnan(out["map"]), np.isnan(want_map))
    keep = ~np.isnan(want_map)
    err = float(np.abs(out["map"].astype(np.float64)[keep] - want_map[keep]).max()) if keep.any() else 0.0
    assert err <= FLIP_MAP_ABS, err
    assert np.array_equal(np.array(res["hist"], np.uint32), _flip_ref.histogram(out["map"]))  # exact, given its own map
    return 0.0


Stage = collections.namedtuple("Stage", "device reference compare")
# device(rtm, inputs, params): the call on device tensors, every output the comparison reads asked for.
# reference(inputs, params): the float64 restatement on the same inputs, read back to the host.
# compare(inputs, outputs, reference, params): the exact parts asserted; returns the worst error of the float parts, which the
# caller holds to TOL (0.0 of a stage that is exact throughout).
STAGES = {
    "firefly": Stage(lambda rtm, i, p: rtm.firefly(i["color"], want=("f32", "u8", "mask", "threshold"), **p),
                     lambda i, p: _firefly_ref.firefly_ref(i["color"], **p), _firefly_check),
    "denoise": Stage(lambda rtm, i, p: rtm.denoise(i["color"], _guides(i), want=("f32", "u8"), **p),
                     lambda i, p: _denoise_ref.denoise_ref(i["color"], *_guide_args(i), **p), _denoise_check),
    "denoise_variance": Stage(lambda rtm, i, p: rtm.denoise_variance(i["color"], _guides(i), want=("f32", "u8", "var"), **p),
                              lambda i, p: _denoise_var_ref.denoise_variance_ref(i["color"], *_guide_args(i), **p),
                              _denoise_var_check),
    "defocus": Stage(lambda rtm, i, p: rtm.defocus(i["color"], i["depth"], want=("f32", "u8", "coc"), **p),
                     lambda i, p: _defocus_ref.defocus_ref(i["color"], i["depth"], **p), _defocus_check),
    "lens": Stage(lambda rtm, i, p: rtm.lens(i["color"], want=("f32", "u8"), **p),
                  lambda i, p: _lens_ref.lens_ref(i["color"], **p), _lens_check),
    "resize": Stage(lambda rtm, i, p: rtm.resize(i["color"], want=("f32", "u8"), **p),
                    lambda i, p: _resize_ref.resize_ref(i["color"], **p), _resize_check),
    "bloom": Stage(lambda rtm, i, p: rtm.bloom(i["color"], want=("f32", "u8", "bloom"), **p),
                   lambda i, p: _bloom_ref.bloom_ref(i["color"], **p), _bloom_check),
    "grade": Stage(lambda rtm, i, p: rtm.grade(i["color"], lut=i.get("lut"), want=("f32", "u8"), **p), _grade_reference, _grade_check),
    "tonemap": Stage(lambda rtm, i, p: rtm.tonemap(i["color"], want=("f32", "u8", "stats"), **p), _tonemap_reference, _tonemap_check),
    "tonemap_local": Stage(lambda rtm, i, p: rtm.tonemap_local(i["color"], stats=i.get("stats"), want=("f32", "u8", "fused"), **p),
                           _local_reference, _local_check),
    "scopes": Stage(lambda rtm, i, p: rtm.scopes(i["color"], want=("histogram", "waveform"), **p), _scopes_reference, _scopes_check),
    "scope_draw": Stage(lambda rtm, i, p: {"u8": rtm.scope_draw(i["waveform"], **p)},
                        lambda i, p: _scope_ref.draw(i["waveform"].view(np.uint32), _scope_ref.LAYOUTS[p.get("layout", "luma")],
                                                     p.get("gain", 1)), _draw_check),
    "matte": Stage(lambda rtm, i, p: {"f32": rtm.matte(i["id"], i["coverage"], **p)},
                   lambda i, p: _matte_ref.matte(i["id"], i["coverage"], **p), _matte_check),
    "composite": Stage(lambda rtm, i, p: rtm.composite(i["color"], i["alpha"], want=("f32", "u8"), **p),
                       lambda i, p: _matte_ref.composite(i["color"], i["alpha"], **p), _composite_check),
    "compare": Stage(lambda rtm, i, p: rtm.compare(i["a"], i["b"], want=("result",), **p),
                     lambda i, p: _compare_ref.compare_ref(i["a"], i["b"], **p), _compare_check),
    "flip": Stage(lambda rtm, i, p: rtm.flip(i["a"], i["b"], want=("result", "map"), **p),
                  lambda i, p: _flip_ref.flip_ref(i["a"], i["b"], **p), _flip_check),
}


# the rows whose comparison is exact (integer counts, float32 arithmetic in a fixed order) or has bars of its own (compare, flip)
EXACT_STAGES = ("scopes", "scope_draw", "matte", "composite", "compare", "flip")


class Chain:
    """The Python side of one chain: chain(stage, params, **inputs) makes the stage's device call, reads its inputs and outputs
    back and keeps them; teacher_force() then holds every call to its row's restatement."""

    def __init__(self, rtm, label):
        self.rtm, self.label, self.calls = rtm, label, []

    def __call__(self, stage, params=None, **inputs):
        import torch
        params = dict(params or {})
        inputs = {k: v for k, v in inputs.items() if v is not None}
        out = STAGES[stage].device(self.rtm, inputs, params)
        torch.cuda.synchronize()
        host = lambda d: {k: v.cpu().numpy().copy() for k, v in d.items()}
        self.calls.append((stage, host(inputs), params, host(out)))
        return out

    def host(self, index=-1):
        """The outputs of a recorded call, on the host."""
        return self.calls[index][3]

    def teacher_force(self):
        """Every recorded call against its restatement, on the input the device took; prints and returns the worst error per
        stage, each held to TOL."""
        worst = {}
        for n, (stage, inputs, params, out) in enumerate(self.calls):
            row = STAGES[stage]
            err = row.compare(inputs, out, row.reference(inputs, params), params)
            assert err <= TOL, (self.label, n, stage, params, err)
            worst[stage] = max(worst.get(stage, 0.0), err)
        for stage, err in worst.items():
            count = sum(1 for c in self.calls if c[0] == stage)
            figure = "exact, or within its own test's bars" if stage in EXACT_STAGES else f"{err:.3e} (bar {TOL})"
            print(f"{self.label} {stage} ({count} call{'s' if count > 1 else ''}): worst error against the float64 reference {figure}")
        return worst
