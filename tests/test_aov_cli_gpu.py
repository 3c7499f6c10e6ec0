"""rtm_cli --aov on a real MI355X (-m gpu): the five files next to --out, PFMs equal to Renderer.render_aov, the image
unchanged, and the multi-GPU flags refused."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "raytracingmin_amd", "rtm_cli")
SCENE = os.path.join(ROOT, "scenes", "cornellBoxSetting.json")
ARGS = ["-json", SCENE, "--width", "64", "--height", "40", "--samples", "4", "--superSamples", "2", "--max-bounces", "8"]


def _run(args, cwd):
    return subprocess.run([CLI] + args, cwd=cwd, capture_output=True, text=True, timeout=300)


def _read_pfm(path):
    raw = open(path, "rb").read()
    kind, dims, scale, body = raw.split(b"\n", 3)
    w, h = (int(v) for v in dims.split())
    assert scale == b"-1.0"
    comp = {b"PF": 3, b"Pf": 1}[kind]
    return np.frombuffer(body, dtype="<f4").reshape(h, w, comp)[::-1].squeeze(-1 if comp == 1 else ())


def test_cli_aov_writes_five_files_equal_to_render_aov(tmp_path):
    import torch
    import raytracingmin_amd as rtm
    plain = _run(ARGS + ["--out", "plain"], tmp_path)
    assert plain.returncode == 0, plain.stderr
    r = _run(ARGS + ["--out", "with", "--aov"], tmp_path)
    assert r.returncode == 0, r.stderr
    for k in ("depth.pfm", "normal.pfm", "albedo.pfm", "normal.bmp", "albedo.bmp"):
        assert (tmp_path / f"with_{k}").stat().st_size > 0, k
    assert (tmp_path / "plain.bmp").read_bytes() == (tmp_path / "with.bmp").read_bytes()
    assert (tmp_path / "plain.jpg").read_bytes() == (tmp_path / "with.jpg").read_bytes()
    data = rtm.LoadData(SCENE).data
    data.width, data.height, data.samples, data.superSamples = 64, 40, 4, 2
    ren = rtm.Renderer(data, mode="repaired", max_bounces=8)
    want = ren.render_aov()
    torch.cuda.synchronize()
    for k in ("depth", "normal", "albedo"):
        got = _read_pfm(tmp_path / f"with_{k}.pfm")
        assert np.array_equal(got.view(np.uint32), want[k].cpu().numpy().view(np.uint32)), k
    # the Python writer gives the same five files
    ren.write_aov(str(tmp_path / "py"))
    for k in ("depth.pfm", "normal.pfm", "albedo.pfm", "normal.bmp", "albedo.bmp"):
        assert (tmp_path / f"py_{k}").read_bytes() == (tmp_path / f"with_{k}").read_bytes(), k


def test_cli_aov_combines_with_passes(tmp_path):
    r = _run(ARGS + ["--out", "p", "--aov", "--passes", "3"], tmp_path)
    assert r.returncode == 0, r.stderr
    assert "pass 3/3" in r.stdout
    assert (tmp_path / "p_normal.pfm").exists()


@pytest.mark.parametrize("flags", [["--gpus", "2"], ["--virtual-strips", "2"], ["--force-rccl"]])
def test_cli_aov_refuses_multi_gpu_flags(tmp_path, flags):
    r = _run(ARGS + ["--out", "x", "--aov"] + flags, tmp_path)
    assert r.returncode == 2
    assert "--aov" in r.stderr
    assert not (tmp_path / "x_depth.pfm").exists()
