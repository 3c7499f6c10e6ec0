"""What the firefly stage costs (rtm_firefly), beside a device-to-device copy of the frame it reads, and what its defaults do
to the Cornell box.

A 1920 x 1080 x 3 float frame: a smooth ramp with seeded noise and one spike in a thousand pixels.  Cases: the defaults
(radius 1, rank 3); the heaviest instantiation (radius 3, rank 8); the defaults on the same frame with 1 % of its pixels made
non-finite and repair on.  The C entry point is called with buffers allocated once (out_f32 only), so a timing holds the
call's one launch and nothing else.  Each case is warmed up, then timed with device events around --launches back-to-back
calls, 7 times: the per-call times of every window are recorded with their median.  A torch device-to-device copy of the same
frame (24.9 MB read, as many written) is timed in the same run in the same way, and every case is also given as a multiple
of it: a copy is the least a stage that reads the frame once and writes it once could cost.  The output bytes of the last
call of every case are checked against those of the first.
Then scenes/cornellBoxSetting.json at its own size through rtm_cli --firefly at 16 and at 1024 samples per pixel: the line
rtm_cli prints, and, from the same render in this process, how many of the clamped pixels show the light (the object plane of
render_aov names the object every pixel sees first).
Every step (the copy, each case, each render) runs under a time limit of its own: an alarm whose default action ends the
process, so a step that hangs starts nothing more on the device.  Nothing is asserted about the times: there is no earlier
implementation to beat; DESIGN.md reads them.  Writes one JSON object to --out and prints it.

    python profiles/firefly_pass.py [--launches 20] [--step-limit 120] [--head SHA] [--out profiles/firefly_pass.json]
"""
import argparse
import ctypes as C
import json
import os
import signal
import statistics
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H = 1920, 1080
WINDOWS = 7
SCENE = os.path.join(ROOT, "scenes", "cornellBoxSetting.json")
CLI = os.path.join(ROOT, "raytracingmin_amd", "rtm_cli")


def head_of_tree():
    try:
        return subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        return "unknown"


def windows(fn, launches):
    """Per-call ms of WINDOWS windows of `launches` back-to-back calls, after a warm-up of three calls."""
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(WINDOWS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / launches)
    return out


def measure(rtm, src, prm, launches):
    """One case: (the per-call ms of every window, whether the bits held, the mask's counts)."""
    import torch
    from raytracingmin_amd import _lib
    L = rtm.lib()
    dev = src.device
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out32 = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
    mask = torch.empty((H, W), dtype=torch.uint8, device=dev)

    def call(m=None):
        _lib.check(L.rtm_firefly(C.byref(prm), W, H, dev.index, src.data_ptr(), out32.data_ptr(), None, m, None, stream), "rtm_firefly")

    call(mask.data_ptr())  # once with the mask, for the counts; the timed calls write out_f32 only
    first = out32.cpu().numpy().copy()
    counts = {"clamped": int((mask == 1).sum().item()), "repaired": int((mask == 2).sum().item())}
    ms = windows(call, launches)
    same = np.array_equal(out32.cpu().numpy().view(np.uint32), first.view(np.uint32))
    return ms, bool(same), counts


def cornell(rtm, spp, limit):
    """rtm_cli --firefly on the Cornell box at `spp`, and the same render here: the line's counts, and the clamped pixels
    whose first hit is an emitter."""
    import torch
    with tempfile.TemporaryDirectory() as tmp:
        p = subprocess.run([CLI, "-json", SCENE, "--spp", str(spp), "--firefly", "--out", "cornell"], cwd=tmp, capture_output=True,
                           text=True, timeout=limit)
    if p.returncode != 0:
        sys.exit(f"rtm_cli --firefly at {spp} spp failed: {p.stdout}{p.stderr}")
    line = [l for l in p.stdout.splitlines() if l.startswith("firefly: ")][0]
    cli = json.loads(line[len("firefly: "):])
    data = rtm.LoadData(SCENE).data
    data.samples = max(1, spp // (data.superSamples * data.superSamples))  # rtm_cli's --spp
    r = rtm.Renderer(data)  # rtm_cli's defaults: repaired, unlimited bounces, seed 0x5EED, host trig
    out, _ = r.render_rows_device(0, data.height, want=("f64",))
    f32 = out["f64"].to(torch.float32)
    mask = rtm.firefly(f32, want=("mask",))["mask"]
    obj = r.render_aov(want=("object",))["object"]
    lights = [i for i, o in enumerate(data.object) if any(float(e) > 0 for e in o.m_material.emission)]
    on_light = torch.zeros_like(mask, dtype=torch.bool)
    for i in lights:
        on_light |= obj == i
    here = {"clamped": int((mask == 1).sum().item()), "repaired": int((mask == 2).sum().item()), "pixels": int(mask.numel())}
    return {"spp": data.samples * data.superSamples ** 2, "width": data.width, "height": data.height, "cli": cli, "python": here,
            "cli_equals_python": cli == here, "light_objects": lights, "light_pixels": int(on_light.sum().item()),
            "light_pixels_clamped": int(((mask == 1) & on_light).sum().item())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--step-limit", type=int, default=120, help="seconds a step may take before the process is ended")
    ap.add_argument("--head", default=None, help="the tree's HEAD, when the tree is a copy without its repository")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "firefly_pass.json"))
    args = ap.parse_args()
    import torch
    import raytracingmin_amd as rtm
    from raytracingmin_amd import renderer
    if not torch.cuda.is_available():
        sys.exit("firefly_pass.py needs a HIP device: nothing is measured without one")
    dev = torch.device("cuda", 0)
    signal.alarm(args.step_limit)
    gen = torch.Generator(device=dev)
    gen.manual_seed(W * 65536 + H)
    xs = torch.arange(W, dtype=torch.float32, device=dev)[None, :].expand(H, W)
    ys = torch.arange(H, dtype=torch.float32, device=dev)[:, None].expand(H, W)
    ramp = torch.stack([0.2 + xs / W, 0.2 + ys / H, 0.2 + (xs + ys) / (W + H)], dim=-1)
    clean = (ramp * (0.95 + 0.1 * torch.rand((H, W, 3), generator=gen, dtype=torch.float32, device=dev))).contiguous()
    spikes = torch.rand((H, W), generator=gen, device=dev) < 1e-3
    clean[spikes] *= 200.0
    holes = clean.clone()
    holes[torch.rand((H, W), generator=gen, device=dev) < 1e-2] = float("nan")
    dst = torch.empty_like(clean)
    cp = windows(lambda: dst.copy_(clean), args.launches)
    copy_median = statistics.median(cp)
    todo = [("defaults", clean, dict()), ("radius 3, rank 8", clean, dict(radius=3, rank=8)),
            ("defaults, 1 % non-finite, repair on", holes, dict(repair=True))]
    cases, ok = [], True
    for name, src, kw in todo:
        signal.alarm(args.step_limit)  # this step's own limit
        prm = renderer._firefly_params(**kw)
        ms, same, counts = measure(rtm, src, prm, args.launches)
        ok = ok and same
        med = statistics.median(ms)
        cases.append({"case": name, "radius": prm.radius, "rank": prm.rank, "call_ms": [round(v, 4) for v in ms],
                      "call_ms_median": round(med, 4), "call_ms_min": round(min(ms), 4), "copies": round(med / copy_median, 3),
                      "clamped": counts["clamped"], "repaired": counts["repaired"], "identical": same})
    renders = []
    for spp in (16, 1024):
        signal.alarm(args.step_limit)
        renders.append(cornell(rtm, spp, args.step_limit))
    signal.alarm(0)
    out = {"config": f"a {W}x{H}x3 frame, a smooth ramp with seeded noise and one spike in a thousand pixels, out_f32 only; rtm_firefly "
                     "(one launch a call) per case, and a device-to-device copy of the frame; device ms per call over windows of "
                     f"{args.launches} calls, {WINDOWS} windows after a warm-up of 3 calls; `copies`: the median over the copy's",
           "head": args.head or head_of_tree(),
           "device": torch.cuda.get_device_name(0),
           "frame_bytes": 12 * W * H,
           "copy_ms": [round(v, 4) for v in cp], "copy_ms_median": round(copy_median, 4),
           "copy_gbytes_per_s": round(2 * 12 * W * H / copy_median * 1e-6, 1),
           "cases": cases,
           "cornell": renders,
           "identical": bool(ok)}
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out), flush=True)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
