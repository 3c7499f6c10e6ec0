"""What the grade stage costs (rtm_grade), beside a device-to-device copy of the frame it reads.

A 1920 x 1080 x 3 float frame in [0, 1), once as seeded random pixels (every pixel falls into a cell of the LUT unrelated to
its neighbour's: the worst case for the gather) and once as a smooth ramp (neighbouring pixels in neighbouring cells, what an
image is like).  Cases: the matrix only (white balance at 3200 K), the full parametric grade (matrix, exposure, contrast, CDL
with three powers, saturation: all three pow sites), a LUT alone at 17^3, 33^3 and 65^3 in both interpolations (a smooth
table; its values do not change the addresses), and everything (the full parametric grade, then the 33^3 LUT, tetrahedral).
The C entry point is called with buffers allocated once (out_f32 only), so a timing holds the call's one launch and nothing
else.  Each case is warmed up, then timed with device events around --launches back-to-back calls, 7 times: the per-call times
of every window are recorded with their median.  A torch device-to-device copy of the same frame (24.9 MB read, as many
written) is timed in the same run in the same way, and every case is also given as a multiple of it: a copy is the least a
stage that reads the frame once and writes it once could cost.  The output bytes of the last call of every case are checked
against those of the first.
Every step (the copy, each case) runs under a time limit of its own: an alarm whose default action ends the process, so a
step that hangs starts nothing more on the device.  Nothing is asserted about the times: there is no earlier implementation
to beat; DESIGN.md reads them.  Writes one JSON object to --out and prints it.

    python profiles/grade_pass.py [--launches 20] [--step-limit 60] [--head SHA] [--out profiles/grade_pass.json]
"""
import argparse
import ctypes as C
import json
import os
import signal
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H = 1920, 1080
WINDOWS = 7
PARAMETRIC = dict(exposure=0.5, contrast=1.3, pivot=0.18, slope=(1.1, 0.9, 1.05), offset=(0.01, -0.02, 0.0), power=(0.8, 1.2, 2.2),
                  saturation=1.3)


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


def smooth_table(n):
    """A smooth look on [0, 1]^3, (N, N, N, 3) float32 indexed [b][g][r]."""
    k = np.arange(n, dtype=np.float64) / (n - 1)
    b, g, r = np.meshgrid(k, k, k, indexing="ij")
    x = np.stack([r, g, b], axis=-1)
    return (x * x * (3.0 - 2.0 * x)).astype(np.float32)


def measure(rtm, src, prm, lut, launches):
    """One case: (the per-call ms of every window, whether the bits held)."""
    import torch
    from raytracingmin_amd import _lib
    L = rtm.lib()
    dev = src.device
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out32 = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
    lut_ptr = lut.data_ptr() if lut is not None else None

    def call():
        _lib.check(L.rtm_grade(C.byref(prm), W, H, dev.index, src.data_ptr(), lut_ptr, out32.data_ptr(), None, stream), "rtm_grade")

    call()
    first = out32.cpu().numpy().copy()
    ms = windows(call, launches)
    same = np.array_equal(out32.cpu().numpy().view(np.uint32), first.view(np.uint32))
    return ms, bool(same)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--step-limit", type=int, default=60, help="seconds a step may take before the process is ended")
    ap.add_argument("--head", default=None, help="the tree's HEAD, when the tree is a copy without its repository")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grade_pass.json"))
    args = ap.parse_args()
    import torch
    import raytracingmin_amd as rtm
    from raytracingmin_amd import renderer
    if not torch.cuda.is_available():
        sys.exit("grade_pass.py needs a HIP device: nothing is measured without one")
    dev = torch.device("cuda", 0)
    signal.alarm(args.step_limit)
    gen = torch.Generator(device=dev)
    gen.manual_seed(W * 65536 + H)
    xs = torch.arange(W, dtype=torch.float32, device=dev)[None, :].expand(H, W)
    ys = torch.arange(H, dtype=torch.float32, device=dev)[:, None].expand(H, W)
    frames = {"random": torch.rand((H, W, 3), generator=gen, dtype=torch.float32, device=dev),
              "smooth": torch.stack([xs / W, ys / H, (xs + ys) / (W + H)], dim=-1).contiguous()}
    dst = torch.empty_like(frames["random"])
    cp = windows(lambda: dst.copy_(frames["random"]), args.launches)
    copy_median = statistics.median(cp)
    matrix = rtm.white_balance(3200)
    tables = {n: torch.from_numpy(smooth_table(n)).to(dev) for n in (17, 33, 65)}
    todo = [("matrix only", dict(matrix=matrix), 0, None), ("full parametric", dict(PARAMETRIC, matrix=matrix), 0, None)]
    for n in (17, 33, 65):
        for interp in renderer.GRADE_INTERPS:
            todo.append((f"lut {n} {interp}", dict(interp=interp), n, tables[n]))
    todo.append(("everything", dict(PARAMETRIC, matrix=matrix, interp="tetrahedral"), 33, tables[33]))
    cases, ok = [], True
    for name, kw, n, lut in todo:
        for kind, src in frames.items():
            signal.alarm(args.step_limit)  # this step's own limit
            prm = renderer._grade_params(lut_size=n, **kw)
            ms, same = measure(rtm, src, prm, lut, args.launches)
            ok = ok and same
            med = statistics.median(ms)
            cases.append({"case": name, "frame": kind, "lut_bytes": 12 * n ** 3, "call_ms": [round(v, 4) for v in ms],
                          "call_ms_median": round(med, 4), "call_ms_min": round(min(ms), 4), "copies": round(med / copy_median, 3),
                          "identical": same})
    signal.alarm(0)
    out = {"config": f"a {W}x{H}x3 frame in [0, 1), seeded random pixels or a smooth ramp, out_f32 only; rtm_grade (one launch a call) per "
                     "case, and a device-to-device copy of the frame; device ms per call over windows of "
                     f"{args.launches} calls, {WINDOWS} windows after a warm-up of 3 calls; `copies`: the median over the copy's",
           "head": args.head or head_of_tree(),
           "device": torch.cuda.get_device_name(0),
           "frame_bytes": 12 * W * H,
           "copy_ms": [round(v, 4) for v in cp], "copy_ms_median": round(copy_median, 4),
           "copy_gbytes_per_s": round(2 * 12 * W * H / copy_median * 1e-6, 1),
           "cases": cases,
           "identical": bool(ok)}
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out), flush=True)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
