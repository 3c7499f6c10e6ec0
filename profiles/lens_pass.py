"""What the lens stage costs (rtm_lens), beside a device-to-device copy of the frame it reads.

A seeded random 1920 x 1080 x 3 float frame (the stage does not care what its input shows), at k1 = -0.2, k2 = 0.03, for every
filter x mode x chroma in {0, 0.01}: the instantiations of the kernel and both position paths (NEAREST takes no chroma: those
two cases are recorded as refused).  The C entry point is called with buffers allocated once (out_f32 only), so a timing holds
the call's one launch and nothing else.  Each case is warmed up, then timed with device events around --launches back-to-back
calls, 7 times: the per-call times of every window are recorded with their median.  A torch device-to-device copy of the same
frame (24.9 MB read, as many written) is timed in the same run in the same way, and every case is also given as a multiple of
it: a copy is the least a stage that reads the frame once and writes it once could cost.  The output bytes of the last call of
every case are checked against those of the first.
Every step (the copy, each case) runs under a time limit of its own: an alarm whose default action ends the process, so a
step that hangs starts nothing more on the device.  Nothing is asserted about the times: there is no earlier implementation
to beat; DESIGN.md reads them.  Writes one JSON object to --out and prints it.

    python profiles/lens_pass.py [--launches 20] [--step-limit 60] [--head SHA] [--out profiles/lens_pass.json]
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
K1, K2 = -0.2, 0.03
WINDOWS = 7


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
    """One case: (the per-call ms of every window, whether the bits held, how many channels lie outside the frame)."""
    import torch
    from raytracingmin_amd import _lib
    L = rtm.lib()
    dev = src.device
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out32 = torch.empty((H, W, 3), dtype=torch.float32, device=dev)

    def call():
        _lib.check(L.rtm_lens(C.byref(prm), W, H, dev.index, src.data_ptr(), out32.data_ptr(), None, stream), "rtm_lens")

    call()
    first = out32.cpu().numpy().copy()
    ms = windows(call, launches)
    same = np.array_equal(out32.cpu().numpy().view(np.uint32), first.view(np.uint32))
    return ms, bool(same), int((first == -7.0).sum())  # the border of these cases is -7, which no filter makes of [0, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--step-limit", type=int, default=60, help="seconds a step may take before the process is ended")
    ap.add_argument("--head", default=None, help="the tree's HEAD, when the tree is a copy without its repository")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lens_pass.json"))
    args = ap.parse_args()
    import torch
    import raytracingmin_amd as rtm
    from raytracingmin_amd import _lib, renderer
    if not torch.cuda.is_available():
        sys.exit("lens_pass.py needs a HIP device: nothing is measured without one")
    dev = torch.device("cuda", 0)
    signal.alarm(args.step_limit)
    gen = torch.Generator(device=dev)
    gen.manual_seed(W * 65536 + H)
    src = torch.rand((H, W, 3), generator=gen, dtype=torch.float32, device=dev) * 4.0
    dst = torch.empty_like(src)
    cp = windows(lambda: dst.copy_(src), args.launches)
    copy_median = statistics.median(cp)
    cases, ok = [], True
    for filt in _lib.LENS_FILTERS:
        for mode in _lib.LENS_MODES:
            for chroma in (0.0, 0.01):
                case = {"filter": filt, "mode": mode, "chroma": chroma}
                if filt == "nearest" and chroma != 0.0:
                    case["refused"] = "NEAREST copies words: it takes no chroma"
                    cases.append(case)
                    continue
                signal.alarm(args.step_limit)  # this step's own limit
                prm = renderer._lens_params(3, k1=K1, k2=K2, chroma=chroma, mode=mode, filter=filt, border=-7.0)
                ms, same, outside = measure(rtm, src, prm, args.launches)
                ok = ok and same
                med = statistics.median(ms)
                case.update({"call_ms": [round(v, 4) for v in ms], "call_ms_median": round(med, 4), "call_ms_min": round(min(ms), 4),
                             "copies": round(med / copy_median, 3), "border_channels": outside, "identical": same})
                cases.append(case)
    signal.alarm(0)
    out = {"config": f"a seeded random {W}x{H}x3 frame, out_f32 only, k1 {K1}, k2 {K2}, zoom 1; rtm_lens (one launch a call) per filter, "
                     "mode and chroma, and a device-to-device copy of the frame; device ms per call over windows of "
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
