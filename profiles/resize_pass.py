"""What a resize costs (rtm_resize), beside a device copy of the bytes it has to move.

A seeded random float frame (the stage does not care what its input shows), C = 3, at three size pairs a user would run:
1920x1080 -> 960x540, 1920x1080 -> 3840x2160 and 3840x2160 -> 1920x1080, each with the four filters.  The C entry point is
called with buffers allocated once (out_f32 only), so a timing holds the call's three launches and nothing else.  Each case is
warmed up, then timed with device events around --launches back-to-back calls, --reps times: the per-call times of every
window are recorded with their minimum and median.  Next to the whole call, the same source resized along x only and along y
only (the other axis at equal size), which says which pass the time goes to.
The bytes a call must move: the source once (12 w h), the records written and read (2 x 16 W h), the output (12 W H); tables
and j0 arrays are a few KiB.  A torch device-to-device copy that moves the same number of bytes (half of them read, half
written) is timed in the same run in the same way; `copy_rate_fraction` is the copy's time over the call's: the share of the
copy's byte rate the call reaches.  The output bytes of the last call of every case are checked against those of the first.
Nothing is asserted about the times: there is no earlier implementation to beat.  Writes one JSON object to --out and prints it.

    python profiles/resize_pass.py [--reps 5] [--launches 50] [--head SHA] [--out profiles/resize_pass.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PAIRS = (("1080p_to_540p", (1920, 1080), (960, 540)), ("1080p_to_4k", (1920, 1080), (3840, 2160)),
         ("4k_to_1080p", (3840, 2160), (1920, 1080)))


def head_of_tree():
    try:
        return subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        return "unknown"


def windows(fn, launches, reps):
    """Per-call ms of `reps` windows of `launches` back-to-back calls, after a warm-up of three calls."""
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / launches)
    return out


def measure(rtm, src, size, which, launches, reps):
    """One call shape: (the per-call ms of every window, the bytes the call must move, whether the bits held)."""
    import torch
    from raytracingmin_amd import _lib
    L = rtm.lib()
    h, w = int(src.shape[0]), int(src.shape[1])
    W, H = size
    dev = src.device
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out32 = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
    work = torch.empty(L.rtm_resize_work_bytes(w, h, W, H, which, 3), dtype=torch.uint8, device=dev)
    prm = _lib.rtm_resize_params(which, 3)

    def call():
        _lib.check(L.rtm_resize(C.byref(prm), w, h, W, H, dev.index, src.data_ptr(), work.data_ptr(), out32.data_ptr(), None, stream),
                   "rtm_resize")

    call()
    first = out32.cpu().numpy().copy()
    ms = windows(call, launches, reps)
    same = np.array_equal(out32.cpu().numpy().view(np.uint32), first.view(np.uint32))
    return ms, 12 * w * h + 2 * 16 * W * h + 12 * W * H, bool(same)


def copy_ms(nbytes, dev, launches, reps):
    """A device copy that moves nbytes in all: nbytes / 2 read and as many written."""
    import torch
    a = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
    b = torch.empty_like(a)
    a.zero_()
    return windows(lambda: b.copy_(a), launches, reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--head", default=None, help="the tree's HEAD, when the tree is a copy without its repository")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resize_pass.json"))
    args = ap.parse_args()
    import torch
    import raytracingmin_amd as rtm
    from raytracingmin_amd import _lib
    dev = torch.device("cuda", 0)
    cases, ok = [], True
    for name, (w, h), (W, H) in PAIRS:
        gen = torch.Generator(device=dev)
        gen.manual_seed(w * 65536 + h)
        src = torch.rand((h, w, 3), generator=gen, dtype=torch.float32, device=dev) * 4.0
        for which, filt in enumerate(_lib.RESIZE_FILTERS):
            ms, nbytes, same = measure(rtm, src, (W, H), which, args.launches, args.reps)
            ms_x, _, same_x = measure(rtm, src, (W, h), which, args.launches, args.reps)
            ms_y, _, same_y = measure(rtm, src, (w, H), which, args.launches, args.reps)
            cp = copy_ms(nbytes, dev, args.launches, args.reps)
            ok = ok and same and same_x and same_y
            cases.append({"case": name, "source": f"{w}x{h}", "destination": f"{W}x{H}", "filter": filt,
                          "call_ms": [round(v, 4) for v in ms], "call_ms_min": round(min(ms), 4),
                          "call_ms_median": round(statistics.median(ms), 4),
                          "x_only_ms_min": round(min(ms_x), 4), "y_only_ms_min": round(min(ms_y), 4),
                          "bytes_moved": nbytes, "gbytes_per_s": round(nbytes / min(ms) * 1e-6, 1),
                          "copy_ms_min": round(min(cp), 4), "copy_gbytes_per_s": round(nbytes / min(cp) * 1e-6, 1),
                          "copy_rate_fraction": round(min(cp) / min(ms), 3)})
    out = {"config": "a seeded random frame, C = 3, out_f32 only; rtm_resize (three launches a call) per size pair and filter, the "
                     "same along x only and along y only, and a device copy that moves the same bytes; device ms per call over "
                     f"windows of {args.launches} calls, {args.reps} windows after a warm-up of 3 calls",
           "head": args.head or head_of_tree(),
           "device": torch.cuda.get_device_name(0),
           "cases": cases,
           "identical": bool(ok)}
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out), flush=True)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
