"""What the frame scopes cost (rtm_scopes), beside a device-to-device copy of the frame they read.

Three 1920 x 1080 x 3 float frames: seeded noise spread over many bins (2^-12 .. 2^12), a constant frame (every lane of every
wave hits one bin per channel: the worst contention), and the Cornell box rendered at that size.  Each frame is measured for
the histogram only, the waveform only (256 columns) and both, in LOG2 mode.  The C entry point is called with buffers
allocated once, so a timing holds the call's zeroing and its one launch and nothing else.  Each case is warmed up, then timed
with device events around --launches back-to-back calls, 7 times: the per-call times of every window are recorded with their
median.  A torch device-to-device copy of the same frame (24.9 MB read, as many written) is timed in the same run in the same
way, and every case is also given as a multiple of it: a copy is the floor of anything that reads the frame once.  The words
of the last call of every case are checked against those of the first, and the histogram against a torch restatement of the
binning rule.
Every step (the copy, each frame's cases, the render) runs under a time limit of its own: an alarm whose default action ends
the process, so a step that hangs starts nothing more on the device.  Nothing is asserted about the times: there is no earlier
implementation to beat; DESIGN.md reads them.  --ab LABEL=FILE embeds the cases of another run of this script (another build
of the kernel, loaded through RTM_LIB_OVERRIDE) under "ab", so that the record of an A/B outlives the switch that made it.
Writes one JSON object to --out and prints it.

    python profiles/scopes_pass.py [--launches 20] [--step-limit 120] [--head SHA] [--label TEXT] [--ab LABEL=FILE ...]
                                   [--out profiles/scopes_pass.json]
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
COLUMNS = 256
WINDOWS = 7
SCENE = os.path.join(ROOT, "scenes", "cornellBoxSetting.json")


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


def torch_histogram(src):
    """The LOG2 histogram's 1032 count words and (pixels, not_counting) by torch, from the bit pattern."""
    import torch
    counts = torch.isfinite(src).all(dim=2)
    r, g, b = src[..., 0], src[..., 1], src[..., 2]
    l = (0.2126 * r + 0.7152 * g) + 0.0722 * b
    y = torch.where(l > 0, l, torch.zeros_like(l))
    words = []
    below, above = [], []
    for v in (y, r, g, b):
        u = v[counts].contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
        top = u >> 20
        low = (top >= 2048) | (top < 888)
        slot = top - 888
        high = ~low & (slot > 255)
        words.append(torch.bincount(slot[~low & ~high], minlength=256))
        below.append(int(low.sum().item()))
        above.append(int(high.sum().item()))
    bins = torch.stack(words).cpu().numpy().astype(np.uint32).reshape(-1)
    return np.concatenate([bins, np.array(below + above, np.uint32)]), int(counts.sum().item()), int((~counts).sum().item())


def measure(rtm, src, launches):
    """One frame: per output set, the per-call ms of every window; whether the words held and agree with torch."""
    import torch
    from raytracingmin_amd import _lib
    L = rtm.lib()
    dev = src.device
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    prm = _lib.rtm_scope_params(_lib.SCOPE_MODES["log2"], COLUMNS)
    hist = torch.empty(C.sizeof(_lib.rtm_scope_histogram) // 4, dtype=torch.int32, device=dev)
    wave = torch.empty((4, 256, COLUMNS), dtype=torch.int32, device=dev)
    want_words, pixels, not_counting = torch_histogram(src)
    out, ok = {}, True
    for name, h, w in (("histogram", hist, None), ("waveform", None, wave), ("both", hist, wave)):
        def call():
            _lib.check(L.rtm_scopes(C.byref(prm), W, H, dev.index, src.data_ptr(), h.data_ptr() if h is not None else None,
                                    w.data_ptr() if w is not None else None, stream), "rtm_scopes")
        call()
        first = [t.cpu().numpy().copy() for t in (h, w) if t is not None]
        ms = windows(call, launches)
        same = all(np.array_equal(t.cpu().numpy(), f) for t, f in zip([t for t in (h, w) if t is not None], first))
        if h is not None:
            got = h.cpu().numpy().view(np.uint32)
            same = same and np.array_equal(got[:1032], want_words) and (int(got[1032]), int(got[1033])) == (pixels, not_counting)
        if w is not None:
            rows = w.cpu().numpy().view(np.uint32).astype(np.int64).sum(axis=2).reshape(-1)
            expect = want_words[:1024].astype(np.int64).reshape(4, 256).copy()
            expect[:, 0] += want_words[1024:1028]
            expect[:, 255] += want_words[1028:1032]
            same = same and np.array_equal(rows, expect.reshape(-1))
        ok = ok and bool(same)
        out[name] = ms
    return out, ok, int(np.count_nonzero(want_words[:256])), pixels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--step-limit", type=int, default=120, help="seconds a step may take before the process is ended")
    ap.add_argument("--head", default=None, help="the tree's HEAD, when the tree is a copy without its repository")
    ap.add_argument("--label", default="", help="what build of the kernel this run measures")
    ap.add_argument("--ab", action="append", default=[], metavar="LABEL=FILE", help="embed another run's cases under \"ab\"")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scopes_pass.json"))
    args = ap.parse_args()
    import torch
    import raytracingmin_amd as rtm
    if not torch.cuda.is_available():
        sys.exit("scopes_pass.py needs a HIP device: nothing is measured without one")
    dev = torch.device("cuda", 0)
    signal.alarm(args.step_limit)
    gen = torch.Generator(device=dev)
    gen.manual_seed(W * 65536 + H)
    noise = torch.exp2(24.0 * torch.rand((H, W, 3), generator=gen, dtype=torch.float32, device=dev) - 12.0).contiguous()
    constant = torch.full((H, W, 3), 0.18, dtype=torch.float32, device=dev)
    data = rtm.LoadData(SCENE).data
    data.width, data.height, data.samples, data.superSamples = W, H, 4, 1
    r = rtm.Renderer(data)
    rendered, _ = r.render_rows_device(0, H, want=("f32",))
    cornell = rendered["f32"].contiguous()
    torch.cuda.synchronize()
    signal.alarm(args.step_limit)
    dst = torch.empty_like(noise)
    cp = windows(lambda: dst.copy_(noise), args.launches)
    copy_median = statistics.median(cp)
    cases, ok = [], True
    for name, src in (("noise", noise), ("constant", constant), ("cornell", cornell)):
        signal.alarm(args.step_limit)  # this step's own limit
        ms, same, y_bins, pixels = measure(rtm, src, args.launches)
        ok = ok and same
        case = {"frame": name, "y_bins_in_use": y_bins, "pixels": pixels, "identical": same}
        for k, v in ms.items():
            med = statistics.median(v)
            case[k] = {"call_ms": [round(x, 4) for x in v], "call_ms_median": round(med, 4), "call_ms_min": round(min(v), 4),
                       "copies": round(med / copy_median, 3)}
        case["both_over_the_two_alone"] = round(case["both"]["call_ms_median"] /
                                                (case["histogram"]["call_ms_median"] + case["waveform"]["call_ms_median"]), 3)
        cases.append(case)
    signal.alarm(0)
    by = {c["frame"]: c for c in cases}
    ratio = lambda cs, k: round(cs["constant"][k]["call_ms_median"] / cs["noise"][k]["call_ms_median"], 3)
    out = {"config": f"{W}x{H}x3 frames (seeded noise over 2^-12..2^12, a constant 0.18, the Cornell box at 4 spp), LOG2 mode, "
                     f"{COLUMNS} waveform columns; rtm_scopes (the zeroing and one launch a call) per case, and a device-to-device "
                     f"copy of the frame; device ms per call over windows of {args.launches} calls, {WINDOWS} windows after a "
                     "warm-up of 3 calls; `copies`: the median over the copy's",
           "label": args.label,
           "head": args.head or head_of_tree(),
           "device": torch.cuda.get_device_name(0),
           "frame_bytes": 12 * W * H,
           "copy_ms": [round(v, 4) for v in cp], "copy_ms_median": round(copy_median, 4),
           "copy_gbytes_per_s": round(2 * 12 * W * H / copy_median * 1e-6, 1),
           "cases": cases,
           "constant_over_noise": {k: ratio(by, k) for k in ("histogram", "waveform", "both")},
           "identical": bool(ok)}
    if args.ab:
        out["ab"] = {}
        for item in args.ab:
            label, path = item.split("=", 1)
            other = json.load(open(path))
            oby = {c["frame"]: c for c in other["cases"]}
            out["ab"][label] = {"label": other.get("label", ""), "copy_ms_median": other["copy_ms_median"],
                                "histogram_ms_median": {k: v["histogram"]["call_ms_median"] for k, v in oby.items()},
                                "histogram_copies": {k: v["histogram"]["copies"] for k, v in oby.items()},
                                "constant_over_noise_histogram": ratio(oby, "histogram"), "identical": other["identical"]}
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out), flush=True)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
