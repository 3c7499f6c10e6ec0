"""What the variance-guided denoiser costs (rtm_denoise_variance), beside rtm_denoise and the render of the same frame.

The headline Cornell frame (cornellBoxSetting.json, 1920x1080, S=64, SS=4, depth cap 8): its render, its AOVs, then on its
f32: the variance kernel alone in each of its three forms (rtm_debug_denoise_variance_kernel: every tap from L2, LDS tiles
of 64 x 4 and of 64 x 8), the whole call at the default sigmas with K = 0 .. 5 levels (the per-level figure is the
difference of consecutive K; K = 0 with a variance output is the prepass and the variance kernel), and rtm_denoise at its
defaults.  Every call is timed with device events on the stream, best of --reps after a warm-up; the output bytes of every
repetition are checked against the first, and the three forms against each other.  Prints one JSON object.

    python profiles/denoise_variance_pass.py [--reps 5]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FORMS = {0: "direct", 1: "lds_64x4", 2: "lds_64x8"}


def timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return out, e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch
    import raytracingmin_amd as rtm
    from raytracingmin_amd import _lib
    data = rtm.LoadData(os.path.join(ROOT, "scenes", "cornellBoxSetting.json")).data
    W, H = 1920, 1080
    data.width, data.height, data.samples, data.superSamples = W, H, 64, 4
    r = rtm.Renderer(data, mode="repaired", max_bounces=8, seed=0x5EED)
    render_ms = []
    for _ in range(args.reps + 1):
        out, t = timed(lambda: r.render_rows_device(want=("f32",), stats=False)[0])
        render_ms.append(round(t, 3))
    render_ms = render_ms[1:]
    f32 = out["f32"]
    aov = r.render_aov()
    ok = True

    def best_of(call):
        nonlocal ok
        ref = {n: v.cpu().numpy() for n, v in timed(call)[0].items()}  # (also the warm-up)
        ms = []
        for _ in range(args.reps):
            got, t = timed(call)
            ms.append(round(t, 4))
            ok = ok and all(np.array_equal(got[n].cpu().numpy().view(np.uint8), ref[n].view(np.uint8)) for n in ref)
        return min(ms), ref

    whole = {k: best_of(lambda: rtm.denoise_variance(f32, aov, iterations=k, want=("f32", "u8", "var")))[0] for k in range(6)}
    plain, _ = best_of(lambda: rtm.denoise(f32, aov, want=("f32", "u8")))
    # the variance kernel alone: the records of a K = 0 call stay in its work buffer
    L = rtm.lib()
    d = rtm.DENOISE_VAR_DEFAULTS
    prm = _lib.rtm_denoise_var_params(0, d["sigma_lum"], d["sigma_normal"], d["sigma_depth"])
    bufs = _lib.rtm_aov_buffers()
    for k, v in aov.items():
        setattr(bufs, k, v.data_ptr())
    work = torch.empty(L.rtm_denoise_variance_work_bytes(W, H), dtype=torch.uint8, device="cuda")
    var = torch.empty((H, W), dtype=torch.float32, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(L.rtm_denoise_variance(C.byref(prm), W, H, 0, f32.data_ptr(), C.byref(bufs), work.data_ptr(), None, None,
                                      var.data_ptr(), stream), "rtm_denoise_variance")

    def form_call(form):
        def call():
            _lib.check(L.rtm_debug_denoise_variance_kernel(form, C.byref(prm), W, H, 0, C.byref(bufs), work.data_ptr(),
                                                           var.data_ptr(), stream), "rtm_debug_denoise_variance_kernel")
            return {"var": var}
        return call

    forms, planes = {}, []
    for form, name in FORMS.items():
        forms[name], ref = best_of(form_call(form))
        planes.append(ref["var"])
    forms_agree = all(np.array_equal(p.view(np.uint32), planes[0].view(np.uint32)) for p in planes)
    row = {"config": "headline cornell 1080p x 1024 spp, variance-guided denoise at the default sigmas",
           "render_ms": render_ms,
           "variance_kernel_ms": forms,
           "variance_forms_bit_identical": bool(forms_agree),
           "denoise_variance_ms": {f"K{k}": whole[k] for k in whole},
           "per_level_ms": [round(whole[k] - whole[k - 1], 4) for k in range(1, 6)],
           "default_ms": whole[d["iterations"]] if d["iterations"] in whole else None,
           "rtm_denoise_default_ms": plain,
           "default_share_of_render": round(whole.get(d["iterations"], 0.0) / min(render_ms), 5),
           "identical": bool(ok)}
    print(json.dumps(row), flush=True)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
