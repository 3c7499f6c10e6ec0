"""png::Renderer on the HIP path (reference src/Renderer.h:8-18, src/Renderer.cpp:20-23,200-258).

    ld = LoadData("cornellBoxSetting.json")
    r = Renderer(ld.data, mode="repaired", max_bounces=8)
    r.Render("result")          # writes result.jpg (q=60) and result.bmp like the reference
    r.image                     # (H, W, 3) float64 — the reference's private Renderer::image

Device memory and streams come from torch (plumbing); every pixel is computed by the HIP kernels
behind rtm_render_device.  There is no CPU fallback.
"""
import ctypes as C
import os
import sys

import numpy as np

from . import _lib
from ._lib import rtm_options, rtm_stats
from .settings import SettingData

# tile-adaptive sampling: the Python / rtm_cli defaults ("Tile-adaptive sampling")
ADAPTIVE_DEFAULTS = {"min_samples": 16, "threshold": 0.05}


def adaptive_preview(accum, tile_samples, n_samples):
    """The f64 view of an adaptive frame: every pixel's accumulator times N / k, k its tile's sample count (the preview
    rule of rtm_render_scene_samples, computed in double like the device's f32 / u8 views; a tile at N is its accumulator)."""
    k = np.repeat(np.repeat(np.asarray(tile_samples, dtype=np.float64), 8, axis=0), 8, axis=1)[:accum.shape[0], :accum.shape[1]]
    return accum * (np.float64(n_samples) / k)[..., None]


def pack_spheres(center, radius, color, emission):
    """rtm_sphere[n] as an (n, 80) uint8 tensor on the tensors' device, for Renderer.set_device_spheres: center, color and
    emission are (n, 3) float64 tensors, radius is (n,) and is cast to float32 (the reference's m_size is a float); the four
    pad bytes of every record are zero.  Pure tensor operations on the current stream: nothing comes to the host."""
    import torch
    parts = {"center": center, "radius": radius, "color": color, "emission": emission}
    for name, t in parts.items():
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} is not a torch tensor")
        if t.device != center.device:
            raise ValueError(f"{name} is on {t.device}, center on {center.device}")
    n = center.shape[0] if center.dim() == 2 else -1
    for name in ("center", "color", "emission"):
        t = parts[name]
        if t.dtype != torch.float64 or tuple(t.shape) != (n, 3):
            raise ValueError(f"{name} must be an (n, 3) float64 tensor, got {tuple(t.shape)} {t.dtype}")
    if tuple(radius.shape) != (n,) or not (radius.dtype.is_floating_point or radius.dtype in (torch.int32, torch.int64)):
        raise ValueError(f"radius must be an (n,) tensor of numbers, got {tuple(radius.shape)} {radius.dtype}")
    out = torch.zeros((n, 80), dtype=torch.uint8, device=center.device)
    d = out.view(torch.float64)  # (n, 10): center, color, emission, (radius, pad)
    d[:, 0:3], d[:, 3:6], d[:, 6:9] = center, color, emission
    out.view(torch.float32)[:, 18] = radius.to(torch.float32)
    return out


class Renderer:
    def __init__(self, data: SettingData, mode="repaired", max_bounces=-1, seed=0x5EED, device=0,
                 variant=0, host_trig=True, count_tests=False, integrator="PathTracing"):
        # host_trig (default): sin/cos of src/Renderer.cpp:93-94 as the HOST's libm returns them, so a
        # render agrees with a CPU run of the reference bit for bit even on scenes that amplify one-ulp
        # differences over many bounces; host_trig=False is the labelled ~2 % faster device-trig row
        self.data = data  # the reference keeps a reference to the caller's SettingData
        # count_tests: rtm_stats.object_tests also for the uniform-grid kernel (its counting instantiation, RTM_MODE_COUNT_TESTS)
        # integrator: "PathTracing" (what the reference's Render always takes, src/Renderer.cpp:238) or "SurfaeSample" (the
        # branch of :234-236 it never takes; RTM_MODE_SURFACE_SAMPLE, served by a general per-object kernel)
        if integrator not in ("PathTracing", "SurfaeSample"):
            raise ValueError(f"unknown integrator {integrator!r}")
        self.mode = _lib.MODES[mode] | (_lib.MODE_HOST_TRIG if host_trig else 0) | (_lib.MODE_COUNT_TESTS if count_tests else 0) \
            | (_lib.MODE_SURFACE_SAMPLE if integrator == "SurfaeSample" else 0)
        self.max_bounces = int(max_bounces)
        self.seed = int(seed)
        self.device = int(device)
        self.variant = int(variant)
        self.image = np.zeros((data.height, data.width, 3), dtype=np.float64)  # src/Renderer.cpp:21
        self.stats = None
        self._scene = None      # rtm_scene* on self.device (made on first use, kept for the renderer's life)
        self._scene_key = None
        self._device_scene = None  # rtm_scene* built from a device sphere array (set_device_spheres); wins over data.object

    # ---- the scene on the device: flattened and uploaded once per renderer -------------------
    def _scene_handle(self):
        """rtm_scene_create once; made again whenever the scene may have changed since — the reference reads the live
        SettingData at render time (src/Renderer.h:16), and so must this.  The key is O(1) per render: the edit epoch of
        settings.py counts every write to a scene object's fields AND every assignment or mutation of a SettingData's
        object list (replaced, reordered, added, removed entries); camera edits do not count (the camera is not part of
        the uploaded scene).  Edits to ANOTHER SettingData also advance the epoch: a needless re-flatten, never a stale
        scene."""
        if self._device_scene is not None:  # set_device_spheres: whatever the edit epoch says
            return self._device_scene
        from .settings import edit_epoch
        objs = self.data.object
        key = (edit_epoch(), id(objs))
        if self._scene is None or key != self._scene_key:
            self.invalidate()
            h = C.c_void_p()
            if self.data.has_planes():  # png::PlaneObject entries: the any-type object list
                arr, n = self.data.objects_c()
                _lib.check(_lib.lib().rtm_scene_create_objects(arr, n, self.device, C.byref(h)),
                           "rtm_scene_create_objects")
            else:
                arr, n = self.data.spheres_c()
                _lib.check(_lib.lib().rtm_scene_create(arr, n, 0, self.device, C.byref(h)), "rtm_scene_create")
            self._scene, self._scene_key = h, key
        return self._scene

    def scratch_bytes(self, row_begin=0, row_end=None, band=None):
        """rtm_scratch_bytes: what a render of these rows asks of the library's per-(device, stream) work buffers."""
        row_end = self.data.height if row_end is None else row_end
        opt = self._options(row_begin, row_end, band)
        st = self.data.settings_c()
        out = (C.c_uint64 * 6)()
        _lib.check(_lib.lib().rtm_scratch_bytes(C.byref(st), self._scene_handle(), C.byref(opt), out), "rtm_scratch_bytes")
        return dict(zip(("total", "terms", "records", "pipeline_state", "steal_rows", "primary_table"), (int(v) for v in out)))

    def set_device_spheres(self, packed, stream=None):
        """Render a sphere array that lives on the device: `packed` is pack_spheres' (n, 80) uint8 tensor (rtm_sphere[n]) on
        this renderer's device.  The scene — tables and grid — is built by rtm_scene_create_device on `stream` (default: the
        current torch stream), ordered after whatever wrote the tensor there, without the array coming to the host; the
        tensor may be overwritten as soon as the call returns.  From then on every render that goes through the renderer's scene
        object (render_rows_device and every stage built on it) uses that scene, whatever happens to data.object; settings
        and camera still come from self.data.  Render() goes through the scene object too while a device scene is set;
        render_rows, the host-array call, reads data.object and would render another scene: it raises RuntimeError then.  Call it again for the next frame
        of an animation; set_device_spheres(None) or invalidate() returns to data.object."""
        if packed is None:
            self.invalidate()
            return
        import torch
        if not isinstance(packed, torch.Tensor):
            raise ValueError("packed is not a torch tensor")
        if packed.dtype != torch.uint8 or packed.dim() != 2 or packed.shape[1] != 80 or not packed.is_contiguous():
            raise ValueError(f"packed must be a contiguous (n, 80) uint8 tensor, got {tuple(packed.shape)} {packed.dtype}")
        if packed.device.type != "cuda" or packed.device.index != self.device:
            raise ValueError(f"packed is on {packed.device}, the renderer on cuda:{self.device}")
        self.invalidate()  # (a refused tensor leaves the renderer's scene as it was)
        if stream is None:
            stream = torch.cuda.current_stream(packed.device)
        hip_stream = stream.cuda_stream if hasattr(stream, "cuda_stream") else int(stream)
        h = C.c_void_p()
        _lib.check(_lib.lib().rtm_scene_create_device(C.c_void_p(packed.data_ptr()), packed.shape[0], self.device,
                                                      C.c_void_p(hip_stream), C.byref(h)), "rtm_scene_create_device")
        self._device_scene = h

    def invalidate(self):
        if self._scene is not None:
            _lib.lib().rtm_scene_destroy(self._scene)
            self._scene = None
        if getattr(self, "_device_scene", None) is not None:
            _lib.lib().rtm_scene_destroy(self._device_scene)
            self._device_scene = None

    def __del__(self):
        if sys.is_finalizing():  # interpreter shutdown: the HIP runtime may be gone already; the process's memory goes with it
            return
        try:
            self.invalidate()
        except Exception:
            pass

    def stream_status(self, stream=None):
        """rtm_stream_status: raises RtmError if a stats-less render on the stream was truncated."""
        import torch
        dev = torch.device("cuda", self.device)
        hip_stream = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
        _lib.check(_lib.lib().rtm_stream_status(self.device, C.c_void_p(hip_stream)), "rtm_stream_status")

    def _options(self, row_begin, row_end, band=None):
        o = rtm_options()
        o.mode, o.max_bounces, o.seed = self.mode, self.max_bounces, self.seed
        o.row_begin, o.row_end = int(row_begin), int(row_end)
        o.device, o.variant = self.device, self.variant
        if band is not None:  # (count, index): only the 8-row bands index, index + count, ...
            o.band_count, o.band_index = int(band[0]), int(band[1])
        return o

    def compare(self, reference, frame=None, **params):
        """compare() of a frame of this renderer against `reference`, decoded: a dict of rtm_compare_result's fields.
        frame=None: the last rendered image (self.image, float64); else an (H, W, 3) array or tensor.  `reference` is an
        (H, W, 3) array or tensor; both go to this renderer's device, and a float64 frame is rounded to float32 when the
        reference is float32 (what out_f32 holds).  params: compare()'s tolerance, peak, rel_epsilon."""
        import torch
        dev = torch.device("cuda", self.device)
        to_dev = lambda v: (v if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(v))).to(dev).contiguous()
        ref = to_dev(reference)
        got = to_dev(self.image if frame is None else frame)
        if got.dtype == torch.float64 and ref.dtype == torch.float32:
            got = got.to(torch.float32)
        out = compare(got, ref, want=("result",), **params)
        torch.cuda.current_stream(dev).synchronize()
        return compare_result(out["result"])

    def flip(self, reference, frame=None, **params):
        """flip() of a frame of this renderer against `reference`, decoded: flip_result()'s dict.  frame=None: the last
        rendered image (self.image); else an (H, W, 3) array or tensor.  Both are DISPLAY-REFERRED frames (pass
        transfer="linear" for frames that are linear; values outside [0, 1] are clamped), go to this renderer's device and
        are rounded to float32.  params: flip()'s transfer, pixels_per_degree."""
        import torch
        dev = torch.device("cuda", self.device)
        to_dev = lambda v: (v if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(v))).to(dev).to(torch.float32).contiguous()
        out = flip(to_dev(self.image if frame is None else frame), to_dev(reference), want=("result",), **params)
        torch.cuda.current_stream(dev).synchronize()
        return flip_result(out["result"])

    def _scope_frame(self, frame):
        """`frame` (an (H, W, 3) array or tensor; None: self.image) on this renderer's device as contiguous float32."""
        import torch
        dev = torch.device("cuda", self.device)
        v = self.image if frame is None else frame
        v = v if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(v))
        return v.to(dev).to(torch.float32).contiguous()

    def scopes(self, frame=None, **params):
        """scopes() of a frame of this renderer, decoded on the host.  frame=None: the last rendered image (self.image)
        rounded to float like out_f32; else an (H, W, 3) array or tensor.  params: scopes()'s mode, columns, want.  Returns a
        dict of the names in `want`: "histogram" as scope_histogram() gives it, "waveform" a (4, 256, columns) uint32 array."""
        import torch
        color = self._scope_frame(frame)
        out = scopes(color, **params)
        torch.cuda.current_stream(color.device).synchronize()
        got = {}
        if "histogram" in out:
            got["histogram"] = scope_histogram(out["histogram"])
        if "waveform" in out:
            got["waveform"] = out["waveform"].cpu().numpy().view(np.uint32)
        return got

    def write_scopes(self, fileName, frame=None, mode=_lib.SCOPE_DEFAULTS["mode"], columns=None, layout="luma", gain=None):
        """<fileName>_scopes.json and <fileName>_waveform.bmp of one frame — what rtm_cli --scopes writes of it.  frame=None:
        the last rendered image; mode "log2" for a linear frame, "code" for a display frame.  columns: the waveform's, default
        min(256, W); layout "luma", "overlay" or "parade"; gain: default max(1, 2040 // H).  The JSON object is scope_summary()
        of the frame plus "histogram": {"bins", "below", "above"}, the counts.  Returns that object."""
        import json
        import torch
        color = self._scope_frame(frame)
        H, W = int(color.shape[0]), int(color.shape[1])
        columns = min(SCOPE_DEFAULTS["columns"], W) if columns is None else columns
        gain = max(1, 2040 // H) if gain is None else gain
        out = scopes(color, mode=mode, columns=columns, want=("histogram", "waveform"))
        picture = np.ascontiguousarray(scope_draw(out["waveform"], layout=layout, gain=gain).cpu().numpy())
        hist = scope_histogram(out["histogram"])
        doc = scope_summary(hist, mode)
        doc["histogram"] = {"bins": hist["bins"].tolist(), "below": hist["below"].tolist(), "above": hist["above"].tolist()}
        with open(fileName + "_scopes.json", "w") as f:
            json.dump(doc, f)
        if not _lib.lib().rtm_write_bmp(os.fsencode(fileName + "_waveform.bmp"), picture.shape[1], 256, 3, picture.ctypes.data):
            raise _lib.RtmError(-3, f"could not write {fileName}_waveform.bmp")
        return doc

    # ---- device-resident render: outputs are torch tensors on the GPU ------------------------
    def render_rows_device(self, row_begin=0, row_end=None, want=("f32",), stats=True,
                           stream=None, band=None):
        """Render rows [row_begin, row_end) into torch CUDA tensors; returns (dict, stats).
        band=(count, index) renders only every count-th 8-row band of the range, stored back to back
        (include/rtm.h, rtm_options.band_count)."""
        import torch
        _need_device("Renderer")
        row_end = self.data.height if row_end is None else row_end
        opt = self._options(row_begin, row_end, band)
        rows, W = _lib.lib().rtm_output_rows(C.byref(opt)), self.data.width
        dev = torch.device("cuda", self.device)
        out = {}
        if "f64" in want:
            out["f64"] = torch.empty((rows, W, 3), dtype=torch.float64, device=dev)
        if "f32" in want:
            out["f32"] = torch.empty((rows, W, 3), dtype=torch.float32, device=dev)
        if "u8" in want:
            out["u8"] = torch.empty((rows, W, 3), dtype=torch.uint8, device=dev)
        st = self.data.settings_c()
        s = rtm_stats()
        hip_stream = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
        ptr = lambda k: C.c_void_p(out[k].data_ptr()) if k in out and rows > 0 else None
        _lib.check(_lib.lib().rtm_render_scene(C.byref(st), self._scene_handle(), C.byref(opt), ptr("f64"),
                                               ptr("f32"), ptr("u8"), C.c_void_p(hip_stream),
                                               C.byref(s) if stats else None), "rtm_render_scene")
        return out, (s.as_dict() if stats else None)

    # ---- progressive rendering: the frame's samples in passes (rtm_render_scene_samples) -------
    def total_samples(self):
        """N = superSamples^2 x samples: the samples of every pixel of a frame."""
        return self.data.superSamples * self.data.superSamples * self.data.samples

    def render_samples_device(self, sample_begin, sample_end, accum, want=("u8",), stats=True, stream=None,
                              row_begin=0, row_end=None, band=None):
        """Trace samples [sample_begin, sample_end) of every pixel of the rows into `accum`, a float64 CUDA tensor laid out
        like render_rows_device's "f64" and updated in place: a pass that starts past 0 continues the fold from what `accum`
        holds.  Returns (dict, stats): "f64" is `accum` itself; "f32" / "u8" are the frame's views after the last pass and
        a preview (accum x N / sample_end) before it."""
        import torch
        _need_device("Renderer")
        row_end = self.data.height if row_end is None else row_end
        opt = self._options(row_begin, row_end, band)
        rows, W = _lib.lib().rtm_output_rows(C.byref(opt)), self.data.width
        dev = torch.device("cuda", self.device)
        if accum.dtype != torch.float64 or accum.device != dev or not accum.is_contiguous() or accum.numel() != rows * W * 3:
            raise ValueError(f"accum must be a contiguous float64 tensor of {rows}x{W}x3 on {dev}")
        out = {"f64": accum}
        if "f32" in want:
            out["f32"] = torch.empty((rows, W, 3), dtype=torch.float32, device=dev)
        if "u8" in want:
            out["u8"] = torch.empty((rows, W, 3), dtype=torch.uint8, device=dev)
        st = self.data.settings_c()
        s = rtm_stats()
        hip_stream = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
        ptr = lambda k: C.c_void_p(out[k].data_ptr()) if k in out and rows > 0 else None
        _lib.check(_lib.lib().rtm_render_scene_samples(C.byref(st), self._scene_handle(), C.byref(opt), int(sample_begin),
                                                       int(sample_end), ptr("f64"), ptr("f32"), ptr("u8"),
                                                       C.c_void_p(hip_stream), C.byref(s) if stats else None),
                   "rtm_render_scene_samples")
        return out, (s.as_dict() if stats else None)

    def progressive(self, passes=None, samples_per_pass=None, want=("u8",), stats=True, stream=None,
                    row_begin=0, row_end=None, band=None):
        """Render the frame in contiguous, near-equal passes (plan_passes); yields (sample_end, outputs, stats) after each.
        The outputs of the last pass are rtm_render_scene's frame bit for bit; "f64" is the accumulator every pass shares."""
        import torch
        row_end = self.data.height if row_end is None else row_end
        opt = self._options(row_begin, row_end, band)
        rows = _lib.lib().rtm_output_rows(C.byref(opt))
        accum = torch.empty((rows, self.data.width, 3), dtype=torch.float64, device=torch.device("cuda", self.device))
        for a, b in plan_passes(self.total_samples(), passes=passes, samples_per_pass=samples_per_pass):
            out, st = self.render_samples_device(a, b, accum, want=want, stats=stats, stream=stream,
                                                 row_begin=row_begin, row_end=row_end, band=band)
            yield b, out, st

    # ---- tile lists and tile-adaptive sampling (rtm_render_scene_tiles, rtm_render_adaptive) ----
    def tiles_shape(self, row_begin=0, row_end=None, band=None):
        """(tiles_y, tiles_x): the 8x8 tiles of the call's output rows; tile t is (t // tiles_x, t % tiles_x)."""
        row_end = self.data.height if row_end is None else row_end
        opt = self._options(row_begin, row_end, band)
        rows = _lib.lib().rtm_output_rows(C.byref(opt))
        return (rows + 7) // 8, (self.data.width + 7) // 8

    def render_tiles_device(self, tiles, sample_begin, sample_end, accum, want=("u8",), out=None, stats=True, stream=None,
                            row_begin=0, row_end=None, band=None):
        """render_samples_device restricted to the listed tiles (`tiles`: a uint32/int32 CUDA tensor or a sequence of tile
        indices): their pixels get the pass's accumulator and f32 / u8 views; every other pixel of `accum` and of the
        tensors in `out` (reused when given, so that unlisted tiles keep what they held) is neither read nor written."""
        import torch
        _need_device("Renderer")
        row_end = self.data.height if row_end is None else row_end
        opt = self._options(row_begin, row_end, band)
        rows, W = _lib.lib().rtm_output_rows(C.byref(opt)), self.data.width
        dev = torch.device("cuda", self.device)
        if accum.dtype != torch.float64 or accum.device != dev or not accum.is_contiguous() or accum.numel() != rows * W * 3:
            raise ValueError(f"accum must be a contiguous float64 tensor of {rows}x{W}x3 on {dev}")
        if not torch.is_tensor(tiles):
            tiles = torch.tensor(np.asarray(tiles, dtype=np.int64).astype(np.uint32).view(np.int32), device=dev)
        tiles = tiles.to(dev).contiguous()
        if tiles.element_size() != 4:
            raise ValueError("tiles must hold 32-bit tile indices")
        res = dict(out or {})
        res["f64"] = accum
        for k, dt in (("f32", torch.float32), ("u8", torch.uint8)):
            if k in want and k not in res:
                res[k] = torch.empty((rows, W, 3), dtype=dt, device=dev)
        st = self.data.settings_c()
        s = rtm_stats()
        hip_stream = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
        ptr = lambda k: C.c_void_p(res[k].data_ptr()) if k in res and rows > 0 else None
        _lib.check(_lib.lib().rtm_render_scene_tiles(C.byref(st), self._scene_handle(), C.byref(opt), int(sample_begin),
                                                     int(sample_end), C.c_void_p(tiles.data_ptr()), int(tiles.numel()),
                                                     ptr("f64"), ptr("f32"), ptr("u8"), C.c_void_p(hip_stream),
                                                     C.byref(s) if stats else None), "rtm_render_scene_tiles")
        return res, (s.as_dict() if stats else None)

    def adaptive(self, threshold=ADAPTIVE_DEFAULTS["threshold"], min_samples=ADAPTIVE_DEFAULTS["min_samples"], want=("u8",),
                 stats=True, stream=None, row_begin=0, row_end=None, band=None):
        """Tile-adaptive rendering (include/rtm.h: rtm_render_adaptive).  Returns (outputs, tile_samples, stats): outputs as
        render_samples_device's ("f64" is the accumulator), tile_samples a (tiles_y, tiles_x) int64 CUDA tensor of the
        samples each tile traced.  Tile t equals rtm_render_scene_samples [0, tile_samples[t]) bit for bit.  Blocks."""
        import torch
        _need_device("Renderer")
        row_end = self.data.height if row_end is None else row_end
        opt = self._options(row_begin, row_end, band)
        L = _lib.lib()
        rows, W = L.rtm_output_rows(C.byref(opt)), self.data.width
        dev = torch.device("cuda", self.device)
        st = self.data.settings_c()
        out = {"f64": torch.empty((rows, W, 3), dtype=torch.float64, device=dev)}
        for k, dt in (("f32", torch.float32), ("u8", torch.uint8)):
            if k in want:
                out[k] = torch.empty((rows, W, 3), dtype=dt, device=dev)
        ty, tx = (rows + 7) // 8, (W + 7) // 8
        tile_samples = torch.zeros((ty, tx), dtype=torch.int32, device=dev)
        work = torch.empty(max(256, L.rtm_adaptive_work_bytes(C.byref(st), C.byref(opt))), dtype=torch.uint8, device=dev)
        prm = _lib.rtm_adaptive_params(int(min_samples), float(threshold))
        s = rtm_stats()
        hip_stream = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
        ptr = lambda k: C.c_void_p(out[k].data_ptr()) if k in out and rows > 0 else None
        _lib.check(L.rtm_render_adaptive(C.byref(st), self._scene_handle(), C.byref(opt), C.byref(prm), ptr("f64"), ptr("f32"),
                                         ptr("u8"), C.c_void_p(tile_samples.data_ptr()) if rows > 0 else None,
                                         C.c_void_p(work.data_ptr()), C.c_void_p(hip_stream),
                                         C.byref(s) if stats else None), "rtm_render_adaptive")
        return out, tile_samples.to(torch.int64), (s.as_dict() if stats else None)

    def write_spp(self, fileName, tile_samples):
        """<fileName>_spp.pfm: the samples each pixel traced, as floats (one channel), from a (tiles_y, tiles_x) map."""
        H, W = self.data.height, self.data.width
        ts = np.asarray(tile_samples.cpu() if hasattr(tile_samples, "cpu") else tile_samples)
        spp = np.ascontiguousarray(np.repeat(np.repeat(ts, 8, axis=0), 8, axis=1)[:H, :W].astype(np.float32))
        if not _lib.lib().rtm_write_pfm(os.fsencode(fileName + "_spp.pfm"), W, H, 1, spp.ctypes.data):
            raise _lib.RtmError(-3, f"could not write {fileName}_spp.pfm")
        return spp

    # ---- first-hit feature buffers (rtm_render_aov) ------------------------------------------
    AOV_PLANES = ("depth", "normal", "albedo", "object")

    def render_aov(self, row_begin=0, row_end=None, band=None, want=AOV_PLANES, stream=None):
        """The first-hit AOVs of rows [row_begin, row_end) as torch CUDA tensors: "depth" (rows, W) float32, "normal" and
        "albedo" (rows, W, 3) float32, "object" (rows, W) int32 (include/rtm.h: rtm_render_aov).  Only the planes named in
        `want` are allocated and computed.  Enqueued on `stream` (default: the current stream); nothing waits for it."""
        import torch
        _need_device("Renderer")
        _check_planes(want)
        row_end = self.data.height if row_end is None else row_end
        opt = self._options(row_begin, row_end, band)
        rows, W = _lib.lib().rtm_output_rows(C.byref(opt)), self.data.width
        dev = torch.device("cuda", self.device)
        out = {k: torch.empty(shape, dtype=dt, device=dev) for k, (shape, dt) in _aov_layout(rows, W).items() if k in want}
        bufs = _lib.rtm_aov_buffers()
        for k, v in out.items():
            setattr(bufs, k, v.data_ptr() if rows > 0 else None)
        st = self.data.settings_c()
        hip_stream = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
        _lib.check(_lib.lib().rtm_render_aov(C.byref(st), self._scene_handle(), C.byref(opt), C.byref(bufs),
                                             C.c_void_p(hip_stream)), "rtm_render_aov")
        return out

    # ---- ray queries on the scene (rtm_scene_nearest, rtm_scene_occluded) ---------------------
    QUERY_PLANES = ("object", "t", "normal")

    def _query_rays(self, org, direction, tmax=None):
        """(n, device) of a ray batch: org and direction contiguous (n, 3) float64 CUDA tensors on the renderer's device,
        tmax None or a contiguous (n,) one.  Anything else: ValueError, before the library is called."""
        import torch
        dev = torch.device("cuda", self.device)
        n = org.shape[0] if isinstance(org, torch.Tensor) and org.dim() == 2 else -1
        for name, v, shape, text in (("org", org, (n, 3), "(n, 3)"), ("direction", direction, (n, 3), "(n, 3)"),
                                     ("tmax", tmax, (n,), "(n,)")):
            if v is None and name == "tmax":
                continue
            if not (isinstance(v, torch.Tensor) and v.device == dev and v.dtype == torch.float64 and n >= 0
                    and tuple(v.shape) == shape and v.is_contiguous()):
                raise ValueError(f"{name} must be a contiguous {text} float64 tensor on {dev}")
        return n, dev

    def nearest(self, org, direction, want=("object", "t"), stream=None):
        """What each ray hits first in the renderer's scene (include/rtm.h: rtm_scene_nearest): a dict of torch CUDA tensors,
        "object" (n,) int32 (-1: nothing), "t" (n,) float64 (+inf: nothing), "normal" (n, 3) float64 — Intersect's normal of the
        hit object, not turned towards the ray (zeros: nothing).  org and direction are contiguous (n, 3) float64 tensors on the
        renderer's device; directions are the caller's to normalise (any length is answered exactly; only unit ones take a large
        scene's grid).  Only the planes named in `want` are allocated and computed.  Enqueued on `stream` (default: the current
        stream); nothing waits for it."""
        import torch
        _need_device("Renderer")
        _check_want(want, self.QUERY_PLANES)
        n, dev = self._query_rays(org, direction)
        s = _stream_of(stream, dev)
        layout = {"object": ((n,), torch.int32), "t": ((n,), torch.float64), "normal": ((n, 3), torch.float64)}
        out, ptr = _stage_tensors(s, dev, want, layout)
        bufs = _lib.rtm_hit_buffers()
        for k in out:
            setattr(bufs, k, ptr(k))
        if n > 0:
            _lib.check(_lib.lib().rtm_scene_nearest(self._scene_handle(), C.c_void_p(org.data_ptr()), C.c_void_p(direction.data_ptr()),
                                                    n, C.byref(bufs), C.c_void_p(s.cuda_stream)), "rtm_scene_nearest")
        return out

    def occluded(self, org, direction, tmax=None, stream=None):
        """Whether each ray hits anything before tmax (include/rtm.h: rtm_scene_occluded): an (n,) bool CUDA tensor, True where
        nearest()'s t is < tmax, strictly.  tmax: a contiguous (n,) float64 tensor on the renderer's device, or None for "any
        hit"; an entry that is NaN, zero or negative is never occluded.  A scene with a grid stops at the first such hit
        instead of finding the nearest.  Enqueued on `stream` (default: the current stream); nothing waits for it."""
        import torch
        _need_device("Renderer")
        n, dev = self._query_rays(org, direction, tmax)
        s = _stream_of(stream, dev)
        out, ptr = _stage_tensors(s, dev, ("occluded",), {"occluded": ((n,), torch.uint8)})
        if n > 0:
            _lib.check(_lib.lib().rtm_scene_occluded(self._scene_handle(), C.c_void_p(org.data_ptr()), C.c_void_p(direction.data_ptr()),
                                                     C.c_void_p(tmax.data_ptr()) if tmax is not None else None, n,
                                                     C.c_void_p(ptr("occluded")), C.c_void_p(s.cuda_stream)), "rtm_scene_occluded")
        return out["occluded"].view(torch.bool)

    # ---- radiance queries on the scene (rtm_scene_radiance) ------------------------------------
    RADIANCE_PLANES = ("radiance", "casts", "draws")

    def radiance(self, org, direction, samples=1, key_base=0, clamp=False, want=("radiance",), stream=None):
        """How much light arrives along each ray in the renderer's scene (include/rtm.h: rtm_scene_radiance): a dict of torch
        CUDA tensors, "radiance" (n, 3) float64 — the sum over s < samples, in order, of PathTracing(ray i; stream (seed,
        key_base + i, s)) / samples, each term clamped to [0, 1] first when `clamp` (then rays equal to a camera's pixels with
        key_base 0 give render()'s frame at superSamples 1, bit for bit) —, "casts" and "draws" (n,) uint32: the nearest-hit
        loops and generator calls of ray i over all its samples, modulo 2^32.  The renderer's mode, max_bounces, seed and
        host-trig setting apply.  org and direction are contiguous (n, 3) float64 tensors on the renderer's device.  One lane
        traces all samples of a ray: few rays with many samples under-fill the device — repeat the rays, each copy has its own
        key.  Only the planes named in `want` are allocated and computed.  Enqueued on `stream` (default: the current stream);
        nothing waits for it (the first call that needs the record pool or the trig table sets it up).  With max_bounces -1 or
        above 16 the call keeps a pool of hit records sized to its rays (3 840 bytes per ray, at most 960 MiB; more than 262 144
        rays run as several launches), so the number of rays never costs a path; a single path that reaches 976 bounces is
        truncated (its sample adds 0) and stream_status() then raises; max_bounces above 976 is refused."""
        import torch
        _need_device("Renderer")
        _check_want(want, self.RADIANCE_PLANES)
        n, dev = self._query_rays(org, direction)
        samples, key_base = int(samples), int(key_base)
        if samples < 1 or samples > 0xFFFFFFFF:
            raise ValueError(f"samples must be in [1, 2^32), got {samples}")
        if key_base < 0 or key_base + n > 1 << 32:
            raise ValueError(f"key_base must be >= 0 with key_base + n <= 2^32, got {key_base} for {n} rays")
        s = _stream_of(stream, dev)
        layout = {"radiance": ((n, 3), torch.float64), "casts": ((n,), torch.uint32), "draws": ((n,), torch.uint32)}
        out, ptr = _stage_tensors(s, dev, want, layout)
        bufs = _lib.rtm_radiance_buffers()
        for k in out:
            setattr(bufs, k, ptr(k))
        prm = _lib.rtm_radiance_params(self.mode & ~_lib.MODE_COUNT_TESTS, self.max_bounces, self.seed, samples, key_base,
                                       _lib.RADIANCE_CLAMP if clamp else 0, 0)
        if n > 0:
            _lib.check(_lib.lib().rtm_scene_radiance(self._scene_handle(), C.c_void_p(org.data_ptr()), C.c_void_p(direction.data_ptr()),
                                                     n, C.byref(prm), C.byref(bufs), C.c_void_p(s.cuda_stream)), "rtm_scene_radiance")
        return out

    def write_aov(self, fileName):
        """<fileName>_depth.pfm, _normal.pfm, _albedo.pfm (exact float planes) and _normal.bmp (quantised 0.5 n + 0.5),
        _albedo.bmp (quantised albedo) of the whole frame — what rtm_cli --aov writes."""
        import torch
        out = self.render_aov(want=("depth", "normal", "albedo"))
        torch.cuda.synchronize(self.device)
        H, W = self.data.height, self.data.width
        L = _lib.lib()
        planes = {k: np.ascontiguousarray(v.cpu().numpy()) for k, v in out.items()}
        ok = True
        for k, comp in (("depth", 1), ("normal", 3), ("albedo", 3)):
            ok = ok and L.rtm_write_pfm(os.fsencode(f"{fileName}_{k}.pfm"), W, H, comp, planes[k].ctypes.data) == 1
        for k, v in (("normal", 0.5 * planes["normal"].astype(np.float64) + 0.5), ("albedo", planes["albedo"].astype(np.float64))):
            v = np.ascontiguousarray(v)
            rgb8 = np.zeros(v.shape, dtype=np.uint8)
            _lib.check(L.rtm_quantise(v.ctypes.data, v.size, rgb8.ctypes.data), "rtm_quantise")
            ok = ok and L.rtm_write_bmp(os.fsencode(f"{fileName}_{k}.bmp"), W, H, 3, rgb8.ctypes.data) == 1
        if not ok:
            raise _lib.RtmError(-3, f"could not write the AOV files of {fileName}")
        return planes

    # ---- coverage AOVs (rtm_render_mattes) ----------------------------------------------------
    MATTE_PLANES = ("id", "coverage", "alpha")

    def render_mattes(self, layers=4, row_begin=0, row_end=None, band=None, want=MATTE_PLANES, stream=None):
        """The coverage AOVs of rows [row_begin, row_end) as torch CUDA tensors: "id" (layers, rows, W) int32 and "coverage"
        (layers, rows, W) float32 — plane l holds the object of rank l behind every pixel (-1: none) and the fraction of the
        pixel's SS^2 sub-pixels it covers, most first — and "alpha" (rows, W) float32, the fraction that hit anything
        (include/rtm.h: rtm_render_mattes).  layers is 1..8; only the planes named in `want` are allocated and written.
        Enqueued on `stream` (default: the current stream); nothing waits for it."""
        layers = _matte_layers(layers)
        unknown = set(want) - set(self.MATTE_PLANES)
        if unknown or not want:
            raise ValueError(f"want names planes among {self.MATTE_PLANES}, got {tuple(want)}")
        import torch
        _need_device("Renderer")
        row_end = self.data.height if row_end is None else row_end
        opt = self._options(row_begin, row_end, band)
        rows, W = _lib.lib().rtm_output_rows(C.byref(opt)), self.data.width
        dev = torch.device("cuda", self.device)
        shapes = {"id": ((layers, rows, W), torch.int32), "coverage": ((layers, rows, W), torch.float32),
                  "alpha": ((rows, W), torch.float32)}
        out = {k: torch.empty(shapes[k][0], dtype=shapes[k][1], device=dev) for k in self.MATTE_PLANES if k in want}
        if rows == 0:
            return out
        bufs = _lib.rtm_matte_buffers()
        for k, v in out.items():
            setattr(bufs, k, v.data_ptr())
        st = self.data.settings_c()
        hip_stream = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
        _lib.check(_lib.lib().rtm_render_mattes(C.byref(st), self._scene_handle(), C.byref(opt), layers, C.byref(bufs),
                                                C.c_void_p(hip_stream)), "rtm_render_mattes")
        return out

    def write_mattes(self, fileName, layers=4, ids=None, background=None, frame=None):
        """<fileName>_alpha.pfm: the frame's alpha plane (render_mattes).  With ids (1..64 object indices): <fileName>_matte.pfm,
        the antialiased matte() of those objects cut from `layers` ranked layers, and a grey <fileName>_matte.bmp.  With
        background (a colour or an (H, W, 3) float32 CUDA tensor): <fileName>_over.bmp and <fileName>_over.jpg (q=60), the
        frame composite()d over it — `frame` an (H, W, 3) float32 CUDA tensor, default self.image rounded to float like
        out_f32.  What rtm_cli --alpha / --matte / --background write.  Returns a dict: "alpha" and "matte" as (H, W) float32
        arrays, "over" the composited (H, W, 3) float32 frame on the device."""
        layers, ids, background = _matte_args(layers, ids, background)
        import torch
        dev = torch.device("cuda", self.device)
        H, W = self.data.height, self.data.width
        L = _lib.lib()
        planes = self.render_mattes(layers, want=self.MATTE_PLANES if ids is not None else ("alpha",))
        res = {}
        if ids is not None:
            m = matte(planes["id"], planes["coverage"], ids)
        if background is not None:
            if frame is None:
                frame = torch.from_numpy(np.ascontiguousarray(self.image, dtype=np.float64)).to(dev).to(torch.float32)
            over = composite(frame, planes["alpha"], background, want=("f32", "u8"))
        torch.cuda.synchronize(self.device)
        res["alpha"] = np.ascontiguousarray(planes["alpha"].cpu().numpy())
        ok = L.rtm_write_pfm(os.fsencode(fileName + "_alpha.pfm"), W, H, 1, res["alpha"].ctypes.data) == 1
        if ids is not None:
            res["matte"] = np.ascontiguousarray(m.cpu().numpy())
            grey = np.ascontiguousarray(np.repeat(res["matte"].astype(np.float64)[..., None], 3, axis=2))
            rgb8 = np.zeros(grey.shape, dtype=np.uint8)
            _lib.check(L.rtm_quantise(grey.ctypes.data, grey.size, rgb8.ctypes.data), "rtm_quantise")
            ok = ok and L.rtm_write_pfm(os.fsencode(fileName + "_matte.pfm"), W, H, 1, res["matte"].ctypes.data) == 1 \
                and L.rtm_write_bmp(os.fsencode(fileName + "_matte.bmp"), W, H, 3, rgb8.ctypes.data) == 1
        if background is not None:
            res["over"] = over["f32"]
            rgb8 = np.ascontiguousarray(over["u8"].cpu().numpy())
            ok = ok and L.rtm_write_bmp(os.fsencode(fileName + "_over.bmp"), W, H, 3, rgb8.ctypes.data) == 1 \
                and L.rtm_write_jpg(os.fsencode(fileName + "_over.jpg"), W, H, 3, rgb8.ctypes.data, 60) == 1
        if not ok:
            raise _lib.RtmError(-3, f"could not write the matte files of {fileName}")
        return res

    # ---- low-resolution preview at full size (rtm_upsample) -----------------------------------
    def preview(self, factor=2, denoise=True, want=("f32",), stream=None):
        """The frame traced at (width / factor) x (height / factor) — same camera, samples, super-samples, seed and mode, so
        factor^2 fewer paths — and brought to full size by upsample() at its default sigmas, guided by the first-hit AOVs at
        both resolutions.  On one stream: the low render, the low AOVs, denoise() at its defaults on the low frame (unless
        denoise=False), the full AOVs, the upsample.  Returns upsample()'s dict ("f32" / "u8" (H, W, 3) CUDA tensors);
        nothing waits for the stream.  factor is 2..8 and must divide both width and height (ValueError)."""
        f = int(factor)
        H, W = int(self.data.height), int(self.data.width)
        if not 2 <= f <= 8:
            raise ValueError(f"factor must be in 2..8, got {factor!r}")
        if W % f or H % f:
            raise ValueError(f"factor {f} does not divide the {W}x{H} frame")
        import torch
        _need_device("Renderer")
        dev = torch.device("cuda", self.device)
        s = _stream_of(stream, dev)
        w, h = W // f, H // f
        st = self.data.settings_c()
        st.width, st.height = w, h
        opt = self._options(0, h)
        L = _lib.lib()
        with torch.cuda.stream(s):  # allocated on the stream that uses them; render_aov and the filters take the current stream
            color = torch.empty((h, w, 3), dtype=torch.float32, device=dev)
            aov_low = {k: torch.empty(shape, dtype=dt, device=dev) for k, (shape, dt) in _aov_layout(h, w).items()}
            bufs = _aov_buffers(aov_low, h, w, dev, "aov[{k!r}]")
            hip_stream = C.c_void_p(s.cuda_stream)
            _lib.check(L.rtm_render_scene(C.byref(st), self._scene_handle(), C.byref(opt), None, C.c_void_p(color.data_ptr()),
                                          None, hip_stream, None), "rtm_render_scene")
            _lib.check(L.rtm_render_aov(C.byref(st), self._scene_handle(), C.byref(opt), C.byref(bufs), hip_stream),
                       "rtm_render_aov")
            if denoise:
                d = DENOISE_DEFAULTS  # (the module's denoise(): this method's flag has its name)
                prm = _lib.rtm_denoise_params(d["iterations"], d["sigma_color"], d["sigma_normal"], d["sigma_depth"])
                color = _denoise_call("rtm_denoise", prm, color, aov_low, ("f32",), ("f32", "u8"), None)["f32"]
            return upsample(color, aov_low, self.render_aov(), factor=f, want=want)

    def write_preview(self, fileName, factor=2, _keep=False):
        """<fileName>_preview.jpg (q=60) and <fileName>_preview.bmp: preview(factor), denoised at the low resolution,
        quantised on the device — what rtm_cli --preview writes.  Returns the (H, W, 3) uint8 pixels (Render's _keep: the
        float32 frame on the device instead, for the display stage; the files are the same)."""
        import torch
        out = self.preview(factor, want=("u8", "f32") if _keep else ("u8",))
        torch.cuda.synchronize(self.device)
        self.stream_status()
        rgb8 = np.ascontiguousarray(out["u8"].cpu().numpy())
        L = _lib.lib()
        H, W = self.data.height, self.data.width
        ok_j = L.rtm_write_jpg(os.fsencode(fileName + "_preview.jpg"), W, H, 3, rgb8.ctypes.data, 60)
        ok_b = L.rtm_write_bmp(os.fsencode(fileName + "_preview.bmp"), W, H, 3, rgb8.ctypes.data)
        if not (ok_j and ok_b):
            raise _lib.RtmError(-3, f"could not write {fileName}_preview.jpg/.bmp")
        return out["f32"] if _keep else rgb8

    # ---- host-buffer render (the blocking C entry point) ------------------------------------
    def render_rows(self, row_begin=0, row_end=None, want=("f64",), band=None):
        if self._device_scene is not None:
            raise RuntimeError("render_rows renders data.object from the host; this renderer has a device scene "
                               "(set_device_spheres): use render_rows_device, or set_device_spheres(None) first")
        row_end = self.data.height if row_end is None else row_end
        opt = self._options(row_begin, row_end, band)
        rows, W = _lib.lib().rtm_output_rows(C.byref(opt)), self.data.width
        out = {}
        if "f64" in want:
            out["f64"] = np.zeros((rows, W, 3), dtype=np.float64)
        if "f32" in want:
            out["f32"] = np.zeros((rows, W, 3), dtype=np.float32)
        if "u8" in want:
            out["u8"] = np.zeros((rows, W, 3), dtype=np.uint8)
        s = rtm_stats()
        ptr = lambda k: out[k].ctypes.data_as(C.c_void_p) if k in out else None
        if self.data.has_planes():  # rtm_render takes sphere arrays; any other object goes through rtm_render_objects
            st = self.data.settings_c()
            arr, n = self.data.objects_c()
            _lib.check(_lib.lib().rtm_render_objects(C.byref(st), arr, n, C.byref(opt), ptr("f64"), ptr("f32"),
                                                     ptr("u8"), C.byref(s)), "rtm_render_objects")
        else:
            st, arr, n = self.data.to_c()
            _lib.check(_lib.lib().rtm_render(C.byref(st), arr, n, C.byref(opt), ptr("f64"), ptr("f32"),
                                             ptr("u8"), C.byref(s)), "rtm_render")
        self.stats = s.as_dict()
        return out, self.stats

    def Render(self, fileName, passes=1, aov=False, denoise=False, adaptive=None, tonemap=False, preview=None, mattes=None, bloom=False,
               dof=None, resize=None, lens=None, grade=None, lut=None, firefly=None, local=False):
        """src/Renderer.cpp:200-258: render, quantise, write <fileName>.jpg and <fileName>.bmp.  passes > 1 renders the
        frame progressively on the device (Renderer.progressive): the same files and the same self.image.  aov=True also
        writes the first-hit feature buffers (write_aov: <fileName>_depth/_normal/_albedo.pfm, _normal/_albedo.bmp).
        denoise=True also writes <fileName>_denoised.jpg (q=60) and _denoised.bmp: the frame's f32 filtered by denoise() at
        the default parameters, guided by its AOVs (write_denoised); the plain files and self.image do not change.
        denoise="variance" writes instead <fileName>_denoised_var.jpg / .bmp and <fileName>_variance.pfm: the frame filtered
        by denoise_variance() at its default parameters, and its per-pixel variance estimate (write_denoised_variance).
        adaptive=T renders tile-adaptively (Renderer.adaptive, threshold T, the default min_samples) and also writes
        <fileName>_spp.pfm, the per-pixel sample count (write_spp); the AOV and denoised files then come from that frame.
        tonemap=True (or a dict of tonemap()'s parameters: op, transfer, exposure, key, white, dither) also writes
        <fileName>_display.bmp and <fileName>_display.jpg (q=60): the display transform (write_display) of the last stage
        asked for — the variance-denoised frame with denoise="variance", the denoised one with denoise=True, else the frame
        itself.  The plain files and self.image do not change.
        bloom=True (or a dict of bloom()'s parameters: threshold, knee, intensity, scatter, levels) blooms every frame the
        display transform is given (write_display's bloom), so the _display, _over_display and _preview_display files are
        those of the bloomed last stage.  It needs tonemap: linear HDR through the reference's quantiser would only clip.
        local=True (or a dict of tonemap_local()'s shadows, highlights, sigma, levels) replaces the tone curve of every frame the
        display transform is given by the local tone operator (write_display's local): exposure fusion on luminance at
        tonemap's exposure, then the transfer function and the dithered store.  It needs tonemap.
        grade=None or False: no grade.  grade (a dict of grade()'s parametric arguments: matrix, exposure, contrast, pivot,
        slope, offset, power, saturation, with temperature and tint as a shorthand for white_balance's matrix) grades every
        frame the display transform is given, in linear light after the bloom (write_display's grade).  lut (the path of a
        .cube file, or load_cube's dict) is a display-referred look applied to the display transform's float frame
        (write_display's lut).  Both need tonemap; a file that does not load raises before anything is rendered.
        dof=None or False: no depth of field.  dof=True (or a dict of focus_distance or focus_pixel, aperture, max_radius:
        write_dof's parameters) also writes
        <fileName>_dof.bmp and <fileName>_dof.jpg (q=60): the last stage asked for (variance-denoised, denoised, else the
        frame) defocused by the frame's depth plane, with the focus at the camera's target distance unless the dict says
        otherwise.  The defocused frame then is the last stage: with tonemap, bloom and the display transform take it (bloom
        is lens glare, so it comes after the lens), and so does mattes' background.
        lens=None or False: no lens.  lens=True (or a dict of lens()'s parameters: k1, k2, zoom, chroma, vignette, falloff,
        border, mode, filter; zoom="auto" takes lens_fit_zoom's value) also writes <fileName>_lens.bmp and <fileName>_lens.jpg
        (q=60): the last stage asked for (defocused, variance-denoised, denoised, else the frame) through that lens
        (write_lens).  The lens frame then is the last stage for resize, tonemap and bloom.  It does not combine with mattes:
        the coverage planes are not warped with the frame.
        resize=None: no resize.  resize=(W, H) or (W, H, filter) (width first, as rtm_cli --resize WxH; filter one of
        RESIZE_FILTERS, default "mitchell") also writes <fileName>_resized.bmp and <fileName>_resized.jpg (q=60): the last
        stage asked for (defocused, variance-denoised, denoised, else the frame) brought to W x H by resize() in linear light
        (write_resized).  The resized frame then is the last stage for tonemap and bloom, whose _display files have its size.
        It does not combine with mattes' background: the composite runs at the render's size.
        preview=F also writes <fileName>_preview.bmp and <fileName>_preview.jpg (q=60): the frame traced at 1 / F of the
        resolution in each axis, denoised there and upsampled by the AOVs (write_preview); with tonemap, the display transform
        of the preview as well, as <fileName>_preview_display.bmp / .jpg.  F must divide the width and the height.
        firefly=None or False: no firefly clamp.  firefly=True (or a dict of firefly()'s parameters: radius, rank, k, floor,
        repair) also writes <fileName>_firefly.bmp and <fileName>_firefly.jpg (q=60): the frame just rendered (plain, passes or
        adaptive) with its fireflies clamped and its non-finite pixels repaired (write_firefly).  The cleaned frame then is what
        every stage that follows takes: denoise, denoise="variance", dof, lens, resize, bloom and the display transform, and
        mattes' background.  The plain files and self.image do not change; the preview is a trace of its own and is not cleaned.
        mattes=True (or a dict of write_mattes' parameters: layers, ids, background) also writes <fileName>_alpha.pfm, with ids
        <fileName>_matte.pfm / .bmp, and with background <fileName>_over.bmp / .jpg: the last stage asked for (plain, denoised,
        variance-denoised) over that background; with tonemap, its display transform as well, as <fileName>_over_display.bmp /
        .jpg.  A bad value raises ValueError before anything is rendered; the other files and self.image do not change."""
        matte_prm = None
        if mattes is not None and mattes is not False:
            if mattes is not True and not isinstance(mattes, dict):
                raise ValueError(f"mattes is None, True or a dict of write_mattes' parameters, got {mattes!r}")
            matte_prm = {} if mattes is True else dict(mattes)
            unknown = set(matte_prm) - {"layers", "ids", "background"}
            if unknown:
                raise ValueError(f"mattes' parameters are ('layers', 'ids', 'background'), got {sorted(unknown)}")
            _matte_args(matte_prm.get("layers", MATTE_DEFAULTS["layers"]), matte_prm.get("ids"), matte_prm.get("background"),
                        frame_shape=(self.data.height, self.data.width))
        if preview is not None:
            f = int(preview)
            if not 2 <= f <= 8 or self.data.width % f or self.data.height % f:
                raise ValueError(f"preview is a factor in 2..8 that divides the {self.data.width}x{self.data.height} frame, "
                                 f"got {preview!r}")
        if isinstance(denoise, str) and denoise != "variance":
            raise ValueError(f'denoise is False, True or "variance", got {denoise!r}')
        display = None
        if tonemap is not False and tonemap is not None:
            if tonemap is not True and not isinstance(tonemap, dict):
                raise ValueError(f"tonemap is False, True or a dict of tonemap()'s parameters, got {tonemap!r}")
            display = {} if tonemap is True else dict(tonemap)
            unknown = set(display) - set(TONEMAP_DEFAULTS)
            if unknown:
                raise ValueError(f"tonemap's parameters are {tuple(TONEMAP_DEFAULTS)}, got {sorted(unknown)}")
            _tonemap_params(**display)  # a bad parameter raises here, before anything is rendered
        firefly_prm = _firefly_option(firefly)
        dof_prm = _dof_option(dof, self.data.width, self.data.height)
        if dof_prm is not None and dof_prm.get("focus_distance") is None:  # a miss raises here, before anything is rendered
            dof_prm["focus_distance"] = self.focus_distance(dof_prm.pop("focus_pixel", None))
        resize_prm = _resize_option(resize)
        if resize_prm is not None and matte_prm is not None and matte_prm.get("background") is not None:
            raise ValueError("resize does not combine with mattes' background: the composite runs at the render's size")
        lens_prm = _lens_option(lens, self.data.width, self.data.height)
        if lens_prm is not None and matte_prm is not None:
            raise ValueError("lens does not combine with mattes: the coverage planes are not warped with the frame")
        bloom_prm = _bloom_option(bloom)
        if bloom_prm is not None:
            if display is None:
                raise ValueError("bloom needs tonemap: it is applied to the frame the display transform shows")
            display["bloom"] = bloom_prm  # write_display's
        local_prm = _local_option(local)
        if local_prm is not None:
            if display is None:
                raise ValueError("local needs tonemap: it replaces the tone curve of the display transform")
            display["local"] = local_prm  # write_display's
        grade_prm, lut_prm = _grade_option(grade), _lut_option(lut)
        if grade_prm is not None or lut_prm is not None:
            if display is None:
                raise ValueError("grade and lut need tonemap: they are applied inside the display path")
            display["grade"] = grade_prm  # write_display's
            if lut_prm is not None:  # (as load_cube's dict, which write_display checks again)
                display["lut"] = {"table": lut_prm["table"], "domain_min": lut_prm["lut_domain"][0],
                                  "domain_max": lut_prm["lut_domain"][1], "interp": lut_prm["interp"]}
        if adaptive is not None:
            if passes > 1:
                raise ValueError("adaptive and passes > 1 do not combine")
            out, tile_samples, _ = self.adaptive(float(adaptive), want=("u8",))
            self.image = adaptive_preview(out["f64"].cpu().numpy(), tile_samples.cpu().numpy(), self.total_samples())
            rgb8 = np.ascontiguousarray(out["u8"].cpu().numpy())
            self.write_spp(fileName, tile_samples)
        elif passes > 1:
            last = None
            for _, out, st in self.progressive(passes=passes, want=("u8",)):
                last = out
            self.image = last["f64"].cpu().numpy()
            rgb8 = np.ascontiguousarray(last["u8"].cpu().numpy())
        elif self._device_scene is not None:  # set_device_spheres: the scene object, not data.object
            out, _ = self.render_rows_device(0, self.data.height, want=("f64", "u8"))
            self.image = out["f64"].cpu().numpy()
            rgb8 = np.ascontiguousarray(out["u8"].cpu().numpy())
        else:
            out, _ = self.render_rows(0, self.data.height, want=("f64", "u8"))
            self.image = out["f64"]
            rgb8 = np.ascontiguousarray(out["u8"])
        L = _lib.lib()
        H, W = self.data.height, self.data.width
        ok_j = L.rtm_write_jpg(os.fsencode(fileName + ".jpg"), W, H, 3, rgb8.ctypes.data, 60)
        ok_b = L.rtm_write_bmp(os.fsencode(fileName + ".bmp"), W, H, 3, rgb8.ctypes.data)
        if not (ok_j and ok_b):
            raise _lib.RtmError(-3, f"could not write {fileName}.jpg/.bmp")
        if aov:
            self.write_aov(fileName)
        frame = None  # the f32 frame the display stage shows, when it is not self.image
        keep = display is not None or (matte_prm is not None and matte_prm.get("background") is not None) or dof_prm is not None
        keep = keep or resize_prm is not None or lens_prm is not None
        if firefly_prm is not None:  # right after the render: every stage below takes the cleaned frame
            frame = self.write_firefly(fileName, **firefly_prm)
        if denoise == "variance":
            frame = self.write_denoised_variance(fileName, _keep=keep, frame=frame)
        elif denoise:
            frame = self.write_denoised(fileName, _keep=keep, frame=frame)
        if dof_prm is not None:
            frame = self.write_dof(fileName, frame=frame, **dof_prm)
        if lens_prm is not None:
            frame = self.write_lens(fileName, frame=frame, **lens_prm)
        if resize_prm is not None:
            frame = self.write_resized(fileName, frame=frame, **resize_prm)
        if display is not None:
            self.write_display(fileName, frame=frame, **display)
        if matte_prm is not None:
            over = self.write_mattes(fileName, frame=frame, **matte_prm).get("over")
            if over is not None and display is not None:
                self.write_display(fileName + "_over", frame=over, **display)
        if preview is not None:
            shown = self.write_preview(fileName, int(preview), _keep=display is not None)
            if display is not None:
                self.write_display(fileName + "_preview", frame=shown, **display)
        return rgb8

    def write_display(self, fileName, frame=None, bloom=None, grade=None, lut=None, local=None, **params):
        """<fileName>_display.bmp and <fileName>_display.jpg (q=60): the display transform tonemap(**params) (default: the
        ACES curve at automatic exposure, sRGB, dithered) of `frame`, an (H, W, 3) float32 CUDA tensor, or of self.image
        rounded to float like out_f32 — what rtm_cli --display writes.  bloom=True (or a dict of bloom()'s parameters) blooms
        the frame first, what rtm_cli --display --bloom writes; `frame` itself is left as it is.  grade (a dict of grade()'s
        parametric arguments: matrix, exposure, contrast, pivot, slope, offset, power, saturation, with temperature and tint as
        a shorthand for white_balance's matrix) grades the frame in linear light, after the bloom and before the display
        transform: what rtm_cli --display --grade-... writes.  lut (the path of a .cube file, or load_cube's dict, which may
        name an "interp") is a display-referred look: it is applied to the display transform's float frame, and the 8-bit
        pixels are then made from its result by a second tonemap() that only clamps and dithers (op "clamp", transfer
        "linear", exposure 0, the same dither): what rtm_cli --display --lut writes.  local=True (or a dict of
        tonemap_local()'s shadows, highlights, sigma, levels) replaces the tone curve by the local tone operator, after the
        grade: with exposure "auto" a statistics-only tonemap() of the frame gives the exposure on the device and the anchor
        is 1, with exposure EV the anchor is 2^EV; the fused frame then goes through a tonemap() that only clamps (op "clamp",
        the same transfer and dither, exposure 0).  `op` and `white` are then unused: what rtm_cli --display local writes.
        Returns the (H, W, 3) uint8 pixels."""
        import torch
        _tonemap_params(**params)
        bloom_prm = _bloom_option(bloom)
        grade_prm = _grade_option(grade)
        lut_prm = _lut_option(lut)
        local_prm = _local_option(local)
        if frame is None:
            dev = torch.device("cuda", self.device)
            frame = torch.from_numpy(np.ascontiguousarray(self.image, dtype=np.float64)).to(dev).to(torch.float32)
        if bloom_prm is not None:
            frame = _bloom(frame, **bloom_prm)["f32"]
        if grade_prm is not None:
            frame = _grade(frame, **grade_prm)["f32"]
        if local_prm is not None:  # the operator is the curve; what follows only clamps, encodes and stores
            auto = isinstance(params.get("exposure", TONEMAP_DEFAULTS["exposure"]), str)
            stats = tonemap(frame, want=("stats",), **params)["stats"] if auto else None
            anchor = 1.0 if auto else float(np.exp2(np.float32(params["exposure"])))
            frame = tonemap_local(frame, anchor=anchor, stats=stats, want=("f32",), **local_prm)["f32"]
            params = {"op": "clamp", "transfer": params.get("transfer", TONEMAP_DEFAULTS["transfer"]), "exposure": 0.0,
                      "dither": params.get("dither", TONEMAP_DEFAULTS["dither"])}
        if lut_prm is None:
            shown = tonemap(frame, want=("u8",), **params)["u8"]
        else:
            look = tonemap(frame, want=("f32",), **params)["f32"]
            table = torch.from_numpy(lut_prm["table"]).to(look.device)
            _grade(look, lut=table, lut_domain=lut_prm["lut_domain"], interp=lut_prm["interp"], out_f32=look)
            shown = tonemap(look, op="clamp", transfer="linear", exposure=0.0, dither=params.get("dither", TONEMAP_DEFAULTS["dither"]),
                            want=("u8",))["u8"]
        rgb8 = np.ascontiguousarray(shown.cpu().numpy())
        L = _lib.lib()
        H, W = rgb8.shape[:2]  # the frame's own size: the render's, unless it was resized
        ok_j = L.rtm_write_jpg(os.fsencode(fileName + "_display.jpg"), W, H, 3, rgb8.ctypes.data, 60)
        ok_b = L.rtm_write_bmp(os.fsencode(fileName + "_display.bmp"), W, H, 3, rgb8.ctypes.data)
        if not (ok_j and ok_b):
            raise _lib.RtmError(-3, f"could not write {fileName}_display.jpg/.bmp")
        return rgb8

    def write_firefly(self, fileName, frame=None, **params):
        """<fileName>_firefly.bmp and <fileName>_firefly.jpg (q=60): firefly(**params) of `frame`, an (H, W, 3) float32 CUDA
        tensor, or of self.image rounded to float like out_f32 — what rtm_cli --firefly writes.  params: firefly()'s radius,
        rank, k, floor, repair.  self.firefly_counts then holds what rtm_cli prints: {"clamped", "repaired", "pixels"},
        counted from the mask.  Returns the cleaned float32 frame on the device."""
        import torch
        params = _firefly_option(params or True)
        if frame is None:
            dev = torch.device("cuda", self.device)
            frame = torch.from_numpy(np.ascontiguousarray(self.image, dtype=np.float64)).to(dev).to(torch.float32)
        out = _firefly(frame, want=("f32", "u8", "mask"), **params)
        rgb8 = np.ascontiguousarray(out["u8"].cpu().numpy())
        mask = out["mask"].cpu().numpy()
        self.firefly_counts = {"clamped": int((mask == 1).sum()), "repaired": int((mask == 2).sum()), "pixels": int(mask.size)}
        L = _lib.lib()
        H, W = rgb8.shape[:2]
        ok_j = L.rtm_write_jpg(os.fsencode(fileName + "_firefly.jpg"), W, H, 3, rgb8.ctypes.data, 60)
        ok_b = L.rtm_write_bmp(os.fsencode(fileName + "_firefly.bmp"), W, H, 3, rgb8.ctypes.data)
        if not (ok_j and ok_b):
            raise _lib.RtmError(-3, f"could not write {fileName}_firefly.jpg/.bmp")
        return out["f32"]

    def focus_distance(self, pixel=None):
        """A focus distance for defocus(), in the depth plane's units.  Without a pixel: |camera.target - camera.origin|,
        computed in double and rounded to float — the look-at point is in focus (no device use).  pixel=(x, y): the depth AOV
        at that pixel, what the primary ray through it hits first; a pixel outside the frame or one whose ray misses is a
        ValueError."""
        if pixel is None:
            cam = self.data.camera
            zf = float(np.float32(np.sqrt(sum((float(t) - float(o)) ** 2 for t, o in zip(cam.target, cam.origin)))))
            if not (np.isfinite(zf) and zf > 0.0):
                raise ValueError("the camera's target is its origin (or out of float's range): there is no target distance")
            return zf
        x, y = _focus_pixel(pixel, self.data.width, self.data.height)
        z = float(self.render_aov(y, y + 1, want=("depth",))["depth"][0, x].item())
        if not (np.isfinite(z) and z > 0.0):
            raise ValueError(f"the focus pixel ({x}, {y}) is a miss: its primary ray hits nothing")
        return z

    def write_dof(self, fileName, frame=None, focus_distance=None, focus_pixel=None, aperture=_lib.DEFOCUS_DEFAULTS["aperture"],
                  max_radius=_lib.DEFOCUS_DEFAULTS["max_radius"]):
        """<fileName>_dof.bmp and <fileName>_dof.jpg (q=60): defocus() of `frame`, an (H, W, 3) float32 CUDA tensor, or of
        self.image rounded to float like out_f32, by the frame's depth AOV — what rtm_cli --dof writes.  The focus is
        focus_distance, else the depth at focus_pixel=(x, y), else the camera's target distance (Renderer.focus_distance).
        Returns the defocused float32 frame on the device."""
        import torch
        if focus_distance is not None and focus_pixel is not None:
            raise ValueError("write_dof takes focus_distance or focus_pixel, not both")
        zf = self.focus_distance(focus_pixel) if focus_distance is None else focus_distance
        _defocus_params(zf, aperture, max_radius)
        if frame is None:
            dev = torch.device("cuda", self.device)
            frame = torch.from_numpy(np.ascontiguousarray(self.image, dtype=np.float64)).to(dev).to(torch.float32)
        depth = self.render_aov(want=("depth",))["depth"]
        out = defocus(frame, depth, zf, aperture, max_radius, want=("f32", "u8"))
        rgb8 = np.ascontiguousarray(out["u8"].cpu().numpy())
        L = _lib.lib()
        H, W = self.data.height, self.data.width
        ok_j = L.rtm_write_jpg(os.fsencode(fileName + "_dof.jpg"), W, H, 3, rgb8.ctypes.data, 60)
        ok_b = L.rtm_write_bmp(os.fsencode(fileName + "_dof.bmp"), W, H, 3, rgb8.ctypes.data)
        if not (ok_j and ok_b):
            raise _lib.RtmError(-3, f"could not write {fileName}_dof.jpg/.bmp")
        return out["f32"]

    def write_lens(self, fileName, frame=None, **params):
        """<fileName>_lens.bmp and <fileName>_lens.jpg (q=60): lens(**params) of `frame`, an (H, W, 3) float32 CUDA tensor, or
        of self.image rounded to float like out_f32 — what rtm_cli --lens writes.  params: lens()'s k1, k2, zoom, chroma,
        vignette, falloff, border, mode, filter, with zoom="auto" for lens_fit_zoom's value.  Returns the float32 frame on the
        device."""
        import torch
        params = _lens_option(params or True, self.data.width, self.data.height)
        if frame is None:
            dev = torch.device("cuda", self.device)
            frame = torch.from_numpy(np.ascontiguousarray(self.image, dtype=np.float64)).to(dev).to(torch.float32)
        out = _lens(frame, want=("f32", "u8"), **params)
        rgb8 = np.ascontiguousarray(out["u8"].cpu().numpy())
        L = _lib.lib()
        H, W = rgb8.shape[:2]
        ok_j = L.rtm_write_jpg(os.fsencode(fileName + "_lens.jpg"), W, H, 3, rgb8.ctypes.data, 60)
        ok_b = L.rtm_write_bmp(os.fsencode(fileName + "_lens.bmp"), W, H, 3, rgb8.ctypes.data)
        if not (ok_j and ok_b):
            raise _lib.RtmError(-3, f"could not write {fileName}_lens.jpg/.bmp")
        return out["f32"]

    def write_resized(self, fileName, size, frame=None, filter=_lib.RESIZE_DEFAULTS["filter"]):
        """<fileName>_resized.bmp and <fileName>_resized.jpg (q=60): resize() of `frame`, an (h, w, 3) float32 CUDA tensor, or
        of self.image rounded to float like out_f32, to size = (H, W) (height first, as resize()) — what rtm_cli --resize
        writes.  Returns the resized float32 frame on the device."""
        import torch
        _resize_args(size, filter)
        if frame is None:
            dev = torch.device("cuda", self.device)
            frame = torch.from_numpy(np.ascontiguousarray(self.image, dtype=np.float64)).to(dev).to(torch.float32)
        out = resize(frame, size, filter, want=("f32", "u8"))
        rgb8 = np.ascontiguousarray(out["u8"].cpu().numpy())
        L = _lib.lib()
        H, W = rgb8.shape[:2]
        ok_j = L.rtm_write_jpg(os.fsencode(fileName + "_resized.jpg"), W, H, 3, rgb8.ctypes.data, 60)
        ok_b = L.rtm_write_bmp(os.fsencode(fileName + "_resized.bmp"), W, H, 3, rgb8.ctypes.data)
        if not (ok_j and ok_b):
            raise _lib.RtmError(-3, f"could not write {fileName}_resized.jpg/.bmp")
        return out["f32"]

    def write_denoised(self, fileName, _keep=False, frame=None):
        """<fileName>_denoised.jpg (q=60) and <fileName>_denoised.bmp: self.image (the frame just rendered) rounded to float
        like out_f32, filtered by denoise() at the default parameters with the frame's four AOVs as guides, quantised on
        the device — what rtm_cli --denoise writes.  Returns the (H, W, 3) uint8 pixels (Render's _keep: the filtered float32
        frame on the device instead, for the display stage; the files are the same).  frame: an (H, W, 3) float32 CUDA tensor
        to filter instead of self.image (Render's: the frame write_firefly cleaned)."""
        import torch
        dev = torch.device("cuda", self.device)
        color = frame
        if color is None:
            color = torch.from_numpy(np.ascontiguousarray(self.image, dtype=np.float64)).to(dev).to(torch.float32)
        guides = self.render_aov()
        out = denoise(color, guides, want=("u8", "f32") if _keep else ("u8",))
        rgb8 = np.ascontiguousarray(out["u8"].cpu().numpy())
        L = _lib.lib()
        H, W = self.data.height, self.data.width
        ok_j = L.rtm_write_jpg(os.fsencode(fileName + "_denoised.jpg"), W, H, 3, rgb8.ctypes.data, 60)
        ok_b = L.rtm_write_bmp(os.fsencode(fileName + "_denoised.bmp"), W, H, 3, rgb8.ctypes.data)
        if not (ok_j and ok_b):
            raise _lib.RtmError(-3, f"could not write {fileName}_denoised.jpg/.bmp")
        return out["f32"] if _keep else rgb8

    def write_denoised_variance(self, fileName, _keep=False, frame=None):
        """<fileName>_denoised_var.jpg (q=60), <fileName>_denoised_var.bmp and <fileName>_variance.pfm: self.image rounded to
        float like out_f32, filtered by denoise_variance() at the default parameters with the frame's four AOVs as guides,
        and the variance estimate v0 — what rtm_cli --denoise-variance writes.  Returns the (H, W, 3) uint8 pixels (Render's
        _keep and frame: as write_denoised)."""
        import torch
        dev = torch.device("cuda", self.device)
        color = frame
        if color is None:
            color = torch.from_numpy(np.ascontiguousarray(self.image, dtype=np.float64)).to(dev).to(torch.float32)
        out = denoise_variance(color, self.render_aov(), want=("u8", "var", "f32") if _keep else ("u8", "var"))
        rgb8 = np.ascontiguousarray(out["u8"].cpu().numpy())
        var = np.ascontiguousarray(out["var"].cpu().numpy())
        L = _lib.lib()
        H, W = self.data.height, self.data.width
        ok = L.rtm_write_jpg(os.fsencode(fileName + "_denoised_var.jpg"), W, H, 3, rgb8.ctypes.data, 60) \
            and L.rtm_write_bmp(os.fsencode(fileName + "_denoised_var.bmp"), W, H, 3, rgb8.ctypes.data) \
            and L.rtm_write_pfm(os.fsencode(fileName + "_variance.pfm"), W, H, 1, var.ctypes.data)
        if not ok:
            raise _lib.RtmError(-3, f"could not write {fileName}_denoised_var.jpg/.bmp or {fileName}_variance.pfm")
        return out["f32"] if _keep else rgb8


# ---- what the stage wrappers below do alike: one helper per step ----------------------------------
def _need_device(who):
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError(f"{who} needs a HIP device; there is no CPU fallback")


def _check_want(want, outputs):
    unknown = set(want) - set(outputs)
    if unknown or not want:
        raise ValueError(f"want names outputs among {outputs}, got {tuple(want)}")


def _stream_of(stream, dev):
    """A torch stream for `stream`: a torch.cuda.Stream, a raw hipStream_t handle, or None for the current stream of `dev`."""
    import torch
    if stream is None:
        return torch.cuda.current_stream(dev)
    return stream if isinstance(stream, torch.cuda.Stream) else torch.cuda.ExternalStream(int(stream), device=dev)


def _frame_size(color, name, dims="(H, W, 3)", non_empty=False):
    """(H, W) of `color`, which must be a contiguous (H, W, 3) float32 CUDA tensor; the ValueError names it as the caller does."""
    import torch
    if not (isinstance(color, torch.Tensor) and color.is_cuda and color.dtype == torch.float32 and color.dim() == 3
            and color.shape[2] == 3 and color.is_contiguous() and (color.numel() > 0 or not non_empty)):
        raise ValueError(f"{name} must be a contiguous{', non-empty' if non_empty else ''} {dims} float32 CUDA tensor")
    return int(color.shape[0]), int(color.shape[1])


def _aov_layout(rows, cols):
    """Renderer.render_aov's planes at rows x cols: name -> (shape, dtype), in Renderer.AOV_PLANES' order."""
    import torch
    return {"depth": ((rows, cols), torch.float32), "normal": ((rows, cols, 3), torch.float32),
            "albedo": ((rows, cols, 3), torch.float32), "object": ((rows, cols), torch.int32)}


def _check_planes(names):
    unknown = set(names) - set(Renderer.AOV_PLANES)
    if unknown:
        raise ValueError(f"unknown AOV plane(s) {sorted(unknown)}; the planes are {Renderer.AOV_PLANES}")


def _aov_buffers(aov, rows, cols, dev, label):
    """An rtm_aov_buffers of the dict's planes (a None entry: no plane), each a contiguous tensor of _aov_layout(rows, cols)
    on `dev`.  `label` names plane k in the ValueError: a format string over k, rows and cols."""
    import torch
    layout = _aov_layout(rows, cols)
    bufs = _lib.rtm_aov_buffers()
    for k, v in aov.items():
        if v is None:
            continue
        shape, dtype = layout[k]
        if not (isinstance(v, torch.Tensor) and v.device == dev and v.dtype == dtype and tuple(v.shape) == shape
                and v.is_contiguous()):
            raise ValueError(f"{label.format(k=k, rows=rows, cols=cols)} must be a contiguous {shape} {dtype} tensor on {dev}")
        setattr(bufs, k, v.data_ptr())
    return bufs


def _stage_tensors(s, dev, want, outputs, work_bytes=0, out_f32=None):
    """The work buffer of `work_bytes` (0: none) and, of `outputs` (name -> (shape, dtype)), the tensors named in `want`,
    allocated under stream `s`, the stream that uses them: the caching allocator then orders any reuse.  out_f32: the
    caller's tensor for "f32".  Returns (out, ptr): the outputs' dict, and ptr(name) -> data pointer or None, which also
    knows "work"."""
    import torch
    with torch.cuda.stream(s):
        held = {"work": torch.empty(work_bytes, dtype=torch.uint8, device=dev) if work_bytes else None}
        out = {k: out_f32 if k == "f32" and out_f32 is not None else torch.empty(shape, dtype=dt, device=dev)
               for k, (shape, dt) in outputs.items() if k in want}
    held.update(out)
    return out, lambda k: held[k].data_ptr() if held.get(k) is not None else None


def _check_out_f32(out_f32, want, H, W, dev):
    import torch
    if out_f32 is None:
        return
    if "f32" not in want:
        raise ValueError('out_f32 is given but "f32" is not in want')
    if not (isinstance(out_f32, torch.Tensor) and out_f32.device == dev and out_f32.dtype == torch.float32
            and tuple(out_f32.shape) == (H, W, 3) and out_f32.is_contiguous()):
        raise ValueError(f"out_f32 must be a contiguous ({H}, {W}, 3) float32 tensor on {dev}")


def _pair_shape(a, b):
    """compare() and flip(): a and b are (H, W, 3) frames of one shape (any array type: no device use)."""
    shape_a, shape_b = tuple(getattr(a, "shape", ())), tuple(getattr(b, "shape", ()))
    if len(shape_a) != 3 or shape_a[2] != 3 or shape_a[0] < 1 or shape_a[1] < 1:
        raise ValueError(f"a must be an (H, W, 3) frame, got shape {shape_a}")
    if shape_a != shape_b:
        raise ValueError(f"a and b must have the same shape, got {shape_a} and {shape_b}")


def _pair_device(a, b):
    """compare() and flip(): a and b are contiguous CUDA tensors on one device; returns (H, W, device)."""
    import torch
    for name, v in (("a", a), ("b", b)):
        if not (isinstance(v, torch.Tensor) and v.is_cuda and v.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous CUDA tensor")
    if a.device != b.device:
        raise ValueError(f"a and b must be on one device, got {a.device} and {b.device}")
    return int(a.shape[0]), int(a.shape[1]), a.device


# include/rtm.h: RTM_DENOISE_DEFAULTS
DENOISE_DEFAULTS = {"iterations": 4, "sigma_color": 16.0, "sigma_normal": 64.0, "sigma_depth": 0.05}


def denoise(color, aov=None, iterations=DENOISE_DEFAULTS["iterations"], sigma_color=DENOISE_DEFAULTS["sigma_color"],
            sigma_normal=DENOISE_DEFAULTS["sigma_normal"], sigma_depth=DENOISE_DEFAULTS["sigma_depth"], want=("f32",),
            stream=None):
    """The à-trous denoiser (include/rtm.h: rtm_denoise) on the device.  `color` is an (H, W, 3) float32 torch CUDA tensor;
    `aov` a dict like Renderer.render_aov returns ("depth" (H, W) float32, "normal" / "albedo" (H, W, 3) float32, "object"
    (H, W) int32), missing planes switch their terms off.  Returns {"f32": (H, W, 3) float32, "u8": (H, W, 3) uint8} for
    the names in `want`.  Enqueued on `stream` (a torch.cuda.Stream or a raw hipStream_t handle; default: the current
    stream) with a work buffer allocated here; nothing waits for it."""
    return _denoise_call("rtm_denoise", _lib.rtm_denoise_params(int(iterations), float(sigma_color), float(sigma_normal),
                                                               float(sigma_depth)), color, aov, want, ("f32", "u8"), stream)


# include/rtm.h: RTM_DENOISE_VAR_DEFAULTS
DENOISE_VAR_DEFAULTS = {"iterations": 5, "sigma_lum": 4.0, "sigma_normal": 64.0, "sigma_depth": 0.05}


def denoise_variance(color, aov=None, iterations=DENOISE_VAR_DEFAULTS["iterations"], sigma_lum=DENOISE_VAR_DEFAULTS["sigma_lum"],
                     sigma_normal=DENOISE_VAR_DEFAULTS["sigma_normal"], sigma_depth=DENOISE_VAR_DEFAULTS["sigma_depth"],
                     want=("f32",), stream=None):
    """The variance-guided à-trous denoiser (include/rtm.h: rtm_denoise_variance) on the device, for frames whose noise is
    uneven: arguments and result as denoise(), with sigma_lum (relative to each pixel's own standard deviation) in place of
    sigma_color, and "var" accepted in `want`: the (H, W) float32 variance estimate v0 of the demodulated luminance.  With
    want=("var",) alone nothing is filtered."""
    return _denoise_call("rtm_denoise_variance", _lib.rtm_denoise_var_params(int(iterations), float(sigma_lum), float(sigma_normal),
                                                                            float(sigma_depth)), color, aov, want,
                         ("f32", "u8", "var"), stream)


def _denoise_call(entry, prm, color, aov, want, outputs, stream):
    """denoise() and denoise_variance(): the checks of the tensors, the work buffer and outputs, and the library call."""
    import torch
    _need_device("denoise")
    _check_want(want, outputs)
    H, W = _frame_size(color, "color")
    dev = color.device
    aov = {} if aov is None else aov
    _check_planes(aov)
    guides = _aov_buffers(aov, H, W, dev, "aov[{k!r}]")
    s = _stream_of(stream, dev)
    L = _lib.lib()
    specs = {"f32": ((H, W, 3), torch.float32), "u8": ((H, W, 3), torch.uint8), "var": ((H, W), torch.float32)}
    out, ptr = _stage_tensors(s, dev, want, specs, max(1, getattr(L, entry + "_work_bytes")(W, H)))
    tail = (ptr("var"),) if "var" in outputs else ()
    _lib.check(getattr(L, entry)(C.byref(prm), W, H, dev.index, color.data_ptr(), C.byref(guides), ptr("work"),
                                 ptr("f32"), ptr("u8"), *tail, C.c_void_p(s.cuda_stream)), entry)
    return out


# include/rtm.h: RTM_UPSAMPLE_DEFAULTS
UPSAMPLE_DEFAULTS = {"factor": 2, "sigma_spatial": 0.5, "sigma_normal": 64.0, "sigma_depth": 0.05}


def upsample(color_low, aov_low=None, aov_high=None, factor=UPSAMPLE_DEFAULTS["factor"],
             sigma_spatial=UPSAMPLE_DEFAULTS["sigma_spatial"], sigma_normal=UPSAMPLE_DEFAULTS["sigma_normal"],
             sigma_depth=UPSAMPLE_DEFAULTS["sigma_depth"], want=("f32",), stream=None):
    """The AOV-guided upsampler (include/rtm.h: rtm_upsample) on the device.  `color_low` is an (h, w, 3) float32 torch CUDA
    tensor; `aov_low` / `aov_high` are dicts like Renderer.render_aov returns, at (h, w) and at (factor h, factor w); a plane
    guides the filter when both hold it, and a plane in one of them only is a ValueError.  Returns {"f32": (H, W, 3) float32,
    "u8": (H, W, 3) uint8} for the names in `want`.  Enqueued on `stream` (a torch.cuda.Stream or a raw hipStream_t handle;
    default: the current stream) with a work buffer allocated here; nothing waits for it."""
    import torch
    _need_device("upsample")
    _check_want(want, ("f32", "u8"))
    h, w = _frame_size(color_low, "color_low", "(h, w, 3)")
    f = int(factor)
    H, W = f * h, f * w
    dev = color_low.device
    aov_low = {k: v for k, v in (aov_low or {}).items() if v is not None}
    aov_high = {k: v for k, v in (aov_high or {}).items() if v is not None}
    _check_planes(set(aov_low) | set(aov_high))
    if set(aov_low) != set(aov_high):
        raise ValueError(f"plane(s) {sorted(set(aov_low) ^ set(aov_high))} are given at one resolution only")
    guides = [_aov_buffers(aov, rows, cols, dev, "the {rows}x{cols} plane {k!r}")
              for aov, (rows, cols) in ((aov_low, (h, w)), (aov_high, (H, W)))]
    s = _stream_of(stream, dev)
    L = _lib.lib()
    prm = _lib.rtm_upsample_params(f, float(sigma_spatial), float(sigma_normal), float(sigma_depth))
    full = (max(H, 0), max(W, 0), 3)
    out, ptr = _stage_tensors(s, dev, want, {"f32": (full, torch.float32), "u8": (full, torch.uint8)},
                              max(16, L.rtm_upsample_work_bytes(w, h)))
    _lib.check(L.rtm_upsample(C.byref(prm), w, h, dev.index, color_low.data_ptr(), C.byref(guides[0]), C.byref(guides[1]),
                              ptr("work"), ptr("f32"), ptr("u8"), C.c_void_p(s.cuda_stream)), "rtm_upsample")
    return out


# include/rtm.h: RTM_TONEMAP_DEFAULTS (exposure "auto" is auto_exposure 1 at ev 0)
# include/rtm.h: RTM_MATTE_DEFAULT_LAYERS
MATTE_DEFAULTS = {"layers": 4}


def _matte_layers(layers):
    if isinstance(layers, bool) or not isinstance(layers, (int, np.integer)) or not 1 <= int(layers) <= 8:
        raise ValueError(f"layers is an integer in 1..8, got {layers!r}")
    return int(layers)


def _matte_ids(ids):
    """matte()'s id list as a tuple of 1..64 ints that fit an int32; a ValueError otherwise.  No device use."""
    try:
        ids = tuple(ids)
    except TypeError:
        raise ValueError(f"ids is a list of 1..64 object indices, got {ids!r}") from None
    if not 1 <= len(ids) <= 64:
        raise ValueError(f"ids is a list of 1..64 object indices, got {len(ids)} of them")
    for i in ids:
        if isinstance(i, bool) or not isinstance(i, (int, np.integer)) or not -2 ** 31 <= int(i) < 2 ** 31:
            raise ValueError(f"ids holds integers that fit an int32, got {i!r}")
    return tuple(int(i) for i in ids)


def _matte_background(background, frame_shape=None):
    """composite()'s background: a colour as a tuple of three finite floats, or the (H, W, 3) float32 CUDA tensor itself; a
    ValueError otherwise.  No device use."""
    if hasattr(background, "is_cuda"):
        import torch
        if not (background.is_cuda and background.dtype == torch.float32 and background.dim() == 3 and background.shape[2] == 3
                and background.is_contiguous()):
            raise ValueError("background must be a colour or a contiguous (H, W, 3) float32 CUDA tensor")
        if frame_shape is not None and tuple(background.shape[:2]) != tuple(frame_shape):
            raise ValueError(f"background is {tuple(background.shape[:2])}, the frame {tuple(frame_shape)}")
        return background
    try:
        rgb = tuple(float(v) for v in background)
    except (TypeError, ValueError):
        raise ValueError(f"background is a colour (three numbers) or an (H, W, 3) float32 CUDA tensor, got {background!r}") from None
    if len(rgb) != 3 or not all(np.isfinite(v) for v in rgb):
        raise ValueError(f"background is a colour of three finite numbers, got {background!r}")
    return rgb


def _matte_args(layers=MATTE_DEFAULTS["layers"], ids=None, background=None, frame_shape=None):
    """Renderer.write_mattes' parameters, checked: (layers, ids or None, background or None).  No device use."""
    return (_matte_layers(layers), None if ids is None else _matte_ids(ids),
            None if background is None else _matte_background(background, frame_shape))


def matte(layer_id, layer_coverage, ids, stream=None):
    """The antialiased matte of a set of objects (include/rtm.h: rtm_matte) on the device.  layer_id (L, H, W) int32 and
    layer_coverage (L, H, W) float32 are Renderer.render_mattes' "id" and "coverage" of a whole frame, L in 1..8; ids a list
    of 1..64 object indices (unsorted, duplicates harmless, a negative entry selects nothing) or an int32 CUDA tensor of them.
    Returns the (H, W) float32 matte: per pixel the summed coverage of the listed objects, at most 1.  Enqueued on `stream` (a
    torch.cuda.Stream or a raw hipStream_t handle; default: the current stream); nothing waits for it."""
    on_device = hasattr(ids, "is_cuda")
    if not on_device:
        ids = _matte_ids(ids)
    import torch
    if not (isinstance(layer_id, torch.Tensor) and layer_id.is_cuda and layer_id.dtype == torch.int32 and layer_id.dim() == 3
            and layer_id.is_contiguous() and 1 <= layer_id.shape[0] <= 8):
        raise ValueError("layer_id must be a contiguous (L, H, W) int32 CUDA tensor, L in 1..8")
    if not (isinstance(layer_coverage, torch.Tensor) and layer_coverage.device == layer_id.device and layer_coverage.dtype == torch.float32
            and layer_coverage.shape == layer_id.shape and layer_coverage.is_contiguous()):
        raise ValueError("layer_coverage must be a contiguous float32 tensor of layer_id's shape on its device")
    dev = layer_id.device
    if on_device and not (ids.device == dev and ids.dtype == torch.int32 and ids.dim() == 1 and 1 <= ids.numel() <= 64
                          and ids.is_contiguous()):
        raise ValueError("ids on the device must be a contiguous int32 vector of 1..64 entries on layer_id's device")
    layers, H, W = (int(v) for v in layer_id.shape)
    if H == 0 or W == 0:
        raise ValueError("the frame is empty")
    s = _stream_of(stream, dev)
    with torch.cuda.stream(s):  # allocated on the stream that uses them: the caching allocator then orders any reuse
        sel = ids if on_device else torch.tensor(ids, dtype=torch.int32, device=dev)
        out = torch.empty((H, W), dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().rtm_matte(W, H, layers, dev.index, layer_id.data_ptr(), layer_coverage.data_ptr(), sel.data_ptr(),
                                    int(sel.numel()), out.data_ptr(), C.c_void_p(s.cuda_stream)), "rtm_matte")
    return out


def composite(color, alpha, background=(0, 0, 0), want=("f32",), stream=None, out_f32=None):
    """A traced frame over a background (include/rtm.h: rtm_composite) on the device: out = color + (1 - alpha) * background per
    channel in float; the frame already holds zero for the part of a pixel that missed.  color (H, W, 3) float32 and alpha
    (H, W) float32 CUDA tensors (Renderer.render_mattes' "alpha"); background a colour or an (H, W, 3) float32 CUDA tensor.
    Returns a dict of the names in `want`: "f32" (H, W, 3) float32, "u8" (H, W, 3) uint8 (rtm_quantise of it).  out_f32: the
    tensor to write "f32" into; `color` itself composites in place.  Enqueued on `stream` (a torch.cuda.Stream or a raw
    hipStream_t handle; default: the current stream); nothing waits for it."""
    background = _matte_background(background)
    _check_want(want, ("f32", "u8"))
    import torch
    H, W = _frame_size(color, "color", non_empty=True)
    dev = color.device
    if not (isinstance(alpha, torch.Tensor) and alpha.device == dev and alpha.dtype == torch.float32
            and tuple(alpha.shape) == (H, W) and alpha.is_contiguous()):
        raise ValueError(f"alpha must be a contiguous ({H}, {W}) float32 tensor on {dev}")
    image = isinstance(background, torch.Tensor)
    if image and not (background.device == dev and tuple(background.shape) == (H, W, 3)):
        raise ValueError(f"a background image must be ({H}, {W}, 3) on {dev}")
    _check_out_f32(out_f32, want, H, W, dev)
    s = _stream_of(stream, dev)
    out, ptr = _stage_tensors(s, dev, want, {"f32": ((H, W, 3), torch.float32), "u8": ((H, W, 3), torch.uint8)}, out_f32=out_f32)
    prm = _lib.rtm_composite_params((C.c_float * 3)(*((0.0, 0.0, 0.0) if image else background)))
    _lib.check(_lib.lib().rtm_composite(C.byref(prm), W, H, dev.index, color.data_ptr(), alpha.data_ptr(),
                                        background.data_ptr() if image else None, ptr("f32"), ptr("u8"),
                                        C.c_void_p(s.cuda_stream)), "rtm_composite")
    return out


TONEMAP_DEFAULTS = {"op": "aces", "transfer": "srgb", "exposure": "auto", "key": 0.18, "white": 0.0, "dither": True}


def _tonemap_params(op=TONEMAP_DEFAULTS["op"], transfer=TONEMAP_DEFAULTS["transfer"], exposure=TONEMAP_DEFAULTS["exposure"],
                    key=TONEMAP_DEFAULTS["key"], white=TONEMAP_DEFAULTS["white"], dither=TONEMAP_DEFAULTS["dither"]):
    """tonemap()'s parameters as an rtm_tonemap_params; a ValueError names what the library would refuse.  No device use."""
    if op not in _lib.TONEMAP_OPS:
        raise ValueError(f"op is one of {tuple(_lib.TONEMAP_OPS)}, got {op!r}")
    if transfer not in _lib.TRANSFERS:
        raise ValueError(f"transfer is one of {tuple(_lib.TRANSFERS)}, got {transfer!r}")
    auto = isinstance(exposure, str)
    if auto and exposure != "auto":
        raise ValueError(f'exposure is "auto" or a number of stops (EV), got {exposure!r}')
    if not auto and isinstance(exposure, bool):
        raise ValueError(f'exposure is "auto" or a number of stops (EV), got {exposure!r}')
    ev = 0.0 if auto else float(exposure)
    key, white = float(key), float(white)
    if not (np.isfinite(ev) and abs(ev) <= 32.0):
        raise ValueError(f"exposure must be finite and within +-32 stops, got {exposure!r}")
    if not (np.isfinite(key) and key > 0.0):
        raise ValueError(f"key must be finite and positive, got {key!r}")
    if not (np.isfinite(white) and white >= 0.0):
        raise ValueError(f"white must be finite and non-negative, got {white!r}")
    if not isinstance(dither, (bool, np.bool_)) and dither not in (0, 1):
        raise ValueError(f"dither is True or False, got {dither!r}")
    return _lib.rtm_tonemap_params(_lib.TONEMAP_OPS[op], _lib.TRANSFERS[transfer], int(auto), int(bool(dither)), ev, key, white)


def tonemap(color, op=TONEMAP_DEFAULTS["op"], transfer=TONEMAP_DEFAULTS["transfer"], exposure=TONEMAP_DEFAULTS["exposure"],
            key=TONEMAP_DEFAULTS["key"], white=TONEMAP_DEFAULTS["white"], dither=TONEMAP_DEFAULTS["dither"], want=("u8",),
            stream=None, out_f32=None):
    """The display transform (include/rtm.h: rtm_tonemap) on the device.  `color` is an (H, W, 3) float32 torch CUDA tensor
    (any 4-byte-aligned contiguous view).  op "clamp" | "reinhard" | "aces"; transfer "srgb" | "linear"; exposure "auto"
    (Reinhard's log-average key: E = key / L_avg) or a number of stops EV (E = 2^EV); white: Reinhard's white point, 0 = the
    exposed frame maximum; dither: the ordered 8 x 8 dither of the 8-bit store.  Returns a dict of the names in `want`:
    "f32" (H, W, 3) float32, "u8" (H, W, 3) uint8, "stats" a 4-word int32 tensor holding the bits of rtm_tonemap_stats
    (tonemap_stats() reads it on the host).  out_f32: the tensor to write "f32" into; `color` itself maps in place.
    Enqueued on `stream` (a torch.cuda.Stream or a raw hipStream_t handle; default: the current stream) with a work buffer
    allocated here; nothing waits for it and nothing is copied to the host."""
    prm = _tonemap_params(op, transfer, exposure, key, white, dither)
    _check_want(want, ("f32", "u8", "stats"))
    import torch
    _need_device("tonemap")
    H, W = _frame_size(color, "color")
    dev = color.device
    _check_out_f32(out_f32, want, H, W, dev)
    s = _stream_of(stream, dev)
    L = _lib.lib()
    specs = {"f32": ((H, W, 3), torch.float32), "u8": ((H, W, 3), torch.uint8), "stats": (4, torch.int32)}
    out, ptr = _stage_tensors(s, dev, want, specs, max(256, L.rtm_tonemap_work_bytes(W, H)), out_f32=out_f32)
    _lib.check(L.rtm_tonemap(C.byref(prm), W, H, dev.index, color.data_ptr(), ptr("work"), ptr("f32"), ptr("u8"),
                             ptr("stats"), C.c_void_p(s.cuda_stream)), "rtm_tonemap")
    return out


# include/rtm.h: RTM_BLOOM_DEFAULTS
BLOOM_DEFAULTS = {"threshold": 1.0, "knee": 0.5, "intensity": 0.2, "scatter": 0.7, "levels": 6}


def _bloom_params(threshold=BLOOM_DEFAULTS["threshold"], knee=BLOOM_DEFAULTS["knee"], intensity=BLOOM_DEFAULTS["intensity"],
                  scatter=BLOOM_DEFAULTS["scatter"], levels=BLOOM_DEFAULTS["levels"]):
    """bloom()'s parameters as an rtm_bloom_params; a ValueError names what the library would refuse.  No device use."""
    if isinstance(levels, bool) or not isinstance(levels, (int, np.integer)) or not 1 <= int(levels) <= 8:
        raise ValueError(f"levels is an integer in 1..8, got {levels!r}")
    for name, v in (("threshold", threshold), ("knee", knee), ("intensity", intensity), ("scatter", scatter)):
        if not isinstance(v, (int, float, np.integer, np.floating)) or isinstance(v, bool) or not np.isfinite(float(v)):
            raise ValueError(f"{name} is a finite number, got {v!r}")
    threshold, knee, intensity, scatter = float(threshold), float(knee), float(intensity), float(scatter)
    if threshold < 0.0 or intensity < 0.0:
        raise ValueError(f"threshold and intensity are non-negative, got {threshold!r} and {intensity!r}")
    if not (0.0 <= knee <= 1.0 and 0.0 <= scatter <= 1.0):
        raise ValueError(f"knee and scatter are in [0, 1], got {knee!r} and {scatter!r}")
    return _lib.rtm_bloom_params(threshold, knee, intensity, scatter, int(levels))


def _bloom_option(bloom):
    """Render's and write_display's `bloom`: None for off, else the dict of bloom()'s parameters, checked.  No device use."""
    if bloom is None or bloom is False:
        return None
    if bloom is not True and not isinstance(bloom, dict):
        raise ValueError(f"bloom is False, True or a dict of bloom()'s parameters, got {bloom!r}")
    prm = {} if bloom is True else dict(bloom)
    unknown = set(prm) - set(BLOOM_DEFAULTS)
    if unknown:
        raise ValueError(f"bloom's parameters are {tuple(BLOOM_DEFAULTS)}, got {sorted(unknown)}")
    _bloom_params(**prm)
    return prm


def bloom(color, threshold=BLOOM_DEFAULTS["threshold"], knee=BLOOM_DEFAULTS["knee"], intensity=BLOOM_DEFAULTS["intensity"],
          scatter=BLOOM_DEFAULTS["scatter"], levels=BLOOM_DEFAULTS["levels"], want=("f32",), stream=None, out_f32=None):
    """Bloom (include/rtm.h: rtm_bloom) on the device: the light the bright parts of an HDR frame scatter into their surround,
    added in linear space; run it before tonemap().  `color` is an (H, W, 3) float32 torch CUDA tensor (any 4-byte-aligned
    contiguous view).  threshold: the luminance above which a pixel blooms; knee in [0, 1]: the soft knee as a fraction of
    the threshold; intensity: how much of the bloom is added; scatter in [0, 1]: how much of each coarser level reaches the
    finer; levels 1..8: the depth of the pyramid.  Returns a dict of the names in `want`: "f32" (H, W, 3) float32 (the frame
    plus intensity times the bloom), "u8" (H, W, 3) uint8 (rtm_quantise of it), "bloom" (H, W, 3) float32 (the bloom alone).
    out_f32: the tensor to write "f32" into; `color` itself blooms in place.  Enqueued on `stream` (a torch.cuda.Stream or a
    raw hipStream_t handle; default: the current stream) with a work buffer allocated here; nothing waits for it and nothing
    is copied to the host."""
    prm = _bloom_params(threshold, knee, intensity, scatter, levels)
    _check_want(want, ("f32", "u8", "bloom"))
    import torch
    _need_device("bloom")
    H, W = _frame_size(color, "color", non_empty=True)
    dev = color.device
    _check_out_f32(out_f32, want, H, W, dev)
    s = _stream_of(stream, dev)
    L = _lib.lib()
    specs = {"f32": ((H, W, 3), torch.float32), "u8": ((H, W, 3), torch.uint8), "bloom": ((H, W, 3), torch.float32)}
    out, ptr = _stage_tensors(s, dev, want, specs, max(256, L.rtm_bloom_work_bytes(W, H, prm.levels)), out_f32=out_f32)
    _lib.check(L.rtm_bloom(C.byref(prm), W, H, dev.index, color.data_ptr(), ptr("work"), ptr("f32"), ptr("u8"), ptr("bloom"),
                           C.c_void_p(s.cuda_stream)), "rtm_bloom")
    return out


_bloom = bloom  # for Renderer's methods, whose own parameter is named bloom


# include/rtm.h: RTM_TONEMAP_LOCAL_DEFAULTS
TONEMAP_LOCAL_DEFAULTS = {"anchor": 1.0, "shadows": 2.0, "highlights": 2.0, "sigma": 0.25, "levels": 5}


def _tonemap_local_params(anchor=TONEMAP_LOCAL_DEFAULTS["anchor"], shadows=TONEMAP_LOCAL_DEFAULTS["shadows"],
                          highlights=TONEMAP_LOCAL_DEFAULTS["highlights"], sigma=TONEMAP_LOCAL_DEFAULTS["sigma"],
                          levels=TONEMAP_LOCAL_DEFAULTS["levels"]):
    """tonemap_local()'s parameters as an rtm_tonemap_local_params; a ValueError names what the library would refuse.  No
    device use."""
    if isinstance(levels, bool) or not isinstance(levels, (int, np.integer)) or not 0 <= int(levels) <= 8:
        raise ValueError(f"levels is an integer in 0..8, got {levels!r}")
    for name, v in (("anchor", anchor), ("shadows", shadows), ("highlights", highlights), ("sigma", sigma)):
        if not isinstance(v, (int, float, np.integer, np.floating)) or isinstance(v, bool) or not np.isfinite(float(v)):
            raise ValueError(f"{name} is a finite number, got {v!r}")
    anchor, shadows, highlights, sigma = float(anchor), float(shadows), float(highlights), float(sigma)
    if not (anchor > 0.0 and np.isfinite(np.float32(anchor)) and np.float32(anchor) > 0):
        raise ValueError(f"anchor is positive (and a float), got {anchor!r}")
    if not (0.0 <= shadows <= 8.0 and 0.0 <= highlights <= 8.0):
        raise ValueError(f"shadows and highlights are in [0, 8], got {shadows!r} and {highlights!r}")
    if not (np.float32(0.1) <= np.float32(sigma) <= 1.0):
        raise ValueError(f"sigma is in [0.1, 1], got {sigma!r}")
    return _lib.rtm_tonemap_local_params(anchor, shadows, highlights, sigma, int(levels))


def _local_option(local):
    """Render's and write_display's `local`: None for off, else the dict of tonemap_local()'s parameters (without anchor, which
    the display path sets from the exposure), checked.  No device use."""
    if local is None or local is False:
        return None
    if local is not True and not isinstance(local, dict):
        raise ValueError(f"local is False, True or a dict of tonemap_local()'s parameters, got {local!r}")
    prm = {} if local is True else dict(local)
    allowed = tuple(k for k in TONEMAP_LOCAL_DEFAULTS if k != "anchor")
    unknown = set(prm) - set(allowed)
    if unknown:
        raise ValueError(f"local's parameters are {allowed}, got {sorted(unknown)}")
    _tonemap_local_params(**prm)
    return prm


def tonemap_local(color, anchor=TONEMAP_LOCAL_DEFAULTS["anchor"], shadows=TONEMAP_LOCAL_DEFAULTS["shadows"],
                  highlights=TONEMAP_LOCAL_DEFAULTS["highlights"], sigma=TONEMAP_LOCAL_DEFAULTS["sigma"],
                  levels=TONEMAP_LOCAL_DEFAULTS["levels"], want=("f32", "u8", "fused"), stats=None, stream=None, out_f32=None):
    """The local tone operator (include/rtm.h: rtm_tonemap_local) on the device: exposure fusion on luminance, chroma kept.
    It replaces tonemap()'s curve: the result is display-linear, nominally in [0, 1]; follow it with tonemap(op="clamp",
    exposure=0.0) for the transfer function and the dithered store.  `color` is an (H, W, 3) float32 torch CUDA tensor (any
    4-byte-aligned contiguous view).  anchor: the exposure in front of the operator; shadows, highlights in [0, 8]: the stops
    by which the shadow exposure is opened and the highlight exposure closed; sigma in [0.1, 1]: the width of the
    well-exposedness weight; levels 0..8: the depth of the pyramid, 0 the pointwise blend.  stats: tonemap()'s "stats" tensor
    (4 int32 words on the device), whose exposure then multiplies the anchor, read by the kernels without a host sync.
    Returns a dict of the names in `want`: "f32" (H, W, 3) float32, "u8" (H, W, 3) uint8 (rtm_quantise of it), "fused"
    (H, W) float32 (the fused luminance F).  out_f32: the tensor to write "f32" into; `color` itself maps in place.  Enqueued
    on `stream` (a torch.cuda.Stream or a raw hipStream_t handle; default: the current stream) with a work buffer allocated
    here; nothing waits for it and nothing is copied to the host."""
    prm = _tonemap_local_params(anchor, shadows, highlights, sigma, levels)
    _check_want(want, ("f32", "u8", "fused"))
    import torch
    _need_device("tonemap_local")
    H, W = _frame_size(color, "color", non_empty=True)
    dev = color.device
    if stats is not None and not (isinstance(stats, torch.Tensor) and stats.device == dev and stats.dtype == torch.int32
                                  and stats.numel() == 4 and stats.is_contiguous()):
        raise ValueError(f'stats is tonemap()\'s "stats": a contiguous tensor of 4 int32 words on {dev}')
    _check_out_f32(out_f32, want, H, W, dev)
    s = _stream_of(stream, dev)
    L = _lib.lib()
    specs = {"f32": ((H, W, 3), torch.float32), "u8": ((H, W, 3), torch.uint8), "fused": ((H, W), torch.float32)}
    out, ptr = _stage_tensors(s, dev, want, specs, max(256, L.rtm_tonemap_local_work_bytes(W, H, prm.levels)), out_f32=out_f32)
    _lib.check(L.rtm_tonemap_local(C.byref(prm), W, H, dev.index, color.data_ptr(), None if stats is None else stats.data_ptr(),
                                   ptr("work"), ptr("f32"), ptr("u8"), ptr("fused"), C.c_void_p(s.cuda_stream)),
               "rtm_tonemap_local")
    return out


# include/rtm.h: RTM_FIREFLY_DEFAULTS
FIREFLY_DEFAULTS = dict(_lib.FIREFLY_DEFAULTS)


def _firefly_params(radius=FIREFLY_DEFAULTS["radius"], rank=FIREFLY_DEFAULTS["rank"], k=FIREFLY_DEFAULTS["k"],
                    floor=FIREFLY_DEFAULTS["floor"], repair=FIREFLY_DEFAULTS["repair"]):
    """firefly()'s parameters as an rtm_firefly_params; a ValueError names what the library would refuse.  No device use."""
    for name, v, lo, hi in (("radius", radius, 1, 3), ("rank", rank, 1, 8)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
            raise ValueError(f"{name} is an integer in {lo}..{hi}, got {v!r}")
    for name, v in (("k", k), ("floor", floor)):
        if not isinstance(v, (int, float, np.integer, np.floating)) or isinstance(v, bool) or not np.isfinite(float(v)):
            raise ValueError(f"{name} is a finite number, got {v!r}")
    # as the library sees them: rounded to float
    with np.errstate(over="ignore", under="ignore"):
        kf, ff = float(np.float32(k)), float(np.float32(floor))
    if not (np.isfinite(kf) and kf >= 1.0):
        raise ValueError(f"k is a finite number that is at least 1, got {k!r}")
    if not (np.isfinite(ff) and ff >= 0.0) or np.signbit(ff):
        raise ValueError(f"floor is a finite number that is not negative (nor -0.0), got {floor!r}")
    if not isinstance(repair, (bool, np.bool_)) and not (isinstance(repair, (int, np.integer)) and int(repair) in (0, 1)):
        raise ValueError(f"repair is False or True (0 or 1), got {repair!r}")
    return _lib.rtm_firefly_params(int(radius), int(rank), kf, ff, int(bool(repair)))


def _firefly_option(firefly):
    """Render's `firefly`: None (or False) for off, else the dict of firefly()'s parameters (True: the defaults), checked."""
    if firefly is None or firefly is False:
        return None
    if firefly is not True and not isinstance(firefly, dict):
        raise ValueError(f"firefly is None, False, True or a dict of {tuple(FIREFLY_DEFAULTS)}, got {firefly!r}")
    prm = {} if firefly is True else dict(firefly)
    unknown = set(prm) - set(FIREFLY_DEFAULTS)
    if unknown:
        raise ValueError(f"firefly's parameters are {tuple(FIREFLY_DEFAULTS)}, got {sorted(unknown)}")
    _firefly_params(**prm)
    return prm


def firefly(color, radius=FIREFLY_DEFAULTS["radius"], rank=FIREFLY_DEFAULTS["rank"], k=FIREFLY_DEFAULTS["k"],
            floor=FIREFLY_DEFAULTS["floor"], repair=FIREFLY_DEFAULTS["repair"], want=("f32",), stream=None):
    """The firefly clamp (include/rtm.h: rtm_firefly) on the device: a pixel whose luminance exceeds k times the rank-th
    largest luminance of its (2 radius + 1)^2 - 1 neighbours, plus floor, is scaled down to that threshold, chroma kept; with
    `repair` a pixel with a non-finite component becomes the mean of its finite neighbours.  Run it right after the render,
    before denoise(), denoise_variance(), defocus(), lens(), resize(), bloom() and tonemap().  `color` is an (H, W, 3) float32
    torch CUDA tensor (any 4-byte-aligned contiguous view).  radius 1..3; rank 1..8 (1: the maximum; the default 3 keeps the
    rim of a bright rectangle and still catches clusters of three); k >= 1; floor >= 0.  Returns a dict of the names in
    `want`: "f32" (H, W, 3) float32, "u8" (H, W, 3) uint8 (rtm_quantise of it), "mask" (H, W) uint8 (0 unchanged, 1 clamped,
    2 repaired), "threshold" (H, W) float32 (+inf where a pixel has none).  The outputs are tensors of the call's own: a
    gather cannot run in place.  Enqueued on `stream` (a torch.cuda.Stream or a raw hipStream_t handle; default: the current
    stream); nothing waits for it and nothing is copied to the host."""
    prm = _firefly_params(radius, rank, k, floor, repair)
    _check_want(want, ("f32", "u8", "mask", "threshold"))
    import torch
    _need_device("firefly")
    H, W = _frame_size(color, "color", non_empty=True)
    dev = color.device
    s = _stream_of(stream, dev)
    specs = {"f32": ((H, W, 3), torch.float32), "u8": ((H, W, 3), torch.uint8), "mask": ((H, W), torch.uint8),
             "threshold": ((H, W), torch.float32)}
    out, ptr = _stage_tensors(s, dev, want, specs)
    _lib.check(_lib.lib().rtm_firefly(C.byref(prm), W, H, dev.index, color.data_ptr(), ptr("f32"), ptr("u8"), ptr("mask"),
                                      ptr("threshold"), C.c_void_p(s.cuda_stream)), "rtm_firefly")
    return out


_firefly = firefly  # for Renderer's methods, whose own parameter is named firefly


# include/rtm.h: RTM_DEFOCUS_DEFAULTS (focus_distance has no default: the caller sets it)
DEFOCUS_DEFAULTS = dict(_lib.DEFOCUS_DEFAULTS)


def _defocus_params(focus_distance, aperture=DEFOCUS_DEFAULTS["aperture"], max_radius=DEFOCUS_DEFAULTS["max_radius"]):
    """defocus()'s parameters as an rtm_defocus_params; a ValueError names what the library would refuse.  No device use."""
    if isinstance(max_radius, bool) or not isinstance(max_radius, (int, np.integer)) or not 1 <= int(max_radius) <= 16:
        raise ValueError(f"max_radius is an integer in 1..16, got {max_radius!r}")
    for name, v in (("focus_distance", focus_distance), ("aperture", aperture)):
        if not isinstance(v, (int, float, np.integer, np.floating)) or isinstance(v, bool) or not np.isfinite(float(v)):
            raise ValueError(f"{name} is a finite number, got {v!r}")
    # as the library sees them: rounded to float
    with np.errstate(over="ignore", under="ignore"):
        zf, a = float(np.float32(focus_distance)), float(np.float32(aperture))
    if not (np.isfinite(zf) and zf > 0.0):
        raise ValueError(f"focus_distance is positive (and finite as a float), got {focus_distance!r}")
    if not (np.isfinite(a) and a >= 0.0):
        raise ValueError(f"aperture is non-negative (and finite as a float), got {aperture!r}")
    return _lib.rtm_defocus_params(zf, a, int(max_radius))


_DOF_KEYS = ("focus_distance", "focus_pixel", "aperture", "max_radius")


def _focus_pixel(pixel, width, height):
    """(x, y) of a focus pixel inside the width x height frame, or a ValueError.  No device use."""
    ok = isinstance(pixel, (tuple, list)) and len(pixel) == 2 and all(
        isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in pixel)
    if not ok or not (0 <= int(pixel[0]) < width and 0 <= int(pixel[1]) < height):
        raise ValueError(f"the focus pixel is (x, y), integers inside the {width}x{height} frame, got {pixel!r}")
    return int(pixel[0]), int(pixel[1])


def _dof_option(dof, width, height):
    """Render's `dof`: None (or False, like Render's other stage arguments) for off, else the dict of its parameters (a
    subset of _DOF_KEYS), checked as far as that needs no device: the focus distance of a focus_pixel is read from the depth plane later."""
    if dof is None or dof is False:
        return None
    if dof is not True and not isinstance(dof, dict):
        raise ValueError(f"dof is None, False, True or a dict of {_DOF_KEYS}, got {dof!r}")
    prm = {} if dof is True else dict(dof)
    unknown = set(prm) - set(_DOF_KEYS)
    if unknown:
        raise ValueError(f"dof's parameters are {_DOF_KEYS}, got {sorted(unknown)}")
    if prm.get("focus_distance") is not None and prm.get("focus_pixel") is not None:
        raise ValueError("dof takes focus_distance or focus_pixel, not both")
    if prm.get("focus_pixel") is not None:
        prm["focus_pixel"] = _focus_pixel(prm["focus_pixel"], width, height)
    lens = {k: prm[k] for k in ("aperture", "max_radius") if k in prm}
    _defocus_params(1.0 if prm.get("focus_distance") is None else prm["focus_distance"], **lens)
    return prm


def defocus(color, depth, focus_distance, aperture=DEFOCUS_DEFAULTS["aperture"], max_radius=DEFOCUS_DEFAULTS["max_radius"],
            want=("f32",), stream=None):
    """Depth of field (include/rtm.h: rtm_defocus) on the device: a depth-aware gather blur of a finished frame whose
    per-pixel circle of confusion follows the thin-lens law; run it after the denoisers and before bloom() and tonemap().
    `color` is an (H, W, 3) float32 torch CUDA tensor (any 4-byte-aligned contiguous view), `depth` the (H, W) float32 plane
    of Renderer.render_aov on the same device.  focus_distance: the depth that is sharp (Renderer.focus_distance gives the
    camera's, or a pixel's); aperture: the blur radius, in pixels, of a point at infinity (0: the identity); max_radius 1..16:
    the clamp of every radius, and the half-width of the window.  Returns a dict of the names in `want`: "f32" (H, W, 3)
    float32, "u8" (H, W, 3) uint8 (rtm_quantise of it), "coc" (H, W) float32 (the signed radius: negative in front of the
    focus).  The outputs are tensors of the call's own: a gather cannot run in place.  Enqueued on `stream` (a
    torch.cuda.Stream or a raw hipStream_t handle; default: the current stream); nothing waits for it and nothing is copied
    to the host."""
    prm = _defocus_params(focus_distance, aperture, max_radius)
    _check_want(want, ("f32", "u8", "coc"))
    import torch
    _need_device("defocus")
    H, W = _frame_size(color, "color", non_empty=True)
    dev = color.device
    if not (isinstance(depth, torch.Tensor) and depth.device == dev and depth.dtype == torch.float32
            and tuple(depth.shape) == (H, W) and depth.is_contiguous()):
        raise ValueError(f"depth must be a contiguous ({H}, {W}) float32 tensor on {dev}")
    s = _stream_of(stream, dev)
    specs = {"f32": ((H, W, 3), torch.float32), "u8": ((H, W, 3), torch.uint8), "coc": ((H, W), torch.float32)}
    out, ptr = _stage_tensors(s, dev, want, specs)
    _lib.check(_lib.lib().rtm_defocus(C.byref(prm), W, H, dev.index, color.data_ptr(), depth.data_ptr(), ptr("f32"), ptr("u8"),
                                      ptr("coc"), C.c_void_p(s.cuda_stream)), "rtm_defocus")
    return out


# include/rtm.h: RTM_RESIZE_DEFAULTS and the RTM_RESIZE_* filters, by name
RESIZE_DEFAULTS = dict(_lib.RESIZE_DEFAULTS)
RESIZE_FILTERS = _lib.RESIZE_FILTERS


def _resize_args(size, filter=RESIZE_DEFAULTS["filter"]):
    """resize()'s size and filter as (H, W, the RTM_RESIZE_* value); a ValueError names what the library would refuse.  No
    device use."""
    if not isinstance(filter, str) or filter not in RESIZE_FILTERS:
        raise ValueError(f"filter is one of {RESIZE_FILTERS}, got {filter!r}")
    ok = isinstance(size, (tuple, list)) and len(size) == 2 and all(
        isinstance(v, (int, np.integer)) and not isinstance(v, bool) and 1 <= int(v) <= 2147483647 for v in size)
    if not ok:
        raise ValueError(f"size is (H, W), two positive integers, got {size!r}")
    return int(size[0]), int(size[1]), RESIZE_FILTERS.index(filter)


def _resize_option(resize):
    """Render's `resize`: None (or False, like Render's other stage arguments) for off, else (W, H) or (W, H, filter), checked,
    as write_resized's parameters.  No device use."""
    if resize is None or resize is False:
        return None
    if not isinstance(resize, (tuple, list)) or len(resize) not in (2, 3):
        raise ValueError(f"resize is None, (W, H) or (W, H, filter), got {resize!r}")
    prm = {"size": (resize[1], resize[0])}
    if len(resize) == 3:
        prm["filter"] = resize[2]
    _resize_args(**prm)
    return prm


def resize(color, size, filter=RESIZE_DEFAULTS["filter"], want=("f32",), stream=None):
    """Filtered resampling (include/rtm.h: rtm_resize) on the device: a frame or a plane brought to another size by a
    separable filter, antialiased when it shrinks; run it in linear light, after defocus() and before bloom() and tonemap().
    `color` is an (h, w, 3) float32 torch CUDA tensor or an (h, w) plane (any 4-byte-aligned contiguous view); size = (H, W),
    any positive integers, the axes independent.  filter: one of RESIZE_FILTERS — "box" (the mean of what a destination pixel
    covers), "triangle", "mitchell" (the default) or "lanczos3"; the last two have negative lobes and may undershoot 0 next to
    a bright edge.  A pixel with a non-finite component contributes nothing; a destination pixel too few of whose taps count
    is NaN.  Returns a dict of the names in `want`: "f32" float32 and "u8" uint8 (rtm_quantise of it), (H, W, 3) or (H, W).
    The outputs are tensors of the call's own: a gather cannot run in place.  Enqueued on `stream` (a torch.cuda.Stream or a
    raw hipStream_t handle; default: the current stream) with a work buffer allocated here; nothing waits for it and nothing
    is copied to the host."""
    H, W, which = _resize_args(size, filter)
    _check_want(want, ("f32", "u8"))
    import torch
    _need_device("resize")
    if not (isinstance(color, torch.Tensor) and color.is_cuda and color.dtype == torch.float32 and color.is_contiguous()
            and color.numel() > 0 and (color.dim() == 2 or (color.dim() == 3 and color.shape[2] == 3))):
        raise ValueError("color must be a contiguous, non-empty (h, w, 3) or (h, w) float32 CUDA tensor")
    h, w = int(color.shape[0]), int(color.shape[1])
    channels = 3 if color.dim() == 3 else 1
    shape = (H, W, 3) if channels == 3 else (H, W)
    dev = color.device
    s = _stream_of(stream, dev)
    L = _lib.lib()
    prm = _lib.rtm_resize_params(which, channels)
    work = L.rtm_resize_work_bytes(w, h, W, H, which, channels)
    if work == C.c_size_t(-1).value:
        raise ValueError(f"resizing {w}x{h} to {W}x{H} needs a work buffer larger than a size_t")
    specs = {"f32": (shape, torch.float32), "u8": (shape, torch.uint8)}
    out, ptr = _stage_tensors(s, dev, want, specs, max(256, work))
    _lib.check(L.rtm_resize(C.byref(prm), w, h, W, H, dev.index, color.data_ptr(), ptr("work"), ptr("f32"), ptr("u8"),
                            C.c_void_p(s.cuda_stream)), "rtm_resize")
    return out


# include/rtm.h: RTM_LENS_DEFAULTS, the RTM_LENS_* filters and modes, by name
LENS_DEFAULTS = dict(_lib.LENS_DEFAULTS)
LENS_FILTERS = _lib.LENS_FILTERS
LENS_MODES = _lib.LENS_MODES
_LENS_RANGES = {"k1": (-0.5, 0.5), "k2": (-0.25, 0.25), "zoom": (0.25, 4.0), "chroma": (-0.05, 0.05), "vignette": (0.0, 1.0),
                "falloff": (0.0, 4.0)}


def _lens_folds_over(k1, k2, zoom, inverse):
    """rtm.h's fold-over check, in double like the library's: k1, k2, zoom as the float32 values the struct holds."""
    k1, k2, iz = float(k1), float(k2), 1.0 / float(zoom)
    a, b = 3.0 * k1, 5.0 * k2
    T = 4.0 * (iz * iz) if inverse else iz * iz
    if not 1.0 + T * (a + T * b) >= 0.25:
        return True
    if b != 0.0:
        tv = -a / (2.0 * b)
        if 0.0 < tv < T and not 1.0 + tv * (a + tv * b) >= 0.25:
            return True
    return bool(inverse) and not 1.0 + T * (k1 + T * k2) >= 0.5


def _lens_params(channels=3, k1=LENS_DEFAULTS["k1"], k2=LENS_DEFAULTS["k2"], zoom=LENS_DEFAULTS["zoom"],
                 chroma=LENS_DEFAULTS["chroma"], vignette=LENS_DEFAULTS["vignette"], falloff=LENS_DEFAULTS["falloff"],
                 border=LENS_DEFAULTS["border"], mode=LENS_DEFAULTS["mode"], filter=LENS_DEFAULTS["filter"], fit=False):
    """lens()'s parameters as an rtm_lens_params; a ValueError names what the library would refuse.  fit=True: for
    lens_fit_zoom, which ignores zoom, holds k1, k2 and chroma to no range and makes the fold-over check part of its search.
    No device use."""
    if not isinstance(mode, str) or mode not in LENS_MODES:
        raise ValueError(f"mode is one of {LENS_MODES}, got {mode!r}")
    if not isinstance(filter, str) or filter not in LENS_FILTERS:
        raise ValueError(f"filter is one of {LENS_FILTERS}, got {filter!r}")
    vals = {}
    for name, v in (("k1", k1), ("k2", k2), ("zoom", 1.0 if fit else zoom), ("chroma", chroma), ("vignette", vignette),
                    ("falloff", falloff)):
        lo, hi = _LENS_RANGES[name]
        if not isinstance(v, (int, float, np.integer, np.floating)) or isinstance(v, bool):
            raise ValueError(f"{name} is a number in [{lo}, {hi}], got {v!r}")
        with np.errstate(over="ignore", under="ignore"):
            f = np.float32(v)  # as the library sees it: rounded to float
        if fit and name in ("k1", "k2", "chroma"):
            if not np.isfinite(f):
                raise ValueError(f"{name} is a finite number, got {v!r}")
        elif not np.float32(lo) <= f <= np.float32(hi):
            raise ValueError(f"{name} is a number in [{lo}, {hi}], got {v!r}")
        vals[name] = f
    try:
        words = np.ascontiguousarray(np.broadcast_to(np.asarray(border, dtype=np.float32), (3,)))  # a float32's bits are kept
    except (TypeError, ValueError):
        raise ValueError(f"border is a number or three, got {border!r}") from None
    if filter != "nearest" and not np.all(np.isfinite(words)):
        raise ValueError(f'border is finite unless filter is "nearest", got {border!r}')
    if vals["chroma"] != 0.0 and channels == 1:
        raise ValueError("chroma is 0 for a plane: it has no colours to separate")
    if filter == "nearest" and (vals["chroma"] != 0.0 or vals["vignette"] != 0.0):
        raise ValueError('filter "nearest" copies words: chroma and vignette are 0')
    if not fit and _lens_folds_over(vals["k1"], vals["k2"], vals["zoom"], mode == "inverse"):
        raise ValueError(f"the radial map folds over inside the frame with k1 {k1!r}, k2 {k2!r}, zoom {zoom!r}, mode {mode!r}")
    prm = _lib.rtm_lens_params()
    for name, f in vals.items():
        setattr(prm, name, float(f))
    C.memmove(prm.border, words.ctypes.data, 12)
    prm.mode, prm.filter, prm.channels = LENS_MODES.index(mode), LENS_FILTERS.index(filter), channels
    return prm


def lens_fit_zoom(width, height, **params):
    """The zoom that hides the border of lens(**params) on a width x height frame (include/rtm.h: rtm_lens_fit_zoom): the
    smallest of its 24-step bisection of [0.25, 4] at which every pixel of the frame's outermost rows and columns has its
    source inside the frame, as a Python float holding a float32.  params: lens()'s, of which k1, k2, chroma and mode are
    read (zoom is ignored; channels=1 for a plane).  Host only: no device use.  RtmError (unsupported) when not even zoom 4
    hides it, which takes a k1, k2 or chroma beyond what lens() accepts."""
    for name, v in (("width", width), ("height", height)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= int(v) <= 2147483647:
            raise ValueError(f"{name} is a positive integer, got {v!r}")
    unknown = set(params) - set(LENS_DEFAULTS) - {"channels"}
    if unknown:
        raise ValueError(f"lens_fit_zoom's parameters are {tuple(LENS_DEFAULTS) + ('channels',)}, got {sorted(unknown)}")
    channels = params.pop("channels", 3)
    if channels not in (1, 3):
        raise ValueError(f"channels is 1 or 3, got {channels!r}")
    prm = _lens_params(channels, fit=True, **params)
    z = C.c_float()
    _lib.check(_lib.lib().rtm_lens_fit_zoom(C.byref(prm), int(width), int(height), C.byref(z)), "rtm_lens_fit_zoom")
    return float(z.value)


def _lens_option(lens, width, height):
    """Render's `lens`: None (or False, like Render's other stage arguments) for off, else the dict of lens()'s parameters
    (True: the defaults), checked, with zoom="auto" replaced by lens_fit_zoom's value.  No device use."""
    if lens is None or lens is False:
        return None
    if lens is not True and not isinstance(lens, dict):
        raise ValueError(f"lens is None, False, True or a dict of {tuple(LENS_DEFAULTS)}, got {lens!r}")
    prm = {} if lens is True else dict(lens)
    unknown = set(prm) - set(LENS_DEFAULTS)
    if unknown:
        raise ValueError(f"lens's parameters are {tuple(LENS_DEFAULTS)}, got {sorted(unknown)}")
    if isinstance(prm.get("zoom"), str):
        if prm["zoom"] != "auto":
            raise ValueError(f'zoom is a number or "auto", got {prm["zoom"]!r}')
        prm["zoom"] = lens_fit_zoom(width, height, **{k: v for k, v in prm.items() if k != "zoom"})
    _lens_params(3, **prm)
    return prm


def lens(color, k1=LENS_DEFAULTS["k1"], k2=LENS_DEFAULTS["k2"], zoom=LENS_DEFAULTS["zoom"], chroma=LENS_DEFAULTS["chroma"],
         vignette=LENS_DEFAULTS["vignette"], falloff=LENS_DEFAULTS["falloff"], border=LENS_DEFAULTS["border"],
         mode=LENS_DEFAULTS["mode"], filter=LENS_DEFAULTS["filter"], want=("f32",), stream=None):
    """Lens distortion, lateral chromatic aberration and vignette (include/rtm.h: rtm_lens) on the device, at the frame's own
    size; run it in linear light, after defocus() and before resize(), bloom() and tonemap().  `color` is an (H, W, 3)
    float32 torch CUDA tensor or an (H, W) plane (any 4-byte-aligned contiguous view).  k1, k2: the radial polynomial
    g(t) = 1 + t (k1 + t k2) over the squared radius t, 1 at the frame's corner (k1 < 0: a barrel); mode "direct" shows at p
    the source at p g(|p|^2), "inverse" takes that distortion out; zoom in [0.25, 4] magnifies about the centre
    (lens_fit_zoom gives the one that hides the border); chroma scales red by 1 + chroma and blue by 1 - chroma; vignette in
    [0, 1] and falloff (the tangent of the half field angle at the corner) darken by the cos^4 law.  filter: one of
    LENS_FILTERS; "nearest" copies words bit for bit (id planes, depth with +inf) and takes no chroma or vignette.  Where a
    channel's source lies outside the frame the result is `border` (a number, or three for a frame; with "nearest" its bits
    are kept, so np.int32(-1).view(np.float32) marks an id plane).  A pixel with a non-finite component contributes nothing; a
    result too few of whose taps count is NaN.  A map that folds over inside the frame is a ValueError.  Returns a dict of the
    names in `want`: "f32" float32 and "u8" uint8 (rtm_quantise of it), shaped like `color`.  The outputs are tensors of the
    call's own: a gather cannot run in place.  Enqueued on `stream` (a torch.cuda.Stream or a raw hipStream_t handle; default:
    the current stream); nothing waits for it and nothing is copied to the host."""
    channels = 1 if getattr(color, "ndim", 3) == 2 else 3
    prm = _lens_params(channels, k1, k2, zoom, chroma, vignette, falloff, border, mode, filter)
    _check_want(want, ("f32", "u8"))
    import torch
    _need_device("lens")
    if not (isinstance(color, torch.Tensor) and color.is_cuda and color.dtype == torch.float32 and color.is_contiguous()
            and color.numel() > 0 and (color.dim() == 2 or (color.dim() == 3 and color.shape[2] == 3))):
        raise ValueError("color must be a contiguous, non-empty (H, W, 3) or (H, W) float32 CUDA tensor")
    H, W = int(color.shape[0]), int(color.shape[1])
    shape = tuple(color.shape)
    dev = color.device
    s = _stream_of(stream, dev)
    specs = {"f32": (shape, torch.float32), "u8": (shape, torch.uint8)}
    out, ptr = _stage_tensors(s, dev, want, specs)
    _lib.check(_lib.lib().rtm_lens(C.byref(prm), W, H, dev.index, color.data_ptr(), ptr("f32"), ptr("u8"),
                                   C.c_void_p(s.cuda_stream)), "rtm_lens")
    return out


_lens = lens  # for Renderer's methods, whose own parameter is named lens


# include/rtm.h: RTM_GRADE_DEFAULTS and the RTM_GRADE_* interpolations, by name
GRADE_DEFAULTS = dict(_lib.GRADE_DEFAULTS)
GRADE_INTERPS = _lib.GRADE_INTERPS
_GRADE_OPTION_KEYS = tuple(GRADE_DEFAULTS) + ("temperature", "tint")
_LUT_KEYS = ("table", "domain_min", "domain_max", "size", "interp")


def _is_number(v):
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool)


def _f32(v):
    with np.errstate(over="ignore", under="ignore"):
        return np.float32(v)  # as the library sees it: rounded to float


def _grade_three(name, v, what):
    """A number or three as three float32; the ValueError names `what` is asked of them."""
    try:
        a = np.asarray(v)
        if a.dtype == np.bool_ or not (np.issubdtype(a.dtype, np.integer) or np.issubdtype(a.dtype, np.floating)):
            raise TypeError
        with np.errstate(over="ignore", under="ignore"):
            return np.ascontiguousarray(np.broadcast_to(a.astype(np.float32), (3,)))
    except (TypeError, ValueError):
        raise ValueError(f"{name} is {what}, one number or three, got {v!r}") from None


def _grade_params(matrix=GRADE_DEFAULTS["matrix"], exposure=GRADE_DEFAULTS["exposure"], contrast=GRADE_DEFAULTS["contrast"],
                  pivot=GRADE_DEFAULTS["pivot"], slope=GRADE_DEFAULTS["slope"], offset=GRADE_DEFAULTS["offset"],
                  power=GRADE_DEFAULTS["power"], saturation=GRADE_DEFAULTS["saturation"], lut_size=0,
                  lut_domain=((0, 0, 0), (1, 1, 1)), interp="tetrahedral"):
    """grade()'s parameters as an rtm_grade_params; a ValueError names what the library would refuse.  No device use."""
    if not isinstance(interp, str) or interp not in GRADE_INTERPS:
        raise ValueError(f"interp is one of {GRADE_INTERPS}, got {interp!r}")
    prm = _lib.rtm_grade_params()
    if matrix is None:
        m = np.eye(3, dtype=np.float32)
    else:
        try:
            m = np.asarray(matrix)
            if m.dtype == np.bool_ or not (np.issubdtype(m.dtype, np.integer) or np.issubdtype(m.dtype, np.floating)) or m.shape != (3, 3):
                raise TypeError
            with np.errstate(over="ignore", under="ignore"):
                m = np.ascontiguousarray(m.astype(np.float32))
        except (TypeError, ValueError):
            raise ValueError(f"matrix is None or a 3 x 3 array of finite numbers, got {matrix!r}") from None
        if not np.all(np.isfinite(m)):
            raise ValueError(f"matrix is None or a 3 x 3 array of finite numbers, got {matrix!r}")
    C.memmove(prm.matrix, m.ctypes.data, 36)
    ranges = (("exposure", exposure, -32.0, 32.0, "a number of stops in [-32, 32]"),
              ("contrast", contrast, 0.25, 4.0, "a number in [0.25, 4]"),
              ("pivot", pivot, None, None, "a finite positive number"),
              ("saturation", saturation, 0.0, 4.0, "a number in [0, 4]"))
    for name, v, lo, hi, what in ranges:
        f = _f32(v) if _is_number(v) else None
        if f is None or not np.isfinite(f) or (lo is not None and not np.float32(lo) <= f <= np.float32(hi)) or (lo is None and not f > 0):
            raise ValueError(f"{name} is {what}, got {v!r}")
        setattr(prm, name, float(f))
    s = _grade_three("slope", slope, "finite and not negative")
    o = _grade_three("offset", offset, "finite")
    p = _grade_three("power", power, "in [0.1, 10]")
    if not (np.all(np.isfinite(s)) and np.all(s >= 0)):
        raise ValueError(f"slope is finite and not negative, one number or three, got {slope!r}")
    if not np.all(np.isfinite(o)):
        raise ValueError(f"offset is finite, one number or three, got {offset!r}")
    if not np.all((p >= np.float32(0.1)) & (p <= np.float32(10.0))):
        raise ValueError(f"power is in [0.1, 10], one number or three, got {power!r}")
    for field, words in ((prm.slope, s), (prm.offset, o), (prm.power, p)):
        C.memmove(field, words.ctypes.data, 12)
    if isinstance(lut_size, bool) or not isinstance(lut_size, (int, np.integer)) or not (lut_size == 0 or 2 <= lut_size <= 256):
        raise ValueError(f"the lut's size is in 2..256, got {lut_size!r}")
    try:
        lo, hi = lut_domain
        lo, hi = _grade_three("lut_domain's min", lo, "finite"), _grade_three("lut_domain's max", hi, "finite")
    except (TypeError, ValueError):
        raise ValueError(f"lut_domain is (min, max), each a finite number or three, with max > min, got {lut_domain!r}") from None
    if not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi)) and np.all(hi > lo)):
        raise ValueError(f"lut_domain is (min, max), each a finite number or three, with max > min, got {lut_domain!r}")
    C.memmove(prm.lut_min, lo.ctypes.data, 12)
    C.memmove(prm.lut_max, hi.ctypes.data, 12)
    prm.lut_size, prm.lut_interp = int(lut_size), GRADE_INTERPS.index(interp)
    return prm


def white_balance(kelvin, tint=0.0):
    """The 3 x 3 float32 matrix (row-major, for grade()'s `matrix`) that takes a scene lit by a black body at `kelvin` to D65
    (include/rtm.h: rtm_grade_white_balance): the Bradford adaptation from that white to D65 in linear Rec.709 primaries.
    kelvin in [1667, 25000]; tint in [-0.05, 0.05] moves the source white along v of CIE 1960 (u, v), positive towards
    green.  Host only: no device use."""
    if not _is_number(kelvin) or not 1667.0 <= _f32(kelvin) <= 25000.0:
        raise ValueError(f"kelvin is a number in [1667, 25000], got {kelvin!r}")
    if not _is_number(tint) or not np.float32(-0.05) <= _f32(tint) <= np.float32(0.05):
        raise ValueError(f"tint is a number in [-0.05, 0.05], got {tint!r}")
    m = (C.c_float * 9)()
    _lib.check(_lib.lib().rtm_grade_white_balance(float(_f32(kelvin)), float(_f32(tint)), m), "rtm_grade_white_balance")
    return np.array(m, dtype=np.float32).reshape(3, 3)


def load_cube(path):
    """A 3D LUT from a .cube file (include/rtm.h: rtm_lut_load_cube): a dict of "table", an (N, N, N, 3) float32 NumPy array
    indexed [b][g][r] (the file's order, red fastest), "domain_min" and "domain_max" (three floats each) and "size" N.
    RtmError names the line of a file that does not parse.  Host only: no device use."""
    L = _lib.lib()
    name = os.fsencode(path)
    n = C.c_int32()
    lo, hi = (C.c_float * 3)(), (C.c_float * 3)()
    _lib.check(L.rtm_lut_load_cube(name, C.byref(n), lo, hi, None, 0), f"rtm_lut_load_cube({os.fsdecode(name)})")
    table = np.empty((n.value, n.value, n.value, 3), dtype=np.float32)
    _lib.check(L.rtm_lut_load_cube(name, C.byref(n), lo, hi, table.ctypes.data, table.size), f"rtm_lut_load_cube({os.fsdecode(name)})")
    return {"table": table, "domain_min": tuple(float(v) for v in lo), "domain_max": tuple(float(v) for v in hi), "size": int(n.value)}


def _grade_option(grade):
    """Render's and write_display's `grade`: None (or False) for off, else the dict of grade()'s parametric arguments (True:
    the defaults), checked, with temperature and tint replaced by white_balance's matrix.  No device use."""
    if grade is None or grade is False:
        return None
    if grade is not True and not isinstance(grade, dict):
        raise ValueError(f"grade is None, False, True or a dict of {_GRADE_OPTION_KEYS}, got {grade!r}")
    prm = {} if grade is True else dict(grade)
    unknown = set(prm) - set(_GRADE_OPTION_KEYS)
    if unknown:
        raise ValueError(f"grade's parameters are {_GRADE_OPTION_KEYS}, got {sorted(unknown)}")
    if "temperature" in prm or "tint" in prm:
        if "temperature" not in prm:
            raise ValueError("tint shifts the white of a temperature: give temperature too")
        if prm.get("matrix") is not None:
            raise ValueError("grade takes a matrix or a temperature, not both")
        prm["matrix"] = white_balance(prm.pop("temperature"), prm.pop("tint", 0.0))
    _grade_params(**prm)
    return prm


def _lut_option(lut):
    """Render's and write_display's `lut`: None for off, a path of a .cube file, or load_cube's dict (which may also name an
    "interp" of GRADE_INTERPS), checked.  A file that does not load raises here.  No device use."""
    if lut is None or lut is False:
        return None
    if isinstance(lut, (str, bytes, os.PathLike)):
        lut = load_cube(lut)
    if not isinstance(lut, dict):
        raise ValueError(f"lut is None, the path of a .cube file or load_cube's dict, got {lut!r}")
    unknown = set(lut) - set(_LUT_KEYS)
    if unknown or "table" not in lut:
        raise ValueError(f"a lut's keys are {_LUT_KEYS} (table is required), got {sorted(lut)}")
    table = lut["table"]
    if not (isinstance(table, np.ndarray) and table.dtype == np.float32 and table.ndim == 4 and table.shape[3] == 3
            and table.shape[0] == table.shape[1] == table.shape[2] and 2 <= table.shape[0] <= 256):
        raise ValueError("a lut's table is an (N, N, N, 3) float32 NumPy array indexed [b][g][r], N in 2..256")
    if lut.get("size", table.shape[0]) != table.shape[0]:
        raise ValueError(f"a lut's size is its table's, {table.shape[0]}, got {lut['size']!r}")
    out = {"table": np.ascontiguousarray(table), "lut_domain": (lut.get("domain_min", (0, 0, 0)), lut.get("domain_max", (1, 1, 1))),
           "interp": lut.get("interp", "tetrahedral")}
    _grade_params(lut_size=table.shape[0], lut_domain=out["lut_domain"], interp=out["interp"])
    return out


def grade(color, matrix=GRADE_DEFAULTS["matrix"], exposure=GRADE_DEFAULTS["exposure"], contrast=GRADE_DEFAULTS["contrast"],
          pivot=GRADE_DEFAULTS["pivot"], slope=GRADE_DEFAULTS["slope"], offset=GRADE_DEFAULTS["offset"], power=GRADE_DEFAULTS["power"],
          saturation=GRADE_DEFAULTS["saturation"], lut=None, lut_domain=((0, 0, 0), (1, 1, 1)), interp="tetrahedral", want=("f32",),
          stream=None, out_f32=None):
    """The colour grade (include/rtm.h: rtm_grade) on the device, a per-pixel transform in this order: `matrix` (3 x 3,
    row-major: white_balance()'s, or any change of primaries), `exposure` in stops, `contrast` as a power curve about `pivot`,
    the ASC CDL's `slope`, `offset` and `power` (a number, or three for R, G, B), `saturation` about the Rec.709 luminance,
    then `lut`, an (N, N, N, 3) float32 CUDA tensor indexed [b][g][r] (load_cube's table on the device) whose input domain is
    lut_domain = (min, max), interpolated by `interp`, one of GRADE_INTERPS.  Run the parametric steps in linear light, after
    bloom() and before tonemap(); a look LUT from a .cube file belongs on tonemap()'s "f32".  `color` is an (H, W, 3)
    float32 torch CUDA tensor (any 4-byte-aligned contiguous view).  A step left at its default is skipped, so the defaults
    copy the frame bit for bit; a pixel with a non-finite component is copied as it is.  Returns a dict of the names in
    `want`: "f32" (H, W, 3) float32 and "u8" (H, W, 3) uint8 (rtm_quantise of it).  out_f32: the tensor to write "f32" into;
    `color` itself grades in place.  Enqueued on `stream` (a torch.cuda.Stream or a raw hipStream_t handle; default: the
    current stream); nothing waits for it and nothing is copied to the host."""
    import torch
    n = 0
    if lut is not None:
        if not (isinstance(lut, torch.Tensor) and lut.dtype == torch.float32 and lut.dim() == 4 and lut.shape[3] == 3
                and lut.shape[0] == lut.shape[1] == lut.shape[2] and 2 <= lut.shape[0] <= 256 and lut.is_contiguous()):
            raise ValueError("lut must be a contiguous (N, N, N, 3) float32 CUDA tensor indexed [b][g][r], N in 2..256")
        n = int(lut.shape[0])
    prm = _grade_params(matrix, exposure, contrast, pivot, slope, offset, power, saturation, n, lut_domain, interp)
    _check_want(want, ("f32", "u8"))
    _need_device("grade")
    H, W = _frame_size(color, "color", non_empty=True)
    dev = color.device
    if lut is not None and lut.device != dev:
        raise ValueError(f"lut must be a contiguous (N, N, N, 3) float32 CUDA tensor on {dev}")
    _check_out_f32(out_f32, want, H, W, dev)
    s = _stream_of(stream, dev)
    specs = {"f32": ((H, W, 3), torch.float32), "u8": ((H, W, 3), torch.uint8)}
    out, ptr = _stage_tensors(s, dev, want, specs, out_f32=out_f32)
    _lib.check(_lib.lib().rtm_grade(C.byref(prm), W, H, dev.index, color.data_ptr(), lut.data_ptr() if lut is not None else None,
                                    ptr("f32"), ptr("u8"), C.c_void_p(s.cuda_stream)), "rtm_grade")
    return out


_grade = grade  # for Renderer's methods, whose own parameter is named grade


def tonemap_stats(words):
    """tonemap()'s "stats" tensor as a dict {"log_average", "max_luminance", "exposure", "pixels"}; copies four words to the
    host (synchronise the stream that wrote them first when it is not the current one)."""
    raw = np.ascontiguousarray(words.cpu().numpy() if hasattr(words, "cpu") else words).view(np.uint32)
    f = raw.view(np.float32)
    return {"log_average": float(f[0]), "max_luminance": float(f[1]), "exposure": float(f[2]), "pixels": int(raw[3])}


# include/rtm.h: RTM_COMPARE_DEFAULTS (the dtype comes from the tensors)
COMPARE_DEFAULTS = {"tolerance": 1e-4, "peak": 1.0, "rel_epsilon": 1e-2, "map": "abs"}


def _compare_params(dtype, tolerance=COMPARE_DEFAULTS["tolerance"], peak=COMPARE_DEFAULTS["peak"],
                    rel_epsilon=COMPARE_DEFAULTS["rel_epsilon"], map=COMPARE_DEFAULTS["map"]):
    """compare()'s parameters as an rtm_compare_params; a ValueError names what the library would refuse.  No device use."""
    if map not in _lib.COMPARE_MAPS:
        raise ValueError(f"map is one of {tuple(_lib.COMPARE_MAPS)}, got {map!r}")
    tolerance, peak, rel_epsilon = float(tolerance), float(peak), float(rel_epsilon)
    if not (np.isfinite(tolerance) and tolerance >= 0.0):
        raise ValueError(f"tolerance must be finite and non-negative, got {tolerance!r}")
    if not (np.isfinite(peak) and peak > 0.0):
        raise ValueError(f"peak must be finite and positive, got {peak!r}")
    if not (np.isfinite(rel_epsilon) and rel_epsilon > 0.0):
        raise ValueError(f"rel_epsilon must be finite and positive, got {rel_epsilon!r}")
    return _lib.rtm_compare_params(_lib.COMPARE_DTYPES[dtype], _lib.COMPARE_MAPS[map], tolerance, peak, rel_epsilon)


def compare(a, b, tolerance=COMPARE_DEFAULTS["tolerance"], peak=COMPARE_DEFAULTS["peak"],
            rel_epsilon=COMPARE_DEFAULTS["rel_epsilon"], map=COMPARE_DEFAULTS["map"], want=("result",), stream=None):
    """Frame comparison (include/rtm.h: rtm_compare) on the device: `a` is the frame under test, `b` the reference, both
    contiguous (H, W, 3) torch CUDA tensors of the same shape, device and dtype, float32 or float64 (the dtype the library
    is told comes from the tensors).  tolerance: `outside` counts the pixels whose largest component error exceeds it; peak:
    PSNR's peak and SSIM's dynamic range; rel_epsilon: the offset of rel_mse's denominator; map "abs" | "ssim": what the
    "map" output holds.  Returns a dict of the names in `want`: "result" a 20-word int32 tensor holding the bits of
    rtm_compare_result (compare_result() reads it on the host), "map" an (H, W) float32 tensor.  A shape or dtype mismatch
    raises before the library is called.  Enqueued on `stream` (a torch.cuda.Stream or a raw hipStream_t handle; default: the
    current stream) with a work buffer allocated here; nothing waits for it and nothing is copied to the host."""
    _check_want(want, ("result", "map"))
    _pair_shape(a, b)
    dtype_a, dtype_b = str(a.dtype).split(".")[-1], str(b.dtype).split(".")[-1]
    if dtype_a != dtype_b:
        raise ValueError(f"a and b must have the same dtype, got {dtype_a} and {dtype_b}")
    if dtype_a not in _lib.COMPARE_DTYPES:
        raise ValueError(f"frames are float32 or float64, got {dtype_a}")
    prm = _compare_params(dtype_a, tolerance, peak, rel_epsilon, map)
    import torch
    _need_device("compare")
    H, W, dev = _pair_device(a, b)
    s = _stream_of(stream, dev)
    L = _lib.lib()
    specs = {"result": (C.sizeof(_lib.rtm_compare_result) // 4, torch.int32), "map": ((H, W), torch.float32)}
    out, ptr = _stage_tensors(s, dev, want, specs, max(256, L.rtm_compare_work_bytes(W, H)))
    _lib.check(L.rtm_compare(C.byref(prm), W, H, dev.index, a.data_ptr(), b.data_ptr(), ptr("work"), ptr("result"),
                             ptr("map"), C.c_void_p(s.cuda_stream)), "rtm_compare")
    return out


def compare_result(words):
    """compare()'s "result" tensor as a dict of rtm_compare_result's fields; copies the record's 20 words to the host
    (synchronise the stream that wrote them first when it is not the current one)."""
    raw = np.ascontiguousarray(words.cpu().numpy() if hasattr(words, "cpu") else words).view(np.uint8)
    rec = _lib.rtm_compare_result.from_buffer_copy(raw.tobytes())
    floats = ("max_abs", "mse", "psnr", "rel_mse", "ssim")
    return {name: (float(getattr(rec, name)) if name in floats else int(getattr(rec, name))) for name, _ in rec._fields_}


# include/rtm.h: RTM_FLIP_DEFAULTS (a 0.7 m wide 3840-pixel monitor viewed from 0.7 m)
FLIP_DEFAULTS = {"transfer": "srgb", "pixels_per_degree": 0.7 * 3840.0 / 0.7 * 3.14159265358979323846 / 180.0}


def _flip_params(transfer=FLIP_DEFAULTS["transfer"], pixels_per_degree=FLIP_DEFAULTS["pixels_per_degree"]):
    """flip()'s parameters as an rtm_flip_params; a ValueError names what the library would refuse.  No device use."""
    if transfer not in _lib.TRANSFERS:
        raise ValueError(f"transfer is one of {tuple(_lib.TRANSFERS)}, got {transfer!r}")
    pixels_per_degree = float(pixels_per_degree)
    if not (np.isfinite(pixels_per_degree) and 8.0 <= pixels_per_degree <= 128.0):
        raise ValueError(f"pixels_per_degree must be finite and in [8, 128], got {pixels_per_degree!r}")
    return _lib.rtm_flip_params(_lib.TRANSFERS[transfer], pixels_per_degree)


def flip(a, b, transfer=FLIP_DEFAULTS["transfer"], pixels_per_degree=FLIP_DEFAULTS["pixels_per_degree"], want=("result",),
         stream=None):
    """Perceptual frame difference (include/rtm.h: rtm_flip, LDR FLIP) on the device: `a` is the frame under test, `b` the
    reference, both contiguous (H, W, 3) float32 torch CUDA tensors of the same shape and device, DISPLAY-REFERRED (what
    tonemap()'s "f32" holds).  transfer "srgb" | "linear": how both are encoded; pixels_per_degree in [8, 128]: the viewing
    condition.  Returns a dict of the names in `want`: "result" a 268-word int32 tensor holding the bits of rtm_flip_result
    (flip_result() reads it on the host), "map" an (H, W) float32 tensor in [0, 1], NaN where a pixel has a non-finite
    component.  A shape or dtype mismatch raises before the library is called.  Enqueued on `stream` (a torch.cuda.Stream or
    a raw hipStream_t handle; default: the current stream) with a work buffer allocated here (112 bytes a pixel); nothing
    waits for it and nothing is copied to the host."""
    _check_want(want, ("result", "map"))
    _pair_shape(a, b)
    for name, v in (("a", a), ("b", b)):
        if str(v.dtype).split(".")[-1] != "float32":
            raise ValueError(f"{name} must be float32, got {v.dtype}")
    prm = _flip_params(transfer, pixels_per_degree)
    import torch
    _need_device("flip")
    H, W, dev = _pair_device(a, b)
    s = _stream_of(stream, dev)
    L = _lib.lib()
    specs = {"result": (C.sizeof(_lib.rtm_flip_result) // 4, torch.int32), "map": ((H, W), torch.float32)}
    out, ptr = _stage_tensors(s, dev, want, specs, max(256, L.rtm_flip_work_bytes(W, H)))
    _lib.check(L.rtm_flip(C.byref(prm), W, H, dev.index, a.data_ptr(), b.data_ptr(), ptr("work"), ptr("result"),
                          ptr("map"), C.c_void_p(s.cuda_stream)), "rtm_flip")
    return out


def _flip_weighted_quantile(hist, q):
    """The published tool's pooling of the histogram: bin i weighs its count times its centre value (i + 0.5) / 256; the
    quantile is the centre of the first bin at which the running weight reaches q of the total (0 for an empty histogram)."""
    centres = (np.arange(256) + 0.5) / 256.0
    run = np.cumsum(np.asarray(hist, np.float64) * centres)  # bin by bin, in ascending order
    if run[-1] <= 0:
        return 0.0
    return float(centres[int(np.searchsorted(run, q * run[-1], side="left"))])


def flip_result(words):
    """flip()'s "result" tensor as a dict of rtm_flip_result's fields ("hist" a list of 256 counts) plus
    "weighted_median", "weighted_first_quartile" and "weighted_third_quartile", derived here from the histogram with each
    bin weighted by its centre value, as the published tool pools: they have the bins' resolution, 1/256.  Copies the
    record's 268 words to the host (synchronise the stream that wrote them first when it is not the current one)."""
    raw = np.ascontiguousarray(words.cpu().numpy() if hasattr(words, "cpu") else words).view(np.uint8)
    rec = _lib.rtm_flip_result.from_buffer_copy(raw.tobytes())
    out = {"mean": float(rec.mean), "max": float(rec.max), "min": float(rec.min), "pixels": int(rec.pixels),
           "nonfinite": int(rec.nonfinite), "argmax_x": int(rec.argmax_x), "argmax_y": int(rec.argmax_y), "hist": list(rec.hist)}
    out["weighted_median"] = _flip_weighted_quantile(out["hist"], 0.5)
    out["weighted_first_quartile"] = _flip_weighted_quantile(out["hist"], 0.25)
    out["weighted_third_quartile"] = _flip_weighted_quantile(out["hist"], 0.75)
    return out


# include/rtm.h: RTM_SCOPE_DEFAULTS
SCOPE_DEFAULTS = dict(_lib.SCOPE_DEFAULTS)
SCOPE_PERCENTILES = (1.0, 50.0, 99.0, 99.9)  # what rtm_cli --scopes and Renderer.write_scopes report of channel Y


def _scope_enum(name, value, table):
    if value not in table:
        raise ValueError(f"{name} is one of {tuple(table)}, got {value!r}")
    return table[value]


def _scope_int(name, v, lo, hi=None):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or int(v) < lo or (hi is not None and int(v) > hi):
        raise ValueError(f"{name} is an integer {f'in {lo}..{hi}' if hi is not None else f'from {lo}'}, got {v!r}")
    return int(v)


def scopes(color, mode=SCOPE_DEFAULTS["mode"], columns=SCOPE_DEFAULTS["columns"], want=("histogram",), stream=None):
    """The frame scopes (include/rtm.h: rtm_scopes) on the device: per-channel histograms (Y, R, G, B) of `color`, an
    (H, W, 3) float32 torch CUDA tensor (any 4-byte-aligned contiguous view), and its per-column waveform.  mode "log2": 8
    bins a stop from 2^-16 to 2^16, for a linear frame; "code": the 256 8-bit code values, for a display frame in [0, 1].
    columns: the waveform's columns, 1..W (ignored without "waveform").  Returns a dict of the names in `want`: "histogram" a
    1036-word int32 tensor holding the bits of rtm_scope_histogram (scope_histogram() reads it on the host; scope_percentile()
    and scope_exposure() take it as it is), "waveform" a (4, 256, columns) int32 tensor of counts, values below the bins in
    row 0 and above them in row 255.  Exact integer counts by integer atomics: every call gives the same words.  Enqueued on
    `stream` (a torch.cuda.Stream or a raw hipStream_t handle; default: the current stream); nothing waits for it and nothing
    is copied to the host."""
    _check_want(want, ("histogram", "waveform"))
    prm = _lib.rtm_scope_params(_scope_enum("mode", mode, _lib.SCOPE_MODES), 0)
    import torch
    _need_device("scopes")
    H, W = _frame_size(color, "color", non_empty=True)
    if "waveform" in want:
        prm.columns = _scope_int("columns", columns, 1, W)
    dev = color.device
    s = _stream_of(stream, dev)
    specs = {"histogram": (C.sizeof(_lib.rtm_scope_histogram) // 4, torch.int32),
             "waveform": ((4, 256, max(1, prm.columns)), torch.int32)}
    out, ptr = _stage_tensors(s, dev, want, specs)
    _lib.check(_lib.lib().rtm_scopes(C.byref(prm), W, H, dev.index, color.data_ptr(), ptr("histogram"), ptr("waveform"),
                                     C.c_void_p(s.cuda_stream)), "rtm_scopes")
    return out


def _scope_record(hist):
    """An rtm_scope_histogram on the host of scopes()'s "histogram" tensor, its words as an array, or scope_histogram()'s dict."""
    if isinstance(hist, _lib.rtm_scope_histogram):
        return hist
    if isinstance(hist, dict):
        raw = np.concatenate([np.asarray(hist["bins"], np.uint32).reshape(-1), np.asarray(hist["below"], np.uint32),
                              np.asarray(hist["above"], np.uint32),
                              np.array([hist["pixels"], hist["not_counting"], 0, 0], np.uint32)])
    else:
        raw = np.ascontiguousarray(hist.cpu().numpy() if hasattr(hist, "cpu") else hist).reshape(-1).view(np.uint32)
    if raw.size != C.sizeof(_lib.rtm_scope_histogram) // 4:
        raise ValueError(f"a histogram is {C.sizeof(_lib.rtm_scope_histogram) // 4} words, got {raw.size}")
    return _lib.rtm_scope_histogram.from_buffer_copy(raw.tobytes())


def scope_histogram(words):
    """scopes()'s "histogram" tensor as a dict of rtm_scope_histogram's fields: "bins" a (4, 256) uint32 array (channels Y, R,
    G, B), "below" and "above" uint32 arrays of 4, "pixels" and "not_counting" ints.  Copies the record's 1036 words to the
    host (synchronise the stream that wrote them first when it is not the current one)."""
    rec = _scope_record(words)
    return {"bins": np.ctypeslib.as_array(rec.bins).astype(np.uint32).reshape(4, 256), "below": np.array(rec.below[:], np.uint32),
            "above": np.array(rec.above[:], np.uint32), "pixels": int(rec.pixels), "not_counting": int(rec.not_counting)}


def scope_draw(waveform, layout="luma", gain=1, stream=None):
    """The picture of a waveform (include/rtm.h: rtm_scope_draw) on the device: `waveform` is scopes()'s (4, 256, columns) int32
    tensor.  layout "luma" (channel Y in grey), "overlay" (R, G, B in their own bytes) or "parade" (three panels side by side);
    a value is min(255, count * gain), gain an integer from 1.  Returns a (256, columns, 3) uint8 tensor, (256, 3 columns, 3)
    for the parade, bin 255 on top.  Enqueued on `stream`."""
    lay = _scope_enum("layout", layout, _lib.SCOPE_LAYOUTS)
    gain = _scope_int("gain", gain, 1, 0xFFFFFFFF)
    import torch
    _need_device("scope_draw")
    if not (isinstance(waveform, torch.Tensor) and waveform.is_cuda and waveform.dtype == torch.int32 and waveform.dim() == 3
            and tuple(waveform.shape[:2]) == (4, 256) and waveform.shape[2] >= 1 and waveform.is_contiguous()):
        raise ValueError("waveform must be a contiguous (4, 256, columns) int32 CUDA tensor")
    columns = int(waveform.shape[2])
    dev = waveform.device
    s = _stream_of(stream, dev)
    out, ptr = _stage_tensors(s, dev, ("u8",), {"u8": ((256, columns * (3 if layout == "parade" else 1), 3), torch.uint8)})
    _lib.check(_lib.lib().rtm_scope_draw(columns, lay, gain, dev.index, waveform.data_ptr(), ptr("u8"), C.c_void_p(s.cuda_stream)),
               "rtm_scope_draw")
    return out["u8"]


def scope_bin_range(mode, bin):
    """(lo, hi) of a histogram bin 0..255 in `mode` ("log2" or "code"), as floats (include/rtm.h: rtm_scope_bin_range).  No
    device use."""
    lo, hi = C.c_float(), C.c_float()
    _lib.check(_lib.lib().rtm_scope_bin_range(_scope_enum("mode", mode, _lib.SCOPE_MODES), _scope_int("bin", bin, 0, 255),
                                              C.byref(lo), C.byref(hi)), "rtm_scope_bin_range")
    return lo.value, hi.value


def _scope_channel(channel):
    if isinstance(channel, str):
        return _scope_enum("channel", channel, {k: i for i, k in enumerate(_lib.SCOPE_CHANNELS)})
    return _scope_int("channel", channel, 0, 3)


def scope_percentile(hist, percent, channel="y", mode=SCOPE_DEFAULTS["mode"]):
    """The value under which `percent` of the counting pixels' channel lies (include/rtm.h: rtm_scope_percentile), linear
    inside its bin: (value, bin).  `hist` is scopes()'s "histogram" tensor (copied to the host here), its words or
    scope_histogram()'s dict; `mode` the mode it was taken in; channel "y", "r", "g", "b" or 0..3.  bin is -2 for a frame
    without a counting pixel (value 1), -1 when the percentile lies below the bins (value 0), 256 past the last one."""
    value, bin_ = C.c_float(), C.c_int32()
    rec = _scope_record(hist)
    _lib.check(_lib.lib().rtm_scope_percentile(C.byref(rec), _scope_enum("mode", mode, _lib.SCOPE_MODES), _scope_channel(channel),
                                               float(percent), C.byref(value), C.byref(bin_)), "rtm_scope_percentile")
    return value.value, bin_.value


def scope_exposure(hist, percent, target=0.18):
    """The exposure in stops that puts the `percent` percentile of a "log2" histogram's luminance at `target`
    (include/rtm.h: rtm_scope_exposure): tonemap(color, exposure=ev).  Clamped to +-32; 0 when the percentile is 0."""
    ev = C.c_float()
    rec = _scope_record(hist)
    _lib.check(_lib.lib().rtm_scope_exposure(C.byref(rec), float(percent), float(target), C.byref(ev)), "rtm_scope_exposure")
    return ev.value


def scope_summary(hist, mode=SCOPE_DEFAULTS["mode"]):
    """What rtm_cli --scopes prints of one frame: {"mode", "pixels", "not_counting", "percentiles" (of Y at 1, 50, 99 and 99.9,
    keyed by the percent's text), "below" and "above" (the share of the counting pixels outside the bins, per channel Y, R, G,
    B)}.  `hist` as scope_percentile() takes it."""
    rec = _scope_record(hist)
    n = int(rec.pixels)
    share = lambda v: [int(x) / n if n else 0.0 for x in v]
    return {"mode": mode, "pixels": n, "not_counting": int(rec.not_counting),
            "percentiles": {f"{p:g}": scope_percentile(rec, p, 0, mode)[0] for p in SCOPE_PERCENTILES},
            "below": share(rec.below), "above": share(rec.above)}


def plan_passes(n_samples, passes=None, samples_per_pass=None):
    """The passes [a, b) of a progressive frame of n_samples samples per pixel: contiguous, covering [0, n_samples), sizes
    that differ by at most one sample.  Give `passes`, or `samples_per_pass` (the pass count is then its ceiling share);
    neither: one pass."""
    n_samples = int(n_samples)
    if n_samples < 1:
        raise ValueError("a frame has at least one sample per pixel")
    if passes is not None and samples_per_pass is not None:
        raise ValueError("give passes or samples_per_pass, not both")
    if samples_per_pass is not None:
        if int(samples_per_pass) < 1:
            raise ValueError("samples_per_pass must be at least 1")
        passes = -(-n_samples // int(samples_per_pass))
    passes = 1 if passes is None else int(passes)
    if passes < 1 or passes > n_samples:
        raise ValueError(f"passes must be in [1, {n_samples}] (one sample per pass at most that many), got {passes}")
    q, r = divmod(n_samples, passes)
    out, a = [], 0
    for i in range(passes):
        b = a + q + (1 if i < r else 0)
        out.append((a, b))
        a = b
    return out


# ---- seams below the renderer, for parity tests --------------------------------------------------
def path_tracing_batch(data: SettingData, org, direction, mode="repaired", max_bounces=-1,
                       seed=0x5EED, device=0, host_trig=True):
    """png::PathTracing (src/Renderer.cpp:57-117) for n rays; ray i draws from stream (seed, i, 0)."""
    org = np.ascontiguousarray(org, dtype=np.float64).reshape(-1, 3)
    direction = np.ascontiguousarray(direction, dtype=np.float64).reshape(-1, 3)
    n_rays = org.shape[0]
    out = np.zeros((n_rays, 3), dtype=np.float64)
    draws = np.zeros(n_rays, dtype=np.uint32)
    casts = np.zeros(n_rays, dtype=np.uint32)
    _, arr, n = data.to_c()
    o = rtm_options()
    o.mode = _lib.MODES[mode] | (_lib.MODE_HOST_TRIG if host_trig else 0)
    o.max_bounces, o.seed, o.device = int(max_bounces), int(seed), device
    _lib.check(_lib.lib().rtm_path_trace_batch(arr, n, C.byref(o), org.ctypes.data,
                                               direction.ctypes.data, n_rays, out.ctypes.data,
                                               draws.ctypes.data, casts.ctypes.data),
               "rtm_path_trace_batch")
    return out, draws, casts


def surface_sample_batch(data: SettingData, org, direction, mode="repaired", max_bounces=-1, seed=0x5EED, device=0):
    """png::SurfaeSample (src/Renderer.cpp:119-198), entered at depth 0, for n rays; ray i draws from stream (seed, i, 0)."""
    org = np.ascontiguousarray(org, dtype=np.float64).reshape(-1, 3)
    direction = np.ascontiguousarray(direction, dtype=np.float64).reshape(-1, 3)
    n_rays = org.shape[0]
    out = np.zeros((n_rays, 3), dtype=np.float64)
    draws = np.zeros(n_rays, dtype=np.uint32)
    casts = np.zeros(n_rays, dtype=np.uint32)
    _, arr, n = data.to_c()
    o = rtm_options()
    o.mode = _lib.MODES[mode]
    o.max_bounces, o.seed, o.device = int(max_bounces), int(seed), device
    _lib.check(_lib.lib().rtm_surface_sample_batch(arr, n, C.byref(o), org.ctypes.data, direction.ctypes.data, n_rays,
                                                   out.ctypes.data, draws.ctypes.data, casts.ctypes.data),
               "rtm_surface_sample_batch")
    return out, draws, casts


def intersect_objects_batch(objects_c, org, direction, mode="repaired", t_init=-1.0, n_init=7.0):
    """Object::Intersect for rtm_object entries (spheres and planes), pair i = (ray i, object i)."""
    org = np.ascontiguousarray(org, dtype=np.float64).reshape(-1, 3)
    direction = np.ascontiguousarray(direction, dtype=np.float64).reshape(-1, 3)
    n = org.shape[0]
    hit = np.zeros(n, dtype=np.int32)
    t = np.full(n, t_init, dtype=np.float64)
    nrm = np.full((n, 3), n_init, dtype=np.float64)
    _lib.check(_lib.lib().rtm_intersect_objects_batch(objects_c, org.ctypes.data, direction.ctypes.data, n,
                                                      _lib.MODES[mode], hit.ctypes.data, t.ctypes.data,
                                                      nrm.ctypes.data), "rtm_intersect_objects_batch")
    return hit, t, nrm


def intersect_batch(spheres_c, org, direction, mode="repaired", t_init=-1.0, n_init=7.0):
    """SphereObject::Intersect (src/SettingData.cpp:197-226), pair i = (ray i, sphere i)."""
    org = np.ascontiguousarray(org, dtype=np.float64).reshape(-1, 3)
    direction = np.ascontiguousarray(direction, dtype=np.float64).reshape(-1, 3)
    n = org.shape[0]
    hit = np.zeros(n, dtype=np.int32)
    t = np.full(n, t_init, dtype=np.float64)
    nrm = np.full((n, 3), n_init, dtype=np.float64)
    _lib.check(_lib.lib().rtm_intersect_batch(spheres_c, org.ctypes.data, direction.ctypes.data, n,
                                              _lib.MODES[mode], hit.ctypes.data, t.ctypes.data,
                                              nrm.ctypes.data), "rtm_intersect_batch")
    return hit, t, nrm
