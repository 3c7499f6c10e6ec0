"""First-hit feature buffers, the parts that need no GPU: the PFM writer round trip, argument checks of rtm_render_aov
(all made before any device call), and the bindings."""
import ctypes as C

import numpy as np
import pytest


def _read_pfm(path):
    raw = open(path, "rb").read()
    kind, dims, scale, body = raw.split(b"\n", 3)
    w, h = (int(v) for v in dims.split())
    comp = {b"PF": 3, b"Pf": 1}[kind]
    return kind, w, h, scale, np.frombuffer(body, dtype="<f4").reshape(h, w * comp)


@pytest.mark.parametrize("comp", [1, 3])
def test_pfm_round_trip_keeps_every_float_bit(tmp_path, comp):
    from raytracingmin_amd import _lib
    w, h = 7, 5
    rng = np.random.default_rng(comp)
    img = rng.standard_normal((h, w * comp)).astype(np.float32)
    img.flat[:6] = [np.inf, -np.inf, -0.0, 0.0, np.float32(1e-45), np.nan]
    path = tmp_path / f"p{comp}.pfm"
    assert _lib.lib().rtm_write_pfm(str(path).encode(), w, h, comp, img.ctypes.data) == 1
    kind, rw, rh, scale, body = _read_pfm(path)
    assert (kind, rw, rh, scale) == (b"PF" if comp == 3 else b"Pf", w, h, b"-1.0")
    assert len(open(path, "rb").read()) == len(kind) + len(f"\n{w} {h}\n-1.0\n") + 4 * w * h * comp
    # rows bottom-up: the file's first row is the image's last
    assert np.array_equal(body[::-1].view(np.uint32), img.view(np.uint32))


def test_pfm_rejects_bad_arguments(tmp_path):
    from raytracingmin_amd import _lib
    L = _lib.lib()
    buf = np.zeros(12, np.float32)
    p = str(tmp_path / "x.pfm").encode()
    assert L.rtm_write_pfm(p, 2, 2, 2, buf.ctypes.data) == 0
    assert L.rtm_write_pfm(p, 0, 2, 1, buf.ctypes.data) == 0
    assert L.rtm_write_pfm(p, 2, 2, 3, None) == 0
    assert L.rtm_write_pfm(None, 2, 2, 3, buf.ctypes.data) == 0
    assert L.rtm_write_pfm(str(tmp_path / "no" / "dir.pfm").encode(), 2, 2, 3, buf.ctypes.data) == 0


def test_render_aov_rejects_null_and_malformed_arguments_without_a_gpu():
    from raytracingmin_amd import _lib
    L = _lib.lib()
    st, opt, bufs = _lib.rtm_settings(), _lib.rtm_options(), _lib.rtm_aov_buffers()
    st.width, st.height, st.samples, st.super_samples = 8, 8, 1, 1
    opt.mode, opt.row_begin, opt.row_end = 1, 0, 8
    fake_scene = C.c_void_p(1)  # never looked at: every check below fails first
    assert L.rtm_render_aov(None, fake_scene, C.byref(opt), C.byref(bufs), None) == -1
    assert L.rtm_render_aov(C.byref(st), fake_scene, None, C.byref(bufs), None) == -1
    assert L.rtm_render_aov(C.byref(st), fake_scene, C.byref(opt), None, None) == -1
    assert b"null" in L.rtm_last_error_detail()
    assert L.rtm_render_aov(C.byref(st), None, C.byref(opt), C.byref(bufs), None) == -1
    for field, value in (("row_end", 9), ("row_begin", -1), ("row_begin", 9), ("mode", 7), ("band_count", -1)):
        bad = _lib.rtm_options.from_buffer_copy(opt)
        setattr(bad, field, value)
        assert L.rtm_render_aov(C.byref(st), fake_scene, C.byref(bad), C.byref(bufs), None) == -1, field
    bad = _lib.rtm_options.from_buffer_copy(opt)
    bad.band_count, bad.band_index = 3, 3
    assert L.rtm_render_aov(C.byref(st), fake_scene, C.byref(bad), C.byref(bufs), None) == -1
    st.width = 0
    assert L.rtm_render_aov(C.byref(st), fake_scene, C.byref(opt), C.byref(bufs), None) == -1


def test_render_aov_and_pfm_are_bound():
    import raytracingmin_amd as rtm
    from raytracingmin_amd import _lib
    assert "rtm_render_aov" in _lib.SIGNATURES and "rtm_write_pfm" in _lib.SIGNATURES
    assert C.sizeof(_lib.rtm_aov_buffers) == 32
    assert callable(rtm.Renderer.render_aov) and callable(rtm.Renderer.write_aov)
    import inspect
    assert "aov" in inspect.signature(rtm.Renderer.Render).parameters
    assert _lib.lib().rtm_abi_version() == 5
