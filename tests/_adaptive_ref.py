"""NumPy float64 restatement of tile-adaptive sampling (include/rtm.h: rtm_render_adaptive): the pass schedule, the
checkpoint's error estimate and the per-tile decision.  No GPU: the tests feed it accumulators."""
import numpy as np


def schedule(n_samples, min_samples):
    """The pass ends b_0 = min(m, N), b_i = min(2^i m, N), up to and including the first that reaches N."""
    if min_samples < 1 or n_samples < 1:
        raise ValueError("min_samples and n_samples must be >= 1")
    ends = [min(min_samples, n_samples)]
    while ends[-1] < n_samples:
        ends.append(min(2 * ends[-1], n_samples))
    return ends


def tile_error(acc, snap, n_samples, a, b, tiles_x, tile):
    """E of one tile: acc after [0, b), snap after [0, a); both (rows, W, 3) float64 arrays of the call's rows."""
    rows, width = acc.shape[0], acc.shape[1]
    ty, tx = divmod(int(tile), tiles_x)
    r0, x0 = ty * 8, tx * 8
    I = acc[r0:min(r0 + 8, rows), x0:min(x0 + 8, width)].reshape(-1, 3) * (np.float64(n_samples) / np.float64(b))
    J = snap[r0:min(r0 + 8, rows), x0:min(x0 + 8, width)].reshape(-1, 3) * (np.float64(n_samples) / np.float64(a))
    with np.errstate(invalid="ignore", divide="ignore"):
        d = (np.abs(I[:, 0] - J[:, 0]) + np.abs(I[:, 1] - J[:, 1])) + np.abs(I[:, 2] - J[:, 2])
        e = d / (np.float64(1e-3) + np.sqrt((I[:, 0] + I[:, 1]) + I[:, 2]))
    if np.isnan(e).any():
        return np.float64("nan")
    return np.float64(e.max())


def stays_active(E, b, n_samples, threshold):
    """The checkpoint's decision: b < N and not (E <= threshold) (threshold as the float the C struct holds)."""
    return bool(b < n_samples and not (E <= np.float64(np.float32(threshold))))


def run(states, n_samples, min_samples, threshold, tiles_x, tiles_y):
    """The whole schedule on the progressive accumulators `states` (dict: pass end b -> (rows, W, 3) float64 array, the
    frame's accumulator after [0, b)).  Returns (tile_samples (tiles_y, tiles_x) int64, the list of (b, active tiles)
    after each checkpoint)."""
    ends = schedule(n_samples, min_samples)
    n_tiles = tiles_x * tiles_y
    samples = np.full(n_tiles, ends[0], dtype=np.int64)
    snap_end = np.full(n_tiles, ends[0], dtype=np.int64)  # the pass end each tile's snapshot holds
    active = list(range(n_tiles))
    trace = []
    for i in range(1, len(ends)):
        if not active:
            break
        a, b = ends[i - 1], ends[i]
        nxt = []
        for t in active:
            assert snap_end[t] == a
            E = tile_error(states[b], states[a], n_samples, a, b, tiles_x, t)
            samples[t] = b
            if stays_active(E, b, n_samples, threshold):
                nxt.append(t)
                snap_end[t] = b
        active = nxt
        trace.append((b, list(active)))
    return samples.reshape(tiles_y, tiles_x), trace


def work_bytes(width, rows):
    """rtm_adaptive_work_bytes: the snapshot plane, two tile lists and the flags (each rounded up to 256 bytes) + 256."""
    if width <= 0 or rows <= 0:
        return 0
    r = lambda b: (b + 255) // 256 * 256
    tiles = ((width + 7) // 8) * ((rows + 7) // 8)
    return r(width * rows * 24) + 3 * r(tiles * 4) + 256
