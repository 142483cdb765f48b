"""numpy restatement of the disparity densification (include/dis_hip.h, section "disparity densification"; csrc/densify.hip): the gated
hole fill from the first valid pixel in each of 8 directions, then the lower median over the valid pixels of a window.  Shifted views of
a zero-padded copy and np.sort; it knows nothing of the kernels' tiles.  Everything is selection and comparison (the gate is one fp32
subtraction), so the kernels are compared with it for equality."""
import numpy as np

F = np.float32
FLT_MAX = float(np.finfo(np.float32).max)
DIRECTIONS = ((0, 1), (0, -1), (1, 0), (-1, 0), (1, 1), (1, -1), (-1, 1), (-1, -1))      # (dy, dx): E, W, S, N, SE, SW, NE, NW
MAX_GAP = 32


def valid_mask(disp):
    """0 < d < inf (NaN: False)"""
    d = np.asarray(disp, dtype=F)
    with np.errstate(invalid='ignore'):
        return (d > 0) & (d < np.inf)


def _shifted(padded, pad, dy, dx, h, w):
    """the view v with v[y, x] = image[y + dy, x + dx], 0 outside the image"""
    return padded[:, pad + dy:pad + dy + h, pad + dx:pad + dx + w]


def _lower_median(values, count):
    """values (..., q) with +inf for the missing entries, count (...) of the finite ones -> v[(count - 1) // 2] of the ascending order
    (count 0: +inf)"""
    v = np.sort(values, axis=-1)
    pos = np.maximum(count - 1, 0) // 2
    return np.take_along_axis(v, pos[..., None], axis=-1)[..., 0]


def fill(clean, max_gap, min_dirs, max_spread):
    """clean (n, h, w): invalid pixels are 0 -> (filled map, state uint8: 0 invalid, 1 valid in the input, 2 filled)"""
    n, h, w = clean.shape
    ok = clean > 0
    state = ok.astype(np.uint8)
    if max_gap == 0:
        return clean.copy(), state
    g = max_gap
    padded = np.zeros((n, h + 2 * g, w + 2 * g), F)
    padded[:, g:g + h, g:g + w] = clean
    found = np.full((n, h, w, 8), np.inf, F)
    for k, (dy, dx) in enumerate(DIRECTIONS):
        first = np.zeros((n, h, w), F)                  # the first valid pixel met on the walk, 0: none yet
        for s in range(1, g + 1):
            v = _shifted(padded, g, s * dy, s * dx, h, w)
            first = np.where(first > 0, first, v)
        found[..., k] = np.where(first > 0, first, F(np.inf))
    hit = found < np.inf
    m = hit.sum(axis=-1)
    lo = found.min(axis=-1)
    hi = np.where(hit, found, F(0)).max(axis=-1)
    with np.errstate(invalid='ignore'):
        spread = (hi - lo).astype(F)                    # one fp32 subtraction (m = 0: 0 - inf, not used)
        take = ~ok & (m >= min_dirs) & (spread <= F(max_spread))
    med = _lower_median(found, m)
    out = np.where(take, med, clean).astype(F)
    state[take] = 2
    return out, state


def median(stage1, r):
    """stage1 (n, h, w): invalid pixels are 0 -> every valid pixel replaced by the lower median of the valid pixels of its
    (2 r + 1)^2 window, clipped to the image"""
    if r == 0:
        return stage1.copy()
    n, h, w = stage1.shape
    padded = np.zeros((n, h + 2 * r, w + 2 * r), F)
    padded[:, r:r + h, r:r + w] = stage1
    win = np.stack([_shifted(padded, r, dy, dx, h, w) for dy in range(-r, r + 1) for dx in range(-r, r + 1)], axis=-1)
    ok = win > 0
    k = ok.sum(axis=-1)
    med = _lower_median(np.where(ok, win, F(np.inf)), k)
    return np.where(stage1 > 0, med, F(0)).astype(F)


def disp_densify(disp, max_gap=16, min_dirs=6, max_spread=2.0, median_r=1):
    """disp (n, h, w) or (n, 1, h, w) float32 -> out (the shape of disp) float32, state (n, h, w) uint8"""
    disp = np.asarray(disp, dtype=F)
    if not (disp.ndim == 3 or (disp.ndim == 4 and disp.shape[1] == 1)):
        raise ValueError('disp (n, h, w) or (n, 1, h, w) is expected')
    max_gap, min_dirs, median_r, max_spread = int(max_gap), int(min_dirs), int(median_r), float(max_spread)
    if not (0 <= max_gap <= MAX_GAP and 1 <= min_dirs <= 8 and median_r in (0, 1, 2) and 0 <= max_spread <= FLT_MAX):
        raise ValueError('max_gap 0 .. 32, min_dirs 1 .. 8, median_r 0, 1 or 2 and max_spread in [0, FLT_MAX] are expected')
    planes = disp.reshape(disp.shape[0], disp.shape[-2], disp.shape[-1])
    clean = np.where(valid_mask(planes), planes, F(0)).astype(F)          # every invalid element is +0.0 from here on
    stage1, state = fill(clean, max_gap, min_dirs, max_spread)
    out = median(stage1, median_r)
    return out.reshape(disp.shape), state
