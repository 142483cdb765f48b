"""numpy restatement of the speckle filter (include/dis_hip.h, section "speckle filter"; csrc/speckle.hip): the 4-connected components
of similar disparity, and the small ones set to 0.  Plain union-find over the list of linked neighbour pairs, one image at a time; it
knows nothing of the kernels' tiles.  Everything it returns is fully determined by the input, so the kernels are compared with it for
equality."""
import numpy as np


def valid_mask(disp):
    """0 < d < inf (NaN: False)"""
    d = np.asarray(disp, dtype=np.float32)
    with np.errstate(invalid='ignore'):
        return (d > 0) & (d < np.inf)


def _links(d, ok, max_diff, axis):
    """the linked pairs of one image along `axis` as two arrays of linear indices (the first pixel of a pair, its neighbour after it)"""
    h, w = d.shape
    idx = np.arange(h * w, dtype=np.int64).reshape(h, w)
    a = (slice(None, -1), slice(None)) if axis == 0 else (slice(None), slice(None, -1))
    b = (slice(1, None), slice(None)) if axis == 0 else (slice(None), slice(1, None))
    with np.errstate(invalid='ignore', over='ignore'):
        diff = np.abs((d[a] - d[b]).astype(np.float32))            # the subtraction in fp32
        link = ok[a] & ok[b] & (diff <= np.float32(max_diff))
    return idx[a][link], idx[b][link]


def label_image(d, max_diff):
    """one image (h, w) -> label (h, w) int32: the lowest y * w + x of the pixel's component, -1 for an invalid pixel; size (h, w) int32:
    the pixels of the component, 0 for an invalid pixel"""
    d = np.asarray(d, dtype=np.float32)
    h, w = d.shape
    ok = valid_mask(d)
    parent = list(range(h * w))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]      # path halving
            x = parent[x]
        return x

    for axis in (1, 0):
        p, q = _links(d, ok, max_diff, axis)
        for a, b in zip(p.tolist(), q.tolist()):
            ra, rb = find(a), find(b)
            if ra < rb:                        # the lower index stays the root: the root is the component's first pixel in row order
                parent[rb] = ra
            elif rb < ra:
                parent[ra] = rb
    root = np.fromiter((find(x) for x in range(h * w)), dtype=np.int64, count=h * w).reshape(h, w)
    count = np.bincount(root[ok], minlength=h * w)
    label = np.where(ok, root, -1).astype(np.int32)
    size = np.where(ok, count[root], 0).astype(np.int32)
    return label, size


def speckle_filter(disp, max_size=100, max_diff=1.0):
    """disp (n, h, w) or (n, 1, h, w) float32 -> out (the shape of disp), label (n, h, w) int32, size (n, h, w) int32.  out keeps the
    bits of every valid pixel whose component has more than max_size pixels; every other element is 0.0."""
    disp = np.asarray(disp, dtype=np.float32)
    if not (disp.ndim == 3 or (disp.ndim == 4 and disp.shape[1] == 1)):
        raise ValueError('disp (n, h, w) or (n, 1, h, w) is expected')
    if not (int(max_size) >= 0 and 0 <= float(max_diff) < np.inf):
        raise ValueError('max_size >= 0 and a finite max_diff >= 0 are expected')
    planes = disp.reshape(disp.shape[0], disp.shape[-2], disp.shape[-1])
    label = np.empty(planes.shape, np.int32)
    size = np.empty(planes.shape, np.int32)
    for k, d in enumerate(planes):
        label[k], size[k] = label_image(d, max_diff)
    out = np.where(size > int(max_size), planes, np.float32(0)).astype(np.float32)
    return out.reshape(disp.shape), label, size
