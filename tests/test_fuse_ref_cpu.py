"""CPU: the numpy restatement of the track fusion (tests/fuse_ref.py) against what the definition implies on inputs whose answer is
known - exact plane disparities, one frame scaled out of agreement, the keep rule, holes - the cap on the pixels the GPU tests exempt,
and the PLY writer of data/ply.py."""
import numpy as np
import pytest

from tests import fuse_inputs as FI
from tests import fuse_ref

SMALL = [s for s in FI.SHAPES if s[2] * s[3] > 4]


def _fuse(a, tol=0.01, min_views=2, dtype=np.float64, disp=None, value=True):
    return fuse_ref.fuse(a['disp'] if disp is None else disp, a['R'], a['t'], a['K'], a['baseline'], a['value'] if value else None, tol,
                         min_views, dtype=dtype)


@pytest.mark.parametrize('shape', SMALL, ids=FI.shape_id)
def test_exact_plane_disparities_agree_wherever_they_are_seen(shape):
    from depthinspace_amd import synth
    a = FI.make_input(shape, 'plane')
    r32, r64 = _fuse(a, dtype=np.float32), _fuse(a)
    assert r64['valid'].all() and int(r64['seen'].max()) == shape[1] - 1      # the comparison is not one of zeros
    for r in (r32, r64):
        assert np.array_equal(r['views'], 1 + r['seen'])
    # resid: the depth of a plane is not linear in the pixel (its inverse is), but at this tilt and focal length the curvature of z
    # over one cell is below the float32 scale, so the residual of exact disparities is zero up to the tolerance of the output
    tol_r = fuse_ref.tolerance(r32['resid'], r64['resid'])
    tol_p = fuse_ref.tolerance(np.moveaxis(r32['point'], 2, -1), np.moveaxis(r64['point'], 2, -1))
    for r in (r32, r64):
        off = np.abs(np.moveaxis(r['point'], 2, -1).astype(np.float64) @ synth._PLANE_N - synth._PLANE_C)
        print(f'{r["resid"].dtype}: max resid {r["resid"].max():.3e} (allowed {tol_r:.3e}), max |n . X - c| {off.max():.3e} (allowed {tol_p:.3e})')
        assert float(r['resid'].max()) <= tol_r
        assert float(off.max()) <= tol_p                                       # the fused points lie in synth's plane n . X = c


@pytest.mark.parametrize('shape', SMALL, ids=FI.shape_id)
def test_a_frame_scaled_out_of_agreement_is_left_out(shape):
    n, tl, H, W = shape
    exact, scaled = _fuse(FI.make_input(shape, 'plane')), _fuse(FI.make_input(shape, 'scaled'))
    assert not scaled['keep'][:, -1].any()
    assert (scaled['views'][:, -1] == 1).all()
    if tl == 2:
        assert not scaled['keep'].any() and (scaled['views'] == 1).all()
    seen_in_last = exact['seen_ij'][:, :, -1]                                  # (n, tl, H, W): pair (i, last)
    assert seen_in_last[:, :-1].any()
    assert np.array_equal(scaled['seen_ij'][:, :-1, -1], seen_in_last[:, :-1])
    assert np.array_equal(scaled['views'][:, :-1], exact['views'][:, :-1] - seen_in_last[:, :-1])


@pytest.mark.parametrize('shape', SMALL, ids=FI.shape_id)
def test_keep_rule_and_packed_list(shape):
    n, tl, H, W = shape
    a = FI.make_input(shape, 'bumps')
    for mv in range(1, tl + 1):
        r = _fuse(a, min_views=mv)
        assert np.array_equal(r['keep'][:, 0], r['valid'][:, 0] & (r['views'][:, 0] >= mv))
        lower = np.zeros(r['keep'].shape, bool)
        for i in range(tl):
            for j in range(i):
                lower[:, i] |= r['cons_ij'][:, i, j]
        assert np.array_equal(r['keep'], r['valid'] & (r['views'] >= mv) & ~lower)
        if mv == 1:
            assert (r['keep'] & (r['seen'] == 0)).any()                          # pixels no other frame sees are kept
        # the packed list: the dense maps gathered at keep, in src order
        src = r['src'].astype(np.int64)
        assert np.all(np.diff(src) > 0) and np.array_equal(src, np.flatnonzero(r['keep'].reshape(-1)))
        assert np.array_equal(r['count'], r['keep'].reshape(n, -1).sum(1)) and r['count'].sum() == len(src)
        flat = lambda m: np.moveaxis(m, 2, -1).reshape(-1, 3)
        assert np.array_equal(r['xyz'], flat(r['point'])[src]) and np.array_equal(r['normal_packed'], flat(r['normal'])[src])
        assert np.array_equal(r['value'], a['value'].reshape(-1)[src])
    assert not _fuse(a, value=False)['value'].any()


@pytest.mark.parametrize('shape', SMALL, ids=FI.shape_id)
def test_holes(shape):
    n, tl, H, W = shape
    a = FI.make_input(shape, 'holes')
    r = _fuse(a)
    d = a['disp']
    hole = ~(np.isfinite(d) & (d > 0))
    for bad in (d == 0, np.isnan(d), np.isposinf(d), d == -1):
        assert bad.any() and (bad & hole).sum() == bad.sum()
    assert np.array_equal(r['valid'], ~hole)
    assert (r['views'][hole] == 0).all() and (r['seen'][hole] == 0).all() and not r['keep'][hole].any()
    assert not r['point'][np.broadcast_to(hole[:, :, None], r['point'].shape)].any()
    # a cell that touches a hole is not seen
    touched = 0
    for i in range(tl):
        for j in range(tl):
            if i == j:
                continue
            s = r['seen_ij'][:, i, j]
            x0 = np.minimum(np.floor(np.where(s, r['uj'][:, i, j], 0)).astype(int), W - 2)
            y0 = np.minimum(np.floor(np.where(s, r['vj'][:, i, j], 0)).astype(int), H - 2)
            k = np.arange(n)[:, None, None]
            cell_hole = hole[:, j][k, y0, x0] | hole[:, j][k, y0, x0 + 1] | hole[:, j][k, y0 + 1, x0] | hole[:, j][k, y0 + 1, x0 + 1]
            assert not (s & cell_hole).any()
            full = _fuse(FI.make_input(shape, 'plane'))['seen_ij'][:, i, j]
            touched += int((full & ~s & ~hole[:, i]).sum())
    assert touched > 0                                                          # holes did cost valid pixels their view
    # normals next to a hole are zero; elsewhere in the interior they are unit vectors
    pad = np.pad(hole, [(0, 0), (0, 0), (1, 1), (1, 1)], mode='constant', constant_values=True)
    near = hole | pad[:, :, 1:-1, :-2] | pad[:, :, 1:-1, 2:] | pad[:, :, :-2, 1:-1] | pad[:, :, 2:, 1:-1]
    ln = np.linalg.norm(r['normal'], axis=2)
    assert (ln[near] == 0).all() and np.allclose(ln[~near], 1.0, atol=1e-12) and (~near).any()


@pytest.mark.parametrize('kind', FI.INPUTS)
@pytest.mark.parametrize('shape', FI.SHAPES, ids=FI.shape_id)
def test_float32_and_float64_disagree_only_inside_the_exemption_and_that_stays_small(shape, kind):
    for pi in range(len(FI.PARAMS)):
        r32, r64, ex, ex_pairs = FI.refs(shape, kind, pi)
        share = ex_pairs.sum() / FI.pair_count(shape)
        print(f'params {pi}: exempt pairs {ex_pairs.sum()} of {FI.pair_count(shape)} ({100 * share:.4f} %), exempt pixels {ex.sum()}')
        assert share <= 0.01
        for k in ('views', 'seen', 'keep'):
            assert not ((r32[k] != r64[k]) & ~ex).any(), k
        assert not ((r32['seen_ij'] != r64['seen_ij']) & ~ex[:, :, None]).any()
        assert not ((r32['cons_ij'] != r64['cons_ij']) & ~ex[:, :, None]).any()
        if shape[2] * shape[3] > 4:
            assert r64['seen'].any()
            if not (kind == 'scaled' and FI.params(shape, pi)[1] == shape[1]):
                assert r64['keep'].any()


def test_default_motion_is_too_large_for_these_sizes():
    """why the inputs use motion = 0.1: at 19 x 37 synth's default jitter moves every pixel out of the other frame"""
    from depthinspace_amd import synth
    b = synth.make_batch(synth.make_settings(19, 37), 1, tl=2, seed=7, motion=1.0, with_primary=False, with_flow=False)
    r = fuse_ref.fuse(b['disp0'][:, :, 0], b['R'], b['t'], synth.make_settings(19, 37).K, synth.DEFAULT_BASELINE)
    assert not r['seen'].any()


def test_ply_round_trip(tmp_path):
    from depthinspace_amd.data import ply
    rng = np.random.RandomState(0)
    m = 257
    xyz, nrm = rng.normal(size=(m, 3)).astype(np.float32), rng.normal(size=(m, 3)).astype(np.float32)
    val, views = rng.uniform(size=m).astype(np.float32), rng.randint(0, 5, m).astype(np.uint8)
    path = tmp_path / 'cloud.ply'
    assert ply.write_ply(path, xyz, nrm, val, views, comments=('a test cloud',)) == m
    assert sorted(p.name for p in tmp_path.iterdir()) == ['cloud.ply']            # no temporary file is left
    raw = path.read_bytes()
    head = raw[:raw.index(b'end_header\n')].decode('ascii').split('\n')
    assert head[0] == 'ply' and head[1] == 'format binary_little_endian 1.0' and f'element vertex {m}' in head
    assert [h for h in head if h.startswith('property')] == ['property float x', 'property float y', 'property float z',
                                                             'property float nx', 'property float ny', 'property float nz',
                                                             'property float intensity', 'property uchar views']
    assert len(raw) == raw.index(b'end_header\n') + len(b'end_header\n') + m * 29
    rec, comments = ply.read_ply(path)
    assert comments == ['a test cloud'] and len(rec) == m
    assert np.array_equal(np.stack([rec['x'], rec['y'], rec['z']], 1), xyz)
    assert np.array_equal(np.stack([rec['nx'], rec['ny'], rec['nz']], 1), nrm)
    assert np.array_equal(rec['intensity'], val) and np.array_equal(rec['views'], views)
    # an empty cloud; positions alone
    assert ply.write_ply(path, np.zeros((0, 3), np.float32)) == 0
    rec, comments = ply.read_ply(path)
    assert len(rec) == 0 and comments == [] and rec.dtype.names == ply.VERTEX_DTYPE.names
    ply.write_ply(path, xyz[:3])
    rec, _ = ply.read_ply(path)
    assert np.array_equal(rec['x'], xyz[:3, 0]) and not rec['nx'].any() and not rec['views'].any()
    with pytest.raises(ValueError):
        ply.write_ply(path, xyz, nrm[:5])
    (tmp_path / 'bad.ply').write_bytes(b'ply\nformat ascii 1.0\nelement vertex 0\nend_header\n')
    with pytest.raises(ValueError):
        ply.read_ply(tmp_path / 'bad.ply')
