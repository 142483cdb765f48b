"""CPU: the numpy restatement of the volumetric fusion (tests/tsdf_ref.py) held to what the GPU tests lean on - the exemption stays a
small share of the (lattice point, frame) pairs and covers every decision the two dtypes take differently - and to the properties of
the mesh it extracts: consistently oriented, normals towards the cameras, vertices on the depth maps.  Plus the PLY mesh writer and
reader (data/ply.py)."""
import os

import numpy as np
import pytest

from tests import tsdf_inputs as TI
from tests import tsdf_ref

SHAPES = list(TI.SHAPES)


@pytest.mark.parametrize('kind', TI.KINDS)
@pytest.mark.parametrize('shape', SHAPES, ids=TI.shape_id)
def test_the_exemption_is_small_and_covers_the_differences(shape, kind):
    for grid in TI.GRIDS:
        r32, r64, ex, ex_pairs = TI.refs(shape, kind, grid)
        share = ex_pairs.sum() / ex_pairs.size
        differ = (r32['use'] != r64['use']) | (r32['inimg'] & r64['inimg'] & ((r32['pu'] != r64['pu']) | (r32['pv'] != r64['pv'])))
        print(f'grid {grid}: exempt pairs {100 * share:.4f} %, pairs the dtypes take differently {100 * differ.mean():.5f} %, observed '
              f'{100 * (r64["weight"] > 0).mean():.1f} %, behind the surface {100 * (r64["tsdf"] < 0).mean():.1f} %')
        assert share <= 0.001
        assert not (differ & ~ex_pairs).any()
        m = ~ex
        assert np.array_equal(r32['weight'][m], r64['weight'][m])
        assert np.array_equal(r32['tsdf'][m] < 0, r64['tsdf'][m] < 0)
        for k in ('tsdf', 'vvalue'):
            assert np.abs(r32[k].astype(np.float64) - r64[k])[m].max() <= tsdf_ref.tolerance(r32[k][m], r64[k][m])
        assert r64['tsdf'].max() <= 1.0 and r64['tsdf'].min() >= -1.0 and np.all(r64['tsdf'][r64['weight'] == 0] == 1.0)
        if grid != (2, 2, 2):
            assert (r64['weight'] > 0).any() and (r64['weight'] == 0).any() and (r64['tsdf'] < 0).any()


def _extractions(shape, kind, grid):
    r32 = TI.refs(shape, kind, grid)[0]
    origin, voxel, _ = TI.volume(shape, kind, grid)
    return [tsdf_ref.extract(r32['tsdf'], r32['weight'], r32['vvalue'], origin, voxel, 1, dtype=dt) for dt in (np.float32, np.float64)]


@pytest.mark.parametrize('kind', ['plane', 'bumps'])
@pytest.mark.parametrize('shape', SHAPES, ids=TI.shape_id)
def test_the_extracted_mesh_is_oriented_and_lies_on_the_depth_maps(shape, kind):
    a = TI.make_input(shape, kind)
    tl, H, W = shape
    K = a['K'].astype(np.float64)
    fb = K[0, 0] * float(a['baseline'])
    for grid in TI.GRIDS[2:]:
        e32, e64 = _extractions(shape, kind, grid)
        origin, voxel, _ = TI.volume(shape, kind, grid)
        # float32 and float64 give the same topology
        for k in ('vid', 'cell', 'faces', 'views', 'count'):
            assert np.array_equal(e32[k], e64[k]), k
        faces, xyz, nrm = e64['faces'].astype(np.int64), e64['xyz'], e64['normal']
        assert len(faces) > 100 and len(faces) % 2 == 0 and faces.min() >= 0 and faces.max() < len(xyz)
        assert np.all(np.diff(e64['cell']) > 0)
        # no directed edge occurs twice
        de = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
        assert len(np.unique(de[:, 0] * len(xyz) + de[:, 1])) == len(de)
        # every triangle's normal has a positive dot product with the mean of its vertices' normals
        tn = np.cross(xyz[faces[:, 1]] - xyz[faces[:, 0]], xyz[faces[:, 2]] - xyz[faces[:, 0]])
        dots = (tn * nrm[faces].mean(1)).sum(1)
        assert (dots > 0).all()
        assert np.allclose(np.linalg.norm(nrm, axis=1), 1.0, atol=1e-9)
        # ... and the normals point towards the cameras
        worst, seen = 0.0, 0
        for f in range(tl):
            R, t = a['R'][f].astype(np.float64), a['t'][f].astype(np.float64)
            Xc = xyz @ R.T + t
            z = Xc[:, 2]
            u = np.floor(K[0, 0] * Xc[:, 0] / z + K[0, 2] + 0.5)
            v = np.floor(K[1, 1] * Xc[:, 1] / z + K[1, 2] + 0.5)
            ok = (z > 0) & (u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1)
            d = a['disp'][f][np.where(ok, v, 0).astype(np.int64), np.where(ok, u, 0).astype(np.int64)].astype(np.float64)
            ok &= np.isfinite(d) & (d > 0)
            assert ((nrm @ R.T)[ok] * Xc[ok]).sum(1).max() < 0          # n . (X - camera centre) < 0
            # every vertex lies within 1 voxel in depth of the depth map of every frame it projects into
            worst = max(worst, float(np.abs(fb / d[ok] - z[ok]).max()) / voxel)
            seen += int(ok.sum())
        print(f'grid {grid}: {len(xyz)} vertices, {len(faces)} triangles, the worst depth distance {worst:.3f} voxel over {seen} projections')
        assert seen >= len(xyz) and worst <= 1.0


def test_a_single_cell_and_an_unobserved_volume_give_empty_meshes():
    for kind in ('plane', 'holes'):
        r32 = TI.refs(SHAPES[1], kind, (2, 2, 2))[0]
        origin, voxel, _ = TI.volume(SHAPES[1], kind, (2, 2, 2))
        e = tsdf_ref.extract(r32['tsdf'], r32['weight'], r32['vvalue'], origin, voxel, 1)
        assert e['faces'].shape == (0, 3) and e['count'][1] == 0 and e['vid'].shape == (1, 1, 1) and e['count'][0] == len(e['xyz']) <= 1
    a = TI.make_input(SHAPES[0], 'plane')
    r = tsdf_ref.integrate(a['disp'], a['R'], a['t'], a['K'], a['baseline'], a['value'], (50.0, 50.0, -50.0), 0.1, 0.3, (9, 8, 7))
    assert not r['weight'].any() and np.all(r['tsdf'] == 1.0) and not r['vvalue'].any()
    e = tsdf_ref.extract(r['tsdf'], r['weight'], r['vvalue'], (50.0, 50.0, -50.0), 0.1, 1)
    assert e['xyz'].shape == (0, 3) and e['faces'].shape == (0, 3) and list(e['count']) == [0, 0] and np.all(e['vid'] == -1)
    # a volume with signs but no weight: nothing is active either
    t = np.where(np.arange(7)[:, None, None] < 3, np.float32(-0.5), np.float32(0.5)) * np.ones((7, 8, 9), np.float32)
    e = tsdf_ref.extract(t, np.zeros((7, 8, 9), np.uint8), np.zeros((7, 8, 9), np.float32), (0, 0, 0), 0.1, 1)
    assert list(e['count']) == [0, 0]
    e = tsdf_ref.extract(t, np.ones((7, 8, 9), np.uint8), np.zeros((7, 8, 9), np.float32), (0, 0, 0), 0.1, 1)
    assert list(e['count']) == [8 * 7, 2 * 7 * 6] and np.allclose(e['xyz'][:, 2], 0.25) and np.allclose(e['normal'], [0, 0, 1])


def test_ply_mesh_round_trip(tmp_path):
    from depthinspace_amd.data import ply
    rs = np.random.RandomState(0)
    m = 11
    xyz, nrm = rs.normal(size=(m, 3)).astype(np.float32), rs.normal(size=(m, 3)).astype(np.float32)
    inten, views = rs.uniform(size=m).astype(np.float32), rs.randint(0, 5, m).astype(np.uint8)
    faces = rs.randint(0, m, (7, 3)).astype(np.int32)
    path = tmp_path / 'mesh.ply'
    assert ply.write_mesh(path, xyz, nrm, inten, views, faces, comments=('a mesh', 'second line')) == (m, 7)
    raw = path.read_bytes()
    head = raw[:raw.index(b'end_header\n')].decode('ascii').split('\n')
    assert head == ['ply', 'format binary_little_endian 1.0', 'comment a mesh', 'comment second line', f'element vertex {m}',
                    'property float x', 'property float y', 'property float z', 'property float nx', 'property float ny', 'property float nz',
                    'property float intensity', 'property uchar views', 'element face 7', 'property list uchar int vertex_indices', '']
    assert len(raw) == raw.index(b'end_header\n') + 11 + m * ply.VERTEX_DTYPE.itemsize + 7 * 13
    rec, f2, comments = ply.read_mesh(path)
    assert rec.dtype == ply.VERTEX_DTYPE and comments == ['a mesh', 'second line']
    assert np.array_equal(f2, faces) and f2.dtype == np.int32
    assert np.array_equal(np.stack([rec['x'], rec['y'], rec['z']], 1), xyz) and np.array_equal(np.stack([rec['nx'], rec['ny'], rec['nz']], 1), nrm)
    assert np.array_equal(rec['intensity'], inten) and np.array_equal(rec['views'], views)
    assert os.listdir(tmp_path) == ['mesh.ply']                         # no temporary file is left behind
    # an empty mesh round-trips too
    assert ply.write_mesh(tmp_path / 'empty.ply', np.zeros((0, 3)), None, None, None, np.zeros((0, 3), np.int32)) == (0, 0)
    rec0, f0, _ = ply.read_mesh(tmp_path / 'empty.ply')
    assert len(rec0) == 0 and f0.shape == (0, 3)
    # a face index >= the vertex count is refused, and nothing is left behind
    for bad in ([[0, 1, m]], [[-1, 0, 1]]):
        with pytest.raises(ValueError):
            ply.write_mesh(tmp_path / 'bad.ply', xyz, nrm, inten, views, np.array(bad, np.int32))
    with pytest.raises(ValueError):
        ply.write_mesh(tmp_path / 'bad.ply', xyz, nrm, inten, views, faces, comments=('two\nlines',))
    assert sorted(os.listdir(tmp_path)) == ['empty.ply', 'mesh.ply']
    # read_ply on a vertex-only file behaves as before; on a mesh it still refuses, and read_mesh wants the face element
    ply.write_ply(tmp_path / 'cloud.ply', xyz, nrm, inten, views, comments=('a cloud',))
    rec1, c1 = ply.read_ply(tmp_path / 'cloud.ply')
    assert rec1.dtype == ply.VERTEX_DTYPE and c1 == ['a cloud'] and np.array_equal(rec1, rec)
    with pytest.raises(ValueError):
        ply.read_ply(path)
    with pytest.raises(ValueError):
        ply.read_mesh(tmp_path / 'cloud.ply')
    with open(path, 'rb') as fp:
        cut = fp.read()[:-5]
    (tmp_path / 'short.ply').write_bytes(cut)
    with pytest.raises(ValueError):
        ply.read_mesh(tmp_path / 'short.ply')
