"""Point clouds as binary little-endian PLY files: per vertex float x y z nx ny nz, float intensity and uchar views - what
data/fuse.py writes.  Written against the PLY format itself (an ASCII header that names the elements and their properties in order,
closed by `end_header`, then the records back to back); the reader understands the files of the writer and any other binary
little-endian file whose single element is `vertex` with scalar properties.  write_mesh / read_mesh: the same vertex element followed
by `element face M` with `property list uchar int vertex_indices`, every face a triangle - what data/mesh.py writes."""
import os

import numpy as np

VERTEX_DTYPE = np.dtype([('x', '<f4'), ('y', '<f4'), ('z', '<f4'), ('nx', '<f4'), ('ny', '<f4'), ('nz', '<f4'), ('intensity', '<f4'),
                         ('views', 'u1')])
_PLY_TYPES = {'float': '<f4', 'float32': '<f4', 'double': '<f8', 'float64': '<f8', 'uchar': 'u1', 'uint8': 'u1', 'char': 'i1', 'int8': 'i1',
              'ushort': '<u2', 'uint16': '<u2', 'short': '<i2', 'int16': '<i2', 'uint': '<u4', 'uint32': '<u4', 'int': '<i4', 'int32': '<i4'}
_PLY_NAMES = {'<f4': 'float', 'u1': 'uchar', '|u1': 'uchar'}


def vertex_records(xyz, normal=None, intensity=None, views=None):
    """(m, 3) positions and the optional (m, 3) normals, (m) intensities and (m) view counts -> a VERTEX_DTYPE array (absent: zeros)"""
    xyz = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
    rec = np.zeros(len(xyz), dtype=VERTEX_DTYPE)
    rec['x'], rec['y'], rec['z'] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    if normal is not None:
        nrm = np.asarray(normal, dtype=np.float32).reshape(-1, 3)
        if len(nrm) != len(xyz):
            raise ValueError('as many normals as points are expected')
        rec['nx'], rec['ny'], rec['nz'] = nrm[:, 0], nrm[:, 1], nrm[:, 2]
    for key, arr in (('intensity', intensity), ('views', views)):
        if arr is not None:
            arr = np.asarray(arr).reshape(-1)
            if len(arr) != len(xyz):
                raise ValueError(f'as many {key} values as points are expected')
            rec[key] = arr
    return rec


def write_ply(path, xyz, normal=None, intensity=None, views=None, comments=()):
    """Writes the cloud to `path` through a temporary file beside it (the file appears whole or not at all).  Returns the number of
    vertices."""
    rec = vertex_records(xyz, normal, intensity, views)
    head = ['ply', 'format binary_little_endian 1.0']
    for c in comments:
        if '\n' in str(c):
            raise ValueError('a comment is one line')
        head.append(f'comment {c}')
    head.append(f'element vertex {len(rec)}')
    head += [f'property {_PLY_NAMES[VERTEX_DTYPE[name].str]} {name}' for name in VERTEX_DTYPE.names]
    head.append('end_header')
    tmp = str(path) + '.tmp'
    try:
        with open(tmp, 'wb') as fp:
            fp.write(('\n'.join(head) + '\n').encode('ascii'))
            fp.write(rec.tobytes())
        os.replace(tmp, str(path))
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    return len(rec)


def read_ply(path):
    """-> (structured array with one field per vertex property, list of the comment lines).  Binary little-endian files with the
    single element `vertex` and scalar properties; anything else raises ValueError."""
    with open(str(path), 'rb') as fp:
        data = fp.read()
    end = data.find(b'end_header\n')
    if not data.startswith(b'ply\n') or end < 0:
        raise ValueError(f'{path}: not a PLY file')
    lines = data[:end].decode('ascii').split('\n')[1:]
    body = data[end + len(b'end_header\n'):]
    count, fields, comments, fmt = None, [], [], None
    for line in lines:
        tok = line.split()
        if not tok:
            continue
        if tok[0] == 'format':
            fmt = tok[1:]
        elif tok[0] == 'comment':
            comments.append(line[len('comment '):])
        elif tok[0] == 'element':
            if tok[1] != 'vertex' or count is not None:
                raise ValueError(f'{path}: only a single `vertex` element is understood')
            count = int(tok[2])
        elif tok[0] == 'property':
            if len(tok) != 3 or tok[1] not in _PLY_TYPES:
                raise ValueError(f'{path}: unsupported property `{line}`')
            fields.append((tok[2], _PLY_TYPES[tok[1]]))
        else:
            raise ValueError(f'{path}: unsupported header line `{line}`')
    if fmt != ['binary_little_endian', '1.0'] or count is None:
        raise ValueError(f'{path}: a binary_little_endian 1.0 file with a vertex element is expected')
    dt = np.dtype(fields)
    if len(body) != count * dt.itemsize:
        raise ValueError(f'{path}: {len(body)} bytes of data for {count} vertices of {dt.itemsize} bytes')
    return np.frombuffer(body, dtype=dt, count=count).copy(), comments


FACE_DTYPE = np.dtype([('n', 'u1'), ('v', '<i4', (3,))])     # a triangle of `property list uchar int vertex_indices`: 13 bytes


def write_mesh(path, xyz, normal, intensity, views, faces, comments=()):
    """Writes the triangle mesh to `path` through a temporary file beside it (the file appears whole or not at all): the vertex element
    of write_ply, then the faces (m, 3) as lists of three int indices.  A face index outside 0 .. vertices - 1 raises ValueError.
    Returns (vertices, faces)."""
    rec = vertex_records(xyz, normal, intensity, views)
    faces = np.asarray(faces)
    if faces.size and not np.issubdtype(faces.dtype, np.integer):
        raise ValueError('integer face indices are expected')
    faces = faces.astype(np.int64).reshape(-1, 3)
    if faces.size and (faces.min() < 0 or faces.max() >= len(rec)):
        raise ValueError(f'a face names a vertex outside 0 .. {len(rec) - 1}')
    frec = np.zeros(len(faces), dtype=FACE_DTYPE)
    frec['n'] = 3
    frec['v'] = faces
    head = ['ply', 'format binary_little_endian 1.0']
    for c in comments:
        if '\n' in str(c):
            raise ValueError('a comment is one line')
        head.append(f'comment {c}')
    head.append(f'element vertex {len(rec)}')
    head += [f'property {_PLY_NAMES[VERTEX_DTYPE[name].str]} {name}' for name in VERTEX_DTYPE.names]
    head += [f'element face {len(frec)}', 'property list uchar int vertex_indices', 'end_header']
    tmp = str(path) + '.tmp'
    try:
        with open(tmp, 'wb') as fp:
            fp.write(('\n'.join(head) + '\n').encode('ascii'))
            fp.write(rec.tobytes())
            fp.write(frec.tobytes())
        os.replace(tmp, str(path))
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    return len(rec), len(frec)


def read_mesh(path):
    """-> (structured array with one field per vertex property, faces (m, 3) int32, list of the comment lines).  Binary little-endian
    files with a `vertex` element of scalar properties followed by a `face` element whose single property is a list of uchar counts
    and int (or uint) indices, every face a triangle; anything else raises ValueError."""
    with open(str(path), 'rb') as fp:
        data = fp.read()
    end = data.find(b'end_header\n')
    if not data.startswith(b'ply\n') or end < 0:
        raise ValueError(f'{path}: not a PLY file')
    lines = data[:end].decode('ascii').split('\n')[1:]
    body = data[end + len(b'end_header\n'):]
    counts, fields, comments, fmt, element, face_prop = {}, [], [], None, None, None
    for line in lines:
        tok = line.split()
        if not tok:
            continue
        if tok[0] == 'format':
            fmt = tok[1:]
        elif tok[0] == 'comment':
            comments.append(line[len('comment '):])
        elif tok[0] == 'element':
            element = tok[1]
            if element not in ('vertex', 'face') or element in counts or (element == 'face' and 'vertex' not in counts):
                raise ValueError(f'{path}: a `vertex` element followed by a `face` element is expected')
            counts[element] = int(tok[2])
        elif tok[0] == 'property' and element == 'vertex':
            if len(tok) != 3 or tok[1] not in _PLY_TYPES:
                raise ValueError(f'{path}: unsupported property `{line}`')
            fields.append((tok[2], _PLY_TYPES[tok[1]]))
        elif tok[0] == 'property' and element == 'face':
            if face_prop is not None or len(tok) != 5 or tok[1] != 'list' or tok[2] not in ('uchar', 'uint8') or tok[3] not in (
                    'int', 'int32', 'uint', 'uint32'):
                raise ValueError(f'{path}: unsupported property `{line}`')
            face_prop = tok[4]
        else:
            raise ValueError(f'{path}: unsupported header line `{line}`')
    if fmt != ['binary_little_endian', '1.0'] or 'vertex' not in counts or 'face' not in counts or face_prop is None:
        raise ValueError(f'{path}: a binary_little_endian 1.0 file with a vertex and a face element is expected')
    dt = np.dtype(fields)
    nv, nf = counts['vertex'], counts['face']
    if len(body) != nv * dt.itemsize + nf * FACE_DTYPE.itemsize:
        raise ValueError(f'{path}: {len(body)} bytes of data for {nv} vertices of {dt.itemsize} bytes and {nf} triangles')
    rec = np.frombuffer(body, dtype=dt, count=nv).copy()
    frec = np.frombuffer(body, dtype=FACE_DTYPE, count=nf, offset=nv * dt.itemsize)
    if nf and not (frec['n'] == 3).all():
        raise ValueError(f'{path}: every face is expected to be a triangle')
    faces = frec['v'].astype(np.int32).reshape(-1, 3)
    if nf and (faces.min() < 0 or faces.max() >= nv):
        raise ValueError(f'{path}: a face names a vertex outside 0 .. {nv - 1}')
    return rec, faces, comments
