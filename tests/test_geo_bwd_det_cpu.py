"""CPU: the host side of the order-free flow-consistency backward - workspace query, argument checks (all before any launch), the
DIS_GEO_BWD / ops.set_geo_bwd_det / --geo_bwd switches.  The kernels are tested in tests/test_geo_bwd_det_gpu.py."""
import ctypes
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    import __graft_entry__ as g
    from depthinspace_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        g.build()
    return lib


def test_workspace_query():
    q = _lib().fn('dis_geo_loss_bwd_det_workspace')
    assert q.restype is ctypes.c_long
    for bad in ((0, 4, 512, 432), (17, 4, 512, 432), (-1, 4, 512, 432), (12, 0, 512, 432), (12, 4, 0, 432), (12, 4, 512, -3)):
        assert q(*bad) == -1, bad
    # 8 bytes of integer cell and 4 of depth0 addend per term and pixel
    assert q(1, 1, 2, 2) == 48 and q(16, 3, 33, 41) == 16 * 3 * 33 * 41 * 12
    assert q(12, 4, 512, 432) == 127401984
    assert q(16, 1 << 10, 1 << 10, 1 << 10) == 16 * 12 * (1 << 30)   # long arithmetic: past 2^31


def test_entry_points_refuse_before_launching():
    lib = _lib()
    from depthinspace_amd import ops
    buf = (ctypes.c_double * 512)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    single, multi = lib.fn('dis_geo_loss_bwd_det'), lib.fn('dis_geo_loss_bwd_multi_det')
    ptrs = [p] * 9
    assert single(*ptrs, -1.0, p, p, p, p, p, 1, 8, 8, None, None) == -3          # no workspace: DIS_ERR_NULL
    assert single(*ptrs, -1.0, p, p, p, None, p, 1, 8, 8, p, None) == -3
    assert single(*ptrs, -1.0, p, p, p, p, p, 0, 8, 8, p, None) == -1             # DIS_ERR_BAD_SHAPE
    assert single(*ptrs, -1.0, p, p, p, p, p, 1, 1, 8, p, None) == -1
    assert single(*ptrs, -1.0, p, p, p, p, p, 1, 8, 8, ctypes.c_void_p(p.value + 4), None) == -1   # workspace not 8-byte aligned
    tab = (ops._GeoTerm * 17)()
    t = ctypes.cast(tab, ctypes.c_void_p)
    assert multi(t, 17, p, p, -1.0, p, p, 1, 8, 8, p, None) == -2                 # DIS_ERR_UNSUPPORTED
    assert multi(t, 0, p, p, -1.0, p, p, 1, 8, 8, p, None) == -1
    assert multi(t, 2, p, p, -1.0, p, p, 1, 8, 8, None, None) == -3
    assert multi(None, 2, p, p, -1.0, p, p, 1, 8, 8, p, None) == -3
    assert multi(t, 2, p, p, -1.0, p, p, 1, 8, 8, p, None) == -3                  # a term with NULL pointers


def test_switches():
    _lib()
    from depthinspace_amd import ops
    from depthinspace_amd.co.args import parse_args
    prev = ops.set_geo_bwd_det(True)
    try:
        assert ops.GEO_BWD_DET is True and ops.set_geo_bwd_det(False) is True and ops.GEO_BWD_DET is False
    finally:
        ops.set_geo_bwd_det(prev)
    assert parse_args([]).geo_bwd is None
    assert parse_args(['--geo_bwd', 'det']).geo_bwd == 'det' and parse_args(['--geo_bwd', 'atomic']).geo_bwd == 'atomic'
    with pytest.raises(SystemExit):
        parse_args(['--geo_bwd', 'other'])


def test_environment_variable_selects_the_mode():
    """DIS_GEO_BWD is read when ops is imported: a fresh interpreter per value"""
    _lib()
    code = 'from depthinspace_amd import ops; print(ops.GEO_BWD_DET)'
    for val, want in ((None, 'False'), ('det', 'True')):
        env = {k: v for k, v in os.environ.items() if k != 'DIS_GEO_BWD'}
        if val is not None:
            env['DIS_GEO_BWD'] = val
        r = subprocess.run([sys.executable, '-c', code], cwd=ROOT, env=env, capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == want, (val, r.stdout, r.stderr[-500:])
