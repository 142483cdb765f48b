"""CPU: the tap and phase planner of the streaming convs (depthinspace_amd/csrc/conv_plan.h) against the definition of the four modes.

tests/conv_plan_driver.cpp instantiates the planner on a plain struct and prints every launch it plans; it is built here with
AddressSanitizer + UBSan and run as a program (nothing is loaded into Python).  A launch computes, per phase p and virtual pixel (vy, vx),
    out[vy * osy + ooy, vx * osx + oox] = sum_t in[vy * S + tdy[t], vx * S + tdx[t]] * W[tsrc[t] // k, tsrc[t] % k]
over the phase's taps (one phase: all taps, (osy, ooy, osx, oox) of the launch; four phases: taps [k0, k0 + kn), stride 2, offset
(ph_oy, ph_ox)), terms outside the input image dropped (zero padding) and pixels outside the output not stored.  Expanded into the
multiset of (oy, ox, iy, ix, ky, kx) contributions this must equal the definition (y, and the same in x):
    CONV        iy = oy * s + ky - pad                 TCONV_DGRAD  the same (input gradient of TCONV: its transpose)
    TCONV       oy = iy * s + ky - pad, cropped        CONV_DGRAD   the same (input gradient of CONV: its transpose)
and the kernels store, they do not accumulate: every output pixel belongs to exactly one (launch, phase).
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'depthinspace_amd', 'csrc')
CONV, CONV_DGRAD, TCONV, TCONV_DGRAD = 0, 1, 2, 3   # include/dis_hip.h DIS_CONVG_*
OK, BAD_SHAPE, UNSUPPORTED = 0, -1, -2
KS = (2, 3, 4, 5, 7)
SIZES = ((1, 1), (2, 3), (5, 6), (7, 4))


def _cases():
    """(mode, k, stride, pad, hin, win, hout, wout) as the entry points take them: hin / win the launch's input, hout / wout its output"""
    out = []
    for k in KS:
        for stride in (1, 2):
            for pad in range(0, k // 2 + 2):
                for h, w in SIZES:
                    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
                    if ho > 0 and wo > 0:   # a conv with an output
                        out.append((CONV, k, stride, pad, h, w, ho, wo))
                        out.append((CONV_DGRAD, k, stride, pad, ho, wo, h, w))
                    for th in range(max(2 * h - 2, 1), 2 * h + 1):      # transposed conv h x w -> th x tw (crop of 2h x 2w)
                        for tw in range(max(2 * w - 2, 1), 2 * w + 1):
                            out.append((TCONV, k, stride, pad, h, w, th, tw))
                            out.append((TCONV_DGRAD, k, stride, pad, th, tw, h, w))
    return out


REFUSED = [(m, 8, s, 1, 5, 6, 5, 6) for m in range(4) for s in (1, 2)] + [(m, 3, 3, 1, 5, 6, 2, 2) for m in range(4)] + \
          [(m, 3, 0, 1, 5, 6, 5, 6) for m in range(4)] + [(4, 3, 1, 1, 5, 6, 5, 6), (-1, 3, 1, 1, 5, 6, 5, 6)]


@pytest.fixture(scope='module')
def plans(tmp_path_factory):
    cxx = shutil.which('g++') or shutil.which(os.path.join(os.environ.get('LLVM_BIN', '/opt/rocm/lib/llvm/bin'), 'clang++'))
    if cxx is None:
        pytest.skip('no host C++ compiler')
    tmp = tmp_path_factory.mktemp('conv_plan')
    exe = str(tmp / 'conv_plan_driver')
    r = subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Werror', '-fsanitize=address,undefined',
                        '-fno-sanitize-recover=undefined', '-fno-omit-frame-pointer', f'-I{CSRC}', '-o', exe,
                        os.path.join(ROOT, 'tests', 'conv_plan_driver.cpp')], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    cases = _cases() + REFUSED
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:abort_on_error=0:exitcode=23', UBSAN_OPTIONS='print_stacktrace=1:halt_on_error=1')
    r = subprocess.run([exe], input=''.join(' '.join(map(str, c)) + '\n' for c in cases), capture_output=True, text=True, env=env,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr, r.stderr[-3000:]
    got = {}
    case = form = launch = None
    for line in r.stdout.splitlines():
        tag, *v = line.split()
        v = [int(x) for x in v] if tag != 'FORM' else v
        if tag == 'CASE':
            case = got[tuple(v)] = {}
        elif tag == 'FORM':
            form = case[v[0]] = {'launches': [], 'rc': None}
        elif tag == 'L':
            launch = dict(zip(('slice', 'halo_only', 'hv', 'wv', 'S', 'osy', 'ooy', 'osx', 'oox', 'nph', 'ntaps', 's_ci', 's_co'), v))
            launch['phases'], launch['taps'] = [], []
            form['launches'].append(launch)
        elif tag == 'P':
            launch['phases'].append(tuple(v))
        elif tag == 'T':
            launch['taps'].append(tuple(v))
        elif tag == 'RC':
            form['rc'] = v[0]
        elif tag == 'NEED':
            case['need'] = v[0]
    assert len(got) == len(set(cases))
    return got


def _key(oy, ox, iy, ix, kidx):
    return (((oy.astype(np.int64) * 64 + ox) * 64 + iy) * 64 + ix) * 64 + kidx   # (all extents and k * k are below 64)


def _definition(mode, k, stride, pad, hin, win, hout, wout):
    """sorted keys of the contributions in[iy, ix] * W[ky, kx] -> out[oy, ox] of the mode"""
    gather = mode in (CONV, TCONV_DGRAD)   # in = out * s + k - pad; else out = in * s + k - pad
    (ha, wa), (hb, wb) = ((hout, wout), (hin, win)) if gather else ((hin, win), (hout, wout))
    ay, ax, ky, kx = np.meshgrid(np.arange(ha), np.arange(wa), np.arange(k), np.arange(k), indexing='ij')
    by, bx = ay * stride + ky - pad, ax * stride + kx - pad
    m = (by >= 0) & (by < hb) & (bx >= 0) & (bx < wb)
    ay, ax, by, bx, kidx = ay[m], ax[m], by[m], bx[m], (ky * k + kx)[m]
    return np.sort(_key(ay, ax, by, bx, kidx) if gather else _key(by, bx, ay, ax, kidx))


def _expand(launches, k, hin, win, hout, wout):
    """-> (sorted keys of the contributions of the planned launches, how often each output pixel is stored)"""
    keys, stores = [np.zeros(0, np.int64)], np.zeros((hout, wout), np.int64)
    for L in launches:
        taps = np.array(L['taps'], np.int64).reshape(-1, 3)
        assert len(taps) == L['ntaps'] and L['nph'] in (1, 4) and len(L['phases']) == (4 if L['nph'] == 4 else 0)
        assert ((taps[:, 2] >= 0) & (taps[:, 2] < k * k)).all()
        phases = [(0, L['ntaps'], L['ooy'], L['oox'])] if L['nph'] == 1 else L['phases']
        if L['nph'] == 4:
            assert (L['osy'], L['osx'], L['S']) == (2, 2, 1)
            # the phases tile the tap list in order, none of them empty
            assert [p[0] for p in phases] == list(np.cumsum([0] + [p[1] for p in phases[:-1]])) and sum(p[1] for p in phases) == L['ntaps']
            assert all(p[1] > 0 for p in phases)
        for k0, kn, oy0, ox0 in phases:
            vy, vx = np.meshgrid(np.arange(L['hv']), np.arange(L['wv']), indexing='ij')
            oy, ox = vy * L['osy'] + oy0, vx * L['osx'] + ox0
            m = (oy < hout) & (ox < wout)
            vy, vx, oy, ox = vy[m], vx[m], oy[m], ox[m]
            np.add.at(stores, (oy, ox), 1)
            t = taps[k0:k0 + kn]
            iy, ix = vy[:, None] * L['S'] + t[None, :, 0], vx[:, None] * L['S'] + t[None, :, 1]
            m = (iy >= 0) & (iy < hin) & (ix >= 0) & (ix < win)
            oy, ox, kidx = (np.broadcast_to(v, m.shape) for v in (oy[:, None], ox[:, None], t[None, :, 2]))
            keys.append(_key(oy[m], ox[m], iy[m], ix[m], kidx[m]))
    return np.sort(np.concatenate(keys)), stores


def test_plans_match_the_definition(plans):
    nfused = 0
    for case in _cases():
        mode, k, stride, pad, hin, win, hout, wout = case
        got = plans[case]
        if mode == TCONV_DGRAD and stride != 2:   # (the entry points take the stride-2 transposed conv only)
            assert all(got[f]['rc'] == UNSUPPORTED and not got[f]['launches'] for f in ('fused', 'split', 'fallback')), case
            continue
        want = _definition(*case)
        phased = mode in (CONV_DGRAD, TCONV) and stride == 2
        for form in ('fused', 'split'):
            plan = got[form]
            assert plan['rc'] == OK, (case, form)
            keys, stores = _expand(plan['launches'], k, hin, win, hout, wout)
            assert np.array_equal(keys, want), (case, form)
            assert (stores == 1).all(), (case, form, stores)
            for L in plan['launches']:
                direct = mode in (CONV, TCONV_DGRAD)   # weight strides: w[co][ci] rows of cin_w = 3, or w[ci][co] rows of cout_w = 5
                assert (L['s_ci'], L['s_co']) == ((k * k, 3 * k * k) if direct else (5 * k * k, k * k)), (case, form)
        fused, split = got['fused']['launches'], got['split']['launches']
        if phased:   # one halo launch of four non-empty phases (checked in _expand), or one launch per class with its own slice
            assert len(fused) == 1 and fused[0]['nph'] == 4 and fused[0]['halo_only'] == 1 and fused[0]['slice'] == 0, case
            assert all(L['nph'] == 1 and not L['halo_only'] and L['slice'] == 2 * L['ooy'] + L['oox'] for L in split), case
            assert len({L['slice'] for L in split}) == len(split), case
            nfused += 1
        else:
            assert fused == split and len(split) == 1 and split[0]['nph'] == 1 and not split[0]['halo_only'], case
        # a refused fused launch falls back to exactly the per-class launches
        assert got['fallback']['rc'] == OK and got['fallback']['launches'] == (fused + split if phased else split), case
        assert got['need'] == len(split), case
    assert nfused > 500


def test_unsupported_shapes_are_refused_by_status(plans):
    """k * k > 49 taps, strides other than 1 / 2 and unknown modes: a status code and no launch (the fixture has checked that the
    sanitizers stayed silent)"""
    for case in REFUSED:
        for form in ('fused', 'split', 'fallback'):
            assert plans[case][form]['rc'] == UNSUPPORTED and not plans[case][form]['launches'], (case, form)
