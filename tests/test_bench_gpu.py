"""GPU: bench.py itself, as the driver runs it - the single-GPU line's roofline object and the 2-rank path (`--backend gloo`: both
ranks on the one GPU of the box, the same code path as RCCL minus the transport), so that the first multi-GPU run of the driver
cannot fail on plumbing.  Child processes (fresh interpreters), small step counts."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, timeout=900):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + args, capture_output=True, text=True, timeout=timeout,
                       env=env, cwd=ROOT)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    lines = [ln for ln in r.stdout.strip().splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_line_times_the_steps_and_dumps_the_same_last_step_every_run(tmp_path):
    """A plain run reports the timed steps only (every --full field null); --dump-outputs writes what the last timed step gives
    its caller - loss terms (= the line's), disparity and updated parameters, DIS-MF whole - and, every step training from the
    same seeded state, two runs write the same outputs: the tolerances of tests/test_determinism_gpu.py for one step (the
    forward and the losses repeat bit for bit in practice, an Adam update moves a parameter by ~1e-4, run-to-run noise ~4e-8)."""
    import numpy as np
    outs = []
    for r in ('a', 'b'):
        d = _run(['--steps', '3', '--warmup', '1', '--dump-outputs', str(tmp_path / r)])
        assert d['steps'] == 3 and d['ms_per_step'] > 0 and d['full'] is False
        assert abs(d['value'] - 4 * 4 * 1e3 / d['ms_per_step']) < 1e-6 * d['value']
        for k in ('roofline', 'roofline_hbm_kernels', 'cpu_baseline', 'disp_l1_vs_ref', 'strict_fp32_frames_per_s', 'extra_dis_sf',
                  'eager_launch_frames_per_s', 'kernel_ms_one_eager_step'):
            assert d[k] is None, k
        assert d['adam_steps_taken'] == 4
        out = {f[:-4]: np.load(str(tmp_path / r / f)) for f in os.listdir(str(tmp_path / r))}
        assert sorted(out) == ['disparity', 'loss_terms', 'parameters']
        assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in out.values())
        assert np.array_equal(out['loss_terms'], np.asarray(d['loss_terms'], np.float32))
        assert out['parameters'].shape == (508993,) and out['disparity'].shape == (4 * 4 * 512 * 432,)
        outs.append(out)
    a, b = outs
    assert np.abs(a['disparity'] - b['disparity']).max() < 1e-5
    np.testing.assert_allclose(a['loss_terms'], b['loss_terms'], rtol=1e-6, atol=0)
    assert np.abs(a['parameters'] - b['parameters']).max() < 1e-6


def test_single_gpu_line_roofline_covers_the_whole_kernel_family():
    d = _run(['--steps', '3', '--warmup', '1', '--full', '--no-cpu-baseline', '--no-extra-legs'])
    assert d['n_gpus'] == 1 and d['config']['hip_graph'] is True and d['step_mode'] == 'graph'
    r = d['roofline']
    # the two kernel families of the 3x3 32 -> 32 layers: conv_f16x2_kernel (forward, GroupNorm-on-load forward, the input gradients that
    # keep a launch of their own) and - round 6 - conv_bwd_fused_kernel (input + weight gradient in one launch); the one with the larger
    # share of the step is `roofline`, the other `roofline.other_family`; together they are the round-5 line's 76 launches
    o = r['other_family']
    assert o is not None and ('conv_bwd_fused' in r['kernel']) != ('conv_bwd_fused' in o['kernel'])
    assert r['launches_per_step'] + o['launches_per_step'] == 76, (r['launches_by_entry_point'], o['launches_by_entry_point'])
    assert sum(r['launches_by_entry_point'].values()) == r['launches_per_step']
    fused = r if 'conv_bwd_fused' in r['kernel'] else o
    assert any(k.startswith('dis_conv2d_bwd_fused_f16x2') for k in fused['launches_by_entry_point'])
    assert 0.05 < o['frac_hbm'] < 1.0 and 0.02 < o['frac_mfma'] < 1.0
    assert r['bound'] in ('hbm', 'mfma') and r['unit'] == ('GB/s' if r['bound'] == 'hbm' else 'TFLOP/s')
    assert abs(r['frac'] - max(r['frac_mfma'], r['frac_hbm'])) < 1e-12
    assert abs(r['frac'] - r['achieved'] / r['peak']) < 1e-9
    assert 0.05 < r['frac_mfma'] < 1.0 and 0.05 < r['frac_hbm'] < 1.0
    assert r['flop_per_algorithmic_byte'] < 2 * 72.0 + 1e-6   # (72 flop/B for one product of a plain conv; the fused launch does two per byte set)
    st = r['step_traffic']
    assert st is None or (st['ratio'] > 1.0 and st['algorithmic_bytes_per_step'] > 8e10)
    # labels say which kernel served an entry point
    assert any('conv_f16x2_kernel' in k or 'conv_bwd_fused_kernel' in k for k in d['kernel_ms_one_eager_step'])


def test_two_ranks_gloo_bench_runs_and_replicas_agree():
    d = _run(['--gpus', '2', '--backend', 'gloo', '--steps', '2', '--warmup', '1', '--full', '--no-cpu-baseline'])
    assert d['n_gpus'] == 2 and d['ranks_seen'] == [0, 1]
    assert d['replicas_equal'] is True
    assert d['config']['global_batch'] == 8 and d['config']['parallelism'] == 'dp2'
    assert d['step_mode'].startswith('eager')
    assert d['multi_gpu_measured'].startswith('gloo')
    assert d['value'] > 0 and d['adam_steps_taken'] >= 3
