"""bench.py's own rank launcher (`python bench.py --gpus N` without torchrun).

CPU: with fewer visible GPUs than --gpus (none here) it stops before touching any GPU with a clear
message and exit status 2.  GPU: two ranks rehearsed on cuda:0 over gloo
(SPHRT_BENCH_ONE_DEVICE=1) print one JSON line with n_gpus 2 and a final all-gather of the
2 x 50-view stack that matches each rank's own shard.
"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_spawn_refuses_missing_gpus():
    env = dict(os.environ)
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'SPHRT_BENCH_ONE_DEVICE'):
        env.pop(k, None)
    env['HIP_VISIBLE_DEVICES'] = ''       # (on a GPU box too: no device visible)
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2'], env=env,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 2, (p.returncode, p.stderr[-2000:])
    assert 'GPU(s) visible' in p.stderr
    assert p.stdout.strip() == ''


def _rehearse(*args, timeout=600):
    """bench.py with two ranks on cuda:0 over gloo (SPHRT_BENCH_ONE_DEVICE=1) -> its JSON line."""
    env = dict(os.environ, SPHRT_BENCH_ONE_DEVICE='1')
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        env.pop(k, None)
    p = subprocess.run([sys.executable, '-u', os.path.join(ROOT, 'bench.py'), '--gpus', '2']
                       + list(args), env=env, capture_output=True, text=True, timeout=timeout,
                       cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def test_strong_args_refused_for_static_headline():
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--scaling', 'strong'],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 2 and 'c4 and c5' in p.stderr


@pytest.mark.gpu
def test_spawned_two_rank_rehearsal(gpu):
    rec = _rehearse('--full', '--steps', '5', '--warmup', '2')
    assert rec['n_gpus'] == 2 and rec['steps'] == 5 and rec['scaling'] == 'weak'
    assert rec['final_gather']['matches_local_shard']
    assert rec['final_gather']['stack_shape'][0] == 100
    assert rec['value'] > 0
    # the strong-scaled C4 / C5 legs every default run carries (BASELINE configs[3], [4])
    c4, c5 = rec['strong']['c4'], rec['strong']['c5_retrieval']
    assert c4.get('matches_1gpu') is True, c4
    assert c4['views_this_rank'] == 25 and c4['stack_shape'] == [50, 100, 50], c4
    assert c5.get('matches_1gpu') is True, c5
    assert c5['views_this_rank'] == 32 and c5['iterations'] == 100, c5


@pytest.mark.gpu
def test_strong_c4_two_rank_rehearsal(gpu):
    """One 50-slice dynamic volume over 2 ranks: each rank forwards its 25 views / slices and
    back-projects its residual into them; the gathered stack and gradient equal one GPU's."""
    rec = _rehearse('--config', 'c4', '--scaling', 'strong', '--steps', '5', '--warmup', '2',
                    '--full', '--no-cpu-baseline')
    assert rec['scaling'] == 'strong' and rec['n_gpus'] == 2
    s = rec['strong']
    assert s['matches_1gpu'] is True, s
    assert s['stack_rel_diff_vs_1gpu'] <= 1e-5 and s['grad_rel_diff_vs_1gpu'] <= 1e-5, s
    assert s['rays'] == 250000 and s['views_this_rank'] == 25
    assert rec['roofline']['frac'] > 0


@pytest.mark.gpu
def test_strong_c5_two_rank_rehearsal(gpu):
    """The static_retrieval.py loop with its 64 views over 2 ranks (distributed.gd: one gradient
    all_reduce per iteration): the iterates and losses equal retrieval.gd on one GPU."""
    rec = _rehearse('--config', 'c5', '--scaling', 'strong', '--steps', '30', '--warmup', '1',
                    '--full', '--no-cpu-baseline')
    s = rec['strong']
    assert rec['scaling'] == 'strong' and s['iterations'] == 30
    assert s['matches_1gpu'] is True, s
    assert s['coeffs_max_abs_diff_vs_1gpu'] <= 1e-9 and s['fidelity_last'] < s['fidelity_first']


def test_dump_outputs_formats_and_fixed_sample(tmp_path, monkeypatch):
    """--dump-outputs' writer: float64 stays, anything else becomes float32, sequences of floats
    become float64; over the size limit an array is written as the same sample in every run."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    a = torch.arange(24, dtype=torch.float16).reshape(2, 3, 4)
    b = torch.linspace(0, 1, 7, dtype=torch.float64)
    bench.dump_outputs(str(tmp_path / 'd0'), {'a': a, 'b': b, 'f': [0.5, 0.25]})
    got = {n: np.load(tmp_path / 'd0' / f'{n}.npy') for n in ('a', 'b', 'f')}
    assert got['a'].dtype == np.float32 and np.array_equal(got['a'], a.float().numpy())
    assert got['b'].dtype == np.float64 and np.array_equal(got['b'], b.numpy())
    assert got['f'].dtype == np.float64 and got['f'].tolist() == [0.5, 0.25]
    big = torch.arange(1000, dtype=torch.float32)
    monkeypatch.setattr(bench, 'DUMP_LIMIT', 800)
    for d in ('d1', 'd2'):
        bench.dump_outputs(str(tmp_path / d), {'big': big, 'b': b})
    s1, s2 = (np.load(tmp_path / d / 'big.npy') for d in ('d1', 'd2'))
    assert s1.shape == (100,) and np.array_equal(s1, s2) and np.all(np.diff(s1) >= 0)
    assert np.array_equal(np.load(tmp_path / 'd1' / 'b.npy'), b.numpy())    # under its share: whole


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_same_outputs(gpu, tmp_path):
    """A plain run prints the headline line without the legs that --full measures, --steps sets
    the timed steps, and two runs with the same arguments dump identical image stacks."""
    import numpy as np
    recs = []
    for d in ('a', 'b'):
        p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1',
                            '--steps', '7', '--warmup', '2', '--dump-outputs', str(tmp_path / d)],
                           capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert p.returncode == 0, p.stderr[-3000:]
        lines = [l for l in p.stdout.splitlines() if l.startswith('{')]
        assert len(lines) == 1, p.stdout
        recs.append(json.loads(lines[0]))
    rec = recs[0]
    assert rec['steps'] == 7 and rec['full'] is False and rec['dtype'] == 'f32'
    assert rec['unit'] == 'rays/s' and rec['higher_is_better'] is True and rec['value'] > 0
    assert abs(rec['value'] * rec['ms_per_step'] * 1e-3 - 250000) <= 1e-6 * 250000
    for moved in ('roofline', 'adjoint', 'cold', 'pcie_inclusive', 'strong', 'cpu_baseline',
                  'final_gather'):
        assert moved not in rec, moved
    ya, yb = (np.load(tmp_path / d / 'y.npy') for d in ('a', 'b'))
    assert ya.dtype == np.float32 and ya.shape == (50, 50, 100)
    assert np.isfinite(ya).all() and ya.max() > 0 and np.array_equal(ya, yb)
