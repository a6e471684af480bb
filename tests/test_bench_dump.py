"""bench.py --dump-outputs: what the timed decode returned in its last step, written as .npy files that two builds can be
compared on (inputs fixed by the arguments alone), --steps as the number of timed steps, and what a plain run leaves to
--full."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, 'bench.py')
sys.path.insert(0, ROOT)


def _fake_corpus():
    """three videos packed out of (task, name) order; labels = 100 * packed index + frame"""
    pc = types.SimpleNamespace(n_videos=3, task_names=['b', 'a', 'a'], video_names=['v0', 'v2', 'v1'],
                               lengths=[4, 2, 3], frame_offset=[0, 4, 6])
    labels = np.concatenate([100 * i + np.arange(n) for i, n in enumerate(pc.lengths)]).astype(np.int64)
    outputs = {'labels': labels, 'best': np.array([-1.5, -2.5, -3.5]), 'n_segs': np.array([1, 2, 3], dtype=np.int32)}
    return pc, outputs


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith('.npy')}


def test_dump_orders_videos_by_task_and_name(tmp_path):
    import bench
    pc, outputs = _fake_corpus()
    shapes = bench.dump_outputs(str(tmp_path), pc, outputs)
    got = _load(str(tmp_path))
    assert set(got) == set(shapes) == {'labels', 'best', 'n_segs', 'lengths'}
    # (a, v1) = packed 2, (a, v2) = packed 1, (b, v0) = packed 0
    np.testing.assert_array_equal(got['labels'], [200, 201, 202, 100, 101, 0, 1, 2, 3])
    np.testing.assert_array_equal(got['best'], [-3.5, -2.5, -1.5])
    np.testing.assert_array_equal(got['n_segs'], [3, 2, 1])
    np.testing.assert_array_equal(got['lengths'], [3, 2, 4])
    assert got['labels'].dtype == np.float32 and got['best'].dtype == np.float64


def test_dump_samples_a_large_output_the_same_way_every_time(tmp_path):
    import bench
    n = 300000
    pc = types.SimpleNamespace(n_videos=1, task_names=['t'], video_names=['v'], lengths=[n], frame_offset=[0])
    outputs = {'labels': np.arange(n, dtype=np.int64), 'best': np.zeros(1), 'n_segs': np.ones(1, dtype=np.int32)}
    budget = (1 << 20) + 600000
    for d in ('one', 'two'):
        bench.dump_outputs(str(tmp_path / d), pc, outputs, max_bytes=budget)
    one, two = _load(str(tmp_path / 'one')), _load(str(tmp_path / 'two'))
    assert sum(v.nbytes for v in one.values()) <= budget
    assert 0 < one['labels'].shape[0] < n
    for k in one:
        np.testing.assert_array_equal(one[k], two[k])
    np.testing.assert_array_equal(one['labels'], one['labels_frame_index'])     # label == its frame here


def test_steps_must_be_positive():
    r = subprocess.run([sys.executable, BENCH, '--steps', '0', '--dry-run'], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and '--steps' in r.stderr


def _bench(args, timeout=900):
    env = dict(os.environ)
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT'):
        env.pop(k, None)
    r = subprocess.run([sys.executable, BENCH] + args, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_bench_dumps_the_same_outputs_on_every_run(tmp_path):
    common = ['--gpus', '1', '--workload', 'tiny', '--warmup', '1', '--no-cpu-baseline', '--no-predict-e2e', '--no-strong-leg']
    lines, dumps = [], []
    for i, steps in enumerate((3, 5)):
        d = str(tmp_path / str(i))
        lines.append(_bench(common + ['--steps', str(steps), '--dump-outputs', d]))
        dumps.append(_load(d))
    for line, steps in zip(lines, (3, 5)):
        assert line['steps'] == steps and line['ms_per_step'] > 0
    one, two = dumps
    assert set(one) == {'labels', 'best', 'n_segs', 'lengths'}
    for k in one:
        np.testing.assert_array_equal(one[k], two[k], err_msg=k)
    assert one['labels'].shape[0] == one['lengths'].sum()
    assert np.all(np.isfinite(one['best'])) and np.all(one['n_segs'] >= 1) and np.all(one['labels'] >= 0)


@pytest.mark.gpu
def test_plain_run_leaves_the_secondary_legs_to_full():
    """A plain run prints the headline and the figures of its own timed steps; --full adds every secondary leg."""
    common = ['--gpus', '1', '--workload', 'tiny', '--strong-workload', 'tiny', '--steps', '2', '--warmup', '1']
    plain = _bench(common)
    full = _bench(common + ['--full'])
    secondary = {'mof', 'evaluation', 'fit_stats', 'strong_scaling', 'predict_end_to_end', 'host_features', 'cpu_baseline',
                 'cpu_factored', 'parity'}
    assert plain['full'] is False and not secondary & set(plain)
    assert full['full'] is True and secondary <= set(full)
    for line in (plain, full):
        assert line['unit'] == 'frames/s' and line['higher_is_better'] is True and line['dtype'] == 'f64'
        assert line['steps'] == 2 and line['ms_per_step'] > 0 and line['value'] > 0
        assert line['roofline']['launches_per_step'] > 0
    assert plain['config'] == full['config']
    assert full['parity']['label_mismatches'] == 0 and full['parity']['frames_checked'] > 0
    assert 'stats' in full['strong_scaling'] and 0.0 < full['mof'] <= 1.0
