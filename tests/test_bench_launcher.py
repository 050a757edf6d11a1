"""bench.py's multi-GPU plumbing on CPU (no GPU, no HIP library): `--gpus N`
spawns N rank processes before anything touches a device, the ranks shard the
volcano grid (strong: the fixed G x G grid; weak: an (N*G) x G grid), the
status counts are all-reduced, the result map is gathered and reassembled,
and rank 0 prints exactly one JSON line with n_gpus = N (gloo backend)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, timeout=240):
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_PORT')}
    env['OMP_NUM_THREADS'] = '1'
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--device', 'cpu-standin'] + args,
                       capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


@pytest.mark.parametrize('scaling, grid', [('strong', [32, 32]), ('weak', [64, 32])])
def test_launcher_world2(scaling, grid):
    line = _run(['--gpus', '2', '--steps', '2', '--warmup', '1', '--grid', '32', '--scaling', scaling])
    assert line['n_gpus'] == 2
    assert line['scaling'] == scaling
    assert line['config']['global_grid'] == grid
    assert line['config']['grid_per_gpu'] == [grid[0] // 2, 32]
    # every rank's statuses are counted once (the stand-in marks every 7th local unit 'degenerate')
    st = line['status']
    assert st['units'] == grid[0] * grid[1]
    local = grid[0] * 32 // 2
    exp_degen = sum(sum(1 for i in range(local) if (i + r) % 7 == 0) for r in range(2))
    assert st['degenerate_root_tight_transient'] == exp_degen
    assert st['regular_root'] + st['degenerate_root_tight_transient'] + st['failed'] == st['units']
    assert line['value'] > 0


def test_default_multi_gpu_layout_is_strong():
    """Without --scaling, the N ranks shard one fixed G x G grid: BASELINE
    configs[2]'s 1024 x 1024 grid sharded over the GPUs of the node."""
    line = _run(['--gpus', '2', '--steps', '1', '--warmup', '0', '--grid', '16'])
    assert line['scaling'] == 'strong'
    assert line['config']['global_grid'] == [16, 16] and line['config']['grid_per_gpu'] == [8, 16]


def test_launcher_single_rank():
    line = _run(['--steps', '1', '--warmup', '0', '--grid', '16'])
    assert line['n_gpus'] == 1 and line['config']['global_grid'] == [16, 16]


def _load(d):
    return {f: np.load(os.path.join(str(d), f)) for f in sorted(os.listdir(str(d)))}


def test_dump_outputs_single_rank(tmp_path):
    """--dump-outputs DIR: the arrays of the last timed step as DIR/<name>.npy,
    float32 / float64, the same from run to run with the same arguments."""
    args = ['--steps', '2', '--warmup', '1', '--grid', '16', '--dump-outputs']
    line = _run(args + [str(tmp_path / 'a')])
    _run(args + [str(tmp_path / 'b')])
    a, b = _load(tmp_path / 'a'), _load(tmp_path / 'b')
    assert sorted(a) == ['nsteps.npy', 'result.npy', 'status.npy']
    E1, E2 = np.meshgrid(np.linspace(-2.5, 0.5, 16), np.linspace(-2.5, 0.5, 16), indexing='ij')
    assert np.array_equal(a['result.npy'], E1.ravel() * 10.0 + E2.ravel())
    for f, x in a.items():
        assert x.dtype in (np.float32, np.float64) and x.shape == (256,), (f, x.dtype, x.shape)
        assert np.array_equal(x, b[f]), f
    assert int((a['status.npy'] == 4).sum()) == line['status']['degenerate_root_tight_transient']
    assert line['steps'] == 2 and line['ms_per_step'] >= 0.0


def test_dump_outputs_per_rank(tmp_path):
    """At N > 1 every rank writes its own share as <name>.rank<r>.npy."""
    _run(['--gpus', '2', '--steps', '1', '--warmup', '0', '--grid', '16', '--dump-outputs', str(tmp_path)])
    a = _load(tmp_path)
    assert sorted(a) == ['%s.rank%d.npy' % (n, r) for n in ('nsteps', 'result', 'status') for r in (0, 1)]
    assert all(x.shape == (128,) for x in a.values())


def test_dump_outputs_sample_is_fixed(tmp_path):
    """Beyond the byte budget the same seeded, sorted sample of the conditions
    is kept of every array, and the files stay within the budget."""
    import torch
    sys.path.insert(0, ROOT)
    import bench
    n = 1000
    out = dict(y=torch.arange(3 * n, dtype=torch.float64).reshape(3, n), tof=torch.arange(n, dtype=torch.float64),
               status=torch.arange(n, dtype=torch.int32))
    budget = 20000
    for d in ('a', 'b'):
        bench.dump_outputs(out, str(tmp_path / d), budget=budget)
    a, b = _load(tmp_path / 'a'), _load(tmp_path / 'b')
    assert sorted(a) == ['sample_index.npy', 'status.npy', 'tof.npy', 'y.npy']
    idx = a['sample_index.npy']
    assert 0 < idx.size < n and np.all(np.diff(idx) > 0)
    assert np.array_equal(a['tof.npy'], idx) and np.array_equal(a['status.npy'], idx)
    assert np.array_equal(a['y.npy'], idx[None, :] + n * np.arange(3)[:, None])
    assert all(x.dtype == np.float64 for x in a.values())
    assert sum(x.nbytes for x in a.values()) <= budget
    assert all(np.array_equal(a[f], b[f]) for f in a)
    # within the budget (40 bytes per condition here) nothing is sampled
    w = bench.dump_outputs(out, str(tmp_path / 'c'), budget=40 * n)
    assert w == {'y.npy': [3, n], 'tof.npy': [n], 'status.npy': [n]}


def test_default_dump_budget_is_below_64_mb():
    sys.path.insert(0, ROOT)
    import bench
    assert bench.DUMP_BUDGET_BYTES < 64 * 10 ** 6


def test_plain_line_has_headline_keys_only_full_adds_the_rest():
    """A plain run states the headline figure; the roofline and the CPU
    baseline are null without --full (and --full is accepted)."""
    for extra in ([], ['--full', '--no-cpu-baseline']):
        line = _run(['--steps', '3', '--warmup', '0', '--grid', '16'] + extra)
        for key in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step'):
            assert key in line, key
        assert line['steps'] == 3 and line['roofline'] is None and line['cpu_baseline'] is None


@pytest.fixture(scope='module')
def gpu_bench(tmp_path_factory):
    """One small plain run and one --full run of the volcano workload on the GPU."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    d = tmp_path_factory.mktemp('bench_dump')
    res = {}
    for name, extra in (('plain', ['--dump-outputs', str(d)]), ('full', ['--full', '--no-cpu-baseline'])):
        p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '2', '--warmup', '1',
                            '--grid', '64'] + extra, capture_output=True, text=True, timeout=150, cwd=ROOT)
        assert p.returncode == 0, p.stderr[-3000:]
        lines = [l for l in p.stdout.splitlines() if l.startswith('{')]
        assert len(lines) == 1, p.stdout
        res[name] = json.loads(lines[0])
    return res, _load(d)


@pytest.mark.gpu
def test_gpu_plain_run_dumps_the_last_step(gpu_bench):
    res, a = gpu_bench
    line = res['plain']
    assert line['roofline'] is None and line['cpu_baseline'] is None
    assert line['steps'] == 2 and line['ms_per_step'] > 0.0 and line['unit'] == 'solves/s' and line['dtype'] == 'f64'
    assert abs(line['value'] - 64 * 64 / (line['ms_per_step'] * 1e-3)) <= 1e-9 * line['value']
    assert sorted(a) == ['nsteps.npy', 'status.npy', 'tof.npy', 'y.npy']
    assert a['y.npy'].ndim == 2 and a['y.npy'].shape[1] == 4096 and a['y.npy'].dtype == np.float64
    for f in ('tof.npy', 'status.npy', 'nsteps.npy'):
        assert a[f].shape == (4096,) and a[f].dtype == np.float64, f
    st = line['status']
    assert int((a['status.npy'] == 0).sum()) == st['regular_root'] > 0
    assert int((a['status.npy'] == 4).sum()) == st['degenerate_root_tight_transient']
    ok = a['status.npy'] == 0
    assert np.all(np.isfinite(a['tof.npy'][ok])) and np.all(np.isfinite(a['y.npy'][:, ok]))
    assert np.all(a['nsteps.npy'][ok] >= 1)


@pytest.mark.gpu
def test_gpu_full_run_states_the_roofline(gpu_bench):
    res, _ = gpu_bench
    roof = res['full']['roofline']
    assert roof is not None and roof['kernel_ms'] > 0.0 and roof['rate_constants_ms'] > 0.0
    assert roof['integrator_steps'] > 0 and 0.0 < roof['lane_efficiency'] <= 1.0
    assert res['full']['status'] == res['plain']['status']


def test_strong_needs_divisible_rows():
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK')}
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--device', 'cpu-standin', '--gpus', '3',
                        '--steps', '1', '--warmup', '0', '--grid', '16', '--scaling', 'strong'], capture_output=True, text=True,
                       timeout=240, env=env, cwd=ROOT)
    assert p.returncode != 0


def test_emulate_rejected_with_ranks():
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK')}
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--device', 'cpu-standin', '--gpus', '2',
                        '--emulate', '0/8'], capture_output=True, text=True, timeout=120, env=env, cwd=ROOT)
    assert p.returncode != 0


def test_flop_count_is_structural():
    """bench.flops_per_step counts structural non-zeros: the volcano plan's
    count is below the dense count of the same step."""
    sys.path.insert(0, ROOT)
    import bench
    import pycatkin_amd as P
    from pycatkin_amd.functions.volcano import set_volcano_energies
    s = P.read_from_input_file(os.path.join(ROOT, 'tests', 'golden', 'inputs', 'COOxVolcano', 'input.json'))
    set_volcano_energies(s)
    plan = s.plan(('CO_ox',))
    f = bench.flops_per_step(plan)
    NS = len(plan.dyn)
    dense_lu = (2 * NS ** 3) // 3
    assert 400 < f < 1000, f
    assert f > dense_lu + 6 * 2 * NS * NS - 6 * NS   # at least the LU and the solves
