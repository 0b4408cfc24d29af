"""bench.py contract on the GPU box: one JSON line with the required keys, and the N>1 code path
(RCCL process group, barrier, MAX all-reduce of the elapsed time) exercised with a single rank under
torch.distributed.run."""
import json
import os
import subprocess
import sys
import time

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REQUIRED = ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling',
            'vs_baseline', 'dtype', 'data', 'config', 'roofline', 'cpu_baseline')


def _last_json(out):
    lines = [l for l in out.strip().splitlines() if l.startswith('{')]
    assert len(lines) == 1, out[-2000:]
    return json.loads(lines[0])


def test_bench_single_process(gpu_device):
    r = subprocess.run([sys.executable, 'bench.py', '--steps', '3', '--warmup', '1', '--full', '--no-cpu-baseline',
                        '--no-extras', '--images-per-gpu', '2'], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    j = _last_json(r.stdout)
    for k in REQUIRED:
        assert k in j, k
    assert j['n_gpus'] == 1 and j['steps'] == 3 and j['value'] > 1e6
    assert j['dtype'].startswith('f32') and 'split-fp16' in j['dtype']         # the label says what the MLP multiplies
    assert 'split-fp16' in j['config']['mlp']
    assert j['ms_per_step_stats']['min'] <= j['ms_per_step_stats']['median'] <= j['ms_per_step_stats']['max']
    assert j['prewarm']['untimed_steps'] >= 10          # steady-state allocator / shader clock before W + K (bench.py docstring)
    assert 'one stream' in j['schedule']                # `value` is what a caller of render() gets; the two-stream figure is a side field
    # scalars inside `config` (the driver's parser keeps config / roofline / cpu_baseline, not unknown top-level keys)
    cfg = j['config']
    for k in ('value_serial', 'value_pipelined', 'value_mlp_exact_fp32', 'value_all_rays_hit'):
        assert cfg[k] > 1e6, k
    assert cfg['value_serial'] == j['value'] and cfg['value_mlp_exact_fp32'] < 1.05 * j['value']
    assert cfg['rays_marched_fraction_all_rays_hit'] > 0.9       # (0.97 - 0.98: the corners of the image see past the cube)
    assert len(j['per_rank']) == 1 and j['per_rank'][0]['kernel_ms'] > 0 and 0 < j['per_rank'][0]['rays_marched_fraction'] <= 1
    rf = j['roofline']
    # algorithmic decoder FLOPs / kernel time against the fp32 matrix / vector peak; the binding pipe
    # (vector ALU) and the utilisation proxy are side fields, each a fraction
    assert rf['bound'] == 'valu' and rf['valu_frac'] == rf['valu_pipe']['frac'] and rf['unit'] == 'TFLOP/s' and rf['source'] and 0.0 < rf['frac'] <= 1.0
    assert abs(rf['frac'] - rf['achieved'] / rf['peak']) < 1e-9
    assert 0.0 < rf['valu_pipe']['frac'] <= 1.0 and rf['traffic'] > 0
    lv = rf['levels']
    for k in ('l2_requests', 'fabric', 'hbm_compulsory'):
        assert 0.0 < lv[k]['frac'] <= 1.0, (k, lv[k])
    assert lv['gather_stream_algorithmic']['x_hbm_peak'] > 0


def test_bench_plain_run_is_the_headline_alone(gpu_device):
    """Without --full the run sets up, warms up, times the K steps and prints the line: no variant legs, no live kernel
    timing or roofline, no extras, no CPU baseline.  The whole process spends at most 30 s outside its W + K steps."""
    steps, warmup = 20, 5
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, 'bench.py', '--gpus', '1', '--steps', str(steps), '--warmup', str(warmup)], cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr[-2000:]
    j = _last_json(r.stdout)
    for k in REQUIRED:
        assert k in j, k
    assert j['full'] is False and j['steps'] == steps and j['value'] > 1e6 and j['ms_per_step'] > 0
    assert j['roofline'] is None and j['cpu_baseline'] is None
    for k in ('variants', 'extras', 'parity', 'kernel_ms_stats'):
        assert k not in j, k
    assert not [k for k in j['config'] if k.startswith(('value_', 'x_'))], j['config']
    assert j['per_rank'][0]['kernel_ms'] is None and 0 < j['per_rank'][0]['rays_marched_fraction'] <= 1
    assert wall - (steps + warmup) * j['ms_per_step'] * 1e-3 <= 30.0, wall


def test_bench_16_bit_texel_storage(gpu_device):
    """--texels bf16 (the storage type BASELINE cfg2 names): the line comes out, the exact-fp32 leg (fp32 texels only) is left
    out, and the run's own parity figure is taken against the ROUNDED planes."""
    r = subprocess.run([sys.executable, 'bench.py', '--steps', '3', '--warmup', '1', '--full', '--no-extras', '--texels', 'bf16',
                        '--images-per-gpu', '2'], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    j = _last_json(r.stdout)
    assert j['config']['texel_storage'].startswith('bf16') and 'value_mlp_exact_fp32' not in j['config']
    assert j['config']['value_all_rays_hit'] > 1e6 and j['parity']['ok'], j['parity']


def test_bench_parity_figure(gpu_device):
    """The bench line carries its own parity check: one image of the timed workload against the CPU oracle."""
    r = subprocess.run([sys.executable, 'bench.py', '--steps', '3', '--warmup', '1', '--full', '--no-extras'], cwd=ROOT,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    j = _last_json(r.stdout)
    assert j['parity']['ok'] and max(j['parity'][k] for k in ('rgb', 'depth', 'mask')) <= 1e-4, j['parity']
    assert j['parity']['mask_mean'] > 0.05
    # the CPU baseline is the reference itself (run.py::render + the real Generator's sampler from the staged oracle/_ref)
    from oracle import reference
    assert j['cpu_baseline']['value'] > 0
    if reference.available():
        assert j['cpu_baseline']['kind'] == 'reference'
        p = j['parity']
        assert p['oracle_equals_reference_cpu_bit_for_bit'], p
        assert max(p['vs_reference_cpu'].values()) <= 1e-4 and p['ok_vs_reference_pytorch_rocm'], p
    else:                                                # (a snapshot without the staged oracle/_ref: the oracle restatement)
        assert j['cpu_baseline']['kind'] == 'port' and j['parity']['ok_vs_pytorch_rocm']


def test_bench_train_mode_single_rank_rccl(gpu_device):
    """--mode train under torch.distributed.run with one rank and --force-dist: the RCCL process group, the bucketed
    gradient all-reduce launched from backward hooks and the per-rank timing report."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0')
    r = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '1',
                        '--master-addr', '127.0.0.1', '--master-port', '29519', 'bench.py', '--gpus', '1', '--mode', 'train',
                        '--steps', '3', '--warmup', '2', '--force-dist'],
                       cwd=ROOT, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    j = _last_json(r.stdout)
    assert j['n_gpus'] == 1 and j['value'] > 1e5 and 'RCCL all_reduce' in j['config']['collective']
    assert j['config']['gradient_bytes_per_step'] > 120e6
    pr = j['per_rank'][0]
    assert pr['fwd_bwd_ms'] > 0 and pr['allreduce_exposed_ms'] >= 0 and pr['buckets_launched_in_backward'] >= 1
    import math
    assert math.isfinite(pr['loss'])


def test_bench_distributed_code_path(gpu_device):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0')
    r = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '1',
                        '--master-addr', '127.0.0.1', '--master-port', '29517', 'bench.py', '--gpus', '1', '--steps', '3',
                        '--warmup', '1', '--full', '--no-cpu-baseline', '--no-extras', '--images-per-gpu', '2', '--force-dist'],
                       cwd=ROOT, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    j = _last_json(r.stdout)
    assert j['n_gpus'] == 1 and j['value'] > 1e6 and j['scaling'] == 'weak'
    # render mode reports every rank's own step time, kernel time and marched fraction (N > 1: one entry per rank)
    assert [pr['rank'] for pr in j['per_rank']] == [0] and j['per_rank'][0]['ms_per_step'] > 0


@pytest.mark.parametrize('mode', ['render', 'train'])
def test_bench_launches_itself_when_called_without_a_launcher(gpu_device, mode):
    """How the driver calls it for N > 1: plain `python bench.py --gpus N ...`, no torchrun, no WORLD_SIZE.  bench.py then
    re-runs its own command line under torch.distributed.run (one process per GPU on 127.0.0.1); exercised here with
    one rank through --force-dist (the box has one GPU): rc 0, ONE JSON line from rank 0, RCCL initialised."""
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    cmd = [sys.executable, 'bench.py', '--gpus', '1', '--force-dist', '--steps', '3', '--warmup', '1']
    cmd += ['--mode', 'train'] if mode == 'train' else ['--no-cpu-baseline', '--no-extras', '--images-per-gpu', '2']
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    j = _last_json(r.stdout)
    assert j['n_gpus'] == 1 and j['value'] > 1e5
    if mode == 'train':
        assert 'RCCL' in j['config']['collective'] and len(j['per_rank']) == 1
    # asking for more GPUs than the box has fails loudly instead of hanging in a rendezvous
    r = subprocess.run([sys.executable, 'bench.py', '--gpus', '64', '--steps', '1', '--warmup', '0'], cwd=ROOT,
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode != 0 and 'GPU(s) are visible' in (r.stderr + r.stdout)


def test_bench_dump_outputs_repeat_exactly(gpu_device, tmp_path):
    """--dump-outputs DIR: the last timed step's rgb / depth / mask as float32 .npy; with equal arguments two runs write the
    same arrays (the timed steps' noise starts from a fixed seed), and --steps is the number of timed steps."""
    import numpy as np
    runs = []
    for name in ('a', 'b'):
        r = subprocess.run([sys.executable, 'bench.py', '--steps', '4', '--warmup', '1', '--no-cpu-baseline', '--no-extras',
                            '--no-variants', '--images-per-gpu', '2', '--dump-outputs', str(tmp_path / name)],
                           cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        j = _last_json(r.stdout)
        assert j['steps'] == 4 and j['ms_per_step'] > 0
        assert j['dump_outputs']['arrays'] == {'rgb': [2, 128, 128, 3], 'depth': [2, 128, 128], 'mask': [2, 128, 128]}
        runs.append({k: np.load(str(tmp_path / name / (k + '.npy'))) for k in ('rgb', 'depth', 'mask')})
    for k, a in runs[0].items():
        assert a.dtype == np.float32 and np.isfinite(a).all(), k
        assert np.array_equal(a, runs[1][k]), k
    assert runs[0]['mask'].max() > 0.5                            # the cameras see the scene
