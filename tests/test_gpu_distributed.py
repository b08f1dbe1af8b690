"""
The multi-process path of bench.py on ONE GPU: `python -m torch.distributed.run --nproc-per-node 1 bench.py --gpus 1` with
NRT_FORCE_DIST=1 creates an `nccl` (= RCCL) process group of size 1, runs the async all-reduce of the Dice numerator /
denominator pair after every step and prints ONE JSON line on stdout.  Not a scaling number: proof on a fresh box that
communicator creation, the collective and the stdout discipline work before an 8-GPU node ever runs the same command
(VERDICT r2 #8).  The reference's only multi-device code is neurite/tf/utils/model.py:298-321.
"""

import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_under_torchrun_with_rccl_world_size_one(dev):
    env = dict(os.environ)
    env.update(NRT_FORCE_DIST='1', HSA_ENABLE_IPC_MODE_LEGACY='0', MASTER_ADDR='127.0.0.1')
    env.pop('RANK', None)
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '1', '--master-addr', '127.0.0.1',
           '--master-port', '29517', os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1', '--size', '64',
           '--batch-per-gpu', '2', '--no-cpu-baseline', '--no-unet', '--no-batch1']
    p = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, 'exactly one JSON line on stdout, got %r' % (lines,)
    j = json.loads(lines[0])
    assert j['n_gpus'] == 1 and j['steps'] == 3 and j['warmup'] == 1
    assert j['rccl_ranks'] == 1                                   # counted by an all-reduce of ones over the nccl group, not read from the env
    assert j['scaling'] == 'weak' and j['higher_is_better'] is True and j['value'] > 0
    assert len(j['ms_per_step_per_rank']) == 1
    # the mean Dice the collective produced equals the single-process value
    p1 = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '3', '--warmup', '1', '--size', '64', '--batch-per-gpu', '2',
                         '--no-cpu-baseline', '--no-unet', '--no-batch1'], cwd=ROOT, env={k: v for k, v in env.items() if k != 'NRT_FORCE_DIST'},
                        stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, text=True)
    assert p1.returncode == 0, p1.stderr[-3000:]
    j1 = json.loads([ln for ln in p1.stdout.splitlines() if ln.strip()][-1])
    assert abs(j['config']['mean_dice'] - j1['config']['mean_dice']) <= 2e-6


def test_bench_self_spawn_forced_on_one_gpu(dev):
    """`python bench.py --gpus 1` with NRT_FORCE_SPAWN=1 takes the path `--gpus N > 1` takes without a launcher: bench.py starts its own
    ranks under torch.distributed.run, the rank builds an RCCL group, ONE JSON line comes back through the parent; --global-batch makes
    the line a strong-scaling one."""
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'NRT_BENCH_CHILD')}
    env.update(NRT_FORCE_SPAWN='1', HSA_ENABLE_IPC_MODE_LEGACY='0')
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1', '--size', '64', '--global-batch', '2',
           '--no-cpu-baseline', '--no-unet', '--no-batch1']
    p = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, 'exactly one JSON line on stdout, got %r' % (lines,)
    j = json.loads(lines[0])
    assert j['n_gpus'] == 1 and j['rccl_ranks'] == 1 and j['steps'] == 3
    assert j['scaling'] == 'strong' and j['config']['volumes_per_gpu'] == 2 and j['config']['global_batch'] == 2 and j['value'] > 0
    assert 'bench.py: launching 1 ranks' in p.stderr


def test_bench_two_ranks_share_one_gpu_over_gloo(dev):
    """The multi-process CONTROL FLOW of bench.py with world size 2 on real kernels: two ranks on the one GPU of the box (NRT_DEVICE=0), the
    collective over gloo (RCCL refuses two ranks per device).  What it proves before an 8-GPU node runs the nccl form of the same code: both
    ranks leave the clock-bounded pre-warming together (an all-reduced flag -- ranks deciding by their own clocks would hang here), the
    strong-scaling default (global batch 32, 16 volumes per rank), one JSON line from rank 0, a mean Dice that is the mean over BOTH shards."""
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'NRT_BENCH_CHILD')}
    env.update(NRT_DIST_BACKEND='gloo', NRT_DEVICE='0', MASTER_ADDR='127.0.0.1')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
           '--master-port', '29533', os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', '4', '--warmup', '1', '--size', '64',
           '--prewarm-ms', '120', '--full', '--no-cpu-baseline', '--no-unet', '--no-batch1']
    p = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip().startswith('{')]
    assert len(lines) == 1, 'exactly one JSON line on stdout, got %r' % (lines,)
    j = json.loads(lines[0])
    assert j['n_gpus'] == 2 and j['rccl_ranks'] == 2 and j['steps'] == 4 and len(j['ms_per_step_per_rank']) == 2
    assert j['scaling'] == 'strong' and j['config']['global_batch'] == 32 and j['config']['volumes_per_gpu'] == 16 and j['value'] > 0
    assert j['weak_per_gpu']['volumes_per_gpu'] == 4 and j['weak_per_gpu']['rccl_ranks'] == 2
    # the global mean is the mean over both ranks' shards: the single-process run over all 32 volumes gives the same number
    env1 = {k: v for k, v in env.items() if k not in ('NRT_DIST_BACKEND', 'NRT_DEVICE')}
    p1 = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '2', '--warmup', '1', '--size', '64', '--batch-per-gpu', '32',
                         '--prewarm-ms', '0', '--no-cpu-baseline', '--no-unet', '--no-batch1', '--no-strong'], cwd=ROOT, env=env1,
                        stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, text=True)
    assert p1.returncode == 0, p1.stderr[-3000:]
    j1 = json.loads([ln for ln in p1.stdout.splitlines() if ln.strip().startswith('{')][-1])
    assert abs(j['config']['mean_dice'] - j1['config']['mean_dice']) <= 3e-6


def test_bench_dump_outputs_are_the_timed_steps_dice(dev, tmp_path):
    """A plain run times its steps only; --dump-outputs writes the Dice values of the last timed step, which are the fused kernel's values
    on the seeded bench inputs (recomputed here), and the global mean the line reports."""
    import numpy as np
    import neurite_amd as ne
    from neurite_amd import synth
    out = tmp_path / 'dump'
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '3', '--warmup', '1', '--size', '64', '--batch-per-gpu', '2',
           '--prewarm-ms', '0', '--dump-outputs', str(out)]
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'NRT_BENCH_CHILD', 'NRT_FORCE_DIST')}
    p = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip().startswith('{')]
    assert len(lines) == 1, lines
    j = json.loads(lines[0])
    assert j['steps'] == 3 and j['ms_per_step'] > 0 and j['full'] is False
    assert not {'dropin_pipeline', 'cpu_baseline', 'unet_fwd', 'config2_batch1', 'cfg4_strong'} & set(j)
    d, mean = np.load(out / 'dice.npy'), np.load(out / 'mean_dice.npy')
    assert d.dtype == np.float32 and d.shape == (2, 32) and mean.dtype == np.float64
    mov, fix, trf = synth.cfg2_batch(2, 64, 32, device=dev, seed0=100)
    want = ne.fused.warp_dice(mov, trf, fix).cpu().numpy()
    np.testing.assert_allclose(d, want, rtol=1e-5, atol=1e-6)
    assert abs(float(mean) - j['config']['mean_dice']) <= 2e-6 and abs(float(mean) - float(want.mean())) <= 2e-6
