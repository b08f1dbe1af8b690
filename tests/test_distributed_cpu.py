"""
world_size-2 `gloo` test of the N > 1 path (CPU): the batch is sharded by entry, each rank reduces
its shard to a handful of floats, ONE all-reduce rebuilds the global mean -- exactly the value the
un-sharded computation gives.  Per-rank Dice values come from the oracle here (tests may use it; the
GPU path produces them with the HIP kernels, test_gpu_pipeline.py).
"""

import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        from neurite_amd import distributed as nd
        from oracle import np_oracle as npo
        rng = np.random.default_rng(2024)                      # same stream on every rank
        B, S, L = 5, (6, 5, 4), 7
        t = rng.random((B,) + S + (L,)).astype(np.float32)
        p = rng.random((B,) + S + (L,)).astype(np.float32)
        w = rng.random((1, L)).astype(np.float32)
        lo, hi = nd.shard_range(B)
        assert (lo, hi) == nd.shard_range(B, rank, world)
        local = torch.from_numpy(npo.dice(t[lo:hi], p[lo:hi]))
        got = nd.all_reduce_mean_dice(local, weights=w)
        pend = nd.all_reduce_mean_dice(local, weights=w, async_op=True)        # collective in flight; collected later
        assert isinstance(pend, nd.PendingMean)
        assert float(pend.result()) == float(got) and float(pend.result()) == float(got)
        want = npo.mean_dice(t, p, weights=w)
        # spatially split batch entry: all-reduce the numerator/denominator partials, then divide
        half = S[0] // 2
        sl = slice(0, half) if rank == 0 else slice(half, None)
        stp, stt, spp = npo.dice_sums(t[:, sl], p[:, sl])
        sums = torch.from_numpy(np.stack([stp, stt, spp], 1).astype(np.float32))
        tot = nd.reduce_dice_sums(sums)
        full = np.stack(npo.dice_sums(t, p), 1)
        # cross-entropy: mean over ALL voxels from per-rank (sum, count)
        lv = npo.cce_per_voxel(t[lo:hi], p[lo:hi])
        ce = nd.all_reduce_mean(torch.tensor(lv.sum(), dtype=torch.float32), lv.size)
        # data-parallel gradients: flat-bucket all-reduce == the mean of the per-rank gradients
        g_all = [rng.standard_normal((world, 3, 3, 3, 2, 4)).astype(np.float32), rng.standard_normal((world, 4)).astype(np.float32),
                 rng.standard_normal((world, 1, 1, 1, 4, 5)).astype(np.float32)]
        params = []
        for ga in g_all:
            prm = torch.nn.Parameter(torch.zeros(ga.shape[1:]))
            prm.grad = torch.from_numpy(ga[rank].copy())
            params.append(prm)
        ncalls = nd.all_reduce_gradients(params)
        gerr = max(float(np.abs(prm.grad.numpy() - ga.mean(0)).max()) for prm, ga in zip(params, g_all))
        ncalls2 = nd.all_reduce_gradients(params, bucket_mb=1e-4, average=False)     # tiny buckets: [216] and [4, 20] floats
        # the persistent form: the gradients LIVE in one flat buffer (views), one collective, nothing packed or copied back
        params_b = [torch.nn.Parameter(torch.zeros(ga.shape[1:])) for ga in g_all]
        params_b[1].grad = torch.from_numpy(g_all[1][rank].copy())          # a gradient that exists already is adopted
        bucket = nd.GradientBucket(params_b)
        assert bucket.intact() and all(prm.grad.data_ptr() >= bucket.flat.data_ptr() for prm in params_b)
        for k, (prm, ga) in enumerate(zip(params_b, g_all)):
            if k != 1:
                prm.grad += torch.from_numpy(ga[rank])                       # what backward() does: accumulate in place
        ptrs = [prm.grad.data_ptr() for prm in params_b]
        assert bucket.all_reduce() == 1
        assert ptrs == [prm.grad.data_ptr() for prm in params_b] and bucket.intact()
        gerr = max(gerr, max(float(np.abs(prm.grad.numpy() - ga.mean(0)).max()) for prm, ga in zip(params_b, g_all)))
        bucket.zero_()
        assert all(float(prm.grad.abs().max()) == 0.0 for prm in params_b)
        params_b[0].grad = None
        try:
            bucket.all_reduce()
            raise AssertionError('a dropped gradient view must be refused')
        except RuntimeError:
            pass
        q.put((rank, float(got), float(want), np.abs(tot.numpy() - full).max() / np.abs(full).max(),
               float(ce), float(npo.cce(t, p)), gerr, ncalls, ncalls2))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(180)
def test_sharded_reductions_world2():
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = 29500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=150) for _ in procs]
    for p in procs:
        p.join(30)
        assert p.exitcode == 0
    for rank, got, want, rel, ce, ce_want, gerr, ncalls, ncalls2 in res:
        assert abs(got - want) <= 1e-6 * abs(want), (rank, got, want)
        assert rel < 1e-6
        assert abs(ce - ce_want) <= 1e-5 * abs(ce_want)
        assert gerr < 1e-6 and ncalls == 1 and ncalls2 == 2
    assert res[0][1] == res[1][1]          # every rank holds the same reduced value


def test_world1_is_identity():
    from neurite_amd import distributed as nd
    d = torch.rand(3, 4)
    assert torch.allclose(nd.all_reduce_mean_dice(d), d.mean())
    assert torch.allclose(nd.all_reduce_mean_dice(d, async_op=True).result(), d.mean())
    s = torch.rand(2, 3, 4)
    assert nd.reduce_dice_sums(s) is s
    assert nd.shard_range(10) == (0, 10)
    prm = torch.nn.Parameter(torch.zeros(3))
    prm.grad = torch.ones(3)
    assert nd.all_reduce_gradients([prm]) == 0 and torch.equal(prm.grad, torch.ones(3))
    b = nd.GradientBucket([prm])
    assert b.all_reduce() == 0 and b.all_reduce(async_op=True) is None and torch.equal(prm.grad, torch.ones(3)) and b.intact()
    (prm * 2).sum().backward()                                   # autograd accumulates INTO the view
    assert b.intact() and torch.equal(b.flat, torch.full((3,), 3.0))
    # a refused model is left as it was (the dtype check used to run after earlier .grad had been re-pointed) ...
    p32, p16 = torch.nn.Parameter(torch.zeros(2)), torch.nn.Parameter(torch.zeros(2, dtype=torch.bfloat16))
    g32 = torch.ones(2)
    p32.grad = g32
    with pytest.raises(ValueError):
        nd.GradientBucket([p32, p16])
    assert p32.grad is g32
    # ... and a bucket whose views were dropped says so at world size 1 too, in zero_() as well as in all_reduce()
    prm.grad = None
    assert not b.intact()
    with pytest.raises(RuntimeError):
        b.zero_()
    with pytest.raises(RuntimeError):
        b.all_reduce()


def _bench_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        import time
        import bench
        from neurite_amd import distributed as nd
        calls = []

        def step(events):
            # stub of one bench step: this rank's "dice" is a constant [B_local, L] block; rank 3 is the straggler
            calls.append(events)
            if rank == 3:
                time.sleep(0.02)
            d = torch.full((4, 8), float(rank + 1))
            return nd.all_reduce_mean_dice(d, async_op=True)

        r = bench.timed(step, steps=5, warmup=2, dist=dist, dev=None)
        q.put((rank, len(calls), r))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(240)
def test_bench_timed_loop_world4():
    """bench.py's timed region (barrier + sync on both sides, EXACTLY K timed steps after W warm-up steps, the collective of
    step k collected after step k + 1 is enqueued, MAX over ranks, rank count taken from a collective) on 4 gloo ranks"""
    world = 4
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = 31500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_bench_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=200) for _ in procs])
    for p in procs:
        p.join(30)
        assert p.exitcode == 0
    for rank, ncalls, r in res:
        assert ncalls == 7                                   # 2 warm-up + 5 timed, no extra step anywhere
        assert r['ranks'] == world                           # counted by an all-reduce of ones, not read from the environment
        assert len(r['per_rank_s']) == world
        assert r['elapsed'] == max(r['per_rank_s'])
        assert r['elapsed'] >= 5 * 0.02                      # everyone waits for the straggler: the closing barrier is inside
        assert abs(r['mean'] - 2.5) < 1e-6                   # global mean over ranks of (rank + 1)
    assert len({r['elapsed'] for _, _, r in res}) == 1       # every rank reports the same (max) time
    # the same loop without a process group (N = 1)
    import bench
    r = bench.timed(lambda ev: None, 3, 1)
    assert r['ranks'] == 1 and r['mean'] is None and len(r['per_rank_s']) == 1


def _prewarm_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        import time
        import bench
        from neurite_amd import distributed as nd
        time.sleep(0.013 * rank)                              # the ranks reach the measurement at different times ...

        def step(events):
            time.sleep(0.001 * (rank + 1))                    # ... and run at different speeds
            return nd.all_reduce_mean_dice(torch.full((2, 4), float(rank)), async_op=True)
        n = bench.prewarm(step, 60.0, dist, None, sync=lambda: None)
        q.put((rank, n))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(240)
def test_bench_prewarm_stops_on_every_rank_together():
    """the untimed pre-warming in front of every measurement runs by the clock; with a collective in every step the ranks must agree on
    when to stop (a rank that went on alone would wait in its all-reduce for ever -- the multi-GPU bench would hang)"""
    world = 3
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = 33500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_prewarm_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=200) for _ in procs])
    for p in procs:
        p.join(30)
        assert p.exitcode == 0
    counts = {n for _, n in res}
    assert len(counts) == 1 and counts.pop() % 8 == 0 and res[0][1] >= 8


@pytest.mark.timeout(300)
def test_bench_self_launches_its_ranks_cpu_stub():
    """`python bench.py --gpus 2` with no launcher around it: bench.py re-runs itself under torch.distributed.run (one process per rank),
    and exactly ONE JSON line comes out of the parent.  --stub-step swaps the kernels for a stub so that the launch, the timed region,
    the collective and the stdout discipline run on CPU ranks (gloo).  An N > 1 run is BASELINE config 4 as written unless told otherwise:
    global batch 32, 32 / N per rank, "scaling": "strong" (VERDICT r5 item 3); --weak and --global-batch override it."""
    import json
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'NRT_BENCH_CHILD')}
    for extra, scaling, per_gpu in (([], 'strong', 16), (['--weak'], 'weak', 4), (['--global-batch', '6'], 'strong', 3)):
        p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', '3', '--warmup', '1', '--stub-step'] + extra,
                           cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=280, text=True)
        assert p.returncode == 0, p.stderr[-3000:]
        lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
        assert len(lines) == 1, lines
        j = json.loads(lines[0])
        assert j['n_gpus'] == 2 and j['rccl_ranks'] == 2 and j['steps'] == 3 and j['warmup'] == 1
        assert j['scaling'] == scaling and j['config']['volumes_per_gpu'] == per_gpu and j['config']['global_batch'] == 2 * per_gpu
        assert abs(j['config']['mean_dice'] - 1.5) < 1e-6 and j['data'] == 'stub'
    # a global batch that the ranks do not divide is an error, not a silent truncation
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', '1', '--warmup', '0', '--stub-step',
                        '--global-batch', '5'], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=280, text=True)
    assert p.returncode != 0 and not p.stdout.strip()


def test_scaling_bookkeeping_worlds_1_2_4_8():
    """What the driver's N = 1, 2, 4, 8 runs will divide: BASELINE config 4 (`--global-batch 32`, strong) keeps 32 volumes in total with
    32 / N per rank; the default (weak) keeps 4 per rank; the shard of rank r is the contiguous range batch entry b -> rank b * W // B,
    every entry exactly once; a batch the ranks do not divide is refused."""
    import bench
    from neurite_amd import distributed as nd
    for world in (1, 2, 4, 8):
        per, total, scaling = bench.batch_plan(32, 4, world)
        assert (per, total, scaling) == (32 // world, 32, 'strong')
        assert bench.batch_plan(0, 4, world) == (4, 4 * world, 'weak')
        # what a run that names no batch gets: N = 1 the 4-volume step, N > 1 config 4 as written; --weak keeps 4 per rank
        g = bench.default_global_batch(0, False, world)
        assert g == (0 if world == 1 else 32)
        assert bench.batch_plan(g, 4, world) == ((4, 4, 'weak') if world == 1 else (32 // world, 32, 'strong'))
        assert bench.default_global_batch(0, True, world) == 0 and bench.default_global_batch(16, False, world) == 16
        seen = []
        for rank in range(world):
            lo, hi = nd.shard_range(32, rank, world)
            assert hi - lo == per
            seen += list(range(lo, hi))
            assert all(b * world // 32 == rank for b in range(lo, hi))
        assert seen == list(range(32))
    with pytest.raises(SystemExit):
        bench.batch_plan(32, 4, 3)
    assert bench.default_global_batch(0, False, 3) == 0       # a world that does not divide 32 stays weak (and says so in the line)


@pytest.mark.timeout(300)
def test_bench_strong_mode_world4_cpu_stub():
    """the strong-scaling line of a 4-rank run (self-launched, gloo, stub step): global batch 32, 8 volumes per rank"""
    import json
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'NRT_BENCH_CHILD')}
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '4', '--steps', '2', '--warmup', '1', '--stub-step',
                        '--global-batch', '32'], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=280, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    j = json.loads(lines[0])
    assert j['n_gpus'] == 4 and j['rccl_ranks'] == 4 and j['scaling'] == 'strong'
    assert j['config']['volumes_per_gpu'] == 8 and j['config']['global_batch'] == 32
    assert abs(j['config']['mean_dice'] - 2.5) < 1e-6                  # mean of the ranks' constants 1, 2, 3, 4


@pytest.mark.timeout(300)
def test_bench_dump_outputs_cpu_stub(tmp_path):
    """--dump-outputs DIR after the timed steps: every rank's Dice values of the last step in global batch order (dice.npy, float32) and
    the global mean (mean_dice.npy, float64); two runs with the same arguments write the same arrays"""
    import json
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'NRT_BENCH_CHILD')}
    dumps = []
    for run in range(2):
        out = tmp_path / ('run%d' % run)
        p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', '2', '--warmup', '1', '--stub-step',
                            '--global-batch', '6', '--dump-outputs', str(out)], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, timeout=280, text=True)
        assert p.returncode == 0, p.stderr[-3000:]
        lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
        assert len(lines) == 1, lines
        j = json.loads(lines[0])
        assert j['steps'] == 2 and j['ms_per_step'] > 0
        assert sorted(os.listdir(out)) == ['dice.npy', 'mean_dice.npy']
        d, mean = np.load(out / 'dice.npy'), np.load(out / 'mean_dice.npy')
        assert d.dtype == np.float32 and d.shape == (6, 8)
        assert np.array_equal(d[:3], np.full((3, 8), 1.0, np.float32)) and np.array_equal(d[3:], np.full((3, 8), 2.0, np.float32))
        assert mean.dtype == np.float64 and abs(float(mean) - j['config']['mean_dice']) < 1e-6
        dumps.append((d, mean))
    assert np.array_equal(dumps[0][0], dumps[1][0]) and np.array_equal(dumps[0][1], dumps[1][1])
