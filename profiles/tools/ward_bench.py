#!/usr/bin/env python3
"""Time tvae.cluster.ward_linkage (HIP events, after a warm-up) against scipy's fp64 `ward` on the same box.

scipy builds the condensed N (N - 1) / 2 fp64 distance matrix, so it only runs where that fits (--scipy-max-n).
Prints one JSON line naming the box (GPU, CPU) and one per shape: wall time of the whole linkage, rounds, launches per
entry point, the time of the first (largest) tvae_ward_nn launch alone and its rate, and, where scipy ran, its time
and whether the two dendrograms agree.

  python profiles/tools/ward_bench.py [--shapes 10000x4,20000x16,100000x4,100000x100] [--scipy-max-n 20000]
                                      [--no-scipy]

Data: blobs with overlapping tails (as kmeans_bench.py).  For the share of time per kernel run it under
`rocprofv3 --kernel-trace --stats` with one shape.
"""
import argparse
import collections
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..', '..', 'target-vae_amd'))

import numpy as np
import torch


def data(N, d, k=20, seed=0):
    rng = np.random.default_rng(seed)
    means = 3.0 * rng.standard_normal((k, d))
    return (means[rng.integers(0, k, N)] + rng.standard_normal((N, d))).astype(np.float32)


def box():
    cpu = ''
    try:
        with open('/proc/cpuinfo') as f:
            cpu = next((ln.split(':', 1)[1].strip() for ln in f if ln.startswith('model name')), '')
    except OSError:
        pass
    return dict(gpu=torch.cuda.get_device_name(0), cpu=cpu)


def main(args):
    from tvae import _cluster_lib as CL, _lib, cluster
    dev = torch.device('cuda:0')
    print(json.dumps(dict(box=box())), flush=True)
    for shp in args.shapes.split(','):
        N, d = [int(v) for v in shp.split('x')]
        X = data(N, d)
        Xd = torch.from_numpy(X).to(dev)
        cluster.ward_linkage(Xd[:2048])                                         # warm-up: library load, kernels
        torch.cuda.synchronize()
        launches = collections.Counter()

        def hook(name, sig, a, do_call):
            launches[name] += 1
            return do_call(a)

        old = _lib.set_call_hook(hook)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        res = cluster.ward_linkage(Xd)
        e1.record()
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        _lib.set_call_hook(old)
        gpu_s = e0.elapsed_time(e1) / 1e3
        # the first round's nearest-neighbour launch alone (M = N: the largest of the run)
        Ct, ldc = cluster._feature_major(Xd)
        cnt = torch.ones(ldc, device=dev)
        nn, nd = torch.zeros(N, dtype=torch.int32, device=dev), torch.zeros(N, device=dev)
        wsf = CL.query('tvae_ward_nn_ws_floats', N, d)
        ws = torch.empty(wsf, device=dev)
        CL.call('tvae_ward_nn', Ct, ldc, cnt, nn, nd, ws, wsf, N, d)
        torch.cuda.synchronize()
        reps = 3
        e0.record()
        for _ in range(reps):
            CL.call('tvae_ward_nn', Ct, ldc, cnt, nn, nd, ws, wsf, N, d)
        e1.record()
        torch.cuda.synchronize()
        nn_ms = e0.elapsed_time(e1) / reps
        flops = 3.0 * N * N * d                                                 # sub + fma per (row, column, feature)
        out = dict(N=N, d=d, gpu_s=round(gpu_s, 4), wall_s=round(wall, 4), rounds=res.n_rounds, launches=dict(launches),
                   nn_first_ms=round(nn_ms, 3), nn_first_tflops=round(flops / nn_ms / 1e9, 2),
                   nn_first_gpairs_s=round(N * N / nn_ms / 1e6, 1), nn_splits=CL.query('tvae_ward_nn_splits', N, d))
        if not args.no_scipy and N <= args.scipy_max_n:
            from scipy.cluster.hierarchy import ward
            t0 = time.perf_counter()
            Zr = ward(X.astype(np.float64))
            sp = time.perf_counter() - t0
            out.update(scipy_s=round(sp, 3), speedup=round(sp / gpu_s, 1),
                       same_tree=bool(np.array_equal(res.Z[:, [0, 1, 3]], Zr[:, [0, 1, 3]])),
                       rows_differ=int((res.Z[:, [0, 1, 3]] != Zr[:, [0, 1, 3]]).any(1).sum()),
                       height_err=float((np.abs(res.Z[:, 2] - Zr[:, 2]) / Zr[:, 2]).max()))
        print(json.dumps(out), flush=True)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='10000x4,20000x16,100000x4,100000x100')
    ap.add_argument('--scipy-max-n', type=int, default=20000)
    ap.add_argument('--no-scipy', action='store_true')
    main(ap.parse_args())
