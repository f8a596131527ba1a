#!/usr/bin/env python3
"""Time tvae.cluster.kmeans (HIP events, after a warm-up) against sklearn's Lloyd on the same box.

Both sides start from the SAME explicit initial centroids (n_init = 100 restarts: sklearn runs one KMeans(init=...,
n_init=1, algorithm='lloyd') per restart, 16 threads), so they do the same kind of iterations; the iteration counts
of both sides are reported.  Prints one JSON line naming the box (GPU, CPU) and one per shape:

  python profiles/tools/kmeans_bench.py [--shapes 10000x4x10,100000x16x50,1000000x16x50] [--n-init 100]
                                        [--sk-restarts 100] [--no-sklearn]

--sk-restarts: sklearn restarts actually run (its time is scaled to n_init restarts when fewer run).
"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..', '..', 'target-vae_amd'))

import numpy as np
import torch


def data(N, d, k, n_init, seed=0):
    """k Gaussian blobs with overlapping tails (so that Lloyd runs tens of iterations)."""
    rng = np.random.default_rng(seed)
    means = 3.0 * rng.standard_normal((k, d))
    y = rng.integers(0, k, N)
    X = (means[y] + rng.standard_normal((N, d))).astype(np.float32)
    init = np.stack([X[rng.permutation(N)[:k]] for _ in range(n_init)])
    return X, init


def box():
    """What the numbers were measured on: GPU name, CPU model, threads given to sklearn."""
    cpu = ''
    try:
        with open('/proc/cpuinfo') as f:
            cpu = next((ln.split(':', 1)[1].strip() for ln in f if ln.startswith('model name')), '')
    except OSError:
        pass
    return dict(gpu=torch.cuda.get_device_name(0), cpu=cpu, sklearn_threads=16)


def main(args):
    from tvae import cluster
    dev = torch.device('cuda:0')
    print(json.dumps(dict(box=box())), flush=True)
    for shp in args.shapes.split(','):
        N, d, k = [int(v) for v in shp.split('x')]
        X, init = data(N, d, k, args.n_init)
        Xd, Id = torch.from_numpy(X).to(dev), torch.from_numpy(init).to(dev)
        cluster.kmeans(Xd[:4096], k, init=Id[:2], max_iter=3)                   # warm-up: library load, kernels
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        res = cluster.kmeans(Xd, k, init=Id)
        e1.record()
        torch.cuda.synchronize()
        gpu_s = e0.elapsed_time(e1) / 1e3
        # one assign + update pair over all restarts, timed alone (the kernel bound is stated against this)
        from tvae import _cluster_lib as CL
        Xt, ldx = cluster._feature_major(Xd)
        R = Id.shape[0]
        wsf = CL.query('tvae_kmeans_ws_floats', N, d, k, R)
        ws = torch.empty(wsf, device=dev)
        lab = torch.full((R, N), -1, dtype=torch.int32, device=dev)
        md = torch.empty(R, N, device=dev)
        chg, done = torch.zeros(R, dtype=torch.int32, device=dev), torch.zeros(R, dtype=torch.int32, device=dev)
        C = Id.clone()
        CL.call('tvae_kmeans_assign', Xt, ldx, C, done, lab, md, chg, ws, wsf, N, d, k, R)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(5):
            CL.call('tvae_kmeans_assign', Xt, ldx, C, done, lab, md, chg, ws, wsf, N, d, k, R)
        e1.record()
        torch.cuda.synchronize()
        assign_ms = e0.elapsed_time(e1) / 5
        flops = 3.0 * N * k * d * R                                             # sub + fma per (point, centroid, feature)
        out = dict(N=N, d=d, k=k, n_init=R, gpu_s=round(gpu_s, 4), gpu_n_iter_best=res.n_iter, gpu_inertia=res.inertia,
                   assign_ms=round(assign_ms, 3), assign_tflops=round(flops / assign_ms / 1e9, 2),
                   assign_x_gbs=round(4.0 * N * d * R / assign_ms / 1e6, 1))
        if not args.no_sklearn:
            from sklearn.cluster import KMeans
            from threadpoolctl import threadpool_limits
            m = min(args.sk_restarts, R)
            iters, best = [], np.inf
            with threadpool_limits(limits=16):
                t0 = time.perf_counter()
                for r in range(m):
                    km = KMeans(n_clusters=k, init=init[r], n_init=1, algorithm='lloyd').fit(X)
                    iters.append(int(km.n_iter_))
                    best = min(best, float(km.inertia_))
                sk = time.perf_counter() - t0
            out.update(sklearn_s=round(sk * R / m, 3), sklearn_restarts_run=m, sklearn_iters_mean=float(np.mean(iters)),
                       sklearn_inertia=best, speedup=round(sk * R / m / gpu_s, 1))
        print(json.dumps(out), flush=True)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='10000x4x10,100000x16x50,1000000x16x50')
    ap.add_argument('--n-init', type=int, default=100)
    ap.add_argument('--sk-restarts', type=int, default=100)
    ap.add_argument('--no-sklearn', action='store_true')
    main(ap.parse_args())
