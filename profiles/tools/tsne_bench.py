#!/usr/bin/env python3
"""Time tvae.tsne.tsne (exact repulsion on the GPU) against sklearn's Barnes-Hut TSNE on the same box and the same
synthetic latents, and measure the pair rate of the repulsion kernel alone.

Both embeddings start from the same explicit init and are judged by the same functions: the exact fp64 KL divergence
over the same sparse P (tvae.tsne.gradient: tvae_tsne_repulsion + tvae_tsne_kl) and sklearn's trustworthiness
(n_neighbors = 10; it builds the N x N distance matrix on the host, --no-trust skips it).  Writes one JSON document,
by default profiles/tsne_bench_<N>x<d>.json.

  python profiles/tools/tsne_bench.py [--n 10000] [--d 4] [--out FILE] [--no-sklearn] [--no-trust]
                                      [--rate-n 10000,100000,737280]

Data: blobs with overlapping tails (as ward_bench.py).  Times are wall clock around a synchronised run after a warm-up
on a 1000-point subset (library load, kernel load).
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
    return dict(gpu=torch.cuda.get_device_name(0), cpu=cpu, cpu_threads=os.environ.get('OMP_NUM_THREADS', ''))


def repulsion_rate(N, dev, scale=20.0, reps=5):
    """Milliseconds of one tvae_tsne_repulsion call (all three launches) on a spread-out embedding, and pairs per second."""
    from tvae import tsne
    st = tsne._State(N, dev)
    st.Y[0][:, :N] = scale * torch.randn(2, N, device=dev)
    st.repulsion(0)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        st.repulsion(0)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / reps
    return dict(N=N, ms=round(ms, 4), pairs_per_s=float('%.4g' % (float(N) * N / ms * 1e3)))


def main(args):
    from tvae import tsne
    dev = torch.device('cuda:0')
    N, d = args.n, args.d
    X = data(N, d)
    Xd = torch.from_numpy(X).to(dev)
    Y0 = (1e-4 * np.random.default_rng(1).standard_normal((N, 2))).astype(np.float32)
    tsne.tsne(Xd[:1000], seed=0)                                               # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = tsne.tsne(Xd, init=torch.from_numpy(Y0))
    torch.cuda.synchronize()
    gpu_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    idx, d2 = tsne.knn(Xd, tsne.n_neighbors(N, 30.0))
    torch.cuda.synchronize()
    knn_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    P = tsne.joint_probabilities(idx, tsne.conditional_probabilities(d2, 30.0))
    torch.cuda.synchronize()
    p_s = time.perf_counter() - t0
    out = dict(box=box(), N=N, d=d, perplexity=30.0, max_iter=1000,
               gpu=dict(wall_s=round(gpu_s, 3), n_iter=res.n_iter, knn_s=round(knn_s, 4), joint_p_s=round(p_s, 4),
                        kl=tsne.gradient(res.embedding, P)[2]),
               repulsion=[repulsion_rate(int(n), dev) for n in args.rate_n.split(',') if n])
    print('# gpu:', json.dumps(out['gpu']), json.dumps(out['repulsion']), file=sys.stderr, flush=True)
    if not args.no_trust:
        from sklearn.manifold import trustworthiness
        out['gpu']['trustworthiness'] = float(trustworthiness(X, res.embedding.cpu().numpy(), n_neighbors=10))
    if not args.no_sklearn:
        from sklearn.manifold import TSNE
        t0 = time.perf_counter()
        sk = TSNE(2, learning_rate=200.0, init=Y0.copy(), perplexity=30.0)
        Ys = sk.fit_transform(X)
        sk_s = time.perf_counter() - t0
        out['sklearn'] = dict(wall_s=round(sk_s, 3), n_iter=int(sk.n_iter_), own_kl=float(sk.kl_divergence_),
                              kl=tsne.gradient(torch.from_numpy(Ys.astype(np.float32)).to(dev), P)[2])
        if not args.no_trust:
            out['sklearn']['trustworthiness'] = float(trustworthiness(X, Ys, n_neighbors=10))
        out['kl_ratio_gpu_over_sklearn'] = out['gpu']['kl'] / out['sklearn']['kl']
        out['speedup'] = round(sk_s / gpu_s, 1)
    path = args.out or os.path.join(HERE, '..', f'tsne_bench_{N}x{d}.json')
    with open(path, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=10000)
    ap.add_argument('--d', type=int, default=4)
    ap.add_argument('--out', default=None)
    ap.add_argument('--no-sklearn', action='store_true')
    ap.add_argument('--no-trust', action='store_true')
    ap.add_argument('--rate-n', default='10000,100000,737280')
    main(ap.parse_args())
