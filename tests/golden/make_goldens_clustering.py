#!/usr/bin/env python3
"""Generate the fixtures of the clustering half from the REAL reference scripts (clustering_*.py).

Like make_goldens.py it runs only where the reference is mounted read-only; plotting, astropy and torchvision imports
are stubbed to reach the real functions.  It writes small data files only (no reference source is copied):

  get_latent_unimodal_unimodal.npz, get_latent_attention_unimodal_gc{4,0}.npz
        clustering_mnist.get_latent on the two secondary inference branches, B = 4 (inputs, parameters, outputs)
  cluster_acc.json              clustering_mnist.cluster_acc on a fixed label pair
  cli_flags_clustering.json     argparse surface of the four clustering scripts (flags, defaults, choices)

Usage:  python tests/golden/make_goldens_clustering.py
"""
import importlib
import json
import os
import sys
import types

sys.dont_write_bytecode = True
REF = '/root/reference'
HERE = os.path.dirname(os.path.abspath(__file__))

import numpy as np
import torch

torch.set_num_threads(8)
SCRIPTS = ('clustering_mnist', 'clustering_particles', 'clustering_galaxy', 'clustering_dsprites')


class _Stub(types.ModuleType):
    def __getattr__(self, k):
        if k.startswith('__'):
            raise AttributeError(k)
        m = _Stub(self.__name__ + '.' + k)
        setattr(self, k, m)
        return m

    def __call__(self, *a, **k):
        return None


def _stub_missing():
    for nm in ('torchvision', 'seaborn', 'astropy', 'astropy.stats', 'astropy.units', 'matplotlib', 'matplotlib.pyplot',
               'matplotlib.cm', 'matplotlib.colors', 'mpl_toolkits', 'mpl_toolkits.mplot3d', 'mpl_toolkits.axes_grid1',
               'pandas'):
        try:
            __import__(nm)
        except Exception:
            sys.modules[nm] = _Stub(nm)


def _reference(name):
    _stub_missing()
    sys.path.insert(0, REF)
    try:
        return importlib.import_module(name)
    finally:
        sys.path.pop(0)


def coords(n):
    xg = np.linspace(-1, 1, n)
    yg = np.linspace(1, -1, n)
    x0, x1 = np.meshgrid(xg, yg)
    return torch.from_numpy(np.stack([x0.ravel(), x1.ravel()], 1)).float()


def save(name, **arrs):
    path = os.path.join(HERE, name + '.npz')
    np.savez_compressed(path, **{k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v))
                                 for k, v in arrs.items()})
    print('wrote', path, os.path.getsize(path) // 1024, 'KiB')


def gen_get_latent():
    cm = _reference('clustering_mnist')
    sys.path.insert(0, REF)
    import src.models as models
    sys.path.pop(0)
    n, zd, B = 20, 2, 4
    torch.manual_seed(9)
    y = torch.rand(B, 1, n, n)
    for name, t_inf, gc in (('get_latent_unimodal_unimodal', 'unimodal', 0),
                            ('get_latent_attention_unimodal_gc4', 'attention', 4),
                            ('get_latent_attention_unimodal_gc0', 'attention', 0)):
        torch.manual_seed(1)
        if t_inf == 'unimodal':
            enc = models.InferenceNetwork_UnimodalTranslation_UnimodalRotation(n * n, zd + 3, 32, num_layers=2)
        else:
            enc = models.InferenceNetwork_AttentionTranslation_UnimodalRotation(n, 1, zd, kernels_num=8, groupconv=gc)
            with torch.no_grad():
                for nm in ('conv_a', 'conv_r', 'conv_z'):
                    getattr(enc, nm).weight.mul_(10.0)
        torch.manual_seed(3)
        zc, th, dx = cm.get_latent(coords(n), y, enc, t_inf, 'unimodal', 'cpu', n)
        out = dict(y=y, z_content=zc, theta_mu=th, dx=dx, cfg=np.array([n, zd, gc]))
        for k_, v in enc.state_dict().items():
            out['p.' + k_] = v
        save(name, **out)


def gen_cluster_acc():
    cm = _reference('clustering_mnist')
    rng = np.random.default_rng(3)
    y_true = rng.integers(0, 5, 200)
    y_pred = np.where(rng.random(200) < 0.7, (y_true * 3 + 1) % 5, rng.integers(0, 7, 200))      # 7 clusters, 5 classes
    mapping, acc = cm.cluster_acc(y_true, y_pred)
    out = dict(y_true=y_true.tolist(), y_pred=y_pred.tolist(), rows=np.asarray(mapping[0]).tolist(),
               cols=np.asarray(mapping[1]).tolist(), acc=float(acc))
    path = os.path.join(HERE, 'cluster_acc.json')
    json.dump(out, open(path, 'w'))
    print('wrote', path, acc)


def gen_cli():
    import argparse

    class _Captured(Exception):
        pass

    out = {}
    for name in SCRIPTS:
        mod = _reference(name)
        orig = argparse.ArgumentParser.parse_args

        def grab(self, *a, **k):
            raise _Captured(self)
        argparse.ArgumentParser.parse_args = grab
        try:
            mod.main()
        except _Captured as e:
            parser = e.args[0]
        finally:
            argparse.ArgumentParser.parse_args = orig
        flags = {}
        for act in parser._actions:
            if act.dest == 'help':
                continue
            flags[act.dest] = dict(flags=list(act.option_strings), default=act.default,
                                   choices=list(act.choices) if act.choices else None,
                                   type=getattr(act.type, '__name__', None), nargs0=(act.nargs == 0))
        out[name] = flags
    path = os.path.join(HERE, 'cli_flags_clustering.json')
    json.dump(out, open(path, 'w'), indent=1, sort_keys=True)
    print('wrote', path, {k: len(v) for k, v in out.items()})


if __name__ == '__main__':
    which = sys.argv[1:] or ['get_latent', 'cluster_acc', 'cli']
    for w in which:
        {'get_latent': gen_get_latent, 'cluster_acc': gen_cluster_acc, 'cli': gen_cli}[w]()
