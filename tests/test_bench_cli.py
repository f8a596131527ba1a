"""bench.py's command line: a plain run prints the headline fields only, `--full` adds the rest, `--dump-outputs DIR` writes
the last timed step's ELBO terms and the parameters after it, and two runs with the same arguments dump the same inputs'
results."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

HEADLINE = ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step', 'steps', 'warmup', 'elbo', 'config')


def test_bench_args_and_dump_layout(tmp_path, monkeypatch):
    """Argument checks and the files dump_outputs writes, on CPU models of every workload."""
    import bench
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--steps', '3', '--dump-outputs', str(tmp_path)])
    a = bench.parse_args()
    assert a.steps == 3 and a.warmup == 3 and not a.full and a.dump_outputs == str(tmp_path)
    for bad in (['--steps', '0'], ['--warmup', '-1']):
        monkeypatch.setattr(sys, 'argv', ['bench.py'] + bad)
        with pytest.raises(SystemExit):
            bench.parse_args()
    for wl in ('S64', 'S128G'):
        gen, enc = bench.build_models(torch.device('cpu'), bench.WORKLOADS[wl])
        terms = (torch.tensor(-1.5, dtype=torch.float64), torch.tensor(-1.0), torch.tensor(0.5, dtype=torch.float64))
        d = tmp_path / wl
        bench.dump_outputs(str(d), terms, gen, enc)
        files = sorted(os.listdir(d))
        n_par = len(list(gen.parameters())) + len(list(enc.parameters()))
        assert len(files) == 3 + n_par and {'elbo.npy', 'log_p.npy', 'kl.npy'} <= set(files)
        assert sum(os.path.getsize(d / f) for f in files) <= 64 << 20
        assert float(np.load(d / 'elbo.npy')) == -1.5 and np.load(d / 'log_p.npy').dtype == np.float32
        w = np.load(d / 'param.enc.conv1.weight.npy')
        assert w.dtype == np.float32 and np.array_equal(w, enc.conv1.weight.detach().numpy())


def _bench(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--workload', 'S28', '--batch', '32', '--steps', '2', '--warmup',
           '1', '--dump-outputs', str(out_dir)]
    env = {k_: v for k_, v in os.environ.items() if k_ not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK')}
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{')][-1])


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_bench_plain_run_and_dump(tmp_path):
    """A plain run: headline fields, no roofline / companions, --steps timed steps; the dump holds the printed ELBO, and a
    second run with the same arguments dumps results of the same inputs (same ELBO terms and parameters to 1e-5)."""
    lines = [_bench(tmp_path / 'a'), _bench(tmp_path / 'b')]
    for line in lines:
        assert all(k_ in line for k_ in HEADLINE), sorted(line)
        assert 'roofline' not in line and 'workloads' not in line and 'exact_f32_mode' not in line
        assert line['steps'] == 2 and line['warmup'] == 1 and line['ms_per_step'] > 0
        assert abs(line['value'] - 32 * 1e3 / line['ms_per_step']) <= 1e-6 * line['value']
    fa, fb = sorted(os.listdir(tmp_path / 'a')), sorted(os.listdir(tmp_path / 'b'))
    assert fa == fb and 'elbo.npy' in fa
    assert float(np.load(tmp_path / 'a' / 'elbo.npy')) == lines[0]['elbo']
    for f in fa:
        a, b = np.load(tmp_path / 'a' / f), np.load(tmp_path / 'b' / f)
        assert a.dtype in (np.float32, np.float64) and a.shape == b.shape and np.isfinite(a).all()
        den = max(float(np.abs(b).max()), 1e-30)
        assert float(np.abs(a - b).max()) / den <= 1e-5, f
