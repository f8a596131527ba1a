"""Step configurations shared by the memory-safety tests (tests/test_hip_modules.py) and the graph-replay tests
(tests/test_graph_gpu.py): the geometry table, the seeded model builders and the bitwise comparison.  A plain helper
module: no fixture, no test, nothing pytest collects."""
import numpy as np
import torch

from conftest import load_golden, tdict

# (n, z_dim, R, B, C, hidden, k, padding, Fourier decoder) of the memory-safety tests and of the graph-replay cases
OOB_CONFIGS = {'small': (20, 2, 8, 8, 8, 32, 20, 4, False),
               'small_fourier': (20, 2, 8, 8, 8, 32, 20, 4, True),
               'S28': (28, 2, 8, 16, 128, 512, 28, 14, False),
               'S28F': (28, 2, 16, 8, 128, 512, 28, 14, True),
               'S64': (64, 2, 8, 4, 128, 512, 64, 16, False),
               # B * Ho a multiple of 32 (as at the bench's B = 256): no ragged last tile
               'S64x': (64, 2, 8, 32, 128, 512, 64, 16, False),
               'M50x': (50, 2, 8, 32, 128, 512, 28, 8, False),
               # the reference's MNIST geometries (k = 28, padding 8): the 44- and 66-wide ring
               # transforms; M28r: a batch whose last 32-column tile is ragged
               'M28': (28, 2, 8, 32, 128, 512, 28, 8, False),
               'M28r': (28, 2, 8, 5, 128, 512, 28, 8, False),
               'M50': (50, 2, 8, 4, 128, 512, 28, 8, False),
               # round 5: a large frame (L = 112, Ho = 97 = 3 x 32 + 1): the WIDE generic transforms
               # along w (workgroup per tile, extra output column on the vector ALU), ragged batch
               'G96': (96, 2, 8, 3, 16, 64, 32, 16, False)}

# (n, k, padding, B) of the encoders with 103 head rows (z_dim = 50, R = 4); the second has a column count that is a multiple of 32
HEADS103_GEOM = {'heads103': (20, 20, 4, 3), 'heads103_x32': (21, 20, 3, 2)}


def dev():
    return torch.device('cuda:0')


def bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and \
        torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))


def build_encoder(fx, prefix):
    import src.models as M
    cfg = [int(v) for v in fx['cfg']]
    n, cin, zd, C, k, p, R, refine, normal = cfg[:9]
    enc = M.InferenceNetwork_AttentionTranslation_AttentionRotation(
        n, cin, zd, kernels_num=C, kernels_size=k, padding=p, groupconv=R, rot_refinement=bool(refine),
        theta_prior=float(fx['theta_prior']), normal_prior_over_r=bool(normal))
    enc.load_state_dict({k_: v for k_, v in tdict(fx, prefix).items()})
    return enc.to(dev())


def build_generator(fx, prefix, zd, hid, n_out, L, resid, fourier, sigma):
    import src.models as M
    gen = M.SpatialGenerator(zd, hid, n_out=n_out, num_layers=L, resid=bool(resid), fourier_expansion=bool(fourier),
                             sigma=sigma)
    gen.load_state_dict({k_: v for k_, v in tdict(fx, prefix).items()})
    return gen.to(dev())


def build_step_models(fx):
    n, cin, zd, C, k, p, R, refine, normal, hid, L, n_out, fourier, resid = [int(v) for v in fx['cfg']]
    enc = build_encoder(fx, 'e.')
    gen = build_generator(fx, 'd.', zd, hid, n_out, L, resid, fourier, float(fx['sigma']))
    return enc, gen, n


def fresh(n, zd, R, B, C, hid, k, pad, four, cin=1, layers=2, resid=False, n_out=1, enc_activation=None, refine=True,
          normal=False, theta_prior=np.pi):
    """Seeded generator and encoder of one OOB_CONFIGS row (the keywords vary what the row does not name), the coordinate
    grid, one normal minibatch and one noise triple."""
    import src.models as M
    from tvae import step, tables
    torch.manual_seed(0)
    gen = M.SpatialGenerator(zd, hid, n_out=n_out, num_layers=layers, resid=resid, fourier_expansion=four,
                             sigma=2.0 / (n - 1)).to(dev())
    act = {} if enc_activation is None else dict(activation=enc_activation)
    enc = M.InferenceNetwork_AttentionTranslation_AttentionRotation(
        n, cin, zd, kernels_num=C, kernels_size=k, padding=pad, groupconv=R, rot_refinement=refine, theta_prior=theta_prior,
        normal_prior_over_r=normal, **act).to(dev())
    x = torch.from_numpy(tables.image_coords(n)).to(dev())
    y = torch.randn(B, cin, n, n, device=dev())
    nz = step.draw_noise(B, R * enc.output_size() ** 2, zd, dev())
    return gen, enc, x, y, nz


def heads103_encoder(case):
    """z_dim = 50: 103 head rows (the wide encoder tail in h3).  Returns (encoder, minibatch, z_dim, R)."""
    import src.models as M
    (n, k, pad, B), R, zd = HEADS103_GEOM[case], 4, 50
    torch.manual_seed(5)
    enc = M.InferenceNetwork_AttentionTranslation_AttentionRotation(n, 1, zd, kernels_num=128, kernels_size=k, padding=pad,
                                                                    groupconv=R, rot_refinement=True, theta_prior=np.pi,
                                                                    normal_prior_over_r=False).to(dev())
    with torch.no_grad():
        for m in (enc.conv_a, enc.conv_r, enc.conv_z):
            m.weight.mul_(8.0)
    return enc, torch.rand(B, 1, n, n, device=dev()), zd, R


def cin3_direct_encoder():
    """Three input channels at a geometry for the DIRECT convolution kernels (fp32 MFMA in f32, the LDS-resident split kernels
    otherwise) once the caller has switched the frequency-domain route off.  Returns (encoder, minibatch, z_dim, R)."""
    import src.models as M
    n, k, pad, B, R, zd = 20, 9, 3, 5, 4, 2
    torch.manual_seed(6)
    enc = M.InferenceNetwork_AttentionTranslation_AttentionRotation(n, 3, zd, kernels_num=128, kernels_size=k, padding=pad,
                                                                    groupconv=R, rot_refinement=True, theta_prior=np.pi,
                                                                    normal_prior_over_r=False).to(dev())
    return enc, torch.rand(B, 3, n, n, device=dev()), zd, R


def golden_step(name):
    """Models, coordinate grid, minibatch and noise triple of a tests/golden/step_*.npz fixture, on the device:
    (fx, enc, gen, x, y, noise)."""
    from oracle import tvae_oracle as O
    fx = load_golden(name)
    enc, gen, n = build_step_models(fx)
    x = O.image_coords(n).to(dev())
    noise = tuple(torch.from_numpy(fx[k_]).to(dev()) for k_ in ('E', 'eps_z', 'eps_theta'))
    return fx, enc, gen, x, torch.from_numpy(fx['y']).to(dev()), noise


# ---------------------------------------------------------------------------------------------
# graph replay (tests/test_graph_gpu.py): the case table and the routes no captured step can take
# ---------------------------------------------------------------------------------------------
# One row per configuration whose forward + backward is captured into a hipGraph and compared bitwise with eager execution.
# 'cfg': a row of OOB_CONFIGS (with 'B' replacing its batch and 'kw' passed on to fresh()); 'golden': the models of a
# tests/golden/step_*.npz fixture; 'encoder': one of the encoder-only builders above plus a small plain decoder.
# 'lik': the likelihood the driver would pair with it; 'dft': False switches the frequency-domain convolution off for both runs.
GRAPH_CASES = {
    'S28': dict(cfg='S28', lik='gauss'),
    'M28r': dict(cfg='M28r', lik='bce'),
    'S28F': dict(cfg='S28F', lik='bce'),
    'S64': dict(cfg='S64', lik='gauss'),
    # 4 x 4096 pixels = 16384 columns with two hidden layers: the padded row stride of the stored activations (dec.ld_pad)
    'S64_deep3': dict(cfg='S64', lik='gauss', kw=dict(layers=3)),
    'M50': dict(cfg='M50', lik='bce'),
    'G96': dict(cfg='G96', lik='gauss'),
    'small_fourier': dict(cfg='small_fourier', lik='gauss'),
    'deep4_resid': dict(cfg='S28', B=8, lik='bce', kw=dict(layers=4, resid=True)),
    'deep3_nout2': dict(cfg='S28', B=8, lik='gauss_var', kw=dict(layers=3, n_out=2)),
    'galaxy': dict(golden='step_galaxy_small', lik='bce3'),
    # 103 head rows at 128 channels: the wide encoder tail (the galaxy fixture has 16 channels and takes the plain one);
    # 'heads103': its data gradient with the generic weight gradients, 'heads103_x32': enc.tail_wgrad_wide
    'heads103': dict(encoder='heads103', lik='bce'),
    'heads103_x32': dict(encoder='heads103_x32', lik='bce'),
    'cin3_direct': dict(encoder='cin3_direct', lik='bce3', dft=False),
    'noref_normal': dict(cfg='small', lik='bce', kw=dict(refine=False, normal=True, theta_prior=np.pi / 4)),
    'tanh': dict(cfg='S28', B=8, lik='gauss', kw=dict(enc_activation=torch.nn.Tanh)),
}
# cases that also run in the other three arithmetic modes (every case runs in the default one, h3)
GRAPH_ARITHMETIC_CASES = ('S28', 'S28F', 'deep4_resid')
GRAPH_ARITHMETIC_MODES = ('f32', 'x6', 'bf16')

# routes of tvae/ops.py that no captured training step can take, each with its reason
GRAPH_EXCLUDED_ROUTES = {
    'enc.inference': 'inference-mode forward: only under no_grad (eval_model, get_latent), never inside a training step',
    'dec.no_h_inference': 'inference-mode forward: only under no_grad (eval_model, get_latent), never inside a training step',
    'trans_attn.plain': 'encoder of --r-inf unimodal: driver.graph_supported() is False for that branch',
    'trans_attn.rot_pool': 'encoder of --r-inf unimodal: driver.graph_supported() is False for that branch',
    'mlp_encoder.kernels': 'encoder of --t-inf unimodal: driver.graph_supported() is False for that branch',
}


def noted_routes():
    """Every route name tvae/ops.py can record: the string literals inside the argument of each `_note(...)` call
    (a conditional expression yields both of its names)."""
    import ast
    import os
    from conftest import PKG
    with open(os.path.join(PKG, 'tvae', 'ops.py')) as f:
        tree = ast.parse(f.read())
    def literals(e):
        if isinstance(e, ast.IfExp):                     # both results; the condition's own constants are no route names
            return literals(e.body) | literals(e.orelse)
        assert isinstance(e, ast.Constant) and isinstance(e.value, str), ast.dump(e)
        return {e.value}
    names = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and node.func.id == '_note':
            names |= literals(node.args[0])
    return names
