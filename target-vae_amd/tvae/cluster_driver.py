"""Driver shared by clustering_{mnist,particles,galaxy,dsprites}.py: the second half of the reference workflow.

Keeps the reference command lines (flags and defaults of the four clustering_*.py parsers, tests/golden/
cli_flags_clustering.json), their default data paths, the whole-module torch.load of the saved encoder and the wording
of results.txt.  The latents of the whole stack are extracted on the device (tvae.latent.extract_latents) and k-means
runs on the HIP kernels (tvae.cluster.kmeans), and so does Ward agglomerative clustering (tvae.cluster.ward_linkage;
TVAE_WARD=host selects the reference's sklearn path).
New optional flags: --seed, --n-init, --out-dir.  Besides results.txt the run writes latents.npy, rotations.npy,
translations.npy and clusters.npy.

TVAE_FIGURES=1 adds the last step of the reference scripts: the t-SNE of the latents (tvae.tsne on the GPU, exact
repulsion, seeded by --seed; saved as tsne.npy and tsne.jpg) and the figures of tvae.figures under the reference's file
names -- confusion_matrix.jpg (mnist, dsprites), z_vals.jpg (galaxy with --z-dim 2; written INTO the output directory,
the reference drops the path separator there), the three predicted_*_vals.jpg histograms (particles).  Without
matplotlib tsne.npy is still written and stderr says that the figures were skipped.  With the switch unset a run is
what it was before the figures existed, the line on stderr that says so included.

TVAE_CLASS_AVERAGES=1 adds the step after the reference scripts: every image resampled into the canonical frame with its
predicted rotation and translation and averaged per cluster on the GPU (tvae.align) -- class_averages.npy
([K][C][n][n]), class_counts.npy, class_averages.mrcs for particles and the montage class_averages.jpg when matplotlib is
present.  class_averages.py computes the same from the saved .npy files alone.  Unset, nothing changes.

TVAE_CLASS_FRC=1 measures those averages (tvae.resolution): the two half-set averages and the variance map of every class
in one pass over the images, the Fourier ring correlation of the halves and a resolution per class -- class_halves.npy,
class_variance.npy, class_frc.npy, class_counts.npy ([K][2], the members of each half; it replaces the [K] file of
TVAE_CLASS_AVERAGES=1 when both are set), class_resolution.txt and, with matplotlib, class_frc.jpg and class_variance.jpg.
Both halves share one encoder and one set of poses: not a gold-standard FRC, it reads optimistic.  class_resolution.py
computes the same from the saved .npy files alone.  Unset, nothing changes.

TVAE_REFINE_POSES=1 refines the run's poses against those averages (tvae.refine: every image scored against the average of
its class over a small neighbourhood of angles and whole-pixel shifts, three rounds) -- rotations_refined.npy,
translations_refined.npy, refine_scores.npy and class_averages_refined.npy (.mrcs, .jpg).  refine_poses.py computes the same
from the saved .npy files alone.  Unset, nothing changes.

TVAE_POLISH_POSES=1 polishes the poses to sub-pixel accuracy against the class averages (tvae.polish: a few Levenberg-Marquardt
steps per image on the cosine score, inside a trust region of one pixel and 0.05 rad; it starts from the refined poses when
TVAE_REFINE_POSES=1 is set as well, else from the run's own) -- rotations_polished.npy, translations_polished.npy,
polish_scores.npy, polish_steps.npy and class_averages_polished.npy (.mrcs, .jpg).  polish_poses.py computes the same from the
saved .npy files alone.  Unset, nothing changes.

TVAE_RECLASSIFY=1 reassigns the run's images to their best-matching class average (tvae.classify: every image scored against
its own class and the classes whose latent centroid is nearest, min(K, 8) candidates in all, three rounds of averaging and
reassigning) -- clusters_reclassified.npy, rotations_reclassified.npy, translations_reclassified.npy, classify_scores.npy,
classify_moved.npy, class_scores.npy and class_averages_reclassified.npy (.mrcs, .jpg).  reclassify_particles.py computes
the same from the saved .npy files alone.  Unset, nothing changes.

TVAE_ML_AVERAGES=1 replaces the arg-max of that loop by its maximum-likelihood form (tvae.ml2d: every image contributes to
every class and pose it is compatible with, with its posterior weight; the same min(K, 8) candidates, three rounds, eight
entries per image, the noise variance and the class priors re-estimated every round) -- class_averages_ml.npy (.mrcs, .jpg),
class_weights.npy, clusters_ml.npy, rotations_ml.npy, translations_ml.npy, ml_log_likelihood.npy, ml_sigma2.npy and
ml_entropy.npy.  ml_class_averages.py computes the same from the saved .npy files alone.  Unset, nothing changes.

TVAE_CLASS_EIGEN=1 describes how the members of a class differ from their average (tvae.eigen: the leading eigenimages of
every class under the default soft mask, the coordinates of every image along them and its residual norm) --
class_eigenimages.npy (.mrcs for particles, .jpg with matplotlib), class_eigenvalues.npy, eigen_coordinates.npy,
eigen_residual.npy and class_eigen.txt.  class_eigenimages.py computes the same from the saved .npy files alone.  Unset,
nothing changes.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

from . import cluster, latent, tables

TITLES = {'mnist': 'Cluster the content latents of MNIST / MNIST-N / MNIST-U', 'particles': 'Cluster the content latents of a particle stack',
          'galaxy': 'Cluster the content latents of the galaxy images', 'dsprites': 'Cluster the content latents of dSprites'}


def build_parser(kind: str) -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(TITLES[kind])
    if kind == 'mnist':
        p.add_argument('--dataset', choices=['mnist', 'mnist-U', 'mnist-N'], default='mnist-U')
    elif kind == 'galaxy':
        p.add_argument('--train-path', default='data/galaxy_zoo/galaxy_zoo_train.npy')
        p.add_argument('--test-path', default='data/galaxy_zoo/galaxy_zoo_test.npy')
    elif kind == 'dsprites':
        p.add_argument('--train-path', default='data/dsprites-dataset-master/imgs_train.npy')
        p.add_argument('--test-path', default='data/dsprites-dataset-master/imgs_test.npy')
        p.add_argument('--train-labels', default='./data/dsprites-dataset-master/latent_train.npy')
        p.add_argument('--test-labels', default='./data/dsprites-dataset-master/latent_test.npy')
    p.add_argument('-z', '--z-dim', type=int, default=2)
    if kind == 'dsprites':
        p.add_argument('--inp-channel', type=int, default=1)
    if kind == 'particles':
        p.add_argument('--test-path', help='stack to cluster (.npy, .mrc or .mrcs)')
    p.add_argument('--path-to-encoder', help='whole-module checkpoint of the trained encoder (inference.sav)')
    if kind == 'mnist':
        p.add_argument('--path-to-mnist-test', default='./data/MNIST/processed/test.pt')
    if kind == 'particles':
        p.add_argument('--path-to-transformations',
                       help='.npy with the ground-truth rotation in the first column and the x, y translations in the next two')
    p.add_argument('--t-inf', default='attention', choices=['unimodal', 'attention'])
    p.add_argument('--r-inf', default='attention+offsets', choices=['unimodal', 'attention', 'attention+offsets'])
    p.add_argument('--clustering', default='k-means' if kind in ('mnist', 'dsprites') else 'agglomerative',
                   choices=['agglomerative', 'k-means'])
    p.add_argument('--n-clusters', default=10, type=int)
    if kind == 'particles':
        p.add_argument('--normalize', action='store_true')
        p.add_argument('--crop', default=0, type=int)
    p.add_argument('--in-channels', type=int, default=3 if kind == 'galaxy' else 1)
    if kind == 'mnist':
        p.add_argument('--image-dim', type=int, default=50)
    p.add_argument('--activation', choices=['tanh', 'leakyrelu'], default='leakyrelu')
    p.add_argument('--minibatch-size', type=int, default=100)
    p.add_argument('-d', '--device', type=int, default=0)
    # additions (do not change any reference flag)
    p.add_argument('--seed', type=int, default=None, help='seed of the k-means++ initialisation (reference: unseeded)')
    p.add_argument('--n-init', type=int, default=100, help='k-means restarts (the reference hard-codes 100)')
    p.add_argument('--out-dir', default=None, help='where results.txt and the .npy files go (default: the directory '
                                                   'of the encoder, as in the reference)')
    return p


def _load_stack(path):
    if path.endswith('mrc') or path.endswith('mrcs'):
        from src import mrc
        return np.asarray(mrc.open_stack(path)[0], dtype=np.float32)
    return np.load(path)


def _load(kind, args):
    """-> (images float tensor (N, Cin, n, m), labels or None, ground truth (r_gt, t_gt) | path | None)."""
    if kind == 'mnist':
        n = args.image_dim
        if args.dataset == 'mnist':
            try:
                import torchvision
            except ImportError as e:
                raise SystemExit('--dataset mnist needs torchvision (not installed here); use mnist-U / mnist-N '
                                 '(.npy) or --synthetic') from e
            ds = torchvision.datasets.MNIST('data/', train=False, download=True)
            arr = np.stack([np.asarray(ds[i][0]) for i in range(len(ds))]).astype(np.uint8)
            truth = None                                   # no transformation on standard MNIST
        else:
            sub = {'mnist-U': 'mnist_U', 'mnist-N': 'mnist_N'}[args.dataset]
            arr = np.load(f'data/{sub}/images_test.npy')
            truth = f'data/{sub}/transforms_test.npy'
        images = (torch.from_numpy(arr).float() / 255).view(-1, 1, n, n)
        labels = torch.load(args.path_to_mnist_test, weights_only=False)[1]
        return images, np.asarray(labels), truth
    if kind == 'particles':
        if not args.test_path:
            raise SystemExit('please provide the test_path')
        a = np.asarray(_load_stack(args.test_path), dtype=np.float32)
        if args.crop > 0:
            si, sj = (a.shape[-2] - args.crop) // 2, (a.shape[-1] - args.crop) // 2     # src/image.py: one offset per axis
            a = a[..., si:si + args.crop, sj:sj + args.crop]
            print('# cropped to:', args.crop, file=sys.stderr)
        if args.normalize:                                  # per-image mean / std, as train_particles applies it
            print('# normalizing particles', file=sys.stderr)
            f = a.reshape(a.shape[0], -1)
            a = (a - f.mean(1)[:, None, None]) / f.std(1)[:, None, None]
        n, m = a.shape[1:]
        images = torch.from_numpy(np.ascontiguousarray(a)).float().view(-1, 1, n, m)
        return images, None, args.path_to_transformations
    a = np.concatenate((np.load(args.train_path), np.load(args.test_path)))
    images = torch.from_numpy(a).float()
    if kind == 'galaxy':
        n, m = images.shape[1:3]
        return images.view(-1, args.in_channels, n, m), None, None
    lab = np.concatenate((np.load(args.train_labels), np.load(args.test_labels)))
    n, m = images.shape[1:]
    # the shape column is the class the reference reads for the accuracy; columns 3 and 4: are rotation and translation
    return images.view(-1, args.in_channels, n, m), lab[:, 1], (lab[:, 3:4], lab[:, 4:])


def _figures(kind, args, out_dir, z_values, rot_pred, tr_pred, clusters, y_labels, mapping):
    """TVAE_FIGURES=1: tsne.npy and the figures of the reference script `kind` (module docstring)."""
    from . import tsne as tsne_mod
    try:
        from . import figures
        figures._plt()
    except ImportError as e:
        figures = None
        print('# matplotlib is not available ({}): the figures are skipped, tsne.npy is still written'.format(e),
              file=sys.stderr)
    print('# saving tsne figure ... ', file=sys.stderr)
    if z_values.shape[0] > 30:
        res = tsne_mod.tsne(z_values.float().contiguous(), learning_rate=200.0, seed=args.seed)
        emb = res.embedding.cpu().numpy()
        print('# t-SNE on the GPU: {} iterations, KL divergence {}'.format(res.n_iter, res.kl_divergence), file=sys.stderr)
        np.save(os.path.join(out_dir, 'tsne.npy'), emb)
        if figures is not None:
            # as the reference: coloured by the true labels (mnist, dsprites), one colour for particles.  Its galaxy script
            # names labels it never loads; the clusters colour that scatter here
            colour = y_labels if y_labels is not None else (None if kind == 'particles' else clusters)
            figures.save_tsne(out_dir, emb, None if colour is None else np.asarray(colour))
    else:
        print('# t-SNE skipped: perplexity 30 needs more than 30 points, there are {}'.format(z_values.shape[0]),
              file=sys.stderr)
    if figures is None:
        return
    if kind in ('mnist', 'dsprites') and y_labels is not None:
        print('# saving confusion matrix ... ', file=sys.stderr)
        figures.save_confusion_matrix(out_dir, np.asarray(y_labels), clusters, mapping[1])
    if kind == 'galaxy' and args.z_dim == 2:
        figures.save_z_vals(out_dir, z_values.cpu().numpy(), clusters)
    if kind == 'particles':
        print('# saving histograms ... ', file=sys.stderr)
        figures.save_histograms(out_dir, rot_pred.cpu().numpy(), tr_pred.cpu().numpy())


def _step_inputs(switch, args, images, device, rot_pred, tr_pred, clusters):
    """What every step after the clustering works from: -> (y, theta, dx, clusters, K, t), the preprocessed images the encoder
    saw on the device and the run's own rotations, translations, clusters, --n-clusters and translation scale."""
    from . import align
    if images.shape[-1] != images.shape[-2]:
        raise SystemExit('{}=1 needs square images, these are {} x {}'.format(switch, *images.shape[-2:]))
    return (images.to(device).float().contiguous(), rot_pred.float().contiguous(), tr_pred.float().contiguous(),
            np.asarray(clusters), args.n_clusters, align.translation_scale(args.t_inf))


def _class_averages(kind, args, out_dir, *run_):
    """TVAE_CLASS_AVERAGES=1: the aligned class averages of the run (tvae.align)."""
    from . import align
    print('# saving aligned class averages ... ', file=sys.stderr)
    y, th, d, lab, K, t = _step_inputs('TVAE_CLASS_AVERAGES', args, *run_)
    avg, counts = align.class_averages(y, th, d, lab, K, t)
    align.save_outputs(out_dir, avg.cpu().numpy(), counts.cpu().numpy(), particles=kind == 'particles')


def _class_frc(kind, args, out_dir, *run_):
    """TVAE_CLASS_FRC=1: half-set averages, variance maps, ring correlation and resolution of the run's classes
    (tvae.resolution)."""
    from . import resolution
    print('# saving class half sets, variance maps and FRC ({}) ... '.format(resolution.NOTE), file=sys.stderr)
    y, th, d, lab, K, t = _step_inputs('TVAE_CLASS_FRC', args, *run_)
    resolution.save_outputs(out_dir, resolution.class_resolution(y, th, d, lab, K, t))


def _class_eigen(kind, args, out_dir, *run_):
    """TVAE_CLASS_EIGEN=1: eigenimages, coordinates and residual norms of the run's classes (tvae.eigen with the defaults of
    class_eigenimages.py)."""
    from . import eigen
    print('# saving class eigenimages, coordinates and residual norms ... ', file=sys.stderr)
    y, th, d, lab, K, t = _step_inputs('TVAE_CLASS_EIGEN', args, *run_)
    eigen.save_outputs(out_dir, eigen.class_eigenimages(y, th, d, lab, K, t_scale=t), particles=kind == 'particles')


def _refine_poses(kind, args, out_dir, *run_):
    """TVAE_REFINE_POSES=1: the run's poses refined against its class averages (tvae.refine, three rounds with the defaults
    of refine_poses.py) and the averages of the refined poses.  -> the refined (theta, dx)."""
    from . import align, refine
    print('# refining the poses against the class averages ... ', file=sys.stderr)
    y, th0, d0, lab, K, t = _step_inputs('TVAE_REFINE_POSES', args, *run_)
    th, d, hist = refine.refine_rounds(y, th0, d0, lab, K, t)
    avg, counts = align.class_averages(y, th, d, lab, K, t)
    refine.save_outputs(out_dir, th, d, hist, avg, counts, kind == 'particles', th0.shape)
    return th, d


def _polish_poses(kind, args, out_dir, *run_, start=None):
    """TVAE_POLISH_POSES=1: the poses polished to sub-pixel accuracy against the class averages (tvae.polish, one round with the
    defaults of polish_poses.py) and the averages of the polished poses.  `start`: the refined poses (theta, dx) where
    TVAE_REFINE_POSES=1 ran before, else the run's own."""
    from . import align, polish
    print('# polishing the poses against the class averages ... ', file=sys.stderr)
    y, th0, d0, lab, K, t = _step_inputs('TVAE_POLISH_POSES', args, *run_)
    rot_shape = th0.shape                                     # (of the run's rotations, whatever the start is)
    if start is not None:
        th0, d0 = start
    th, d, hist = polish.polish_rounds(y, th0, d0, lab, K, t)
    avg, counts = align.class_averages(y, th, d, lab, K, t)
    polish.save_outputs(out_dir, th, d, hist, avg, counts, kind == 'particles', rot_shape)


def _reclassify(kind, args, out_dir, *run_, z_values):
    """TVAE_RECLASSIFY=1: the run's images reassigned to their best-matching class average (tvae.classify, three rounds with
    the defaults of reclassify_particles.py, the candidates from the run's latents with m = min(K, 8)) and the averages of the
    new labels and poses."""
    from . import align, classify
    print('# reassigning the images to their best-matching class averages ... ', file=sys.stderr)
    y, th0, d0, lab, K, t = _step_inputs('TVAE_RECLASSIFY', args, *run_)
    new, th, d, hist = classify.classify_rounds(y, th0, d0, lab, K, t, latents=z_values, candidates=min(K, 8))
    avg, counts = align.class_averages(y, th, d, new.cpu().numpy(), K, t)
    classify.save_outputs(out_dir, new, th, d, hist, avg, counts, kind == 'particles', th0.shape)


def _ml_averages(kind, args, out_dir, *run_, z_values):
    """TVAE_ML_AVERAGES=1: the maximum-likelihood class averages of the run (tvae.ml2d, three rounds with the defaults of
    ml_class_averages.py, the candidates from the run's latents with m = min(K, 8)), the labels and top-1 poses they imply."""
    from . import ml2d
    print('# maximum-likelihood class averages: soft assignment over classes and poses ... ', file=sys.stderr)
    y, th0, d0, lab, K, t = _step_inputs('TVAE_ML_AVERAGES', args, *run_)
    avg, wsum, new, th, d, hist = ml2d.ml_rounds(y, th0, d0, lab, K, t, latents=z_values, candidates=min(K, 8))
    ml2d.save_outputs(out_dir, avg, wsum, new, th, d, hist, kind == 'particles', th0.shape)


def run(kind: str, argv=None):
    args = build_parser(kind).parse_args(argv)
    from src import models  # noqa: F401     (whole-module checkpoints unpickle as src.models.*)
    if not args.path_to_encoder:
        raise SystemExit('please provide --path-to-encoder')
    if not torch.cuda.is_available() or args.device == -1:
        raise SystemExit('the MI355X build has no CPU compute path (reference CPU mode -d -1 is not available)')
    images, y_labels, truth = _load(kind, args)
    torch.cuda.set_device(args.device)
    device = torch.device('cuda', args.device)
    print('# using device:', device, file=sys.stderr)
    n, m = images.shape[-2:]
    x_coord = torch.from_numpy(tables.image_coords(n, m)).to(device)
    t_inf, r_inf = args.t_inf, args.r_inf
    print('# clustering with z-dim:', args.z_dim, file=sys.stderr)
    print('# translation inference is {}'.format(t_inf), file=sys.stderr)
    print('# rotation inference is {}'.format(r_inf), file=sys.stderr)
    path_to_encoder = args.path_to_encoder
    encoder = torch.load(path_to_encoder, weights_only=False).to(device)
    encoder.eval()
    out_dir = args.out_dir if args.out_dir is not None else (os.path.dirname(path_to_encoder) or '.')
    os.makedirs(out_dir, exist_ok=True)

    mb = args.minibatch_size
    z_values, rot_pred, tr_pred = latent.extract_latents(images, encoder, x_coord, t_inf, r_inf, mb, device)
    if z_values.shape[1] != 2 * args.z_dim:
        raise SystemExit(f'--z-dim {args.z_dim} does not match the encoder (z-dim {z_values.shape[1] // 2})')

    rot_corr = tr_corr = None
    if kind == 'mnist' and args.dataset != 'mnist':
        # the digits of plain MNIST are slightly rotated and shifted themselves: the prediction on the untransformed test
        # set is subtracted before the correlation (clustering_mnist.py:331-354)
        print('# calculating the correlation for the rotation and translation ... ', file=sys.stderr)
        plain = torch.load(args.path_to_mnist_test, weights_only=False)[0] / 255
        pad = (n - plain[0].shape[1]) // 2
        plain = torch.nn.functional.pad(plain, (pad, pad, pad, pad)).view(-1, 1, n, n)
        _, rot0, tr0 = latent.extract_latents(plain, encoder, x_coord, t_inf, r_inf, mb, device)
        rot_corr, tr_corr = cluster.measure_correlations(truth, (rot_pred - rot0).cpu(), (tr_pred - tr0).cpu())
    elif kind == 'particles' and truth:
        rot_corr, tr_corr = cluster.measure_correlations(truth, rot_pred.cpu(), tr_pred.cpu())
    elif kind == 'dsprites':
        rot_corr, tr_corr = cluster.measure_correlations(truth[0], truth[1], rot_pred.cpu(), tr_pred.cpu())

    if args.clustering == 'agglomerative':
        # TVAE_WARD=host: the reference's sklearn path on a host copy (needs the N x N matrix); default: the GPU kernels
        on_host = os.environ.get('TVAE_WARD', '') == 'host'
        print('# ward linkage on the host (sklearn)' if on_host else '# ward linkage on the GPU', file=sys.stderr)
        clusters = np.asarray(cluster.agglomerative(z_values.cpu().numpy() if on_host else z_values, args.n_clusters))
    else:
        res = cluster.kmeans(z_values, args.n_clusters, n_init=args.n_init, seed=args.seed)
        clusters = res.labels.cpu().numpy()
        print('# k-means: best of {} restarts is {} (inertia {}, {} iterations)'.format(
            res.all_inertia.numel(), res.best, res.inertia, res.n_iter), file=sys.stderr)
    acc = mapping = None
    if y_labels is not None:
        mapping, acc = cluster.cluster_acc(np.asarray(y_labels), clusters)
    if os.environ.get('TVAE_FIGURES', '') == '1':
        _figures(kind, args, out_dir, z_values, rot_pred, tr_pred, clusters, y_labels, mapping)
    else:
        print('# the t-SNE, confusion-matrix and histogram figures of the reference are not built', file=sys.stderr)
    run_ = (images, device, rot_pred, tr_pred, clusters)      # what _step_inputs takes
    if os.environ.get('TVAE_CLASS_AVERAGES', '') == '1':
        _class_averages(kind, args, out_dir, *run_)
    if os.environ.get('TVAE_CLASS_FRC', '') == '1':
        _class_frc(kind, args, out_dir, *run_)
    if os.environ.get('TVAE_CLASS_EIGEN', '') == '1':
        _class_eigen(kind, args, out_dir, *run_)
    refined = None
    if os.environ.get('TVAE_REFINE_POSES', '') == '1':
        refined = _refine_poses(kind, args, out_dir, *run_)
    if os.environ.get('TVAE_POLISH_POSES', '') == '1':
        _polish_poses(kind, args, out_dir, *run_, start=refined)
    if os.environ.get('TVAE_RECLASSIFY', '') == '1':
        _reclassify(kind, args, out_dir, *run_, z_values=z_values)
    if os.environ.get('TVAE_ML_AVERAGES', '') == '1':
        _ml_averages(kind, args, out_dir, *run_, z_values=z_values)

    np.save(os.path.join(out_dir, 'latents.npy'), z_values.cpu().numpy())
    np.save(os.path.join(out_dir, 'rotations.npy'), rot_pred.cpu().numpy())
    np.save(os.path.join(out_dir, 'translations.npy'), tr_pred.cpu().numpy())
    np.save(os.path.join(out_dir, 'clusters.npy'), clusters)
    with open(os.path.join(out_dir, 'results.txt'), 'w') as f:
        f.write('using the encoder model from {}\n\n'.format(path_to_encoder))
        if acc is not None:
            f.write('The accuracy for clustering is {} \n'.format(acc))
        if rot_corr is not None:
            f.write('The circular correlation for the rotation is {}\n'.format(rot_corr))
            f.write('The Pearson correlation for the x and y values in the translation is {}\n'.format(tr_corr))
    return acc, rot_corr, tr_corr
