"""The figures of the reference clustering_*.py, drawn from host arrays alone (matplotlib, Agg backend; no GPU, no
seaborn): tsne.jpg, confusion_matrix.jpg, z_vals.jpg and the three histograms of clustering_particles.py.  File names,
figure sizes, colour maps and axis labels are the reference's; every function returns the path it wrote.
"""
from __future__ import annotations

import os

import numpy as np


def _plt():
    import matplotlib
    matplotlib.use('Agg')
    import matplotlib.pyplot as plt
    return plt


def _rainbow_norm(plt):
    from matplotlib import colors
    cmap = plt.cm.rainbow
    return cmap, colors.BoundaryNorm(np.arange(0, 11, 1), cmap.N)


def save_tsne(out_dir, embedding, labels=None):
    """Scatter of the [N][2] embedding coloured by `labels`, with the reference's thin colour bar whose ticks sit in the
    middle of each class; None draws one colour and no bar (what the reference's particles scatter shows: it passes no
    `c`).  The caller chooses: true labels for mnist and dsprites as in the reference, None for particles, the clusters
    for galaxy, whose reference script names labels that it never loads."""
    from mpl_toolkits.axes_grid1 import make_axes_locatable
    plt = _plt()
    Y = np.asarray(embedding)
    fig = plt.figure(figsize=(10, 10))
    cmap, norm = _rainbow_norm(plt)
    if labels is None:
        plt.scatter(Y[:, 0], Y[:, 1], s=2)
    else:
        plt.scatter(Y[:, 0], Y[:, 1], c=np.asarray(labels), cmap=cmap, norm=norm, s=2)
        cax = make_axes_locatable(plt.gca()).append_axes('right', size='2%', pad=0.2)
        cb = plt.colorbar(cax=cax)
        ticks = np.arange(0, 10, 1)
        cb.set_ticks(ticks + .5)
        cb.set_ticklabels(ticks)
    path = os.path.join(out_dir, 'tsne.jpg')
    plt.savefig(path)
    plt.close(fig)
    return path


def confusion_counts(y_true, y_pred):
    """sklearn's confusion_matrix over the sorted union of the labels: rows = true labels, columns = clusters."""
    y_true, y_pred = np.asarray(y_true).astype(np.int64), np.asarray(y_pred).astype(np.int64)
    classes = np.unique(np.concatenate([y_true, y_pred]))
    cm = np.zeros((classes.size, classes.size), dtype=np.int64)
    np.add.at(cm, (np.searchsorted(classes, y_true), np.searchsorted(classes, y_pred)), 1)
    return cm


def save_confusion_matrix(out_dir, y_true, y_pred, mapping_cols=None):
    """Heat map (Blues, annotated counts) of the confusion matrix with its columns permuted by the cluster_acc mapping
    (mapping[1]), so that a good clustering shows on the diagonal.  The permutation is applied when it fits the matrix, as
    it does whenever labels and clusters are numbered from 0 without gaps (the reference's situation)."""
    plt = _plt()
    cm = confusion_counts(y_true, y_pred)
    if mapping_cols is not None and sorted(np.asarray(mapping_cols).tolist()) == list(range(cm.shape[1])):
        cm = cm[:, np.asarray(mapping_cols)]
    n = cm.shape[0]
    fig = plt.figure(figsize=(10, 10))
    ax = plt.gca()
    im = ax.imshow(cm, cmap='Blues')
    plt.colorbar(im, ax=ax, fraction=0.046, pad=0.04)
    half = cm.max() / 2.0 if cm.size else 0
    for r in range(n):
        for c in range(cm.shape[1]):
            ax.text(c, r, format(int(cm[r, c]), 'd'), ha='center', va='center',
                    color='white' if cm[r, c] > half else 'black')
    ax.set_xticks(np.arange(cm.shape[1]))
    ax.set_xticklabels(np.arange(cm.shape[1]))
    ax.set_yticks(np.arange(n))
    ax.set(xlabel='clusters', ylabel='true_labels')
    path = os.path.join(out_dir, 'confusion_matrix.jpg')
    plt.savefig(path)
    plt.close(fig)
    return path


def save_z_vals(out_dir, z_values, clusters):
    """The first two latent coordinates coloured by cluster (clustering_galaxy.py when z_dim == 2)."""
    plt = _plt()
    z = np.asarray(z_values)
    fig = plt.figure(figsize=(10, 10))
    cmap, norm = _rainbow_norm(plt)
    plt.scatter(z[:, 0], z[:, 1], c=np.asarray(clusters), cmap=cmap, norm=norm, s=0.1)
    path = os.path.join(out_dir, 'z_vals.jpg')
    plt.savefig(path)
    plt.close(fig)
    return path


def save_histograms(out_dir, rot_pred, tr_pred):
    """The three histograms of clustering_particles.py: predicted rotation, x and y translation."""
    plt = _plt()
    rot, tr = np.asarray(rot_pred), np.asarray(tr_pred)
    paths = []
    for values, label, name in ((rot.reshape(rot.shape[0], -1), 'predicted rotation angles', 'predicted_rotation_vals.jpg'),
                                (tr[:, 0], 'predicted translation values for x', 'predicted_translation_x_vals.jpg'),
                                (tr[:, 1], 'predicted translation values for y', 'predicted_translation_y_vals.jpg')):
        fig = plt.figure(figsize=(10, 10))
        plt.hist(values)
        plt.xlabel(label)
        plt.ylabel('samples')
        paths.append(os.path.join(out_dir, name))
        plt.savefig(paths[-1])
        plt.close(fig)
    return paths


def save_class_averages(out_dir, averages, counts, name='class_averages.jpg'):
    """Montage of the aligned class averages [K][C][n][n]: one grey panel per class (three channels as RGB scaled to the
    panel's own range, any other number averaged over the channels), titled with the class and its number of members."""
    plt = _plt()
    avg, counts = np.asarray(averages, dtype=np.float64), np.asarray(counts).reshape(-1)
    K = avg.shape[0]
    cols = min(K, 10)
    rows = (K + cols - 1) // cols
    fig, axes = plt.subplots(rows, cols, figsize=(2 * cols, 2.3 * rows), squeeze=False)
    for k, ax in enumerate(axes.ravel()):
        ax.axis('off')
        if k >= K:
            continue
        a = avg[k]
        if a.shape[0] == 3:
            lo, hi = a.min(), a.max()
            ax.imshow(np.moveaxis((a - lo) / (hi - lo) if hi > lo else np.zeros_like(a), 0, -1))
        else:
            ax.imshow(a.mean(0), cmap='gray')
        ax.set_title('{}: {}'.format(k, int(counts[k])), fontsize=9)
    path = os.path.join(out_dir, name)
    plt.savefig(path, bbox_inches='tight')
    plt.close(fig)
    return path


def save_class_frc(out_dir, curves, thresholds=(0.143, 0.5), n=None, apix=None):
    """The ring-correlation curve of every class [K][R] against the spatial frequency (1 / pixel, or 1 / Angstrom with
    `apix`; the ring index without `n`), with a dashed line at every threshold."""
    plt = _plt()
    c = np.asarray(curves, dtype=np.float64)
    K, R = c.shape
    x = np.arange(R, dtype=np.float64)
    label = 'ring'
    if n is not None:
        x, label = x / (n * (apix if apix is not None else 1.0)), '1 / Angstrom' if apix is not None else '1 / pixel'
    fig = plt.figure(figsize=(10, 6))
    cmap = plt.cm.rainbow
    for k in range(K):
        plt.plot(x, c[k], color=cmap(k / max(K - 1, 1)), linewidth=1, label=str(k) if K <= 20 else None)
    for t in thresholds:
        plt.axhline(t, color='k', linestyle='--', linewidth=0.8)
    plt.xlabel('spatial frequency ({})'.format(label))
    plt.ylabel('FRC of the two half-set averages')
    plt.ylim(-0.2, 1.05)
    if K <= 20:
        plt.legend(title='class', fontsize=8)
    path = os.path.join(out_dir, 'class_frc.jpg')
    plt.savefig(path, bbox_inches='tight')
    plt.close(fig)
    return path


def save_class_variance(out_dir, variance, counts):
    """Montage of the per-pixel variance maps [K][C][n][n] (averaged over the channels), one panel per class on its own
    scale, titled with the class and its number of members."""
    plt = _plt()
    var, counts = np.asarray(variance, dtype=np.float64), np.asarray(counts).reshape(-1)
    K = var.shape[0]
    cols = min(K, 10)
    rows = (K + cols - 1) // cols
    fig, axes = plt.subplots(rows, cols, figsize=(2 * cols, 2.3 * rows), squeeze=False)
    for k, ax in enumerate(axes.ravel()):
        ax.axis('off')
        if k >= K:
            continue
        ax.imshow(var[k].mean(0), cmap='magma')
        ax.set_title('{}: {}'.format(k, int(counts[k])), fontsize=9)
    path = os.path.join(out_dir, 'class_variance.jpg')
    plt.savefig(path, bbox_inches='tight')
    plt.close(fig)
    return path


def save_class_eigenimages(out_dir, eigenimages, eigenvalues, counts):
    """Montage of the eigenimages [K][J][C][n][n] (averaged over the channels): one row per class, one panel per component on
    a scale symmetric about 0, titled with the class, the component and its eigenvalue."""
    plt = _plt()
    eig, lam = np.asarray(eigenimages, dtype=np.float64), np.asarray(eigenvalues, dtype=np.float64)
    counts = np.asarray(counts).reshape(-1)
    K, J = eig.shape[:2]
    fig, axes = plt.subplots(K, J, figsize=(2 * J, 2.3 * K), squeeze=False)
    for k in range(K):
        for j in range(J):
            ax = axes[k][j]
            ax.axis('off')
            a = eig[k, j].mean(0)
            top = np.abs(a).max() or 1.0                          # (a zero eigenimage: rank below J)
            ax.imshow(a, cmap='gray', vmin=-top, vmax=top)
            ax.set_title('{} ({}) / {}: {:.3g}'.format(k, int(counts[k]), j, lam[k, j]), fontsize=8)
    path = os.path.join(out_dir, 'class_eigenimages.jpg')
    plt.savefig(path, bbox_inches='tight')
    plt.close(fig)
    return path
