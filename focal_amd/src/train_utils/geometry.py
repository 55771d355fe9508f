"""Geometry of an embedding space, for eval_geometry.py [build extension]: the silhouette of the frozen features against the class
labels, the uniformity of the embeddings on the sphere with the alignment of the positive pairs (Wang & Isola, 2020), and the effective
rank (RankMe, Garrido et al., 2023).

Silhouette and uniformity are sums over all n^2 pairs of a function of the distance.  The fused forms never write the [n, n] matrix:
ops.pair_sums adds f(d2) per query row and per group of gallery rows inside the epilogue of focal_knn_search's exact-fp32 distance
product.  fused=False is the plain torch form (torch.cdist in chunks of `chunk` queries: a [chunk, n] fp32 matrix at a time), the
measurement's baseline (tools/mb_geometry.py) and a cross-check; measured (profiles/geometry_fused.txt), the fused uniformity is the
faster one at both shapes and the fused silhouette at 16 384 x 512 but not at 65 536 x 1024, so eval_geometry.py calls the fused
uniformity and the torch silhouette."""
import math
import os
import sys

import torch

_ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "..", ".."))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

from focal_amd import ops  # noqa: E402
from train_utils.retrieval import unit_rows  # noqa: E402


def group_counts(labels, n_groups):
    """Rows per class id 0 .. n_groups - 1 (int64 [n_groups]).  Refused: an id outside that range."""
    labels = labels.reshape(-1).long()
    if labels.numel() and (int(labels.min()) < 0 or int(labels.max()) >= n_groups):
        raise ValueError(f"silhouette: class ids must lie in [0, {n_groups}) (got {int(labels.min())} .. {int(labels.max())})")
    return torch.bincount(labels, minlength=n_groups)


def silhouette_from_sums(S, labels, counts):
    """sklearn's silhouette_samples from S [n, G] = the sum of row i's distances to the rows of each class (its own distance to itself
    left out or zero), the rows' class ids [n] and the class sizes [G], in float64: a = own-class sum / (size - 1), b = the smallest mean
    over the other NON-EMPTY classes, s = (b - a) / max(a, b); the row of a singleton class gets 0, and so does a = b = 0.  Returns
    (s [n] float64, their mean, per-class means [G] float64 with NaN for a class without rows).  With fewer than two classes present
    the silhouette is undefined: every value and the mean are NaN."""
    S = S.to(torch.float64)
    labels = labels.reshape(-1).long().to(S.device)
    counts = counts.reshape(-1).long().to(S.device)
    n, G = S.shape
    if int((counts > 0).sum()) < 2:
        nan = torch.full((n,), float("nan"), dtype=torch.float64, device=S.device)
        return nan, float("nan"), torch.full((G,), float("nan"), dtype=torch.float64, device=S.device)
    own_count = counts[labels]
    a = S.gather(1, labels[:, None]).squeeze(1) / (own_count - 1).clamp_min(1).to(torch.float64)
    means = S / counts.clamp_min(1).to(torch.float64)[None, :]
    inf = torch.full_like(means, float("inf"))
    means = torch.where((counts > 0)[None, :], means, inf)
    means = means.scatter(1, labels[:, None], float("inf"))
    b = means.min(dim=1).values
    top = torch.maximum(a, b)
    s = torch.where(top > 0, (b - a) / top.clamp_min(torch.finfo(torch.float64).tiny), torch.zeros_like(a))
    s = torch.where(own_count > 1, s, torch.zeros_like(s))
    # (a masked column sum, not index_add_: no atomics, so the per-class means repeat bit for bit)
    per_class = (torch.nn.functional.one_hot(labels, G).to(torch.float64) * s[:, None]).sum(0)
    per_class = torch.where(counts > 0, per_class / counts.clamp_min(1).to(torch.float64), torch.full_like(per_class, float("nan")))
    return s, float(s.mean()), per_class


@torch.no_grad()
def class_distance_sums(x, labels, n_groups, fused=True, chunk=8192):
    """S fp32 [n, n_groups]: the sum of the Euclidean distances from row i of x (fp32 [n, D]) to the rows of each class, row i itself left
    out by its index."""
    x = x.detach().float().contiguous()
    labels = labels.reshape(-1)
    n = x.shape[0]
    if fused:
        return ops.pair_sums(x, x, (x * x).sum(1), labels.to(torch.int32).contiguous(), G=n_groups, fn="dist", self_offset=0)
    onehot = torch.nn.functional.one_hot(labels.long(), n_groups).to(torch.float32)
    parts = []
    for lo in range(0, n, chunk):
        dist = torch.cdist(x[lo:lo + chunk], x)  # [chunk, n]
        rows = torch.arange(dist.shape[0], device=x.device)
        dist[rows, lo + rows] = 0.0
        parts.append(dist @ onehot)
    return torch.cat(parts)


@torch.no_grad()
def silhouette(x, labels, n_groups, fused=True, chunk=8192, return_sums=False):
    """The silhouette of the rows of x (fp32 [n, D], on the device) against their class ids (sklearn.metrics.silhouette_samples with the
    Euclidean metric): (per-row values float64 [n], their mean, per-class means float64 [n_groups]); return_sums=True appends the S
    tensor that was scored.  See silhouette_from_sums for the definition's corner cases."""
    counts = group_counts(labels, n_groups)
    S = class_distance_sums(x, labels, n_groups, fused=fused, chunk=chunk)
    out = silhouette_from_sums(S, labels, counts)
    return out + (S,) if return_sums else out


@torch.no_grad()
def gauss_pair_sums(q, t=2.0, fused=True, chunk=8192):
    """S fp32 [n, 1]: per row of q (fp32 [n, D]) the sum over the OTHER rows j of exp(-t |q_i - q_j|^2)."""
    n = q.shape[0]
    if fused:
        return ops.pair_sums(q, q, (q * q).sum(1), None, G=1, fn="gauss", scale=float(t), self_offset=0)
    parts = []
    for lo in range(0, n, chunk):
        d = torch.cdist(q[lo:lo + chunk], q)
        e = torch.exp(-float(t) * d * d)
        rows = torch.arange(e.shape[0], device=q.device)
        e[rows, lo + rows] = 0.0
        parts.append(e.sum(1, keepdim=True))
    return torch.cat(parts)


@torch.no_grad()
def uniformity(z, t=2.0, fused=True, chunk=8192, return_sums=False):
    """Wang & Isola's uniformity of the rows of z on the unit sphere: log mean_{i != j} exp(-t |z_i - z_j|^2) over all ordered pairs, the
    rows made unit length first (unit_rows); the final sum over the rows is taken in float64.  Lower is more uniform; 0 is a collapse
    to one point.  Needs n >= 2 rows.  return_sums=True: (value, S [n, 1])."""
    q = unit_rows(z)
    n = q.shape[0]
    if n < 2:
        raise ValueError(f"uniformity: need n >= 2 rows (got {n})")
    S = gauss_pair_sums(q, t=t, fused=fused, chunk=chunk)
    total = float(S.to(torch.float64).sum())
    value = math.log(total / (float(n) * (n - 1))) if total > 0 else float("-inf") if total == 0 else float("nan")
    return (value, S) if return_sums else value


@torch.no_grad()
def alignment(za, zb):
    """Wang & Isola's alignment (alpha = 2) of the positive pairs: the mean of |za_i - zb_i|^2 over unit rows, in float64."""
    if za.dim() != 2 or za.shape != zb.shape:
        raise ValueError(f"alignment: need two [n, D] matrices of one shape (got {tuple(za.shape)} and {tuple(zb.shape)})")
    a, b = unit_rows(za).to(torch.float64), unit_rows(zb).to(torch.float64)
    return float(((a - b) ** 2).sum(1).mean())


@torch.no_grad()
def effective_rank(x, chunk=8192):
    """RankMe: exp of the entropy of the normalised singular values of the centred rows of x [n, D].  The D x D scatter matrix of the
    centred rows is accumulated in float64 over chunks of rows; its eigenvalues (numpy.linalg.eigvalsh on the host, clipped at 0) are the
    squared singular values.  Between 1 (one direction, or no variation at all) and min(n - 1, D)."""
    import numpy as np
    x = x.detach()
    n, D = x.shape
    mean = torch.zeros(D, dtype=torch.float64, device=x.device)
    for lo in range(0, n, chunk):
        mean += x[lo:lo + chunk].to(torch.float64).sum(0)
    mean /= max(n, 1)
    cov = torch.zeros(D, D, dtype=torch.float64, device=x.device)
    for lo in range(0, n, chunk):
        c = x[lo:lo + chunk].to(torch.float64) - mean
        cov += c.T @ c
    lam = np.clip(np.linalg.eigvalsh(cov.cpu().numpy()), 0.0, None)
    sigma = np.sqrt(lam)
    total = sigma.sum()
    if not total > 0:
        return 1.0
    p = sigma / total
    p = p[p > 0]
    return float(np.exp(-(p * np.log(p)).sum()))
