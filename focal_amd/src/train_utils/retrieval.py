"""Cross-modal retrieval on the projected embeddings, for eval_retrieval.py [build extension].

The FOCAL loss (models/loss.py) trains the per-modality projected embeddings, cut into a shared and a private half
(models/FOCALModules.py: split_features): the shared halves of two modalities of one window agree, the private halves do not carry that
agreement, and shared / private (and private / private across modalities) are orthogonal.  Retrieval measures the first two on a saved
checkpoint -- query with modality a's embedding of window i, rank all n embeddings of modality b, report where window i lands -- and
`orthogonality` the third.  Positives are same-index pairs; nothing here reads a label.

`cross_modal_ranks` never forms the [n, n] distances: ops.rank_positive counts, inside the distance product's epilogue, the gallery rows
that order before each query's positive under focal_knn_search's exact-fp32 distance and (d2, index) order.  fused=False is the plain
torch form, kept as the measurement's baseline (tools/mb_retrieval.py) and as a cross-check."""
import os
import sys

import torch

_ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "..", ".."))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

from focal_amd import ops  # noqa: E402


def unit_rows(x):
    """Rows over max(norm, 1e-12) in fp32 (F.normalize's clamp): a zero row stays zero."""
    return torch.nn.functional.normalize(x.detach().float(), p=2.0, dim=1, eps=1e-12).contiguous()


@torch.no_grad()
def cross_modal_ranks(a, b, fused=True, chunk=8192):
    """a, b: [n, D] on the device, row i of both from window i.  Returns (ranks, tied, q, t): ranks int64 [n] = 1 + the rows of b ordering
    before b[i] for query a[i] under squared Euclidean distance of the L2-normalised rows (the order of cosine similarity), ties to the
    smaller index; tied int64 [n] = the other rows at exactly the positive's distance (a collapsed projector shows as tied ~ n); q, t the
    normalised fp32 copies that were ranked."""
    if a.dim() != 2 or a.shape != b.shape:
        raise ValueError(f"cross_modal_ranks: need two [n, D] matrices of one shape (got {tuple(a.shape)} and {tuple(b.shape)})")
    q, t = unit_rows(a), unit_rows(b)
    n = q.shape[0]
    t_sq = (t * t).sum(1)
    if fused:
        pos = torch.arange(n, dtype=torch.int32, device=q.device)
        before, tied = ops.rank_positive(q, t, t_sq, pos)
        return before.long() + 1, tied.long(), q, t
    # ops.linear takes an output width that is a multiple of 4: zero rows fill the gallery up and their columns are dropped
    t_pad = t if n % 4 == 0 else torch.cat([t, t.new_zeros(4 - n % 4, t.shape[1])])
    cols = torch.arange(n, device=q.device)
    ranks, ties = [], []
    for lo in range(0, n, chunk):
        qc = q[lo:lo + chunk]
        dots, _ = ops.linear(qc, t_pad, None, compute=torch.float32, y_dtype=torch.float32)  # [chunk, n] = q . t^T
        d2 = ((qc * qc).sum(1, keepdim=True) + t_sq[None, :]) - 2.0 * dots[:, :n]
        p = cols[lo:lo + qc.shape[0]]
        dp = d2.gather(1, p[:, None])
        same = d2 == dp
        ranks.append(((d2 < dp) | (same & (cols[None, :] < p[:, None]))).sum(1) + 1)
        ties.append(same.sum(1) - 1)
    return torch.cat(ranks), torch.cat(ties), q, t


def retrieval_metrics(ranks, tied, ks):
    """{"n", "recall": {k: share of queries with rank <= k}, "mrr", "median_rank", "mean_rank", "mean_tied"} of a rank vector (1-based) and
    its tie counts; sums in float64; the median of an even n is the mean of the two middle ranks.  Pure torch: host tensors are taken as
    they are, device tensors come down in one copy."""
    ranks, tied = torch.as_tensor(ranks), torch.as_tensor(tied)
    n = ranks.numel()
    if n < 1 or tied.numel() != n:
        raise ValueError(f"retrieval_metrics: need n >= 1 ranks and as many tie counts (got {n} and {tied.numel()})")
    ks = [int(k) for k in ks]
    r = ranks.reshape(-1).to(torch.float64)
    srt = r.sort().values
    median = (srt[(n - 1) // 2] + srt[n // 2]) / 2
    parts = [(r <= k).to(torch.float64).sum() / n for k in ks]
    parts += [(1.0 / r).sum() / n, median, r.sum() / n, tied.reshape(-1).to(torch.float64).sum() / n]
    host = torch.stack(parts).cpu().tolist()
    return {"n": n, "recall": dict(zip(ks, host[:len(ks)])), "mrr": host[-4], "median_rank": host[-3], "mean_rank": host[-2],
            "mean_tied": host[-1]}


def orthogonality(proj, modalities):
    """The cosines the loss's orthogonality term sees, in float64 on the device from the un-normalised halves of proj = {mod: [n, 2h]}:
    {"shared_private": {mod: (mean cos, mean max(0, cos))}, "private_private": {(a, b): (mean cos, mean max(0, cos))}} over the
    modalities and the unordered pairs a before b.  mean max(0, cos) is what CosineEmbeddingLoss(target = -1) penalises.  One copy to
    the host."""
    cos = torch.nn.functional.cosine_similarity
    modalities = list(modalities)
    keys, parts = [], []
    halves = {}
    for mod in modalities:
        x = proj[mod].detach().to(torch.float64)
        h = x.shape[1] // 2
        halves[mod] = (x[:, :h], x[:, h:2 * h])
    for mod in modalities:
        c = cos(halves[mod][0], halves[mod][1], dim=1)
        keys.append(("shared_private", mod))
        parts += [c.mean(), c.clamp_min(0).mean()]
    for i, a in enumerate(modalities):
        for b in modalities[i + 1:]:
            c = cos(halves[a][1], halves[b][1], dim=1)
            keys.append(("private_private", (a, b)))
            parts += [c.mean(), c.clamp_min(0).mean()]
    host = torch.stack(parts).cpu().tolist()
    out = {"shared_private": {}, "private_private": {}}
    for i, (kind, key) in enumerate(keys):
        out[kind][key] = (host[2 * i], host[2 * i + 1])
    return out
