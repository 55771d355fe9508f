"""The temporal constraint of the FOCAL loss, measured on a whole split, for eval_temporal.py [build extension].

The loss's fourth term (models/loss.py: forward_temporal_inter_ranking_loss) asks that the windows of one subsequence lie closer to each
other than to the windows of any other subsequence, by `inter_rank_margin`: with Dbar(a, b) the mean Euclidean distance between the
windows of sequences a and b (the diagonal block without its own diagonal), its value is the mean over a != b of
max(0, Dbar(a, a) - Dbar(a, b) + margin).  During training only one batch sees it.  Here rows k L .. k L + L - 1 of z are subsequence k.

`sequence_ranking` never forms the [n, n] distances or the [S, S] block means: ops.seq_rank pools each LDS distance tile of
focal_knn_search's exact-fp32 product into L x L blocks and compares each pooled value with its row sequence's thresholds.  fused=False
is the plain torch form, kept as the measurement's baseline (tools/mb_temporal.py) and as a cross-check; it also runs on host tensors.
`neighbour_ranks` asks the per-window question: where does a window's nearest sibling land among all other windows."""
import math
import os
import sys

import torch

_ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "..", ".."))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

from focal_amd import _lib, ops  # noqa: E402

SEQ_LENGTHS = _lib.SEQRANK_LENGTHS
FNS = tuple(_lib.SEQRANK_FNS)
CHUNK = 8192


@torch.no_grad()
def sequence_ranking(z, seq_len, margin, fused=True, slices=None, fn="dist", chunk=CHUNK):
    """z: [n, D], n = S L, rows a L .. a L + L - 1 = sequence a.  With f = sqrt (fn="dist", the loss's distance) or the identity
    (fn="sqdist") of max(d2, 0) and P(a, b) the sum of f over the L x L block of sequences a and b, returns the dict
    intra_d2 [n, L] (d2 of every window to its sequence's windows), intra_sum [S] (the sum of f over i != j in a), before [S] (the b != a
    with P(a, b) (L^2 - L) < intra_sum[a] L^2: another sequence nearer, on average, than the sequence is to itself), viol [S] (the same
    with margin L^2 (L^2 - L) on the right: the loss's hinge active), hinge_sum [S] (the sum over b != a of max(0, intra_sum[a] / (L^2 -
    L) - P(a, b) / L^2 + margin)) and inter_sum [S] (the sum over b != a of P(a, b)).  A NaN pooled value is not counted and makes the two
    sums NaN.  fused=True: z fp32 on the device, ops.seq_rank.  fused=False: torch.cdist in chunks of at most `chunk` query rows, in z's
    dtype and on z's device."""
    L = int(seq_len)
    if z.dim() != 2:
        raise ValueError(f"sequence_ranking: need an [n, D] matrix (got {tuple(z.shape)})")
    n = z.shape[0]
    if fused:
        z = z.detach().float().contiguous()
        return ops.seq_rank(z, (z * z).sum(1), L, float(margin), fn=fn, slices=slices)
    if L not in SEQ_LENGTHS or n % L or n // L < 2:
        raise ValueError(f"sequence_ranking: need seq_len in {SEQ_LENGTHS}, n % seq_len == 0 and at least 2 sequences (got n={n} "
                         f"seq_len={L})")
    if fn not in FNS:
        raise ValueError(f"sequence_ranking: fn is one of {', '.join(FNS)} (got {fn})")
    z = z.detach()
    if not z.is_floating_point():
        z = z.float()
    S, L2, L2L = n // L, float(L * L), float(L * L - L)
    z_sq = (z * z).sum(1)
    step = max(L, min(int(chunk), CHUNK) // L * L)
    eye = torch.eye(L, dtype=torch.bool, device=z.device)
    out = {k: [] for k in ("intra_d2", "intra_sum", "before", "viol", "hinge_sum", "inter_sum")}
    for lo in range(0, n, step):
        zc = z[lo:lo + step]
        c = zc.shape[0]
        if fn == "dist":
            # (on the host the differences themselves: the matrix-product form loses half the digits of a small distance)
            f = torch.cdist(zc, z, compute_mode="use_mm_for_euclid_dist_if_necessary" if z.is_cuda else "donot_use_mm_for_euclid_dist")
        else:
            f = ((z_sq[lo:lo + c, None] + z_sq[None, :]) - 2.0 * (zc @ z.t())).clamp_min(0)
        blocks = f.view(c // L, L, S, L)
        own = torch.arange(lo // L, lo // L + c // L, device=z.device)
        diag = blocks[torch.arange(c // L, device=z.device), :, own, :]  # [c / L, L, L]
        out["intra_d2"].append((diag * diag if fn == "dist" else diag).reshape(c, L))
        intra = diag.masked_fill(eye, 0).sum((1, 2))
        P = blocks.sum((1, 3))  # [c / L, S]
        other = torch.ones_like(P, dtype=torch.bool)
        other[torch.arange(c // L, device=z.device), own] = False
        thr = intra[:, None] * L2
        out["before"].append(((P * L2L < thr) & other).sum(1).to(torch.int32))
        thr_v = thr + float(margin) * (L2 * L2L)
        out["viol"].append(((P * L2L < thr_v) & other).sum(1).to(torch.int32))
        hinge = (thr_v - P * L2L).clamp_min(0)  # the hinge times L^2 (L^2 - L), as the kernel carries it
        scaled = torch.where(other, hinge, torch.zeros_like(hinge)).sum(1)
        out["hinge_sum"].append(scaled / torch.full_like(scaled, L2 * L2L))  # (a tensor divisor: a true division, as the kernel's)
        out["inter_sum"].append(torch.where(other, P, torch.zeros_like(P)).sum(1))
        out["intra_sum"].append(intra)
    return {k: torch.cat(v) for k, v in out.items()}


def temporal_metrics(rank, seq_len):
    """The split's numbers from sequence_ranking's per-sequence tensors, in float64 on the host after one read per tensor:
    {"sequences", "ranking_loss" = sum hinge_sum / (S (S - 1)), the loss term's own value over the whole split; "margin_satisfied" = 1 -
    sum viol / (S (S - 1)); "ordered" = 1 - sum before / (S (S - 1)); "mean_intra", "mean_inter" (of f over the pairs of windows within
    and across sequences) and "ratio" = mean_intra / mean_inter}."""
    L = int(seq_len)
    host = {k: torch.as_tensor(rank[k]).detach().cpu().to(torch.float64) for k in ("hinge_sum", "viol", "before", "intra_sum", "inter_sum")}
    S = host["hinge_sum"].numel()
    if S < 2 or any(v.numel() != S for v in host.values()):
        raise ValueError(f"temporal_metrics: need the per-sequence tensors of S >= 2 sequences (got {[v.numel() for v in host.values()]})")
    pairs = float(S) * (S - 1)
    mean_intra = float(host["intra_sum"].sum()) / (S * float(L * L - L))
    mean_inter = float(host["inter_sum"].sum()) / (pairs * L * L)
    return {"sequences": S, "ranking_loss": float(host["hinge_sum"].sum()) / pairs,
            "margin_satisfied": 1.0 - float(host["viol"].sum()) / pairs, "ordered": 1.0 - float(host["before"].sum()) / pairs,
            "mean_intra": mean_intra, "mean_inter": mean_inter,
            "ratio": mean_intra / mean_inter if mean_inter != 0 else math.nan}


def _orders_before(a, b):
    """a before b in the search's order of distances: a NaN orders behind every number (and -0 == +0)."""
    return (a < b) | (~torch.isnan(a) & torch.isnan(b))


def _same_key(a, b):
    return (a == b) | (torch.isnan(a) & torch.isnan(b))


def nearest_siblings(intra_d2, seq_len):
    """pos int64 [n] on the host: each window's nearest OTHER window of its own sequence by intra_d2 [n, L], ties to the smaller index."""
    L = int(seq_len)
    d = torch.as_tensor(intra_d2).detach().cpu()
    n = d.shape[0]
    if d.dim() != 2 or d.shape[1] != L or n % L or L < 2:
        raise ValueError(f"nearest_siblings: need intra_d2 [n, {L}] with n % {L} == 0 (got {tuple(d.shape)})")
    me = torch.arange(n) % L
    best = torch.full((n,), -1, dtype=torch.int64)
    best_d = torch.full((n,), math.nan, dtype=d.dtype)
    for c in range(L):
        better = (me != c) & ((best < 0) | _orders_before(d[:, c], best_d))
        best = torch.where(better, torch.full_like(best, c), best)
        best_d = torch.where(better, d[:, c], best_d)
    return torch.arange(n) - me + best


@torch.no_grad()
def neighbour_ranks(z, seq_len, intra_d2, slices=None):
    """Where each window's nearest sibling (nearest_siblings) lands among the n - 1 OTHER windows ranked for that window under
    focal_knn_search's distance and (d2, index) order.  ops.rank_positive(q = t = z) counts the rows before the positive, the window
    itself among them when it orders before it; that is decided on the host from the window's own two intra_d2 values (the bits the
    rank kernel sees) and taken out.  Returns (ranks int64 [n], 1-based; tied int64 [n], the other windows at exactly the positive's
    distance; pos int64 [n]), on the host."""
    L = int(seq_len)
    z = z.detach().float().contiguous()
    n = z.shape[0]
    d = torch.as_tensor(intra_d2).detach().cpu()
    pos = nearest_siblings(d, L)
    before, tied = ops.rank_positive(z, z, (z * z).sum(1), pos.to(torch.int32).to(z.device), slices=slices)
    rows = torch.arange(n)
    d_self = d[rows, rows % L]
    d_pos = d[rows, pos % L]
    same = _same_key(d_self, d_pos)
    self_before = _orders_before(d_self, d_pos) | (same & (rows < pos))
    ranks = before.cpu().long() - self_before.long() + 1
    return ranks, tied.cpu().long() - same.long(), pos
