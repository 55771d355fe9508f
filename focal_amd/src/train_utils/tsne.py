"""Exact t-SNE of un-projected backbone features, for eval_tsne.py [build extension].

`GpuTSNE` is sklearn's `TSNE(method="exact")` with its defaults -- perplexity 30, early exaggeration 12 for 250 iterations at momentum
0.5, then momentum 0.8, learning rate max(n / 12 / 4, 50), gains +0.2 / x0.8 floored at 0.01 -- written for the machine: the joint
probabilities P [n, n] are built once, in one buffer (ops.tsne_affinities), and an iteration is ops.tsne_grad_step: two launches that
read P once, no [n, n] temporary, no allocation and no host read.  Every 50th iteration (and the last) also evaluates KL(P || Q) and the
gradient norm into a device record, which the host then reads as one small copy; the descent stops early only when that norm is at most
`min_grad_norm`.  There is no floating-point atomic on the path: two fits with equal arguments give the same bits.

Deviations from sklearn: each row's beta takes exactly 64 steps (doubling, then bisection) where sklearn stops at an entropy tolerance of
1e-5; the recorded KL is that of P itself at every iteration (sklearn's, during early exaggeration, is that of 12 P); there is no
`n_iter_without_progress` stop.  Exact method only: no Barnes-Hut, and no `transform` for rows that were not fitted."""
import logging
import math
import os
import sys

import torch

_ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "..", ".."))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

from focal_amd import ops  # noqa: E402

CHECK_EVERY = 50    # iterations between two reads of the record (sklearn's n_iter_check)
BISECT_STEPS = 64   # focal_tsne_perplexity's step count


def pca_init(x):
    """[n, 2] float32: the rows of x on the two leading principal components, each component signed so that its largest-magnitude loading
    is positive (sklearn's svd_flip), scaled so that the first column's standard deviation is 1e-4.  The D x D covariance is formed
    where x lives; its eigenvectors are taken in float64 on the host."""
    xc = x.double()
    xc = xc - xc.mean(0, keepdim=True)
    cov = (xc.T @ xc) / max(x.shape[0] - 1, 1)
    _, vec = torch.linalg.eigh(cov.cpu())  # ascending eigenvalues
    comps = vec[:, [-1, -2]].T.contiguous()
    for c in comps:
        if c[c.abs().argmax()] < 0:
            c.neg_()
    y = xc @ comps.T.to(xc.device)
    return (y / y[:, 0].std(unbiased=False) * 1e-4).float().contiguous()


def affinities_torch(x, perplexity):
    """ops.tsne_affinities restated in plain torch ops (cdist, dense exp): the same 64 steps per row.  The baseline of tools/mb_tsne.py
    and a test's cross-check, nothing else.  Returns (P, beta, p_log_p)."""
    n = x.shape[0]
    d2 = torch.cdist(x, x).square_()
    eye = torch.eye(n, dtype=torch.bool, device=x.device)
    d2 -= d2.masked_fill(eye, float("inf")).min(1, keepdim=True).values
    d2.masked_fill_(eye, 0.0)  # (-dmin on the diagonal would overflow the exponential before the mask removes it)
    off = ~eye
    beta = torch.ones(n, 1, device=x.device)
    lo, hi = torch.zeros_like(beta), torch.full_like(beta, float("inf"))
    target = math.log(perplexity)
    for _ in range(BISECT_STEPS):
        p = torch.exp(-d2 * beta) * off
        sp = p.sum(1, keepdim=True)
        H = sp.log() + beta * (d2 * p).sum(1, keepdim=True) / sp
        up = H > target
        lo, hi, prev = torch.where(up, beta, lo), torch.where(up, hi, beta), beta
        beta = torch.where(up, torch.where(torch.isinf(hi), prev * 2, (prev + hi) * 0.5), (prev + lo) * 0.5)
    p = torch.exp(-d2 * beta) * off
    p /= p.sum(1, keepdim=True)
    P = (p + p.T) / (2.0 * n)
    p_log_p = torch.where(P > 0, P.double() * P.double().clamp_min(1e-300).log(), torch.zeros((), dtype=torch.float64, device=x.device)).sum()
    return P, beta[:, 0].contiguous(), p_log_p.view(1)


def grad_step_torch(y, P, p_log_p, upd, gains, lr, momentum, exaggeration, record=None, want_kl=False):
    """ops.tsne_grad_step restated in plain torch ops: cdist, a dense q and two [n, n] x [n, 2] products (float atomics and library
    reductions: two runs may differ)."""
    q = 1.0 / (1.0 + torch.cdist(y, y).square_())
    q.fill_diagonal_(0.0)
    Z = q.double().sum()
    pq = P * q
    attr = pq.sum(1, keepdim=True) * y - pq @ y
    q2 = q * q
    rep = q2.sum(1, keepdim=True) * y - q2 @ y
    g = 4.0 * (exaggeration * attr - rep * (1.0 / Z).float())
    if record is not None:
        record[0] += 1
        if want_kl:
            k = int(record[1].item())
            plq = torch.where(P > 0, P.double() * q.double().clamp_min(1e-300).log(), torch.zeros((), dtype=torch.float64, device=y.device)).sum()
            record[2 + 3 * k:5 + 3 * k] = torch.stack([record[0], p_log_p[0] - plq + Z.log(), g.double().square().sum().sqrt()])
            record[1] += 1
    inc = upd * g < 0
    gains.copy_(torch.where(inc, gains + 0.2, gains * 0.8).clamp_min_(0.01))
    upd.copy_(momentum * upd - lr * (gains * g))
    y += upd
    return y


class GpuTSNE:
    def __init__(self, perplexity=30.0, n_iter=1000, exaggeration=12.0, exaggeration_iters=250, learning_rate="auto", init="pca", seed=0,
                 min_grad_norm=1e-7):
        self.perplexity, self.n_iter, self.exaggeration = float(perplexity), int(n_iter), float(exaggeration)
        self.exaggeration_iters, self.learning_rate, self.init, self.seed = int(exaggeration_iters), learning_rate, init, int(seed)
        self.min_grad_norm = float(min_grad_norm)
        self.embedding_ = self.kl_divergence_ = self.n_iter_ = self.betas_ = self.record_ = None

    def _initial(self, x):
        n = x.shape[0]
        if torch.is_tensor(self.init):
            if tuple(self.init.shape) != (n, 2):
                raise ValueError(f"GpuTSNE: init {tuple(self.init.shape)} is not [{n}, 2]")
            return self.init.detach().to(x.device).float().contiguous().clone()
        if self.init == "pca":
            return pca_init(x)
        if self.init == "random":
            gen = torch.Generator().manual_seed(self.seed)
            return (torch.randn(n, 2, generator=gen) * 1e-4).to(x.device)
        raise ValueError(f"GpuTSNE: init is 'pca', 'random' or a tensor [n, 2] (got {self.init!r})")

    def _lr(self, n):
        if self.learning_rate == "auto":
            return max(n / self.exaggeration / 4.0, 50.0)
        return float(self.learning_rate)

    @torch.no_grad()
    def descend(self, P, p_log_p, y, fused=True, slices=None):
        """`n_iter` iterations from y (changed in place) on the joint probabilities P.  Returns (y, iterations run, record entries
        float64 [k, 3] of (iteration, KL, gradient norm))."""
        n = y.shape[0]
        lr = self._lr(n)
        upd, gains = torch.zeros_like(y), torch.ones_like(y)
        record = ops.tsne_record(self.n_iter // CHECK_EVERY + 1, y.device)
        if fused:
            slices = ops.tsne_default_slices(n, y.device) if slices is None else int(slices)
            ws = ops.tsne_workspace(n, slices, y.device)
        it, entries = 0, None
        while it < self.n_iter:
            early = it < self.exaggeration_iters
            e, momentum = (self.exaggeration, 0.5) if early else (1.0, 0.8)
            it += 1
            check = it % CHECK_EVERY == 0 or it == self.n_iter
            if fused:
                ops.tsne_grad_step(y, P, p_log_p, upd, gains, lr, momentum, e, record=record, want_kl=check, slices=slices, workspace=ws)
            else:
                grad_step_torch(y, P, p_log_p, upd, gains, lr, momentum, e, record=record, want_kl=check)
            if check:
                _, entries = ops.tsne_read_record(record)  # the record's one read
                _, kl, gnorm = entries[-1].tolist()
                logging.info(f"iteration {it}: KL {kl:.5f}, gradient norm {gnorm:.3e}")
                if gnorm <= self.min_grad_norm:
                    break
        return y, it, entries

    @torch.no_grad()
    def fit(self, x, fused=True, slices=None):
        x = x.detach().float().contiguous()
        n, D = x.shape
        ops.tsne_check_limits(n, D, self.perplexity)
        y = self._initial(x)
        P, beta, p_log_p = ops.tsne_affinities(x, self.perplexity) if fused else affinities_torch(x, self.perplexity)
        y, self.n_iter_, self.record_ = self.descend(P, p_log_p, y, fused=fused, slices=slices)
        self.embedding_, self.betas_ = y, beta
        self.kl_divergence_ = float(self.record_[-1, 1].item())
        return self
