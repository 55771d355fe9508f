"""The yardstick of the t-SNE tests: exact t-SNE restated in numpy, in float64 or -- with dtype=np.float32 -- with every array and every
operation in float32.  The same 64 steps per row as focal_tsne_perplexity (beta = 1; doubled while no upper bound exists, bisected
after; no early exit), a dense q, sklearn's gains / momentum update.  tests/test_eval_tsne_cpu.py pins it to sklearn's own
`_joint_probabilities` and `_kl_divergence`; tests/test_tsne_gpu.py measures the kernels against it."""
import functools

import numpy as np

BISECT_STEPS = 64


@functools.lru_cache(maxsize=None)
def blobs(n, D, C, sep, seed):
    r = np.random.default_rng(seed)
    mu = r.standard_normal((C, D)) * sep
    y = np.arange(n) % C
    X = (mu[y] + r.standard_normal((n, D))).astype(np.float32)
    X.setflags(write=False)
    return X, y


def squared_distances(X, dtype=np.float64):
    X = X.astype(dtype)
    d2 = ((X[:, None, :] - X[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(d2, 0)
    return d2.astype(dtype)


def conditional(d2, perplexity, dtype=np.float64):
    """(conditional matrix p_j|i with a zero diagonal, beta [n]) of squared distances d2 [n, n]."""
    n = d2.shape[0]
    off = ~np.eye(n, dtype=bool)
    d = d2.astype(dtype)
    d = d - np.where(off, d, np.inf).min(1, keepdims=True)
    beta = np.ones((n, 1), dtype)
    lo, hi = np.zeros((n, 1), dtype), np.full((n, 1), np.inf, dtype)
    target = dtype(np.log(perplexity))
    two, half = dtype(2), dtype(0.5)
    with np.errstate(over="ignore", invalid="ignore"):
        for _ in range(BISECT_STEPS):
            p = np.where(off, np.exp(-d * beta), dtype(0))
            sp = p.sum(1, keepdims=True)
            H = np.log(sp) + beta * (d * p).sum(1, keepdims=True) / sp
            up = H > target
            new = np.where(up, np.where(np.isinf(hi), beta * two, (beta + hi) * half), (beta + lo) * half)
            lo, hi = np.where(up, beta, lo), np.where(up, hi, beta)
            beta = new.astype(dtype)
        p = np.where(off, np.exp(-d * beta), dtype(0))
    p = (p / p.sum(1, keepdims=True)).astype(dtype)
    return p, beta[:, 0]


def joint(X, perplexity, dtype=np.float64):
    """(P [n, n], conditional [n, n], beta [n]) of the rows of X."""
    p, beta = conditional(squared_distances(X, dtype), perplexity, dtype)
    n = p.shape[0]
    return ((p + p.T) / dtype(2 * n)).astype(dtype), p, beta


def gradient(Y, P, exaggeration=1.0, dtype=np.float64):
    """The gradient [n, 2] of KL(e P || Q), KL(P || Q), and what the rounding bounds are written in: the per-row sums of |terms| of the
    attraction and of the repulsion (already divided by Z), sum |P log P|, sum P |log q| and Z."""
    Y, P = Y.astype(dtype), P.astype(dtype)
    diff = Y[:, None, :] - Y[None, :, :]
    q = dtype(1) / (dtype(1) + (diff ** 2).sum(-1))
    np.fill_diagonal(q, 0)
    Z = q.sum(dtype=dtype)
    attr = ((P * q)[:, :, None] * diff).sum(1)
    rep = ((q * q)[:, :, None] * diff).sum(1) / Z
    g = dtype(4) * (dtype(exaggeration) * attr - rep)
    pos = P > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        plogp = np.where(pos, P * np.log(np.where(pos, P, 1)), 0)
        plogq = np.where(pos, P * np.log(np.where(q > 0, q, 1)), 0)
    kl = plogp.sum(dtype=dtype) - plogq.sum(dtype=dtype) + np.log(Z)
    sums = {"attr": ((P * q)[:, :, None] * np.abs(diff)).sum(1), "rep": ((q * q)[:, :, None] * np.abs(diff)).sum(1) / Z,
            "plogp": np.abs(plogp).sum(), "plogq": np.abs(plogq).sum(), "Z": Z}
    return g.astype(dtype), dtype(kl), sums


def descend(P, Y0, iters, lr, exaggeration=12.0, exaggeration_iters=250, dtype=np.float64):
    """`iters` iterations of sklearn's update from Y0 with upd = 0 and gains = 1 (momentum 0.5 during exaggeration, 0.8 after)."""
    Y = Y0.astype(dtype).copy()
    upd, gains = np.zeros_like(Y), np.ones_like(Y)
    lr = dtype(lr)
    for it in range(iters):
        e, momentum = (exaggeration, 0.5) if it < exaggeration_iters else (1.0, 0.8)
        g, _, _ = gradient(Y, P, e, dtype)
        inc = upd * g < 0
        gains = np.maximum(np.where(inc, gains + dtype(0.2), gains * dtype(0.8)), dtype(0.01)).astype(dtype)
        upd = (dtype(momentum) * upd - lr * (gains * g)).astype(dtype)
        Y = (Y + upd).astype(dtype)
    return Y
