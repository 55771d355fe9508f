"""Exact t-SNE on the GPU (focal_tsne_*, ops.tsne_affinities / ops.tsne_grad_step, GpuTSNE, eval_tsne.py) against the float64 numpy
restatement of tests/tsne_reference.py -- which tests/test_eval_tsne_cpu.py pins to sklearn's own helpers -- and against sklearn itself.

Data: blobs(n, D, C, sep, seed) of tsne_reference (class means sep * N(0, 1), unit noise, float32).  u = 2^-24 throughout.  Every bound
below is derived, not measured; the measured values are printed and recorded (tests/golden/OBSERVED_tsne.json).

Distances.  focal_tsne_dist is focal_knn_search's function written out, so the check is equality of bits, not a bound.

sum P.  A conditional row is e_j / s with s the fp32 sum of the e_j: its exact sum is off 1 by the summation error of s plus one division
rounding per entry, and any order of adding n terms is within (n - 1) u; the joint matrix adds two roundings (the add, the division by
2n).  So |sum P - 1| <= (n + 3) u, the sum taken in float64 on the host.

Entropy.  The bisection compares the fp32 value of H = log s + beta t / s (t = sum d e) with log(perplexity).  With m = ceil(n / 256) + 10
the depth of the sums (per-thread chain, wave tree, waves in order), B = beta t / s <= H <= ln n and x = beta d: an e_j carries (2 + x_j) u
(product rounding in the exponent, expf), so s is within (2 + B + m) u and t within (3 + m + B + Var(x) / B) u of themselves, and
|dH| <= [(m + 4 + H)(1 + 2 B) + B^2 + Var(x)] u <= eta(n) := 4 (m + ln n + 4)(1 + ln n) u  (Var(x) <~ ln^2 n for these rows).  After 64
steps the bracket is two adjacent floats, whose H differ by 2 Var(x) u, so the final beta has |H - log perplexity| <= eta up to that
term, and every row's exp(H) -- evaluated in float64 from the stored fp32 row, another 2 u (1 + H) -- is within 2 eta of the target,
relatively.

P against float64.  Two sources.  (a) d2: a correct fp32 d2 is within eps_i = 2 D u (|x_i|^2 + max |x|^2) of the float64 one
(tests/test_knn_fused_gpu.py).  At fixed beta that moves log p_j|i by at most 2 beta eps (numerator, normaliser); it moves H by at most
beta^2 eps sigma (sigma^2 = Var_p(d)), which the search undoes with |d beta| <= beta eps / sigma (dH / d beta = -beta sigma^2), moving
log p_j by |d beta| |d_j - mean|.  (b) the entropy's own error eta moves beta by eta / (beta sigma^2).  So
|d p_j|i| <= p_j|i [2 beta eps + (beta eps / sigma + eta / (beta sigma^2)) |d_j - mean_i|] =: E_ij, to first order, and
max |P - P64| <= 2 max (E + E^T) / 2n + 4 u max P (the factor 2 for the second order).  Against sklearn's `_joint_probabilities` the bound
is 5e-5 of max P: about 6x the gap a float32 emulation of this search shows on the CPU (sklearn stops at an entropy tolerance of 1e-5).

Gradient.  g_i = 4 (e A_i - R_i / Z) where A and R cancel heavily, so the bound is per row in the sums of |terms|: SA_i = sum_j P q
|y_i - y_j| and SR_i = sum_j q^2 |y_i - y_j| / Z (per component).  A term carries at most 12 roundings (the difference, the fused square
sum, 1 + ., the division, the products, the fused add), a sum of depth m = ceil(n / 64) + 6 + slices (lane chain, xor tree, slices) m
more; Z is a double sum of such fp32 row sums and 1 / Z is rounded once, which the factor 2 on SR covers.  So
|g_i - g64_i| <= 4 (12 + m) u (e SA_i + 2 SR_i) + 4 u |g64_i|  (the last term: the gradient is read back from the update, upd = -0.8 g).
The recorded norm is within the 2-norm of those bounds.  KL = sum P log P - sum P log q + log Z: a term P log q carries the 6 u of q
plus logf's, a sum its depth, log Z the relative error of Z: |KL - KL64| <= (12 + m) u (sum |P log P| + sum P |log q| + 2).  sklearn's
`_kl_divergence` evaluates sum P log(P Z / q), which carries log Z sum P where the formula above has log Z; the fp32 P sums to 1 within
(n + 3) u, so against sklearn's value the bound grows by |sum P - 1| |log Z|, computed from the same P, and by what sklearn's clamp of P
and q / Z at 2.2e-16 inside the logarithm adds (entries below it exist from n ~ 2000 on), computed likewise.

Trajectories.  Ten iterations from a 1e-4 start are compared with the float64 restatement at 10 x the largest relative gap between the
float32 and float64 numpy restatements on the same P (not below 1e-5), computed here; not beyond ten iterations -- by fifty the two
restatements have nothing in common (the map is chaotic from a 1e-4 start)."""
import copy
import functools
import importlib.util
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import record_observed
from tsne_reference import blobs, descend, gradient, joint, squared_distances

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SRC = os.path.join(ROOT, "focal_amd", "src")
DEV = "cuda"
U = 2.0 ** -24
CASES = {"case1": (300, 32, 5, 1.5, 0), "case2": (257, 36, 4, 1.0, 0)}
AFFINITY_SHAPES = [(2, 4, 1.5), (129, 36, 30.0), (257, 132, 30.0), (300, 36, 30.0)]


@pytest.fixture(scope="module")
def ops():
    from focal_amd import ops as o
    return o


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)  # (a copy: the cached inputs are read-only)


def eta(n):
    return 4 * (math.ceil(n / 256) + 10 + math.log(n) + 4) * (1 + math.log(n)) * U


@functools.lru_cache(maxsize=None)
def gpu_affinities(n, D, perplexity, C=4, sep=1.0, seed=1):
    """(X, P, beta, p_log_p, conditional) for blobs(n, D, C, sep, seed): P float32 on the host, the rest as returned."""
    from focal_amd import ops as o
    X, _ = blobs(n, D, C, sep, seed)
    P, beta, plogp, cond = o.tsne_affinities(dev(X), perplexity, want_conditional=True)
    return X, P, beta, plogp, cond


# ------------------------------------------------------------------------------------------ 1: distances
def test_dist_is_the_search_distance(ops):
    n, D, k = 129, 36, 16
    X, y = blobs(n, D, 4, 1.0, 1)
    x = dev(X)
    d2, x_sq = ops.tsne_dist(x, want_norms=True)
    assert torch.equal(d2.diagonal().view(torch.int32), torch.zeros(n, dtype=torch.int32, device=DEV))  # +0, not -0
    _, nbr_idx, nbr_d2 = ops.knn_search_vote(x, x, x_sq, dev(y.astype(np.int64)), k, 4, want_neighbours=True, slices=2)
    rows = torch.arange(n, device=DEV)
    # the search's own d2(i, i) is whatever the expanded form gives; every other entry of a row is compared, in the search's order
    off = d2.clone()
    off[rows, rows] = float("inf")
    val, idx = torch.sort(off, dim=1, stable=True)  # (stable: equal distances by index, the search's order)
    for i in range(n):
        keep = nbr_idx[i] != i
        assert int(keep.sum()) == k - 1, i
        assert torch.equal(nbr_idx[i][keep].long(), idx[i, :k - 1]), i
        assert torch.equal(nbr_d2[i][keep].view(torch.int32), val[i, :k - 1].view(torch.int32)), i


# ------------------------------------------------------------------------------------------ 2: affinities
@pytest.mark.parametrize("n,D,perplexity", AFFINITY_SHAPES, ids=lambda v: str(v))
def test_affinities(ops, n, D, perplexity):
    X, P, beta, plogp, cond = gpu_affinities(n, D, perplexity)
    assert torch.equal(P.view(torch.int32), P.T.contiguous().view(torch.int32))
    assert not P.diagonal().any() and not cond.diagonal().any()
    Ph, ch = P.cpu().numpy().astype(np.float64), cond.cpu().numpy().astype(np.float64)
    assert (Ph >= 0).all() and np.isfinite(Ph).all()
    total = abs(Ph.sum() - 1)
    record_observed(f"tsne/sum_P_minus_1/n{n}", total)
    print(f"n = {n}: |sum P - 1| = {total:.3e} (bound {(n + 3) * U:.3e})")
    assert total <= (n + 3) * U
    if n == 2:
        assert Ph[0, 1] == 0.5 == Ph[1, 0]
        return
    H = -(np.where(ch > 0, ch * np.log(np.where(ch > 0, ch, 1)), 0)).sum(1)
    perp_gap = np.abs(np.exp(H) / perplexity - 1).max()
    record_observed(f"tsne/perplexity_rel_gap/n{n}", perp_gap)
    print(f"n = {n}: rows' perplexity within {perp_gap:.3e} of {perplexity} (bound {2 * eta(n):.3e})")
    assert perp_gap <= 2 * eta(n)
    # against float64
    d2 = squared_distances(X)
    P64, c64, b64 = joint(X, perplexity)
    sq = (X.astype(np.float64) ** 2).sum(1)
    eps = (2 * D * U * (sq + sq.max()))[:, None]
    off = ~np.eye(n, dtype=bool)
    d = d2 - np.where(off, d2, np.inf).min(1, keepdims=True)
    mean = (c64 * d).sum(1, keepdims=True)
    sigma = np.sqrt((c64 * (d - mean) ** 2).sum(1, keepdims=True))
    b = b64[:, None]
    E = c64 * (2 * b * eps + (b * eps / sigma + eta(n) / (b * sigma ** 2)) * np.abs(d - mean))
    bound = 2 * ((E + E.T) / (2 * n)).max() / P64.max() + 4 * U
    gap = np.abs(Ph - P64).max() / P64.max()
    record_observed(f"tsne/P_against_float64/n{n}", gap)
    print(f"n = {n}: max |P - P64| / max P64 = {gap:.3e} (bound {bound:.3e}); beta within {np.abs(beta.cpu().numpy() / b64 - 1).max():.3e}")
    assert gap <= bound
    # against sklearn
    from scipy.spatial.distance import squareform
    from sklearn.manifold._t_sne import _joint_probabilities
    sk = squareform(_joint_probabilities(d2.astype(np.float32), perplexity, 0))
    sk_gap = np.abs(Ph - sk).max() / sk.max()
    record_observed(f"tsne/P_against_sklearn/n{n}", sk_gap)
    print(f"n = {n}: max |P - sklearn| / max = {sk_gap:.3e} (bound 5e-5)")
    assert sk_gap <= 5e-5
    # sum P log P, the constant of the KL value
    want = np.where(Ph > 0, Ph * np.log(np.where(Ph > 0, Ph, 1)), 0).sum()
    assert abs(float(plogp.item()) - want) <= (12 + 16) * U * abs(want)


# ------------------------------------------------------------------------------------------ 3: gradient and KL
def grad_cases():
    out = []
    for n, D, slices in [(2, 4, 1), (129, 36, 1), (129, 36, 3), (257, 132, 2), (300, 36, 1), (300, 36, 2), (300, 36, 7)]:
        for kind in ("tiny", "spread"):
            for e in (1.0, 12.0):
                out.append((n, D, slices, kind, e))
    # more than one 2048-column chunk, with and without 16-byte loads of P (n % 4)
    out += [(2052, 4, 1, "spread", 1.0), (2052, 4, 2, "tiny", 12.0), (2050, 4, 1, "spread", 12.0), (2050, 4, 3, "tiny", 1.0)]
    return out


@pytest.mark.parametrize("n,D,slices,kind,e", grad_cases(), ids=lambda v: str(v))
def test_gradient_and_kl(ops, n, D, slices, kind, e):
    from scipy.spatial.distance import squareform
    from sklearn.manifold._t_sne import _kl_divergence
    _, P, _, plogp, _ = gpu_affinities(n, D, 30.0 if n > 30 else 1.5)
    r = np.random.default_rng(n + slices)
    Y = (r.standard_normal((n, 2)) * (1e-4 if kind == "tiny" else 10.0)).astype(np.float32)
    y, upd, gains = dev(Y), torch.zeros(n, 2, device=DEV), torch.ones(n, 2, device=DEV)
    record = ops.tsne_record(1, DEV)
    ops.tsne_grad_step(y, P, plogp, upd, gains, 1.0, 0.0, e, record=record, want_kl=True, slices=slices)
    its, entries = ops.tsne_read_record(record)
    assert its == 1 and entries.shape == (1, 3) and entries[0, 0] == 1
    assert torch.equal(gains, torch.full_like(gains, 0.8)) and torch.equal(y, dev(Y) + upd)
    g = (-upd.cpu().numpy().astype(np.float64)) / np.float64(np.float32(0.8))
    P64, Y64 = P.cpu().numpy().astype(np.float64), Y.astype(np.float64)
    sk_kl, sk_g = _kl_divergence(Y64.ravel(), squareform(e * P64, checks=False), 1.0, n, 2)
    g64, kl64, sums = gradient(Y64, P64, e)
    # sklearn's value carries log Z sum P where ours has log Z (P sums to 1 within (n + 3) u), and it raises P and Q = q / Z to 2.2e-16
    # inside the logarithm: both differences are computed here from the same P and Y
    tiny, diff = np.finfo(np.float64).eps, Y64[:, None, :] - Y64[None, :, :]
    Q = 1.0 / (1.0 + (diff ** 2).sum(-1)) / sums["Z"]
    low_p, low_q = (P64 > 0) & (P64 < tiny), (P64 > 0) & (Q < tiny)
    unit = (abs(P64.sum() - 1) * abs(np.log(sums["Z"])) + (P64[low_p] * np.log(tiny / P64[low_p])).sum()
            + (P64[low_q] * np.log(tiny / Q[low_q])).sum()) * (1 + 1e-9)
    if n > 2:  # (n = 2: q / Z = 1/2 exactly, and sklearn's value is that of 12 P)
        assert np.abs(g64 - sk_g.reshape(n, 2)).max() <= 1e-12 * max(np.abs(sk_g).max(), 1e-300)
        if e == 1.0:
            assert abs(kl64 - sk_kl) <= 1e-12 * max(1.0, abs(sk_kl)) + unit
    m = math.ceil(n / 64) + 6 + slices
    bound = 4 * (12 + m) * U * (e * sums["attr"] + 2 * sums["rep"]) + 4 * U * np.abs(g64)
    worst = (np.abs(g - g64) / bound).max()
    kl_bound = (12 + m) * U * (sums["plogp"] + sums["plogq"] + 2)
    kl_gap = abs(entries[0, 1].item() - kl64)
    norm_gap = abs(entries[0, 2].item() - np.linalg.norm(g64))
    key = f"n{n}_s{slices}_{kind}_e{e:g}"
    record_observed(f"tsne/grad_gap_over_bound/{key}", worst)
    record_observed(f"tsne/kl_gap/{key}", kl_gap)
    print(f"{key}: max |g - g64| / bound = {worst:.3e}; |KL - KL64| = {kl_gap:.3e} (bound {kl_bound:.3e}); "
          f"| |g| - |g64| | = {norm_gap:.3e} (bound {np.linalg.norm(bound):.3e})")
    assert worst <= 1.0
    assert kl_gap <= kl_bound
    if n > 2 and e == 1.0:
        assert abs(entries[0, 1].item() - sk_kl) <= kl_bound + unit
    assert norm_gap <= np.linalg.norm(bound)


# ------------------------------------------------------------------------------------------ 4, 6: ten iterations
@functools.lru_cache(maxsize=None)
def ten_iterations(name):
    """P of the case from the GPU, the start, the float64 restatement's map after ten iterations, and the tolerance: 10 x the float32
    restatement's relative gap to it, not below 1e-5."""
    n, D, C, sep, seed = CASES[name]
    X, P, _, plogp, _ = gpu_affinities(n, D, 30.0, C, sep, seed)
    Y0 = (np.random.default_rng(1).standard_normal((n, 2)) * 1e-4).astype(np.float32)
    Ph = P.cpu().numpy()
    lr = max(n / 12.0 / 4.0, 50.0)
    Y64 = descend(Ph.astype(np.float64), Y0, 10, lr)
    Y32 = descend(Ph, Y0, 10, lr, dtype=np.float32)
    gap = np.abs(Y32.astype(np.float64) - Y64).max() / np.abs(Y64).max()
    record_observed(f"tsne/float32_numpy_gap_10_iterations/{name}", gap)
    return P, plogp, Y0, Y64, max(10 * gap, 1e-5), gap


def run_ten(P, plogp, Y0, fused, slices=None):
    from train_utils.tsne import GpuTSNE
    est = GpuTSNE(n_iter=10)
    y, its, entries = est.descend(P, plogp, dev(Y0), fused=fused, slices=slices)
    assert its == 10 and entries.shape == (1, 3) and entries[0, 0] == 10
    return y.cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("slices", [1, 3])
def test_update_rule_ten_iterations(name, slices):
    P, plogp, Y0, Y64, tol, gap32 = ten_iterations(name)
    got = run_ten(P, plogp, Y0, True, slices)
    gap = np.abs(got - Y64).max() / np.abs(Y64).max()
    record_observed(f"tsne/gpu_gap_10_iterations/{name}_s{slices}", gap)
    print(f"{name}, slices {slices}: GPU against float64 after 10 iterations {gap:.3e}; float32 numpy {gap32:.3e}; tolerance {tol:.3e}")
    assert gap <= tol


@pytest.mark.parametrize("name", list(CASES))
def test_fused_against_torch_form(name):
    P, plogp, Y0, _, tol, _ = ten_iterations(name)
    fused, plain = run_ten(P, plogp, Y0, True), run_ten(P, plogp, Y0, False)
    gap = np.abs(fused - plain).max() / np.abs(plain).max()
    record_observed(f"tsne/fused_against_torch_10_iterations/{name}", gap)
    print(f"{name}: fused against torch form after 10 iterations {gap:.3e} (tolerance {tol:.3e})")
    assert gap <= tol


def test_torch_affinities_agree():
    """The baseline's setup is the same search: its P is within the float64 bound's order of the kernels' (both float32)."""
    from train_utils.tsne import affinities_torch
    X, P, beta, plogp, _ = gpu_affinities(300, 36, 30.0)
    Pt, bt, plt = affinities_torch(dev(X), 30.0)
    assert float((Pt - P).abs().max() / P.max()) <= 5e-5 and abs(float(plt.item() - plogp.item())) <= 1e-4


# ------------------------------------------------------------------------------------------ 5: repeatability
def test_two_fits_give_the_same_bits():
    from train_utils.tsne import GpuTSNE
    X, _ = blobs(300, 36, 4, 1.0, 1)
    x = dev(X)
    a, b = GpuTSNE(n_iter=100).fit(x), GpuTSNE(n_iter=100).fit(x)
    assert a.n_iter_ == b.n_iter_ == 100 and a.record_.shape == (2, 3)
    assert torch.equal(a.embedding_.view(torch.int32), b.embedding_.view(torch.int32))
    assert torch.equal(a.betas_.view(torch.int32), b.betas_.view(torch.int32))
    assert torch.equal(a.record_.view(torch.int64), b.record_.view(torch.int64)) and a.kl_divergence_ == b.kl_divergence_
    c = GpuTSNE(n_iter=100).fit(x, slices=3)  # another order of the sums: allowed to differ, not to go wrong
    assert torch.isfinite(c.embedding_).all() and c.record_.shape == (2, 3)
    r = GpuTSNE(n_iter=50, init="random", seed=3).fit(x)
    assert torch.equal(r.embedding_, GpuTSNE(n_iter=50, init="random", seed=3).fit(x).embedding_)
    assert not torch.equal(r.embedding_, GpuTSNE(n_iter=50, init="random", seed=4).fit(x).embedding_)


# ------------------------------------------------------------------------------------------ 7: quality against sklearn
@functools.lru_cache(maxsize=None)
def sklearn_map(name):
    from sklearn.manifold import TSNE, trustworthiness
    X, _ = blobs(*CASES[name])
    est = TSNE(method="exact", init="random", random_state=0, perplexity=30, max_iter=750).fit(X)
    return float(est.kl_divergence_), float(trustworthiness(X, est.embedding_, n_neighbors=5))


@pytest.mark.parametrize("name", list(CASES))
def test_quality_against_sklearn(name):
    from sklearn.manifold import trustworthiness
    from train_utils.tsne import GpuTSNE
    X, _ = blobs(*CASES[name])
    n = X.shape[0]
    Y0 = (np.random.default_rng(1).standard_normal((n, 2)) * 1e-4).astype(np.float32)
    est = GpuTSNE(perplexity=30.0, n_iter=750, init=torch.from_numpy(Y0)).fit(dev(X))
    assert est.n_iter_ == 750
    kl, trust = est.kl_divergence_, float(trustworthiness(X, est.embedding_.cpu().numpy(), n_neighbors=5))
    sk_kl, sk_trust = sklearn_map(name)
    for k, v in (("kl", kl), ("kl_sklearn", sk_kl), ("trustworthiness", trust), ("trustworthiness_sklearn", sk_trust)):
        record_observed(f"tsne/quality/{name}/{k}", v)
    print(f"{name}: KL {kl:.4f} (sklearn {sk_kl:.4f}), trustworthiness {trust:.4f} (sklearn {sk_trust:.4f})")
    assert kl <= 1.10 * sk_kl
    assert trust >= sk_trust - 0.02


# ------------------------------------------------------------------------------------------ 8: limits
def test_limits_name_the_limit(ops):
    from focal_amd import _lib
    import ctypes as C
    g = torch.Generator().manual_seed(0)
    with pytest.raises(_lib.FocalHipError, match=re.escape("D % 4 == 0 (got D=6)")):
        ops.tsne_affinities(torch.randn(40, 6, generator=g).to(DEV), 5.0)
    with pytest.raises(_lib.FocalHipError, match=re.escape("2 <= n <= 32768 (got n=1)")):
        ops.tsne_affinities(torch.randn(1, 8, generator=g).to(DEV), 1.0)
    with pytest.raises(_lib.FocalHipError, match=re.escape("2 <= n <= 32768 (got n=32769)")):
        ops.tsne_check_limits(32769, 8, 30.0)
    ops.tsne_check_limits(32768, 8, 30.0)
    with pytest.raises(_lib.FocalHipError, match=re.escape("1 <= perplexity < n (got perplexity=40.0 n=40)")):
        ops.tsne_affinities(torch.randn(40, 8, generator=g).to(DEV), 40.0)
    with pytest.raises(_lib.FocalHipError, match=re.escape("1 <= perplexity < n")):
        ops.tsne_affinities(torch.randn(40, 8, generator=g).to(DEV), 0.5)
    from train_utils.tsne import GpuTSNE
    with pytest.raises(_lib.FocalHipError, match=re.escape("1 <= perplexity < n (got perplexity=30.0 n=20)")):
        GpuTSNE().fit(torch.randn(20, 8, generator=g).to(DEV))
    # the library refuses the same descriptors before any launch
    lib = _lib.load()
    assert lib.focal_tsne_grad_workspace(C.byref(_lib.TsneDesc(32769, 8, 1))) == 0
    assert lib.focal_tsne_grad_workspace(C.byref(_lib.TsneDesc(1, 8, 1))) == 0
    buf = torch.zeros(64, device=DEV)
    assert lib.focal_tsne_dist(C.byref(_lib.TsneDesc(4, 6, 1)), buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), None) != 0
    assert b"D % 4 == 0" in lib.focal_last_error()
    assert lib.focal_tsne_perplexity(C.byref(_lib.TsneDesc(4, 8, 1)), 4.0, buf.data_ptr(), buf.data_ptr(), None) != 0
    assert b"1 <= perplexity < n" in lib.focal_last_error()


# ------------------------------------------------------------------------------------------ 9: eval_tsne.py
def tsne_entry():
    spec = importlib.util.spec_from_file_location("focal_eval_tsne_entry", os.path.join(SRC, "eval_tsne.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def tsne_parsed(monkeypatch, argv):
    from params.tsne_params import parse_tsne_params
    monkeypatch.setattr(sys, "argv", ["eval_tsne.py"] + argv)
    return parse_tsne_params()


def write_seeded_backbone(args):
    """Name-seeded weights under the name the pretraining loop would use (its checkpoints are the backbone's whole state dict)."""
    from oracle.weights import fill_state_dict_
    from train_utils.model_selection import init_backbone_model
    net = init_backbone_model(copy.copy(args))
    torch.save(fill_state_dict_({k: v.detach().cpu().clone() for k, v in net.state_dict().items()}), args.backbone_weight)


@pytest.mark.parametrize("model", ["DeepSense", "SW_Transformer"])
def test_eval_tsne_end_to_end(monkeypatch, tmp_path, capsys, model):
    """Both backbones on HAR3LOC in fp32.  The last condition -- a second run writes the same bytes -- needs two things: the map of
    equal features repeats bit for bit (asserted on its own just before), and the backbone's evaluation forward repeats bit for bit (the
    features of the two runs are compared exactly).  The second did not hold for SW_Transformer while its mod_in product summed split-K
    partials with fp32 atomics in evaluation passes too (features 7e-07 .. 9e-07 apart between two runs); an evaluation pass now takes
    one k-ordered sum (swin_engine.py)."""
    argv =[f"-model={model}", "-dataset=HAR3LOC", "-learn_framework=FOCAL", f"-model_weight={tmp_path}", "-batch_size=16", "-compute_dtype=fp32",
            "-synthetic_batches=2", "-tsne_iters=60", "-tsne_perplexity=5"]
    first = tsne_parsed(monkeypatch, argv + [f"-tsne_out={tmp_path / 'a.npz'}"])
    assert first.backbone_weight == os.path.join(str(tmp_path), f"HAR3LOC_{model}_pretrain_best.pt")
    assert len(first.dataset_config["location_names"]) > 1 and first.tsne_split == "test"
    write_seeded_backbone(first)
    capsys.readouterr()
    out, kept = tsne_entry().evaluate_tsne(first, keep=True)
    text = capsys.readouterr().out
    n = kept["features"].shape[0]
    assert n == 16 == out["n"] and out["path"] == str(tmp_path / "a.npz")
    m = re.search(rf"t-SNE \(perplexity=5, n={n}, iterations=60\) KL divergence:\s*([-\d.]+)\n", text)
    assert m, text[-2000:]
    est = kept["estimator"]
    last = est.record_[-1]
    assert last[0] == 60 and out["kl"] == float(last[1]) and abs(float(m.group(1)) - out["kl"]) <= 5.1e-6  # five decimals
    z = np.load(out["path"])
    assert sorted(z.files) == ["betas", "embedding", "kl", "labels", "n_iter", "perplexity", "rows"]
    assert z["embedding"].shape == (n, 2) and z["embedding"].dtype == np.float32 and np.isfinite(z["embedding"]).all()
    assert z["labels"].shape == (n,) and np.array_equal(z["labels"], kept["labels"].cpu().numpy())
    assert z["rows"].shape == (n,) and np.array_equal(z["rows"], np.arange(n))  # sorted, unique: every row of the split
    assert z["betas"].shape == (n,) and (z["betas"] > 0).all()
    assert float(z["kl"]) == out["kl"] and float(z["perplexity"]) == 5.0 and int(z["n_iter"]) == 60
    assert np.array_equal(z["embedding"], est.embedding_.cpu().numpy())
    # a second run writes the same bytes
    from train_utils.tsne import GpuTSNE
    again = GpuTSNE(perplexity=5.0, n_iter=60, init="pca", seed=0).fit(kept["features"])  # the map of the same features: the same bits
    assert torch.equal(again.embedding_.view(torch.int32), est.embedding_.view(torch.int32)) and again.kl_divergence_ == out["kl"]
    second = tsne_parsed(monkeypatch, argv + [f"-tsne_out={tmp_path / 'b.npz'}"])
    _, kept2 = tsne_entry().evaluate_tsne(second, keep=True)
    moved = float((kept2["features"] - kept["features"]).abs().max() / kept["features"].abs().max())
    record_observed(f"tsne/end_to_end/{model}/features_rel_gap_between_two_runs", moved)
    print(f"{model}: the backbone's features of two runs differ by {moved:.3e} of their largest entry")
    assert torch.equal(kept2["features"].view(torch.int32), kept["features"].view(torch.int32))
    assert (tmp_path / "a.npz").read_bytes() == (tmp_path / "b.npz").read_bytes()
    if model == "DeepSense":  # a split larger than -tsne_max_rows: a seeded, sorted subset
        third = tsne_parsed(monkeypatch, argv + [f"-tsne_out={tmp_path / 'c.npz'}", "-tsne_max_rows=12", "-tsne_seed=5", "-tsne_init=random"])
        capsys.readouterr()
        out3, kept3 = tsne_entry().evaluate_tsne(third, keep=True)
        assert "t-SNE maps 12 of 16 rows" in capsys.readouterr().out and out3["n"] == 12
        rows = np.load(out3["path"])["rows"]
        assert rows.shape == (12,) and (np.diff(rows) > 0).all() and rows.min() >= 0 and rows.max() < 16
        assert np.array_equal(rows, tsne_entry().subset_rows(16, 12, 5).numpy())
        assert torch.equal(kept3["features"], kept["features"][torch.from_numpy(rows).to(DEV)])
