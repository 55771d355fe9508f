"""The K-means kernels (focal_kmeans_assign / focal_kmeans_update, ops.kmeans_assign / ops.kmeans_update), GpuKMeans and eval_cluster.py.

Bounds (derived, not measured), u = 2^-24.  A centroid element is the fp32 sum of n_k rows in some fixed order, then one division:
|c_gpu - c_f64| <= (n_k - 1) u sum|x_i| / n_k + u |c_f64| to first order.  The expanded-form distance d2 = |x|^2 + |c|^2 - 2 x.c of width
D is off by at most (D + 4) 2^-23 (|x| + |c|)^2 / 2 per row (two norms, a dot product, three more roundings), and the fp32 sum of n of
them by (n - 1) u sum d2; the inertia bound is the sum of the two with the first term doubled, as the issue states it."""
import copy
import ctypes
import functools
import importlib.util
import os
import re
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SRC = os.path.join(ROOT, "focal_amd", "src")
DEV = "cuda"
U = 2.0 ** -24
RANDOM_SEED = 3  # init="random" on the blobs (seeds 0 .. 15 all end in the generating partition there)


@pytest.fixture(scope="module")
def ops():
    from focal_amd import ops as o
    return o


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def bits(t):
    return t.detach().cpu().contiguous().numpy().tobytes()


@functools.lru_cache(maxsize=None)
def normal(n, D, rows_c, seed):
    r = np.random.default_rng(seed)
    return r.standard_normal((n, D)).astype(np.float32), r.standard_normal((rows_c, D)).astype(np.float32)


def assign(ops, x, c, K, **kw):
    c = c.contiguous()
    return ops.kmeans_assign(x, c, (c * c).sum(1), K, want_min_d2=True, **kw)


# ------------------------------------------------------------------------------------------ 1: assignment == knn, bit for bit
@pytest.mark.parametrize("n,D,K", [(1, 4, 1), (129, 36, 7), (257, 32, 2), (300, 132, 64)], ids=lambda v: str(v))
def test_assignment_is_knn_nearest_neighbour(ops, n, D, K):
    X, Cm = normal(n, D, K, 100 + n)
    x, c = dev(X), dev(Cm)
    c_sq = (c * c).sum(1)
    labels, min_d2 = ops.kmeans_assign(x, c, c_sq, K, want_min_d2=True)
    _, nbr_idx, nbr_d2 = ops.knn_search_vote(x, c, c_sq, torch.zeros(K, dtype=torch.int64, device=DEV), 1, 1, want_neighbours=True)
    assert labels.shape == (1, n) and labels.dtype == torch.int32 and min_d2.shape == (1, n) and min_d2.dtype == torch.float32
    assert torch.equal(labels[0], nbr_idx[:, 0])
    assert bits(min_d2[0]) == bits(nbr_d2[:, 0])
    d2 = ((X.astype(np.float64)[:, None] - Cm.astype(np.float64)[None]) ** 2).sum(2)  # (and it is the nearest centroid)
    chosen = np.take_along_axis(d2, labels[0].cpu().numpy().astype(np.int64)[:, None], 1)[:, 0]
    assert (chosen - d2.min(1) <= 8 * D * U * ((X.astype(np.float64) ** 2).sum(1) + (Cm.astype(np.float64) ** 2).sum(1).max())).all()


# ------------------------------------------------------------------------------------------ 2: restart segmentation
@pytest.mark.parametrize("R,K", [(3, 7), (10, 7), (2, 64), (16, 64)], ids=lambda v: str(v))
def test_restart_segmentation(ops, R, K):
    n, D = 257, 36
    X, Cm = normal(n, D, R * K, 200 + R)
    x, c = dev(X), dev(Cm)
    c_sq = (c * c).sum(1)
    entry = torch.from_numpy(np.random.default_rng(R).integers(0, K, (R, n)).astype(np.int32)).to(DEV)
    labels, min_d2 = entry.clone(), torch.empty(R, n, device=DEV)
    changed = torch.zeros(R, dtype=torch.int32, device=DEV)
    ops.kmeans_assign(x, c, c_sq, K, labels=labels, min_d2=min_d2, changed=changed)
    for r in range(R):
        cr = c[r * K:(r + 1) * K].contiguous()
        one_l, one_d = ops.kmeans_assign(x, cr, c_sq[r * K:(r + 1) * K].contiguous(), K, want_min_d2=True)
        assert torch.equal(labels[r], one_l[0]), r
        assert bits(min_d2[r]) == bits(one_d[0]), r
    assert torch.equal(changed.long(), (labels != entry).sum(1))
    assert int(changed.sum()) > 0
    ops.kmeans_assign(x, c, c_sq, K, labels=labels, min_d2=min_d2, changed=changed)  # += : nothing moves the second time
    assert torch.equal(changed.long(), (labels != entry).sum(1))


# ------------------------------------------------------------------------------------------ 3: order
def test_order_ties_nan_and_slices(ops):
    from focal_amd import _lib
    n, D, R, K = 200, 36, 10, 7
    X, Cm = normal(n, D, R * K, 300)
    X, Cm = X.copy(), Cm.copy()
    # duplicates: restart 9 holds columns 63 .. 69, across the 64-column tile boundary; its centroids 0 and 5 are one row, and so are 2 and 4
    Cm[9 * K + 5] = Cm[9 * K + 0]
    Cm[9 * K + 4] = Cm[9 * K + 2]
    X[:40] = Cm[9 * K + 0] + 0.01 * X[:40]
    X[40:80] = Cm[9 * K + 2] + 0.01 * X[40:80]
    x, c = dev(X), dev(Cm)
    labels, min_d2 = assign(ops, x, c, K)
    assert (labels[9, :40] == 0).all() and (labels[9, 40:80] == 2).all()
    assert not ((labels[9] == 5) | (labels[9] == 4)).any()
    # a NaN centroid never beats a number: the result is the one without it
    Cn = Cm.copy()
    Cn[3 * K + 2, 7] = np.nan
    Cn[9 * K + 0, 0] = np.nan                                               # (now the copy, index 5, is the nearest of rows 0 .. 39)
    ln, dn = assign(ops, x, dev(Cn), K)
    for r, dead in ((3, 2), (9, 0)):
        keep = [k for k in range(K) if k != dead]
        lo, do = assign(ops, x, dev(Cm[r * K:(r + 1) * K][keep]), K - 1)
        assert torch.equal(ln[r].long(), torch.tensor(keep, device=DEV)[lo[0].long()]), r
        assert bits(dn[r]) == bits(do[0]), r
    assert (ln[9, :40] == 5).all()
    for r in (0, 1, 2, 4, 5, 6, 7, 8):
        assert torch.equal(ln[r], labels[r]) and bits(dn[r]) == bits(min_d2[r])
    # all NaN: a NaN row of x, and a restart of NaN centroids
    Xn = X.copy()
    Xn[17, 3] = np.nan
    Ca = Cm.copy()
    Ca[4 * K:5 * K, 0] = np.nan
    la, da = assign(ops, dev(Xn), dev(Ca), K)
    assert (la[:, 17] == 0).all() and torch.isnan(da[:, 17]).all()
    assert (la[4] == 0).all() and torch.isnan(da[4]).all()
    assert torch.equal(la[3, :17], labels[3, :17]) and not torch.isnan(da[3, :17]).any()
    # the descriptor's `slices` (the update's) plays no part in the assignment
    lib = _lib.load()
    c_sq = (c * c).sum(1)
    for s in (1, 3, 64):
        l2, d2 = torch.full((R, n), -1, dtype=torch.int32, device=DEV), torch.empty(R, n, device=DEV)
        d = _lib.KMeansDesc(n, D, K, R, s)
        _lib.check(lib.focal_kmeans_assign(ctypes.byref(d), x.data_ptr(), c.data_ptr(), c_sq.data_ptr(), l2.data_ptr(), d2.data_ptr(), None,
                                           torch.cuda.current_stream().cuda_stream))
        assert torch.equal(l2, labels) and bits(d2) == bits(min_d2), s


# ------------------------------------------------------------------------------------------ 4: update, exact
def exact_case(n, D, R, K=5):
    r = np.random.default_rng(n * 1000 + D * 10 + R)
    X = r.integers(-8, 9, (n, D)).astype(np.float32)
    empty, single = 1, 3
    lab = r.choice([0, 2, 4], (R, n)).astype(np.int32)
    lab[:, n // 2] = single
    prev = r.standard_normal((R * K, D)).astype(np.float32)
    prev_sq = r.standard_normal(R * K).astype(np.float32)
    return X, lab, prev, prev_sq, empty, single


@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("D", [4, 36, 132])
@pytest.mark.parametrize("n", [1, 129, 1000])
def test_update_exact(ops, n, D, R):
    K = 5
    X, lab, prev, prev_sq, empty, single = exact_case(n, D, R)
    x = dev(X)
    results = []
    for slices in (None, 1, 3):
        c, c_sq = dev(prev), dev(prev_sq)
        counts, inertia = ops.kmeans_update(x, dev(lab), c, c_sq, K, slices=slices)
        assert inertia is None and counts.shape == (R, K) and counts.dtype == torch.int32
        results.append((counts.cpu().numpy(), c.cpu().numpy().reshape(R, K, D), c_sq.cpu().numpy().reshape(R, K)))
    for counts, c, c_sq in results:
        for r in range(R):
            want_n = np.bincount(lab[r], minlength=K)
            assert np.array_equal(counts[r], want_n) and want_n[empty] == 0 and want_n[single] == 1
            for k in range(K):
                if want_n[k] == 0:
                    assert c[r, k].tobytes() == prev[r * K + k].tobytes() and c_sq[r, k].tobytes() == prev_sq[r * K + k].tobytes()
                    continue
                want = X[lab[r] == k].astype(np.float64).sum(0).astype(np.float32) / np.float32(want_n[k])  # (integers: the sum is exact)
                assert want.dtype == np.float32 and c[r, k].tobytes() == want.tobytes(), (r, k)
                sq = (want.astype(np.float64) ** 2).sum()
                assert abs(float(c_sq[r, k]) - sq) <= (D + 16) * U * sq
            assert c[r, single].tobytes() == X[n // 2].tobytes()


# ------------------------------------------------------------------------------------------ 5: update, rounded
def centre_bound(X64, lab, K, c64):
    """[K, D] bound of the module docstring on the centroids of labels `lab`, given the float64 centroids."""
    out = np.zeros_like(c64)
    for k in range(K):
        rows = X64[lab == k]
        if len(rows):
            out[k] = (len(rows) - 1) * U * np.abs(rows).sum(0) / len(rows) + U * np.abs(c64[k])
    return out


@pytest.mark.parametrize("n,D,R,K", [(1000, 132, 3, 7), (129, 36, 1, 5)], ids=lambda v: str(v))
def test_update_rounded(ops, n, D, R, K):
    X, Cm = normal(n, D, R * K, 500 + n)
    x, c = dev(X), dev(Cm)
    c_sq = (c * c).sum(1)
    labels, min_d2 = ops.kmeans_assign(x, c, c_sq, K, want_min_d2=True)
    counts, inertia = ops.kmeans_update(x, labels, c, c_sq, K, min_d2=min_d2)
    X64, C64, lab = X.astype(np.float64), Cm.astype(np.float64).reshape(R, K, D), labels.cpu().numpy()
    got, got_n, got_i = c.cpu().numpy().astype(np.float64).reshape(R, K, D), counts.cpu().numpy(), inertia.cpu().numpy().astype(np.float64)
    for r in range(R):
        assert np.array_equal(got_n[r], np.bincount(lab[r], minlength=K))
        want = np.stack([X64[lab[r] == k].mean(0) if (lab[r] == k).any() else C64[r, k] for k in range(K)])
        err, bound = np.abs(got[r] - want), centre_bound(X64, lab[r], K, want)
        chosen = C64[r][lab[r]]
        d2 = ((X64 - chosen) ** 2).sum(1)
        xn, cn = np.sqrt((X64 ** 2).sum(1)), np.sqrt((chosen ** 2).sum(1))
        i_bound = ((D + 4) * 2.0 ** -23 * (xn + cn) ** 2).sum() + (n - 1) * U * d2.sum()
        print(f"update_rounded n={n} D={D} r={r}: max centroid error / bound = {(err[bound > 0] / bound[bound > 0]).max():.4f}, "
              f"inertia error / bound = {abs(got_i[r] - d2.sum()) / i_bound:.4f}")
        assert (err <= bound).all()
        assert abs(got_i[r] - d2.sum()) <= i_bound


# ------------------------------------------------------------------------------------------ blobs and their float64 restatement
@functools.lru_cache(maxsize=None)
def blobs():
    """K = 5 blobs of 120 rows in 36 dimensions, centres 10 apart, unit noise; two explicit inits: near the centres, and five data rows
    (two of blob 0, none of blob 4) from which the float64 restatement takes 5 iterations."""
    r = np.random.default_rng(0)
    y = np.arange(600) % 5
    centres = (10.0 / np.sqrt(2.0)) * np.eye(5, 36)
    X = (centres[y] + r.standard_normal((600, 36))).astype(np.float32)
    near = (centres + 0.5 * np.random.default_rng(1000).standard_normal(centres.shape)).astype(np.float32)
    rows = X[[210, 165, 381, 192, 123]].copy()
    return X, y, near, rows


def lloyd64(X, init, max_iter=100):
    """Lloyd in float64 with the kernels' rules (an empty cluster keeps its centroid; converged when no label moved).  Returns labels,
    centres, the iterations run (the confirming one included) and the smallest relative margin (d2_second - d2_first) / d2_second of any row
    at any iteration."""
    X, c = X.astype(np.float64), init.astype(np.float64).copy()
    prev, margin, it = np.full(len(X), -1), np.inf, 0
    while it < max_iter:
        d2 = ((X[:, None, :] - c[None]) ** 2).sum(2)
        s = np.sort(d2, 1)
        margin = min(margin, ((s[:, 1] - s[:, 0]) / s[:, 1]).min())
        lab = d2.argmin(1)
        it += 1
        for k in range(len(c)):
            if (lab == k).any():
                c[k] = X[lab == k].mean(0)
        if (lab == prev).all():
            break
        prev = lab
    return lab, c, it, margin


@functools.lru_cache(maxsize=None)
def restated(which):
    X, _, near, rows = blobs()
    return lloyd64(X, near if which == "near" else rows)


def same_partition(a, b):
    from sklearn.metrics import adjusted_rand_score
    return adjusted_rand_score(np.asarray(a), np.asarray(b)) == 1.0


# ------------------------------------------------------------------------------------------ 6: reproducible, idempotent, capturable
def test_fit_is_reproducible():
    from train_utils.kmeans import GpuKMeans
    X = blobs()[0]
    x = dev(X)
    fits = [GpuKMeans(5, n_init=4, init=init, seed=11).fit(x) for init in ("k-means++", "k-means++", "random", "random")]
    for a, b in ((fits[0], fits[1]), (fits[2], fits[3])):
        assert bits(a.cluster_centers_) == bits(b.cluster_centers_) and torch.equal(a.labels_, b.labels_)
        assert a.inertia_ == b.inertia_ and a.n_iter_ == b.n_iter_ and a.restart_ == b.restart_
        assert bits(a.all_centers_) == bits(b.all_centers_) and bits(a.inertias_) == bits(b.inertias_)


def lloyd_step(ops, x, c, c_sq, K, labels, min_d2, changed, counts, inertia, ws, slices):
    changed.zero_()
    ops.kmeans_assign(x, c, c_sq, K, labels=labels, min_d2=min_d2, changed=changed)
    ops.kmeans_update(x, labels, c, c_sq, K, min_d2=min_d2, counts=counts, inertia=inertia, slices=slices, workspace=ws)


def step_state(ops, n, D, R, K, slices):
    return dict(labels=torch.full((R, n), -1, dtype=torch.int32, device=DEV), min_d2=torch.empty(R, n, device=DEV),
                changed=torch.zeros(R, dtype=torch.int32, device=DEV), counts=torch.empty(R, K, dtype=torch.int32, device=DEV),
                inertia=torch.empty(R, device=DEV), ws=ops.kmeans_workspace(n, D, K, R, slices, DEV), slices=slices)


def test_iterations_past_convergence_change_nothing(ops):
    from focal_amd import _lib
    X, _, near, rows = blobs()
    x = dev(X)
    c = dev(np.concatenate([near, rows]))
    c_sq = (c * c).sum(1)
    st = step_state(ops, 600, 36, 2, 5, 4)
    seen = []
    for _ in range(12):
        lloyd_step(ops, x, c, c_sq, 5, **st)
        seen.append(st["changed"].cpu().numpy().copy())
        if not seen[-1].any():
            break
    assert not seen[-1].any() and seen[0].tolist() == [600, 600] and len(seen) == max(restated("near")[2], restated("rows")[2])
    before = [bits(t) for t in (c, c_sq, st["labels"], st["min_d2"], st["counts"], st["inertia"])]
    lib = _lib.load()
    _lib.check(lib.focal_trace_begin(64, _lib.TRACE_DISPATCH))
    try:
        lloyd_step(ops, x, c, c_sq, 5, **st)
        torch.cuda.synchronize()
    finally:
        lib.focal_trace_end()
    assert lib.focal_trace_count() == 3  # assign, accumulate, finish: all restarts together
    assert not st["changed"].any()
    assert before == [bits(t) for t in (c, c_sq, st["labels"], st["min_d2"], st["counts"], st["inertia"])]


def test_capture_and_replay(ops):
    n, D, R, K = 300, 36, 3, 7
    r = np.random.default_rng(77)
    sets = [dev(r.standard_normal((n, D)).astype(np.float32)) for _ in range(3)]
    c0 = dev(r.standard_normal((R * K, D)).astype(np.float32))
    sq0 = (c0 * c0).sum(1)
    slices = 3

    def run(x, c, c_sq, st):
        c.copy_(c0)
        c_sq.copy_(sq0)
        st["labels"].fill_(-1)
        lloyd_step(ops, x, c, c_sq, K, **st)
        lloyd_step(ops, x, c, c_sq, K, **st)

    eager = []
    for x in sets[1:]:
        c, c_sq, st = torch.empty_like(c0), torch.empty_like(sq0), step_state(ops, n, D, R, K, slices)
        run(x, c, c_sq, st)
        eager.append([t.clone() for t in (c, c_sq, st["labels"], st["min_d2"], st["changed"], st["counts"], st["inertia"])])
    static_x, c, c_sq, st = sets[0].clone(), torch.empty_like(c0), torch.empty_like(sq0), step_state(ops, n, D, R, K, slices)
    run(static_x, c, c_sq, st)  # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run(static_x, c, c_sq, st)
    for x, want in zip(sets[1:], eager):
        static_x.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip((c, c_sq, st["labels"], st["min_d2"], st["changed"], st["counts"], st["inertia"]), want):
            assert bits(a) == bits(b)


# ------------------------------------------------------------------------------------------ 7: Lloyd against float64 and sklearn
@pytest.mark.parametrize("which", ["near", "rows"])
def test_lloyd_against_float64_and_sklearn(which):
    from sklearn.cluster import KMeans
    from train_utils.kmeans import GpuKMeans
    X, y, near, rows = blobs()
    init = near if which == "near" else rows
    lab, c64, iters, margin = restated(which)
    print(f"lloyd {which}: float64 restatement {iters} iterations, smallest relative margin {margin:.3e}")
    assert margin > 1e-3  # a condition on the inputs, met by the reference alone: no row at any iteration is left out
    if which == "rows":
        assert iters >= 3
    for check_every in (1, 8):
        est = GpuKMeans(5, init=torch.from_numpy(init)[None], check_every=check_every).fit(dev(X))
        got = est.labels_.cpu().numpy()
        assert np.array_equal(got, lab)
        assert est.n_iter_ == iters and est.restart_ == 0 and len(est.record_["changed"]) == -(-iters // check_every) * check_every
        err = np.abs(est.cluster_centers_.cpu().numpy().astype(np.float64) - c64)
        bound = centre_bound(X.astype(np.float64), lab, 5, c64)
        print(f"lloyd {which}: max centroid error / bound = {(err / bound).max():.4f}")
        assert (err <= bound).all()
        # the inertia: item 5's bound on the distances (their sum is taken in float64) plus what the centroids' own error can move them
        X64 = X.astype(np.float64)
        d2 = ((X64 - c64[lab]) ** 2).sum(1)
        xn, cn = np.sqrt((X64 ** 2).sum(1)), np.sqrt((c64[lab] ** 2).sum(1))
        i_bound = ((36 + 4) * 2.0 ** -23 * (xn + cn) ** 2).sum() + (2.0 * np.sqrt(d2) * np.sqrt((bound ** 2).sum(1))[lab]).sum()
        print(f"lloyd {which}: inertia error / bound = {abs(est.inertia_ - d2.sum()) / i_bound:.4f}")
        assert abs(est.inertia_ - d2.sum()) <= i_bound
    sk = KMeans(n_clusters=5, init=init.astype(np.float64), n_init=1, algorithm="lloyd", tol=0).fit(X.astype(np.float64))
    assert same_partition(sk.labels_, got)


# ------------------------------------------------------------------------------------------ 8: GpuKMeans whole
@pytest.mark.parametrize("init,seed", [("k-means++", 0), ("random", RANDOM_SEED)])
def test_gpu_kmeans_recovers_the_blobs(init, seed):
    from train_utils.kmeans import GpuKMeans
    X, y, _, _ = blobs()
    x = dev(X)
    est = GpuKMeans(5, n_init=10, init=init, seed=seed).fit(x)
    assert same_partition(est.labels_.cpu().numpy(), y)
    inertias = est.inertias_.cpu().numpy()
    assert inertias.shape == (10,) and est.inertia_ == inertias.min() and est.restart_ == int(np.flatnonzero(inertias == inertias.min())[0])
    assert torch.equal(est.predict(x), est.labels_)
    assert bits(est.cluster_centers_) == bits(est.all_centers_[est.restart_])
    assert est.labels_.dtype == torch.int64 and est.cluster_centers_.shape == (5, 36) and 1 <= est.n_iter_ <= 100


def test_winner_ties_go_to_the_smaller_restart():
    from train_utils.kmeans import GpuKMeans
    X, y, near, rows = blobs()
    both = GpuKMeans(5, init=torch.from_numpy(np.stack([rows, near, near]))).fit(dev(X))
    inertias = both.inertias_.cpu().numpy()
    assert inertias[1] == inertias[2] and both.restart_ == int(np.flatnonzero(inertias == inertias.min())[0]) and both.restart_ in (0, 1)
    twin = GpuKMeans(5, init=torch.from_numpy(np.stack([near, near]))).fit(dev(X))
    assert twin.restart_ == 0


def test_kmeans_pp_never_picks_a_row_twice():
    from train_utils.kmeans import GpuKMeans
    r = np.random.default_rng(8)
    n, D = 40, 8
    while True:
        X = r.integers(-8, 9, (n, D)).astype(np.float32)
        if len(np.unique(X, axis=0)) == n:
            break
    est = GpuKMeans(n, n_init=4, init="k-means++", seed=5)
    c = est._initial(dev(X)).cpu().numpy()  # the seeding alone: K = n, so every row is drawn exactly once per restart
    assert c.shape == (4, n, D)
    for r_ in range(4):
        assert len(np.unique(c[r_], axis=0)) == n and {row.tobytes() for row in c[r_]} == {row.tobytes() for row in X}


def test_torch_form_gives_the_same_partition():
    from train_utils.kmeans import GpuKMeans
    X, y, near, rows = blobs()
    init = torch.from_numpy(np.stack([near, rows]))
    a, b = GpuKMeans(5, init=init).fit(dev(X)), GpuKMeans(5, init=init).fit(dev(X), fused=False)
    assert same_partition(a.labels_.cpu().numpy(), b.labels_.cpu().numpy())
    assert abs(a.inertia_ - b.inertia_) <= 1e-4 * a.inertia_


# ------------------------------------------------------------------------------------------ 9: limits
@pytest.mark.parametrize("name,D,K,R,offset,match", [("D=34", 34, 7, 1, 0, "D % 4 == 0"), ("K=0", 36, 0, 1, 0, "1 <= K <= 64"),
                                                    ("K=65", 36, 65, 1, 0, "1 <= K <= 64"), ("RK=1025", 36, 41, 25, 0, "R * K <= 1024"),
                                                    ("misaligned x", 36, 7, 1, 1, "16-byte aligned")],
                         ids=["D=34", "K=0", "K=65", "RK=1025", "misaligned-x"])
def test_limits_refused_before_any_launch(ops, name, D, K, R, offset, match):
    from focal_amd import _lib
    lib = _lib.load()
    n, slices, rk = 20, 2, max(R * K, 1)
    x = torch.zeros(n * D + 4, device=DEV)[offset:offset + n * D].view(n, D)
    c, c_sq = torch.full((rk, D), -7.0, device=DEV), torch.full((rk,), -7.0, device=DEV)
    labels = torch.full((R, n), -7, dtype=torch.int32, device=DEV)
    min_d2, changed = torch.full((R, n), -7.0, device=DEV), torch.full((R,), -7, dtype=torch.int32, device=DEV)
    counts, inertia = torch.full((rk,), -7, dtype=torch.int32, device=DEV), torch.full((R,), -7.0, device=DEV)
    ws = torch.full((1 << 20,), 0xF9, dtype=torch.uint8, device=DEV)
    d = _lib.KMeansDesc(n, D, K, R, slices)
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.focal_trace_begin(64, _lib.TRACE_DISPATCH))
    try:
        with pytest.raises(_lib.FocalHipError, match=re.escape(match)):
            _lib.check(lib.focal_kmeans_assign(ctypes.byref(d), x.data_ptr(), c.data_ptr(), c_sq.data_ptr(), labels.data_ptr(), min_d2.data_ptr(),
                                               changed.data_ptr(), st))
        with pytest.raises(_lib.FocalHipError, match=re.escape(match)):
            _lib.check(lib.focal_kmeans_update(ctypes.byref(d), x.data_ptr(), labels.data_ptr(), min_d2.data_ptr(), c.data_ptr(), c_sq.data_ptr(),
                                               counts.data_ptr(), inertia.data_ptr(), ws.data_ptr(), ws.numel(), st))
        with pytest.raises(_lib.FocalHipError, match=re.escape(match)):  # and through the tensor-level wrappers
            ops.kmeans_assign(x, c, c_sq, K)
        with pytest.raises(_lib.FocalHipError, match=re.escape(match)):
            ops.kmeans_update(x, labels, c, c_sq, K, slices=slices, workspace=ws)
        torch.cuda.synchronize()
    finally:
        lib.focal_trace_end()
    assert lib.focal_trace_count() == 0
    if not offset:
        assert lib.focal_kmeans_update_workspace(ctypes.byref(d)) == 0
    for buf, v in ((c, -7), (c_sq, -7), (labels, -7), (min_d2, -7), (changed, -7), (counts, -7), (inertia, -7), (ws, 0xF9)):
        assert (buf == v).all()


def test_gpu_kmeans_names_the_limit():
    from focal_amd._lib import FocalHipError
    from train_utils.kmeans import GpuKMeans
    g = torch.Generator().manual_seed(11)
    with pytest.raises(FocalHipError, match=re.escape("D % 4 == 0")):
        GpuKMeans(3).fit(torch.randn(40, 34, generator=g).to(DEV))
    with pytest.raises(FocalHipError, match="1 <= K <= 64"):
        GpuKMeans(65, n_init=1).fit(torch.randn(80, 36, generator=g).to(DEV))
    with pytest.raises(FocalHipError, match=re.escape("R * K <= 1024")):
        GpuKMeans(64, n_init=17).fit(torch.randn(80, 36, generator=g).to(DEV))


# ------------------------------------------------------------------------------------------ 10: eval_cluster.py
def cluster_entry():
    spec = importlib.util.spec_from_file_location("focal_eval_cluster_entry", os.path.join(SRC, "eval_cluster.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def cluster_parsed(monkeypatch, argv):
    from params.cluster_params import parse_cluster_params
    monkeypatch.setattr(sys, "argv", ["eval_cluster.py"] + argv)
    return parse_cluster_params()


def write_seeded_backbone(args):
    """Name-seeded weights under the name the pretraining loop would use (its checkpoints are the backbone's whole state dict)."""
    from oracle.weights import fill_state_dict_
    from train_utils.model_selection import init_backbone_model
    net = init_backbone_model(copy.copy(args))
    torch.save(fill_state_dict_({k: v.detach().cpu().clone() for k, v in net.state_dict().items()}), args.backbone_weight)


def parse_cluster_report(text, K, n_init):
    m = re.search(rf"K-means \(K={K}, n_init={n_init}\) train inertia:\s*([-\d.]+)\n"
                  rf"K-means \(K={K}\) val ARI:\s*([-\d.]+), val NMI:\s*([-\d.]+)\nK-means \(K={K}\) test ARI:\s*([-\d.]+), test NMI:\s*([-\d.]+)\n"
                  r"Val contingency matrix \(classes x clusters\):\n(.*)Test contingency matrix \(classes x clusters\):\n(.*)", text, re.S)
    assert m, text[-2000:]
    return [float(m.group(i)) for i in range(1, 6)], [int(v) for v in re.findall(r"\d+", m.group(6))], [int(v) for v in re.findall(r"\d+", m.group(7))]


@pytest.mark.parametrize("model,dataset", [("DeepSense", "MOD"), ("SW_Transformer", "HAR3LOC")])
def test_eval_cluster_end_to_end(monkeypatch, tmp_path, capsys, model, dataset):
    """(No agreement with a float64 K-means is asserted on these features: at their width the distances concentrate and near-ties are
    common -- tests/test_knn_fused_gpu.py::test_eval_knn_end_to_end_deepsense has the numbers.)"""
    from sklearn.metrics import adjusted_rand_score, normalized_mutual_info_score
    argv = [f"-model={model}", f"-dataset={dataset}", "-learn_framework=FOCAL", f"-model_weight={tmp_path}", "-batch_size=32", "-compute_dtype=fp32",
            "-synthetic_batches=2"]
    args = cluster_parsed(monkeypatch, argv)
    assert args.backbone_weight == os.path.join(str(tmp_path), f"{dataset}_{model}_pretrain_best.pt")
    n_cls = args.dataset_config[args.task]["num_classes"]
    K, n_init, n_train = n_cls, 10, 2 * 32
    assert args.n_clusters == K
    if dataset == "HAR3LOC":
        assert len(args.dataset_config["location_names"]) > 1
    write_seeded_backbone(args)
    capsys.readouterr()
    out, kept = cluster_entry().evaluate_cluster(args, keep=True)
    printed = parse_cluster_report(capsys.readouterr().out, K, n_init)
    saved = torch.load(args.backbone_weight, map_location="cpu")
    loaded = {k: v.detach().cpu() for k, v in args.classifier.state_dict().items()}
    assert set(loaded) == set(saved)  # loaded strictly
    for k, v in saved.items():
        assert torch.equal(loaded[k], v), k
    x, y, ids = kept["train"]
    assert x.shape[0] == n_train == ids.numel() and x.dtype == torch.float32 and kept["centers"].shape == (K, x.shape[1])
    assert torch.equal(kept["estimator"].predict(x), ids)
    assert abs(printed[0][0] - out["inertia"]) <= 5.1e-6
    for i, split in enumerate(("val", "test")):
        feats, labels, got = kept[split]
        conf = kept["conf"][split]
        assert conf.shape == (n_cls, K) and int(conf.sum()) == feats.shape[0] == labels.numel() == got.numel() == 32
        want = np.zeros((n_cls, K), dtype=np.int64)
        np.add.at(want, (labels.cpu().numpy(), got.cpu().numpy()), 1)
        assert np.array_equal(conf, want) and printed[1 + i] == want.ravel().tolist()
        ari = adjusted_rand_score(labels.cpu().numpy(), got.cpu().numpy())
        nmi = normalized_mutual_info_score(labels.cpu().numpy(), got.cpu().numpy())
        assert abs(out[split][0] - ari) <= 1e-12 and abs(out[split][1] - nmi) <= 1e-12
        assert abs(printed[0][1 + 2 * i] - ari) <= 5.1e-6 and abs(printed[0][2 + 2 * i] - nmi) <= 5.1e-6  # five decimals
        assert torch.equal(kept["estimator"].predict(feats), got)  # a second predict: the same ids
