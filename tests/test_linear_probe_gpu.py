"""The linear-probe kernels (focal_probe_forward / focal_probe_grad, ops.probe_forward / ops.probe_grad), GpuLinearProbe and eval_linear.py.

Bounds (derived, not measured), u = 2^-24.  A logit is a k-ordered fp32 fma chain of D products plus the bias:
    |dz| <= (D + 1) u (sum_d |x_d w_d| + |b|).
The cross entropy lse - z_y moves by at most 2 max_c |dz| under perturbed logits (lse is 1-Lipschitz in the max norm, z_y one logit), and
its own evaluation -- C exponentials, C - 1 adds, a log, two more adds, each rounded once, expf / logf within a few ulp -- adds
    (C + 8) u (1 + |CE| + max_c |z|),        so  |dCE| <= 2 max_c |dz| + (C + 8) u (1 + |CE| + max_c |z|).
f = mean CE + lambda / 2 |W|^2: the per-row bounds averaged, plus (n - 1) u sum CE / n for the sum (taken in double on the device: slack),
plus lambda u |W|^2 for the squares (each rounded once in fp32, relative u; the bound states twice that).  lambda is the fp32 value on both
sides.  A gradient entry of the softmax, p_c - onehot_c, with p_c = exp(z_c - lse):
    |dg_c| <= p_c (2 max|dz| + (C + 8) u) + u,
and gw = g^T x / n + lambda W carries it through a sum of n fp32 terms cut into `slices` partial sums:
    |dgw_cd| <= sum_i |dg_ic| |x_id| / n + (n + slices) u sum_i |g_ic x_id| / n + 2 u (sum_i |g_ic x_id| / n + lambda |w_cd|),
the last term being the division and the fma that end it; gb is the same with x = 1 and no lambda.  The arg-max equals the float64 one
wherever the float64 top-2 gap exceeds 2 max|dz|.

Fit against sklearn (item 4): F64(theta_gpu) - F64(theta_sklearn) <= 1e-5 max(1, F*), about 300 x what an fp32 numpy evaluation under
scipy's L-BFGS showed on the CPU (3.1e-8) and below the smallest objective difference between two grid points; predictions equal
sklearn's on every test row whose sklearn top-2 logit gap is >= 0.05 (largest centred-logit difference seen on the CPU: 1.7e-2), and at
most 6 % of the rows may be excluded (sklearn alone leaves out 1.6 - 5.2 % on these cases)."""
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

from conftest import record_observed

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SRC = os.path.join(ROOT, "focal_amd", "src")
DEV = "cuda"
U = 2.0 ** -24


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
def problem(n, D, C, R, seed, scale=0.3):
    """x, w, b, lam (fp32) and labels arange(n) % C, permuted."""
    r = np.random.default_rng(seed)
    x = r.standard_normal((n, D)).astype(np.float32)
    w = (scale * r.standard_normal((R * C, D))).astype(np.float32)
    b = (scale * r.standard_normal(R * C)).astype(np.float32)
    lam = np.logspace(-3, -1, R).astype(np.float32)
    y = r.permutation(np.arange(n) % C).astype(np.int32)
    return x, w, b, lam, y


def evaluate(ops, x, w, b, lam, y, C, slices, **kw):
    """One evaluation on the device: (ce, g, preds, f, gw, gb)."""
    ce, g, preds = ops.probe_forward(x, w, b, C, y=y, want_ce=True, want_g=True, want_preds=True, **kw)
    f, gw, gb = ops.probe_grad(x, g, ce, w, lam, C, slices=slices)
    return ce, g, preds, f, gw, gb


def reference(X, W, B, LAM, Y, C, slices):
    """The float64 evaluation and the docstring's bounds for it."""
    n, D = X.shape
    R = W.shape[0] // C
    x, w, b, lam = X.astype(np.float64), W.astype(np.float64), B.astype(np.float64), LAM.astype(np.float64)
    z = (x @ w.T + b).reshape(n, R, C)
    dz = ((D + 1) * U * (np.abs(x) @ np.abs(w).T + np.abs(b))).reshape(n, R, C).max(2)           # [n, R]: max over the problem's classes
    m = z.max(2, keepdims=True)
    lse = m[..., 0] + np.log(np.exp(z - m).sum(2))
    zy = np.take_along_axis(z, np.broadcast_to(Y.astype(np.int64)[:, None, None], (n, R, 1)), 2)[..., 0]
    ce = lse - zy                                                                                  # [n, R]
    ce_b = 2 * dz + (C + 8) * U * (1 + np.abs(ce) + np.abs(z).max(2))
    p = np.exp(z - lse[..., None])
    onehot = np.eye(C)[Y.astype(np.int64)][:, None, :]
    g = (p - onehot).reshape(n, R * C)
    g_b = (p * (2 * dz + (C + 8) * U)[..., None] + U).reshape(n, R * C)
    lam_rows = np.repeat(lam, C)[:, None]
    absgx = np.abs(g).T @ np.abs(x) / n
    gw = g.T @ x / n + lam_rows * w
    gw_b = g_b.T @ np.abs(x) / n + (n + slices) * U * absgx + 2 * U * (absgx + lam_rows * np.abs(w))
    absg = np.abs(g).sum(0) / n
    gb = g.sum(0) / n
    gb_b = g_b.sum(0) / n + (n + slices) * U * absg + 2 * U * absg
    w2 = (w ** 2).reshape(R, -1).sum(1)
    f = ce.mean(0) + 0.5 * lam * w2
    f_b = ce_b.mean(0) + (n - 1) * U * np.abs(ce).sum(0) / n + lam * U * w2
    srt = np.sort(z, axis=2)
    return dict(z=z, dz=dz, ce=ce.T, ce_b=ce_b.T, g=g, g_b=g_b, gw=gw, gw_b=gw_b, gb=gb, gb_b=gb_b, f=f, f_b=f_b, pred=z.argmax(2).T,
                gap=(srt[..., -1] - srt[..., -2]).T)


def check_against(ref, out, tag, record=True):
    ce, g, preds, f, gw, gb = (t.cpu().numpy() for t in out)
    worst = {}
    for name, got, want, bound in (("ce", ce, ref["ce"], ref["ce_b"]), ("g", g, ref["g"], ref["g_b"]), ("f", f, ref["f"], ref["f_b"]),
                                   ("gw", gw, ref["gw"], ref["gw_b"]), ("gb", gb, ref["gb"], ref["gb_b"])):
        assert np.isfinite(got).all(), name
        ratio = np.abs(got.astype(np.float64) - want) / bound
        worst[name] = float(ratio.max())
        print(f"{tag}: {name} max error / bound = {worst[name]:.4f} (max |error| {np.abs(got - want).max():.3e})")
        if record:
            record_observed(f"linear_probe.eval.{tag}.{name}.err_over_bound", worst[name])
    for name, got, want, bound in (("ce", ce, ref["ce"], ref["ce_b"]), ("g", g, ref["g"], ref["g_b"]), ("f", f, ref["f"], ref["f_b"]),
                                   ("gw", gw, ref["gw"], ref["gw_b"]), ("gb", gb, ref["gb"], ref["gb_b"])):
        assert (np.abs(got.astype(np.float64) - want) <= bound).all(), (tag, name, worst[name])
    sure = ref["gap"] > 2 * ref["dz"].T
    assert sure.mean() > 0.9 or sure.size < 10
    assert (preds[sure] == ref["pred"][sure]).all()
    assert preds.dtype == np.int32 and ((preds >= 0) & (preds < ref["z"].shape[2])).all()


# ------------------------------------------------------------------------------------------ 1: evaluation against float64
SHAPES = [(1, 4, 2, 1), (129, 36, 7, 1), (257, 32, 2, 3), (300, 132, 64, 2), (200, 36, 7, 10)]


@pytest.mark.parametrize("n,D,C,R", SHAPES, ids=lambda v: str(v))
def test_evaluation_against_float64(ops, n, D, C, R):
    X, W, B, LAM, Y = problem(n, D, C, R, 100 + n)
    slices = 3
    out = evaluate(ops, dev(X), dev(W), dev(B), dev(LAM), dev(Y), C, slices)
    assert out[0].shape == (R, n) and out[1].shape == (n, R * C) and out[2].shape == (R, n) and out[3].dtype == torch.float64
    assert out[4].shape == (R * C, D) and out[5].shape == (R * C,)
    check_against(reference(X, W, B, LAM, Y, C, slices), out, f"n{n}_D{D}_C{C}_R{R}")
    # a predict-only call: the same ids, no labels
    _, _, only = ops.probe_forward(dev(X), dev(W), dev(B), C, want_preds=True)
    assert torch.equal(only, out[2])


# ------------------------------------------------------------------------------------------ 2: segmentation
@pytest.mark.parametrize("R,C", [(3, 7), (10, 7), (2, 64), (16, 64)], ids=lambda v: str(v))
def test_problem_segmentation(ops, R, C):
    n, D, slices = 257, 36, 3
    X, W, B, LAM, Y = problem(n, D, C, R, 200 + R)
    x, w, b, lam, y = dev(X), dev(W), dev(B), dev(LAM), dev(Y)
    ce, g, preds, f, gw, gb = evaluate(ops, x, w, b, lam, y, C, slices)
    for r in range(R):
        rows = slice(r * C, (r + 1) * C)
        one = evaluate(ops, x, w[rows].contiguous(), b[rows].contiguous(), lam[r:r + 1].contiguous(), y, C, slices)
        assert bits(ce[r]) == bits(one[0][0]), r
        assert bits(g[:, rows]) == bits(one[1]), r
        assert torch.equal(preds[r], one[2][0]), r
        assert bits(f[r]) == bits(one[3][0]), r
        assert bits(gw[rows]) == bits(one[4]), r
        assert bits(gb[rows]) == bits(one[5]), r


# ------------------------------------------------------------------------------------------ 3: determinism and order
def test_two_evaluations_give_the_same_bits_and_slices_move_gw_only(ops):
    n, D, C, R = 200, 36, 7, 10
    X, W, B, LAM, Y = problem(n, D, C, R, 300)
    x, w, b, lam, y = dev(X), dev(W), dev(B), dev(LAM), dev(Y)
    a, again = evaluate(ops, x, w, b, lam, y, C, 3), evaluate(ops, x, w, b, lam, y, C, 3)
    for s, t in zip(a, again):
        assert bits(s) == bits(t)
    moved = False
    for slices in (1, 7, 64, 300):  # (300 > n: empty slices)
        other = evaluate(ops, x, w, b, lam, y, C, slices)
        check_against(reference(X, W, B, LAM, Y, C, slices), other, f"slices{slices}", record=False)
        assert bits(other[0]) == bits(a[0]) and bits(other[1]) == bits(a[1]) and torch.equal(other[2], a[2]) and bits(other[3]) == bits(a[3])
        moved = moved or bits(other[4]) != bits(a[4])
    assert moved  # (the order of the sums is what `slices` fixes)


def test_huge_logits_give_a_finite_objective(ops):
    n, D, C, R = 200, 36, 7, 10
    X, W, B, LAM, Y = problem(n, D, C, R, 300)
    z = X.astype(np.float64) @ W.astype(np.float64).T + B
    k = np.float32(3e4 / np.abs(z).max())
    W, B = (W * k).astype(np.float32), (B * k).astype(np.float32)
    ref = reference(X, W, B, LAM, Y, C, 3)
    assert 2.9e4 < np.abs(ref["z"]).max() < 3.1e4
    out = evaluate(ops, dev(X), dev(W), dev(B), dev(LAM), dev(Y), C, 3)
    for t in out:
        assert torch.isfinite(t.double()).all()
    check_against(ref, out, "logits3e4")


def test_ties_go_to_the_smaller_class_and_nan_never_wins(ops):
    n, D, C, R = 200, 36, 7, 10
    X, W, B, LAM, Y = problem(n, D, C, R, 300)
    W, B = W.copy(), B.copy()
    # problem 9 holds columns 63 .. 69, across the 64-column tile boundary: its classes 0 and 4 are one row (on both sides of the boundary),
    # and so are 2 and 5; problem 3's classes 1 and 6 likewise; problem 5 is all zeros
    for r, c0, c1 in ((9, 0, 4), (9, 2, 5), (3, 1, 6)):
        W[r * C + c1], B[r * C + c1] = W[r * C + c0], B[r * C + c0]
    W[5 * C:6 * C], B[5 * C:6 * C] = 0, 0
    x, y = dev(X), dev(Y)
    _, _, preds = ops.probe_forward(x, dev(W), dev(B), C, want_preds=True)
    p = preds.cpu().numpy()
    assert not np.isin(p[9], (4, 5)).any() and not (p[3] == 6).any() and (p[5] == 0).all()
    z = (X.astype(np.float64) @ W.astype(np.float64).T + B).reshape(n, R, C)
    assert (z[:, 9].argmax(1) == 0).any() and (z[:, 9].argmax(1) == 2).any()  # (the duplicated classes do win rows)
    # a NaN logit never beats a number: the ids are those of the problem without that class
    Wn = W.copy()
    Wn[9 * C + 0, 0] = np.nan   # (now the copy, class 4, takes class 0's rows)
    Wn[2 * C + 3, 7] = np.nan
    pn = ops.probe_forward(x, dev(Wn), dev(B), C, want_preds=True)[2].cpu().numpy()
    for r, dead in ((9, 0), (2, 3)):
        keep = [c for c in range(C) if c != dead]
        rows = [r * C + c for c in keep]
        alone = ops.probe_forward(x, dev(W[rows]), dev(B[rows]), C - 1, want_preds=True)[2].cpu().numpy()[0]
        assert np.array_equal(pn[r], np.array(keep)[alone]), r
    assert (pn[9][p[9] == 0] == 4).all()
    for r in (0, 1, 3, 4, 5, 6, 7, 8):
        assert np.array_equal(pn[r], p[r])
    Xn = X.copy()
    Xn[17, 3] = np.nan  # an all-NaN row: class 0
    assert (ops.probe_forward(dev(Xn), dev(W), dev(B), C, want_preds=True)[2][:, 17] == 0).all()


def test_capture_and_replay(ops):
    n, D, C, R, slices = 300, 36, 7, 3, 3
    r = np.random.default_rng(77)
    X, W, B, LAM, Y = problem(n, D, C, R, 400)
    thetas = [(dev((0.3 * r.standard_normal(W.shape)).astype(np.float32)), dev((0.3 * r.standard_normal(B.shape)).astype(np.float32)))
              for _ in range(3)]
    x, lam, y = dev(X), dev(LAM), dev(Y)
    w, b = thetas[0][0].clone(), thetas[0][1].clone()
    ce, g = torch.empty(R, n, device=DEV), torch.empty(n, R * C, device=DEV)
    preds = torch.empty(R, n, dtype=torch.int32, device=DEV)
    f, gw, gb = torch.empty(R, dtype=torch.float64, device=DEV), torch.empty(R * C, D, device=DEV), torch.empty(R * C, device=DEV)
    ws = ops.probe_workspace(n, D, C, R, slices, DEV)

    def run():
        ops.probe_forward(x, w, b, C, y=y, ce=ce, g=g, preds=preds, check_labels=False)
        ops.probe_grad(x, g, ce, w, lam, C, gw=gw, gb=gb, f=f, slices=slices, workspace=ws)

    eager = []
    for tw, tb in thetas[1:]:
        w.copy_(tw)
        b.copy_(tb)
        run()
        eager.append([t.clone() for t in (ce, g, preds, f, gw, gb)])
    w.copy_(thetas[0][0])
    b.copy_(thetas[0][1])
    run()  # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    for (tw, tb), want in zip(thetas[1:], eager):
        w.copy_(tw)
        b.copy_(tb)
        graph.replay()
        torch.cuda.synchronize()
        for got, exp in zip((ce, g, preds, f, gw, gb), want):
            assert bits(got) == bits(exp)


def test_launch_count(ops):
    from focal_amd import _lib
    lib = _lib.load()
    X, W, B, LAM, Y = problem(200, 36, 7, 10, 300)
    args = (dev(X), dev(W), dev(B), dev(LAM), dev(Y))
    evaluate(ops, *args, 7, 3)
    torch.cuda.synchronize()
    _lib.check(lib.focal_trace_begin(64, _lib.TRACE_DISPATCH))
    try:
        evaluate(ops, *args, 7, 3, check_labels=False)
        torch.cuda.synchronize()
    finally:
        lib.focal_trace_end()
    assert lib.focal_trace_count() == 3  # forward, accumulate, finish: all problems together


# ------------------------------------------------------------------------------------------ 4: fit against sklearn
def recipe(n, D, C, seed):
    r = np.random.default_rng(seed)
    cen = r.standard_normal((C, D)) * 0.35
    y = r.permutation(np.arange(n) % C)
    x = (cen[y] + r.standard_normal((n, D))).astype(np.float32)
    return x, y


def objective64(x, y, C, lam, theta):
    n, D = x.shape
    w, b = theta[:C * D].reshape(C, D), theta[C * D:]
    z = x @ w.T + b
    m = z.max(1, keepdims=True)
    lse = m[:, 0] + np.log(np.exp(z - m).sum(1))
    return (lse - z[np.arange(n), y]).mean() + 0.5 * lam * (w ** 2).sum()


CASES = {(36, 7, 5): (1e-3, 1e-2, 1e-1), (132, 64, 6): (1e-3, 1e-2)}


@functools.lru_cache(maxsize=None)
def fitted(D, C, seed, fused=True):
    """The estimator fitted on the recipe's first 1000 rows, the standardised splits in float64, and sklearn's optimum per strength."""
    from sklearn.linear_model import LogisticRegression
    from train_utils.linear_probe import GpuLinearProbe
    l2 = CASES[(D, C, seed)]
    X, Y = recipe(1500, D, C, seed)
    x, y = dev(X), dev(Y)
    est = GpuLinearProbe(l2=l2).fit(x[:1000], y[:1000], C, fused=fused)
    xs = est.transform(x).cpu().numpy().astype(np.float64)  # standardised by the train statistics, the very values the fit saw
    sk = []
    if fused:
        for lam in l2:
            m = LogisticRegression(C=1.0 / (lam * 1000), tol=1e-10, max_iter=20000).fit(xs[:1000], Y[:1000])
            sk.append((np.concatenate([m.coef_.ravel(), m.intercept_]), m.decision_function(xs[1000:]), m.predict(xs[1000:])))
    return est, x, xs, Y, sk


@pytest.mark.parametrize("D,C,seed", list(CASES), ids=lambda v: str(v))
def test_fit_against_sklearn(D, C, seed):
    est, x, xs, Y, sk = fitted(D, C, seed)
    l2 = CASES[(D, C, seed)]
    preds = est.predict(x[1000:]).cpu().numpy()
    assert preds.shape == (len(l2), 500) and est.coef_.shape == (len(l2), C, D) and est.intercept_.shape == (len(l2), C)
    assert len(est.objective_) == len(l2) and len(est.converged_) == len(l2) and est.n_eval_ >= 2
    for r, lam in enumerate(l2):
        theta_sk, logits, sk_pred = sk[r]
        f_star = objective64(xs[:1000], Y[:1000], C, lam, theta_sk)
        ours = objective64(xs[:1000], Y[:1000], C, lam, est.theta_[r])
        srt = np.sort(logits, axis=1)
        sure = srt[:, -1] - srt[:, -2] >= 0.05
        wrong = int((preds[r][sure] != sk_pred[sure]).sum())
        print(f"D={D} C={C} l2={lam:g}: F* {f_star:.9f}, gap {ours - f_star:.3e}, device objective {est.objective_[r]:.9f}, "
              f"{est.n_iter_[r]} steps / {est.n_eval_} evaluations, converged {bool(est.converged_[r])}; excluded {1 - sure.mean():.3f}, "
              f"{wrong} of {int(sure.sum())} predictions differ, {int((preds[r] != sk_pred).sum())} of all 500")
        record_observed(f"linear_probe.fit.D{D}_C{C}.l2_{lam:g}.objective_gap", ours - f_star)
        record_observed(f"linear_probe.fit.D{D}_C{C}.l2_{lam:g}.excluded_fraction", 1 - sure.mean())
        record_observed(f"linear_probe.fit.D{D}_C{C}.l2_{lam:g}.differing_predictions_all_rows", int((preds[r] != sk_pred).sum()))
        assert ours - f_star <= 1e-5 * max(1.0, f_star)
        assert 1 - sure.mean() <= 0.06
        assert wrong == 0


# ------------------------------------------------------------------------------------------ 5: fit reproducibility
def test_fit_is_reproducible_and_the_torch_form_reaches_the_same_objective():
    from train_utils.linear_probe import GpuLinearProbe
    D, C, seed = 36, 7, 5
    est, x, xs, Y, sk = fitted(D, C, seed)
    l2 = CASES[(D, C, seed)]
    again = GpuLinearProbe(l2=l2).fit(x[:1000], dev(Y)[:1000], C)
    assert bits(again.coef_) == bits(est.coef_) and bits(again.intercept_) == bits(est.intercept_) and again.n_eval_ == est.n_eval_
    assert again.theta_.tobytes() == est.theta_.tobytes()
    plain = fitted(D, C, seed, fused=False)[0]
    for r, lam in enumerate(l2):
        f_star = objective64(xs[:1000], Y[:1000], C, lam, sk[r][0])
        gap = objective64(xs[:1000], Y[:1000], C, lam, plain.theta_[r]) - f_star
        print(f"torch form l2={lam:g}: gap {gap:.3e}")
        assert gap <= 1e-5 * max(1.0, f_star)


# ------------------------------------------------------------------------------------------ 6: limits
@pytest.mark.parametrize("name,D,C,R,offset,match", [("D=34", 34, 7, 1, 0, "D % 4 == 0"), ("C=1", 36, 1, 1, 0, "2 <= C <= 64"),
                                                    ("C=65", 36, 65, 1, 0, "2 <= C <= 64"), ("RC=1025", 36, 41, 25, 0, "R * C <= 1024"),
                                                    ("misaligned x", 36, 7, 1, 1, "16-byte aligned")],
                         ids=["D=34", "C=1", "C=65", "RC=1025", "misaligned-x"])
def test_limits_refused_before_any_launch(ops, name, D, C, R, offset, match):
    from focal_amd import _lib
    lib = _lib.load()
    n, slices, rc = 20, 2, R * C
    x = torch.zeros(n * D + 4, device=DEV)[offset:offset + n * D].view(n, D)
    w, b, lam = torch.full((rc, D), -7.0, device=DEV), torch.full((rc,), -7.0, device=DEV), torch.full((R,), -7.0, device=DEV)
    y = torch.zeros(n, dtype=torch.int32, device=DEV)
    ce, g = torch.full((R, n), -7.0, device=DEV), torch.full((n, rc), -7.0, device=DEV)
    preds = torch.full((R, n), -7, dtype=torch.int32, device=DEV)
    gw, gb, f = torch.full((rc, D), -7.0, device=DEV), torch.full((rc,), -7.0, device=DEV), torch.full((R,), -7.0, dtype=torch.float64, device=DEV)
    ws = torch.full((1 << 20,), 0xF9, dtype=torch.uint8, device=DEV)
    d = _lib.ProbeDesc(n, D, C, R, slices)
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.focal_trace_begin(64, _lib.TRACE_DISPATCH))
    try:
        with pytest.raises(_lib.FocalHipError, match=re.escape(match)):
            _lib.check(lib.focal_probe_forward(ctypes.byref(d), x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), ce.data_ptr(), g.data_ptr(),
                                               preds.data_ptr(), st))
        with pytest.raises(_lib.FocalHipError, match=re.escape(match)):
            _lib.check(lib.focal_probe_grad(ctypes.byref(d), x.data_ptr(), g.data_ptr(), ce.data_ptr(), w.data_ptr(), lam.data_ptr(), gw.data_ptr(),
                                            gb.data_ptr(), f.data_ptr(), ws.data_ptr(), ws.numel(), st))
        with pytest.raises(_lib.FocalHipError, match=re.escape(match)):  # and through the tensor-level wrappers
            ops.probe_forward(x, w, b, C, y=y, ce=ce, g=g, preds=preds, check_labels=False)
        with pytest.raises(_lib.FocalHipError, match=re.escape(match)):
            ops.probe_grad(x, g, ce, w, lam, C, gw=gw, gb=gb, f=f, slices=slices, workspace=ws)
        torch.cuda.synchronize()
    finally:
        lib.focal_trace_end()
    assert lib.focal_trace_count() == 0
    if not offset:
        assert lib.focal_probe_grad_workspace(ctypes.byref(d)) == 0
    for buf, v in ((ce, -7), (g, -7), (preds, -7), (gw, -7), (gb, -7), (f, -7), (ws, 0xF9)):
        assert (buf == v).all()


def test_labels_outside_the_classes_are_refused_before_the_launch(ops):
    from focal_amd import _lib
    from train_utils.linear_probe import GpuLinearProbe
    lib = _lib.load()
    X, W, B, LAM, Y = problem(129, 36, 7, 1, 229)
    x, w, b = dev(X), dev(W), dev(B)
    ce = torch.full((1, 129), -7.0, device=DEV)
    for bad in (7, -1):
        Yb = Y.copy()
        Yb[5] = bad
        _lib.check(lib.focal_trace_begin(64, _lib.TRACE_DISPATCH))
        try:
            with pytest.raises(_lib.FocalHipError, match=re.escape("labels must lie in [0, 7)")):
                ops.probe_forward(x, w, b, 7, y=dev(Yb), ce=ce)
            torch.cuda.synchronize()
        finally:
            lib.focal_trace_end()
        assert lib.focal_trace_count() == 0 and (ce == -7).all()
        with pytest.raises(ValueError, match=re.escape("labels must lie in [0, 7)")):
            GpuLinearProbe(l2=(1e-2,)).fit(x, dev(Yb), 7)


def test_gpu_linear_probe_names_the_limit():
    from focal_amd._lib import FocalHipError
    from train_utils.linear_probe import GpuLinearProbe
    g = torch.Generator().manual_seed(11)
    y = torch.arange(40) % 3
    with pytest.raises(FocalHipError, match=re.escape("D % 4 == 0")):
        GpuLinearProbe().fit(torch.randn(40, 34, generator=g).to(DEV), y.to(DEV), 3)
    with pytest.raises(FocalHipError, match="2 <= C <= 64"):
        GpuLinearProbe().fit(torch.randn(40, 36, generator=g).to(DEV), y.to(DEV), 65)
    with pytest.raises(FocalHipError, match=re.escape("R * C <= 1024")):
        GpuLinearProbe(l2=[1e-3] * 17).fit(torch.randn(40, 36, generator=g).to(DEV), y.to(DEV), 64)


# ------------------------------------------------------------------------------------------ 7: eval_linear.py
def linear_entry():
    spec = importlib.util.spec_from_file_location("focal_eval_linear_entry", os.path.join(SRC, "eval_linear.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def linear_parsed(monkeypatch, argv):
    from params.linear_params import parse_linear_params
    monkeypatch.setattr(sys, "argv", ["eval_linear.py"] + argv)
    return parse_linear_params()


def write_seeded_backbone(args):
    """Name-seeded weights under the name the pretraining loop would use (its checkpoints are the backbone's whole state dict)."""
    from oracle.weights import fill_state_dict_
    from train_utils.model_selection import init_backbone_model
    net = init_backbone_model(copy.copy(args))
    torch.save(fill_state_dict_({k: v.detach().cpu().clone() for k, v in net.state_dict().items()}), args.backbone_weight)


def parse_linear_report(text, l2):
    val = []
    for lam in l2:
        m = re.search(rf"Linear probe \(l2={lam:g}\) val acc:\s*([-\d.]+), val f1:\s*([-\d.]+)\n", text)
        assert m, text[-2000:]
        val.append((float(m.group(1)), float(m.group(2))))
    m = re.search(r"Linear probe chosen l2=(\S+) \((\d+) training rows, \d+ evaluations\)\n"
                  r"Linear probe \(l2=(\S+)\) test acc:\s*([-\d.]+), test f1:\s*([-\d.]+)\n"
                  r"Val confusion matrix:\n(.*)Test confusion matrix:\n(.*)", text, re.S)
    assert m, text[-2000:]
    assert m.group(1) == m.group(3)
    return (val, float(m.group(1)), int(m.group(2)), (float(m.group(4)), float(m.group(5))), [int(v) for v in re.findall(r"\d+", m.group(6))],
            [int(v) for v in re.findall(r"\d+", m.group(7))])


@pytest.mark.parametrize("model,dataset", [("DeepSense", "MOD"), ("SW_Transformer", "HAR3LOC")])
def test_eval_linear_end_to_end(monkeypatch, tmp_path, capsys, model, dataset):
    from sklearn.metrics import accuracy_score, confusion_matrix, f1_score
    argv = [f"-model={model}", f"-dataset={dataset}", "-learn_framework=FOCAL", f"-model_weight={tmp_path}", "-batch_size=32", "-compute_dtype=fp32",
            "-synthetic_batches=2"]
    args = linear_parsed(monkeypatch, argv)
    assert args.backbone_weight == os.path.join(str(tmp_path), f"{dataset}_{model}_pretrain_best.pt") and args.stage == "pretrain"
    n_cls = args.dataset_config[args.task]["num_classes"]
    l2 = (1e-4, 1e-3, 1e-2, 1e-1)
    if dataset == "HAR3LOC":
        assert len(args.dataset_config["location_names"]) > 1
    write_seeded_backbone(args)
    capsys.readouterr()
    out, kept = linear_entry().evaluate_linear(args, keep=True)
    val_p, chosen_p, rows_p, test_p, val_conf_p, test_conf_p = parse_linear_report(capsys.readouterr().out, l2)
    assert args.stage == "pretrain"
    saved = torch.load(args.backbone_weight, map_location="cpu")
    loaded = {k: v.detach().cpu() for k, v in args.classifier.state_dict().items()}
    assert set(loaded) == set(saved)  # loaded strictly
    for k, v in saved.items():
        assert torch.equal(loaded[k], v), k
    x, y = kept["train"]
    est = kept["estimator"]
    assert x.shape[0] == 2 * 32 == y.numel() == rows_p and x.dtype == torch.float32 and est.coef_.shape == (4, n_cls, x.shape[1])
    assert out["l2"] == l2 and len(out["val"]) == 4
    accs = []
    for split in ("val", "test"):
        feats, labels, got = kept[split]
        assert got.shape == (4, 32) and feats.shape[0] == labels.numel() == 32
        assert torch.equal(est.predict(feats), got)  # a second predict: the same ids
    feats, labels, got = kept["val"]
    for r in range(4):
        want = confusion_matrix(labels.cpu().numpy(), got[r].cpu().numpy())
        assert np.array_equal(kept["conf"]["val"][r], want)
        acc = accuracy_score(labels.cpu().numpy(), got[r].cpu().numpy())
        f1 = f1_score(labels.cpu().numpy(), got[r].cpu().numpy(), average="macro")
        accs.append(acc)
        assert abs(out["val"][r][0] - acc) <= 1e-12 and abs(out["val"][r][1] - f1) <= 1e-12
        assert abs(val_p[r][0] - out["val"][r][0]) <= 5.1e-6 and abs(val_p[r][1] - out["val"][r][1]) <= 5.1e-6  # five decimals
        print(f"{model} l2={l2[r]:g}: val acc {acc:.5f}, val f1 {f1:.5f}")
    chosen = max(range(4), key=lambda r: (accs[r], l2[r]))  # the arg-max of the validation accuracies, ties to the larger strength
    assert out["chosen"] == chosen and out["chosen_l2"] == l2[chosen] == chosen_p
    assert val_conf_p == kept["conf"]["val"][chosen].ravel().tolist()
    feats, labels, got = kept["test"]
    want = confusion_matrix(labels.cpu().numpy(), got[chosen].cpu().numpy())
    assert np.array_equal(kept["conf"]["test"], want) and test_conf_p == want.ravel().tolist()
    assert abs(out["test"][0] - accuracy_score(labels.cpu().numpy(), got[chosen].cpu().numpy())) <= 1e-12
    assert abs(test_p[0] - out["test"][0]) <= 5.1e-6 and abs(test_p[1] - out["test"][1]) <= 5.1e-6
    # half the labels: the fit sees half the rows
    half = linear_parsed(monkeypatch, argv + ["-label_ratio=0.5"])
    capsys.readouterr()
    out_h, kept_h = linear_entry().evaluate_linear(half, keep=True)
    assert kept_h["train"][0].shape[0] == 32 and torch.equal(kept_h["train"][1], y[:32])  # the first half, the file loader's rule
    assert torch.allclose(kept_h["train"][0], x[:32], rtol=1e-4, atol=1e-5)
    assert parse_linear_report(capsys.readouterr().out, l2)[2] == 32
