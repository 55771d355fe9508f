"""Linear probe on un-projected backbone features, for eval_linear.py [build extension].

`GpuLinearProbe` fits multinomial softmax regression on standardised features for every regularisation strength of `l2` TOGETHER: problem
r minimises

    F_r = (1/n) sum_i CE(softmax(W_r x_i + b_r), y_i) + (l2_r / 2) |W_r|^2        (sklearn's LogisticRegression with C = 1 / (l2_r n))

and the problems' weights are one matrix [R * C, D].  One evaluation of all of them is ops.probe_forward + ops.probe_grad (three launches,
the features read twice while R * C <= 64, no allocation, no floating-point atomic): every problem's trial point goes up in one copy and
(f, gw, gb) come down in one copy.  The minimiser, `lbfgs_minimize`, is host code in float64 that takes the evaluation as a callable; the
problems advance in lock-step, each through its own two-loop recursion and Armijo backtracking, and a problem's iterates do not depend on
which other problems run beside it.  Two fits with equal arguments give the same bits."""
import os
import sys

import numpy as np
import torch

_ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "..", ".."))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

from focal_amd import ops  # noqa: E402

ARMIJO, MAX_BACKTRACK = 1e-4, 40


class _Problem:
    """One problem's L-BFGS state: the accepted point (theta, f, g), the search direction and step of the open line search, the pairs."""

    def __init__(self, theta, history):
        self.theta, self.f, self.g = theta.copy(), None, None
        self.history, self.pairs = history, []
        self.d = self.t = self.slope = None
        self.trial, self.backtracks, self.n_iter = self.theta, 0, 0
        self.done = self.converged = False

    def _direction(self):
        q = self.g.copy()
        alphas = []
        for s, y, rho in reversed(self.pairs):
            a = rho * s.dot(q)
            alphas.append(a)
            q -= a * y
        if self.pairs:
            s, y, _ = self.pairs[-1]
            q *= s.dot(y) / y.dot(y)
        for (s, y, rho), a in zip(self.pairs, reversed(alphas)):
            q += (a - rho * y.dot(q)) * s
        return -q

    def _open_search(self, first):
        self.d = self._direction()
        self.slope = self.g.dot(self.d)
        if not self.slope < 0:  # not a descent direction (the pairs have gone stale): steepest descent, history dropped
            self.pairs, self.d = [], -self.g
            self.slope = -self.g.dot(self.g)
        norm = np.sqrt(self.g.dot(self.g))
        self.t = 1.0 / norm if (first or not self.pairs) and norm > 0 else 1.0
        self.backtracks = 0
        self.trial = self.theta + self.t * self.d

    def _stop(self, converged):
        self.done, self.converged, self.trial = True, converged, self.theta

    def advance(self, f, g, max_iter, tol, stop):
        """Take the evaluation of `self.trial`; leave the next trial point in `self.trial`."""
        if self.done:
            return
        if self.f is None:  # the starting point
            self.f, self.g = float(f), g.copy()
            if stop and np.abs(self.g).max() <= tol:
                return self._stop(True)
            return self._open_search(True)
        if np.isfinite(f) and f <= self.f + ARMIJO * self.t * self.slope:
            s, y = self.trial - self.theta, g - self.g
            sy = s.dot(y)
            if sy > 0:  # (a pair with s.y <= 0 is skipped)
                self.pairs.append((s, y, 1.0 / sy))
                if len(self.pairs) > self.history:
                    self.pairs.pop(0)
            self.theta, self.f, self.g = self.trial, float(f), g.copy()
            self.n_iter += 1
            if stop and np.abs(self.g).max() <= tol:
                return self._stop(True)
            if self.n_iter >= max_iter:
                return self._stop(False)
            return self._open_search(False)
        self.backtracks += 1
        if self.backtracks > MAX_BACKTRACK:  # no decrease along a descent direction: the resolution of the evaluation
            return self._stop(False)
        self.t *= 0.5
        self.trial = self.theta + self.t * self.d


def lbfgs_minimize(evaluate, theta0, max_iter=200, tol=1e-5, history=10, stop=True, max_eval=None):
    """Minimise R problems in lock-step.  evaluate(theta float64 [R, P]) -> (f [R], grad [R, P]) evaluates every problem's trial point at
    once; theta0 is [R, P].  A problem stops when |g|_inf <= tol, after max_iter accepted steps, or when its line search finds no
    decrease; a stopped problem resubmits its final point and its outputs are ignored.  stop=False switches the gradient test off and
    runs exactly max_eval evaluations (measurement).  Returns {"theta" [R, P], "f" [R], "grad" [R, P], "n_iter" [R], "converged" [R],
    "n_eval"}."""
    theta0 = np.array(theta0, dtype=np.float64, ndmin=2)
    probs = [_Problem(t, int(history)) for t in theta0]
    n_eval = 0
    while (not stop or not all(p.done for p in probs)) and (max_eval is None or n_eval < max_eval):
        if not stop and max_eval is None:
            raise ValueError("lbfgs_minimize: stop=False needs max_eval")
        f, g = evaluate(np.stack([p.trial for p in probs]))
        n_eval += 1
        f, g = np.asarray(f, dtype=np.float64), np.asarray(g, dtype=np.float64)
        for r, p in enumerate(probs):
            p.advance(f[r], g[r], max_iter, tol, stop)
    return {"theta": np.stack([p.theta for p in probs]), "f": np.array([np.nan if p.f is None else p.f for p in probs]),
            "grad": np.stack([p.theta * np.nan if p.g is None else p.g for p in probs]),
            "n_iter": np.array([p.n_iter for p in probs]), "converged": np.array([p.converged for p in probs]), "n_eval": n_eval}


class GpuLinearProbe:
    def __init__(self, l2=(1e-4, 1e-3, 1e-2, 1e-1), max_iter=200, tol=1e-5, history=10):
        self.l2 = tuple(float(v) for v in (l2 if hasattr(l2, "__iter__") else (l2,)))
        if not self.l2 or any(not v > 0 for v in self.l2):
            raise ValueError(f"GpuLinearProbe: l2 holds positive strengths (got {l2!r})")
        self.R, self.max_iter, self.tol, self.history = len(self.l2), int(max_iter), float(tol), int(history)
        self.C = self.mean_ = self.scale_ = None
        self.coef_ = self.intercept_ = self.objective_ = self.n_eval_ = self.converged_ = self.theta_ = self.n_iter_ = None

    # ------------------------------------------------------------------------------------------ features
    def _standardise(self, x, fit):
        x = x.detach().float()
        if fit:
            self.mean_ = x.mean(0)
            std = x.std(0, unbiased=False) if x.shape[0] > 1 else torch.zeros_like(self.mean_)
            self.scale_ = torch.where(std > 0, std, torch.ones_like(std))  # (a constant column: left as it is, centred)
        out = x - self.mean_  # (one copy of the features, divided in place)
        out /= self.scale_
        return out.contiguous()

    @torch.no_grad()
    def transform(self, x):
        """The standardised features the fitted weights apply to (fp32)."""
        return self._standardise(x, False)

    # ------------------------------------------------------------------------------------------ evaluations
    def _fused_evaluation(self, x, y, C):
        n, D = x.shape
        R, dev = self.R, x.device
        rows = R * C
        up = torch.empty(rows * D + rows, dtype=torch.float32, device=dev)
        w, b = up[:rows * D].view(rows, D), up[rows * D:]
        down = torch.empty(8 * R + 4 * (rows * D + rows), dtype=torch.uint8, device=dev)
        f, gw = down[:8 * R].view(torch.float64), down[8 * R:8 * R + 4 * rows * D].view(torch.float32).view(rows, D)
        gb = down[8 * R + 4 * rows * D:].view(torch.float32)
        lam = torch.tensor(self.l2, dtype=torch.float32, device=dev)
        ce = torch.empty(R, n, dtype=torch.float32, device=dev)
        g = torch.empty(n, rows, dtype=torch.float32, device=dev)
        slices = ops.probe_default_slices(n, D, dev)
        ws = ops.probe_workspace(n, D, C, R, slices, dev)

        def evaluate(theta):
            host = np.concatenate([theta[:, :C * D].ravel(), theta[:, C * D:].ravel()]).astype(np.float32)
            up.copy_(torch.from_numpy(host))
            ops.probe_forward(x, w, b, C, y=y, ce=ce, g=g, check_labels=False)
            ops.probe_grad(x, g, ce, w, lam, C, gw=gw, gb=gb, f=f, slices=slices, workspace=ws)
            raw = down.cpu().numpy()
            grad_w = raw[8 * R:8 * R + 4 * rows * D].view(np.float32).astype(np.float64).reshape(R, C * D)
            grad_b = raw[8 * R + 4 * rows * D:].view(np.float32).astype(np.float64).reshape(R, C)
            return raw[:8 * R].view(np.float64).copy(), np.concatenate([grad_w, grad_b], axis=1)
        return evaluate

    def _torch_evaluation(self, x, y, C):
        """The plain torch form of the same evaluation: the baseline of tools/mb_linear_probe.py and nothing else."""
        n, D = x.shape
        R, dev = self.R, x.device
        lam = torch.tensor(self.l2, dtype=torch.float32, device=dev)
        onehot = torch.nn.functional.one_hot(y.long(), C).float()

        def evaluate(theta):
            th = torch.from_numpy(theta.astype(np.float32)).to(dev)
            w, b = th[:, :C * D].reshape(R, C, D), th[:, C * D:]
            z = torch.einsum("nd,rcd->nrc", x, w) + b
            lse = torch.logsumexp(z, dim=2)
            ce = lse - (z * onehot[:, None, :]).sum(2)
            g = torch.softmax(z, dim=2) - onehot[:, None, :]
            gw = torch.einsum("nrc,nd->rcd", g, x) / n + lam[:, None, None] * w
            gb = g.sum(0) / n
            f = ce.double().mean(0) + 0.5 * lam.double() * (w.double() ** 2).sum((1, 2))
            out = torch.cat([f, gw.reshape(R, C * D).double().reshape(-1), gb.double().reshape(-1)]).cpu().numpy()
            return out[:R], np.concatenate([out[R:R + R * C * D].reshape(R, C * D), out[R + R * C * D:].reshape(R, C)], axis=1)
        return evaluate

    # ------------------------------------------------------------------------------------------ fit
    @torch.no_grad()
    def fit(self, x, y, num_classes, fused=True, stop=True, max_eval=None):
        C = int(num_classes)
        x = self._standardise(x, True)
        n, D = x.shape
        ops.probe_check_limits(D, C, self.R)
        y = y.detach().to(x.device).to(torch.int32).contiguous()
        if y.numel() != n:
            raise ValueError(f"GpuLinearProbe: {y.numel()} labels against {n} rows")
        low, high = (int(v) for v in torch.stack([y.min(), y.max()]).cpu())  # the fit's one look at the labels
        if low < 0 or high >= C:
            raise ValueError(f"GpuLinearProbe: labels must lie in [0, {C}) (got {low} .. {high})")
        evaluate = (self._fused_evaluation if fused else self._torch_evaluation)(x, y, C)
        res = lbfgs_minimize(evaluate, np.zeros((self.R, C * D + C)), max_iter=self.max_iter, tol=self.tol, history=self.history, stop=stop,
                             max_eval=max_eval)
        self.C, self.theta_ = C, res["theta"]
        th = torch.from_numpy(res["theta"].astype(np.float32)).to(x.device)
        self.coef_ = th[:, :C * D].reshape(self.R, C, D).contiguous()
        self.intercept_ = th[:, C * D:].contiguous()
        self.objective_, self.n_eval_, self.converged_, self.n_iter_ = res["f"], res["n_eval"], res["converged"], res["n_iter"]
        return self

    @torch.no_grad()
    def predict(self, x):
        """Class ids [R, n] (int64) of every problem's classifier: the softmax pass without labels."""
        x = self._standardise(x, False)
        w = self.coef_.view(self.R * self.C, -1)
        return ops.probe_forward(x, w, self.intercept_.view(-1), self.C, want_preds=True)[2].long()
