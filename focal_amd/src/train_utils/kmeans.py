"""K-means on un-projected backbone features, for eval_cluster.py [build extension].

`GpuKMeans` runs `n_init` restarts of Lloyd's algorithm TOGETHER: the restarts' centroids are one matrix [n_init * K, D], one iteration of
all of them is ops.kmeans_assign + ops.kmeans_update (three launches, the features read twice while n_init * K <= 160, no [n, K] matrix, no allocation, no host
read), and the host reads the per-iteration record -- changed rows and inertia per restart -- once every `check_every` iterations.  There
is no floating-point atomic on the path: two fits with equal arguments give the same bits.  Iterations run past a restart's convergence
change nothing (same labels -> same sums in the same order -> same centroids), so the coarse check costs time only.

Deviation from sklearn: an EMPTY cluster keeps its previous centroid (sklearn relocates it to the row farthest from its centroid).  There
is no `tol`: a restart has converged when no row changed its label.  The winner is the restart with the lowest inertia (ties: the smallest
index), the inertia taken from the final centroids."""
import os
import sys

import torch

_ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "..", ".."))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

from focal_amd import ops  # noqa: E402


class GpuKMeans:
    def __init__(self, n_clusters, n_init=10, max_iter=100, init="k-means++", seed=0, check_every=8):
        self.K, self.R, self.max_iter, self.init, self.seed = int(n_clusters), int(n_init), int(max_iter), init, int(seed)
        self.check_every = max(1, int(check_every))
        self.cluster_centers_ = self.labels_ = self.inertia_ = self.n_iter_ = self.restart_ = None
        self.inertias_ = self.all_centers_ = self.record_ = self._center_sq = None

    # ------------------------------------------------------------------------------------------ seeding
    def _initial(self, x):
        """[R, K, D] starting centroids (no host read)."""
        n, D = x.shape
        R, K = self.R, self.K
        if torch.is_tensor(self.init):
            c = self.init.detach().to(x.device).float()
            if c.dim() == 2:
                c = c[None]
            if tuple(c.shape[1:]) != (K, D):
                raise ValueError(f"GpuKMeans: init {tuple(self.init.shape)} is not [n_init, {K}, {D}]")
            self.R = c.shape[0]
            return c.contiguous().clone()
        gen = torch.Generator(device=x.device).manual_seed(self.seed)
        if self.init == "random":
            if n < K:
                raise ValueError(f"GpuKMeans: init='random' takes {K} distinct rows of {n}")
            rows = torch.stack([torch.randperm(n, generator=gen, device=x.device)[:K] for _ in range(R)])
            return x[rows]
        if self.init != "k-means++":
            raise ValueError(f"GpuKMeans: init is 'k-means++', 'random' or a tensor [n_init, K, D] (got {self.init!r})")
        # k-means++ from the assignment kernel: min_d2 [R, n] against the j centroids chosen so far is the sampling weight of the next one
        c = torch.empty(R, K, D, dtype=torch.float32, device=x.device)
        c[:, 0] = x[torch.randint(0, n, (R,), generator=gen, device=x.device)]
        for j in range(1, K):
            cj = c[:, :j].reshape(R * j, D).contiguous()
            _, min_d2 = ops.kmeans_assign(x, cj, (cj * cj).sum(1), j, want_min_d2=True)
            w = min_d2.clamp_min(0)
            w = torch.where(w.sum(1, keepdim=True) > 0, w, torch.ones_like(w))  # (every row already chosen: any row)
            c[:, j] = x[torch.multinomial(w, 1, generator=gen)[:, 0]]
        return c

    # ------------------------------------------------------------------------------------------ fit
    @torch.no_grad()
    def fit(self, x, fused=True, check_convergence=True):
        x = x.detach().float().contiguous()
        n, D = x.shape
        ops.kmeans_check_limits(D, self.K, self.R)
        c3 = self._initial(x)
        R, K = self.R, self.K
        ops.kmeans_check_limits(D, K, R)
        if not fused:
            return self._fit_torch(x, c3, check_convergence)
        c = c3.reshape(R * K, D).contiguous()
        c_sq = (c * c).sum(1)
        labels = torch.full((R, n), -1, dtype=torch.int32, device=x.device)
        min_d2 = torch.empty(R, n, dtype=torch.float32, device=x.device)
        changed = torch.zeros(self.max_iter, R, dtype=torch.int32, device=x.device)
        inertia = torch.zeros(self.max_iter, R, dtype=torch.float32, device=x.device)
        counts = torch.empty(R, K, dtype=torch.int32, device=x.device)
        slices = ops.kmeans_default_slices(n, D, x.device)
        ws = ops.kmeans_workspace(n, D, K, R, slices, x.device)
        it, n_iter = 0, self.max_iter
        while it < self.max_iter:
            ops.kmeans_assign(x, c, c_sq, K, labels=labels, min_d2=min_d2, changed=changed[it])
            ops.kmeans_update(x, labels, c, c_sq, K, min_d2=min_d2, counts=counts, inertia=inertia[it], slices=slices, workspace=ws)
            it += 1
            if check_convergence and (it % self.check_every == 0 or it == self.max_iter):
                still = (changed[:it] != 0).any(1).cpu()  # the record's one read
                if not bool(still[-1]):
                    n_iter = int(still.nonzero().max().item()) + 2 if bool(still.any()) else 1  # the first iteration that moved no row
                    break
        # the labels and distances of the final centroids (after convergence: the ones the last iteration already held)
        ops.kmeans_assign(x, c, c_sq, K, labels=labels, min_d2=min_d2)
        self.record_ = {"changed": changed[:it], "inertia": inertia[:it]}
        return self._finish(c.view(R, K, D), c_sq, labels, min_d2.double().sum(1), n_iter if check_convergence else it)

    def _finish(self, c3, c_sq, labels, inertias, n_iter):
        host = inertias.cpu()
        low = (host == host.min()).nonzero()  # (argmin's choice among equal minima is not specified: the smallest index, explicitly)
        self.restart_ = int(low[0].item()) if low.numel() else 0
        self.inertias_, self.all_centers_ = inertias, c3
        self.cluster_centers_ = c3[self.restart_].contiguous()
        self._center_sq = c_sq.view(self.R, self.K)[self.restart_].contiguous()
        self.labels_ = labels[self.restart_].long()
        self.inertia_ = float(host[self.restart_].item())
        self.n_iter_ = n_iter
        return self

    def _fit_torch(self, x, c3, check_convergence):
        """The plain torch form, restart by restart: cdist / argmin / index_add_ (float atomics: two runs may differ).  The baseline of
        tools/mb_kmeans.py and nothing else."""
        R, K = self.R, self.K
        n, D = x.shape
        all_labels, inertias, iters = [], [], 0
        c3 = c3.clone()
        for r in range(R):
            c = c3[r]
            prev = torch.full((n,), -1, dtype=torch.int64, device=x.device)
            for it in range(self.max_iter):
                lab = torch.cdist(x, c).argmin(1)
                sums = torch.zeros(K, D, dtype=torch.float32, device=x.device).index_add_(0, lab, x)
                cnt = torch.bincount(lab, minlength=K)
                c = torch.where((cnt > 0)[:, None], sums / cnt.clamp_min(1)[:, None].float(), c)
                iters = max(iters, it + 1)
                if check_convergence and (it + 1) % self.check_every == 0:
                    if bool((lab == prev).all().item()):
                        break
                prev = lab
            d = torch.cdist(x, c)
            lab = d.argmin(1)
            c3[r] = c
            all_labels.append(lab.int())
            inertias.append((d.gather(1, lab[:, None])[:, 0].double() ** 2).sum())
        return self._finish(c3, (c3 * c3).sum(2), torch.stack(all_labels), torch.stack(inertias), iters)

    @torch.no_grad()
    def predict(self, x):
        """The nearest of the winner's centroids (int64 [n]): the assignment kernel with one restart."""
        x = x.detach().float().contiguous()
        return ops.kmeans_assign(x, self.cluster_centers_, self._center_sq, self.K)[0].long()
