"""Fused AdamW over the parameter arena (reference: torch.optim.AdamW built in train_utils/optimizer.py:27-32).

Keeps the torch.optim.Optimizer surface the reference loop and timm-style schedulers use (`param_groups[i]["lr"]`,
`zero_grad()`, `step()`), but `step()` is one streaming HIP kernel over the arena's hot region; parameters whose
`.grad` is None (frozen patch embedding, unused heads) are skipped entirely, exactly as torch does.
`FocalLAMB` is the same surface with LAMB's per-tensor trust ratios on AdamW's state (two launches per arena).
"""
import torch

from . import distributed, ops, runtime


class FocalAdamW(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, l2_decay=False, max_grad_norm=None):
        """l2_decay=True gives torch.optim.Adam semantics (g += wd * p): the reference's finetune optimizer.
        max_grad_norm (None: off): torch.nn.utils.clip_grad_norm_(params, max_grad_norm) between backward and the update, inside step() --
        a norm pass over the gradient spans and the update on g * coef, no host read; inf clips nothing and still records the norms
        (clip_stats()).  A step whose gradient norm is not finite is skipped (torch would write NaN into the weights)."""
        if max_grad_norm is not None:
            max_grad_norm = float(max_grad_norm)
            if not max_grad_norm > 0.0:
                raise ValueError(f"FocalAdamW: max_grad_norm = {max_grad_norm} must be positive (inf: record the norms, clip nothing)")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self._l2 = bool(l2_decay)
        self.max_grad_norm = max_grad_norm
        self._clip_state = None  # device (partial sums of squares, record): ops.new_clip_state
        self._lr_dev = None
        self._lr_host = None
        self._step_state = None  # device {., step}: this optimizer's own step counter (AdamW bias correction)

    def _arenas(self):
        arenas, seen = [], set()
        for group in self.param_groups:
            for p in group["params"]:
                ar = getattr(p, "_focal_arena", None)
                if ar is None or not ar.owns(p):
                    if p.grad is not None:
                        raise ops._lib.FocalHipError("FocalAdamW: a parameter with a gradient lives outside the arena")
                    continue
                if id(ar) not in seen:
                    seen.add(id(ar))
                    arenas.append(ar)
        return arenas

    def _span(self, ar):
        """[lo, hi) of the arena this optimizer updates.  Pretraining: everything.  Finetuning hands the optimizer only the
        head's parameters (general_utils/weight_utils.py:61-80): they sit back to back at the arena's end, and the frozen
        encoder weights in front of them must not even see weight decay -- torch skips parameters it was not given."""
        mine = {id(p) for g in self.param_groups for p in g["params"]}
        owned = [(ar.index[n][0], ar.index[n][1], id(p) in mine) for n, p in ar.params.items()]
        if all(t for _, _, t in owned):
            return 0, ar.size
        sel = [(o, k) for o, k, t in owned if t]
        lo, hi = min(o for o, _ in sel), max(o + k for o, k in sel)
        hi = min(ar.size, (hi + 7) // 8 * 8)
        if any((lo <= o < hi) and not t for o, _, t in owned):
            raise ops._lib.FocalHipError("FocalAdamW: the parameters to update are not contiguous in the arena")
        return lo, hi

    def zero_grad(self, set_to_none=True):
        # gradients are views of the arena's grad buffer: zero the buffer, keep the views
        for ar in self._arenas():
            runtime.join_all(ar.device)  # encoder backward kernels run on side streams and write the arena directly
            ar.zero_grad()

    def sync_lr(self):
        """Push param_groups[0]['lr'] to the device scalar the kernel reads (call outside graph capture)."""
        lr = float(self.param_groups[0]["lr"])
        if self._lr_dev is None:
            dev = self._arenas()[0].device
            self._lr_dev = torch.empty(1, dtype=torch.float32, device=dev)
        if lr != self._lr_host:
            self._lr_dev.fill_(lr)
            self._lr_host = lr

    @torch.no_grad()
    def reduce_gradients(self):
        """Data parallel: exact global-batch gradient = SUM over ranks of the flat gradient arena (no-op on one rank)."""
        arenas = self._arenas()
        if arenas:
            runtime.join_all(arenas[0].device)
        for ar in arenas:
            distributed.all_reduce_gradients(ar)

    @torch.no_grad()
    def reduce_buckets(self, model):
        """Data parallel, split backward pass (HipBackbone.split_backward): ([spans final after the first phase], [the rest]) per
        arena, or None when the model's backward cannot be split (DeepSense; supervised stages)."""
        bb = getattr(model, "backbone", model)
        if distributed.grad_reduce_dtype() != "fp32":
            return None   # (the bf16-wire reduction is an all-to-all + all-gather over the whole arena: one blocking call behind backward)
        if not hasattr(bb, "final_after_first_phase") or not hasattr(bb, "_encoders"):
            return None
        if not all(hasattr(e, "backward_rest") for e in bb._encoders.values()):
            return None
        arenas = self._arenas()
        if len(arenas) != 1 or arenas[0] is not bb.arena():
            return None
        ar = arenas[0]
        first = set(bb.final_after_first_phase())
        rest = [n for n in ar.index if n not in first]
        if not rest:
            return None
        return ar, ar.spans(first), ar.spans(rest)

    @torch.no_grad()
    def reduce_async(self, ar, spans):
        runtime.join_all(ar.device)
        self._works = getattr(self, "_works", []) + distributed.all_reduce_spans_async(ar, spans)

    def wait_reductions(self):
        distributed.wait_all(getattr(self, "_works", []))
        self._works = []

    @torch.no_grad()
    def step(self, closure=None, reduce=True):
        """reduce=False: the caller already ran reduce_gradients() (bench.py does, eagerly, between captured graph segments)."""
        arenas = self._arenas()
        if not arenas:
            raise ops._lib.FocalHipError("FocalAdamW: no arena-backed parameters (run the backbone on the GPU first)")
        if not torch.cuda.is_current_stream_capturing():
            self.sync_lr()
        runtime.join_all(arenas[0].device)
        if reduce:
            self.reduce_gradients()
        g0 = self.param_groups[0]
        dev = arenas[0].device
        if self._step_state is None:
            self._step_state = ops.new_step_state(dev)
        # this optimizer's step count (on the device: graph-replay safe) and the dropout seed of the next forward pass are advanced
        # by the AdamW kernel itself -- its last workgroup -- instead of two one-thread launches on the serial tail of the step
        segs = []
        for ar in arenas:
            m, v = ar.moments()
            lo, hi = self._span(ar)
            segs.append((ar.flat[lo:hi], ar.grad[lo:hi], m[lo:hi], v[lo:hi], ar.shadow[lo:hi] if ar.shadow is not None else None))
        clip = None
        if self.max_grad_norm is not None:
            # behind the gradient reduction: every rank takes the norm of the same reduced gradient (no collective of its own)
            if self._clip_state is None:
                self._clip_state = ops.new_clip_state(dev)
            ops.grad_norm([s[1] for s in segs], self._clip_state)
            clip = (self._clip_state, self.max_grad_norm)
        self._update(arenas, segs, g0, clip, dev)
        for ar in arenas:
            ar.mark_shadow_fresh()

    def _update(self, arenas, segs, g0, clip, dev):
        """The update launches of step(): segs[i] = (w, g, m, v, shadow) of arenas[i]'s span."""
        ops.adamw_multi(segs, self._lr_dev, self._step_state, g0["betas"][0], g0["betas"][1], g0["eps"],
                        g0["weight_decay"], self._l2, advance=True, seed_state=runtime.rng_state(dev), clip=clip)

    def clip_stats(self):
        """Gradient-norm statistics since the last call (one device-to-host copy; the record is reset), or None with clipping off or
        before the first step: {steps, clipped, skipped, norm_mean, norm_max, last_norm, ...} (ops.read_clip_stats)."""
        if self._clip_state is None:
            return None
        return ops.read_clip_stats(self._clip_state)

    # ---- resume support (the reference saves weights only; SURVEY 8f rank 3 asks for optimizer state as well)
    def train_state(self):
        """Everything `step()` depends on besides the weights: the step count and both moment buffers of every arena."""
        torch.cuda.synchronize()
        arenas = self._arenas()
        return {"step": int(self._step_state[1].item()) if self._step_state is not None else 0,
                "lr": float(self.param_groups[0]["lr"]),  # informational: on resume the replayed scheduler owns the LR
                "moments": [tuple(t.detach().cpu().clone() for t in ar.moments()) for ar in arenas]}

    def load_train_state(self, state):
        arenas = self._arenas()
        if len(arenas) != len(state["moments"]):
            raise ops._lib.FocalHipError("FocalAdamW.load_train_state: arena count differs (run one forward/backward first)")
        for ar, (m, v) in zip(arenas, state["moments"]):
            am, av = ar.moments()
            if am.numel() != m.numel():
                raise ops._lib.FocalHipError("FocalAdamW.load_train_state: moment size differs from the arena")
            am.copy_(m.to(am.device))
            av.copy_(v.to(av.device))
        dev = arenas[0].device
        if self._step_state is None:
            self._step_state = ops.new_step_state(dev)
        self._step_state[1] = int(state["step"])


class FocalLAMB(FocalAdamW):
    """LAMB (You et al. 2020, Algorithm 2) over the arena, with AdamW's conventions and AdamW's state (m, v, the device step count): a
    "layer" is one tensor of ParamArena.index inside the optimizer's span,
        u = r + wd * w,  phi = |w| / |u| (1 where a norm is zero or not finite, or the tensor is not adapted),  w -= lr * min(phi, max_trust) * u
    in two launches per arena (ops.lamb_multi).  exclude_1d (the published BERT recipe): tensors with ndim <= 1 -- biases, norm scales and
    shifts -- are neither adapted nor decayed.  Everything else -- zero_grad, sync_lr, the reductions, clipping, train_state -- is FocalAdamW's."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=None, exclude_1d=True, max_trust=float("inf")):
        if not isinstance(exclude_1d, bool):
            raise ValueError(f"FocalLAMB: exclude_1d = {exclude_1d!r} must be a bool")
        max_trust = float(max_trust)
        if not max_trust > 0.0:
            raise ValueError(f"FocalLAMB: max_trust = {max_trust} must be positive (inf: no clamp)")
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, l2_decay=False, max_grad_norm=max_grad_norm)
        self.exclude_1d = exclude_1d
        self.max_trust = max_trust
        self._tables = {}  # (arena, span) -> (arena, uploaded ops.lamb_table)

    def _table(self, ar, lo, hi):
        key = (id(ar), lo, hi)
        hit = self._tables.get(key)
        if hit is None or hit[0] is not ar:
            if torch.cuda.is_current_stream_capturing():
                raise ops._lib.FocalHipError("FocalLAMB: the piece table is uploaded outside graph capture (run one eager step first)")
            hit = self._tables[key] = (ar, ops.lamb_table_upload(ops.lamb_table(ar.index.values(), lo, hi, self.exclude_1d), ar.device))
        return hit[1]

    def _update(self, arenas, segs, g0, clip, dev):
        # (a segment is the arena's flat buffer cut to the span: its storage offset is the span's start)
        tables = [self._table(ar, s[0].storage_offset(), s[0].storage_offset() + s[0].numel()) for ar, s in zip(arenas, segs)]
        ops.lamb_multi(segs, tables, self._lr_dev, self._step_state, g0["betas"][0], g0["betas"][1], g0["eps"], g0["weight_decay"],
                       max_trust=self.max_trust, advance=True, seed_state=runtime.rng_state(dev), clip=clip)

    def trust_stats(self):
        """The trust ratios of the last step that was not skipped (one device-to-host copy), or None before the first step:
        {tensors, min, min_name, median, max, max_name} over the adapted tensors (all of them if none is adapted), and "phi": {name: phi}."""
        arenas = self._arenas()
        live = [(ar, t) for ar, t in self._tables.values() if any(ar is a for a in arenas)]
        if not live or self._step_state is None:
            return None
        rec = torch.cat([t["record"] for _, t in live]).cpu().view(-1, ops._lib.LAMB_RECORD_WORDS)
        names, adapted = [], []
        for ar, t in live:
            keys = list(ar.index)
            names += [keys[i] for i in t["rows"]]
            adapted += [bool(f & ops._lib.LAMB_ADAPT) for _, _, f in t["tensors"]]
        phi = rec[:len(names), 0].tolist()
        pick = [i for i, a in enumerate(adapted) if a] or list(range(len(names)))
        order = sorted(pick, key=lambda i: phi[i])
        lo, hi, mid = order[0], order[-1], order[len(order) // 2]
        median = phi[mid] if len(order) % 2 else 0.5 * (phi[order[len(order) // 2 - 1]] + phi[mid])
        return {"tensors": len(order), "min": phi[lo], "min_name": names[lo], "median": median, "max": phi[hi], "max_name": names[hi],
                "phi": dict(zip(names, phi))}
