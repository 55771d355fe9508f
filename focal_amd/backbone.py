"""Shared plumbing of the two backbones: arena ownership, operand dtype, autograd glue."""
from typing import NamedTuple, Tuple

import torch
import torch.nn as nn

from . import runtime
from ._lib import FocalHipError
from .arena import ParamArena

APE_PREFIX = "absolute_pos_embed."


class HotRule(NamedTuple):
    """Which parameters live in the arena: `rule(name)` = not under a `dead` prefix, or under an `also` prefix.  `has_head`: the
    classifier head (class layer, modality fusion) is among them, so `class_head=True` can run."""
    dead: Tuple[str, ...]
    also: Tuple[str, ...]
    has_head: bool

    def __call__(self, name):
        return (not name.startswith(self.dead)) or name.startswith(self.also)


def hot_rule(stage="pretrain", supervised=False, ape=False, deepsense_multiloc=False):
    """The whole table of hot sets.  (loc_context_layers. / loc_fusion_layer. -- SW_Transformer's location fusion -- exist only on
    multi-location datasets and are hot there: focal_amd/loc_engine.py.  DeepSense's loc_fusion_layers. (MeanFusionBlock, no parameters
    on the shipped configs) stays dead.)"""
    if supervised:
        # Supervised training from scratch (train_utils/supervised_train.py: every parameter is handed to the optimizer): everything
        # `backbone(freq_x, class_head=True)` touches gets a gradient -- the patch embedding included (it is frozen only in FOCAL
        # pretraining) -- and the projection heads of the contrastive path do not (torch skips their `grad is None`).
        dead = (APE_PREFIX, "mod_extractors.", "loc_fusion_layers.", "loc_context_layers.", "loc_fusion_layer.", "mod_projectors.")
        return HotRule(dead, (APE_PREFIX,) if ape else (), True)
    # Parameters that receive a gradient in FOCAL pretraining; on a multi-location dataset that includes the location
    # fusion of SW_Transformer (on single-location datasets those parameters do not exist: the set is unchanged).
    dead = ("patch_embed.", "class_layer.", "mod_fusion_layers.", APE_PREFIX, "mod_extractors.", "loc_fusion_layers.")
    if stage == "finetune":
        # Classifier / finetune stage: the head (class layer, modality fusion) joins the arena; it is what finetuning trains
        # (general_utils/weight_utils.py:61-80), the encoder weights stay there as the frozen operands of the forward pass.  The position
        # embedding stays out: it is a frozen operand there, read where it lives.
        return HotRule(dead, ("class_layer.", "mod_fusion_layers."), True)
    also = ()
    if ape:
        # FOCAL pretraining with `APE: true`: the absolute position embedding is added to the tokens and trains (the reference's
        # freeze_patch_embedding matches "patch_embed" only, general_utils/weight_utils.py:85-94), so it joins the arena.
        also += (APE_PREFIX,)
    if deepsense_multiloc:
        # FOCAL pretraining of DeepSense on a multi-location dataset: the second ConvBlock of every modality (mod_extractors.*, behind
        # the mean over the locations) runs and trains (focal_amd/deepsense_engine.py: DeepSenseMultiLocEncoder); on single-location
        # datasets those parameters are dead (the reference skips the block).
        also += ("mod_extractors.",)
    return HotRule(dead, also, False)


class HipBackbone(nn.Module):
    def _init_hip(self, args, deepsense_multiloc=False):
        self.compute_dtype = runtime.compute_dtype_from(args)
        self.supervised = getattr(args, "train_mode", "") == "supervised"
        # (with APE off -- every shipped config -- the rule, and with it the arena's layout, is what it was)
        ape = bool((getattr(self, "config", None) or {}).get("APE", False))
        self._hot = hot_rule(getattr(args, "stage", "pretrain"), self.supervised, ape, deepsense_multiloc)
        self._arena = None
        self._named = None
        self._fwd_calls = 0
        # data parallel: encoders stop their backward pass where most gradient bytes are final (focal_amd/graph_step.py issues the first
        # all-reduce bucket there) and park the rest here for backward_continue()
        self.split_backward = False
        self.pending_backward = []
        self.register_load_state_dict_post_hook(lambda module, keys: module._after_load())

    def _after_load(self):
        if self._arena is not None and self._arena.intact():
            self._arena.sync_shadow(force=True)

    def arena(self):
        if self._arena is None or not self._arena.intact():
            self._arena = ParamArena(self, self._hot, self.compute_dtype)
            self._named = None
        self._arena.sync_shadow()
        return self._arena

    def param(self, name):
        if self._named is None:
            self._named = dict(self.named_parameters())
        return self._named[name]

    def backward_continue(self):
        """The parked second halves of the encoders' backward passes (split_backward), each on the stream its first half ran on,
        all started from one fork point and joined back before returning."""
        pend, self.pending_backward = self.pending_backward, []
        if not pend:
            return
        dev = pend[0][2].device
        cur = torch.cuda.current_stream(dev)
        point = runtime.fork_point(dev)
        with torch.no_grad():
            for engine, saved, st in pend:
                if st != cur:
                    st.wait_event(point)
                with torch.cuda.stream(st):
                    engine.backward_rest(saved)
        runtime.join_all(dev)

    def final_after_first_phase(self):
        """Names of the arena parameters whose gradients are final when the first phase of a split backward pass ends: everything but
        the encoder stages in front of the last one (their blocks and the PatchMerging that follows them)."""
        import re
        ar = self.arena()
        stage_of = {n: re.match(r"(freq_interval_layers\.[^.]+\.[^.]+)\.(\d+)\.", n) for n in ar.index}
        last = {}
        for m in stage_of.values():
            if m:
                last[m.group(1)] = max(last.get(m.group(1), 0), int(m.group(2)))
        # (the position embedding's gradient is the LAST thing an encoder's backward pass writes: never final after the first phase)
        return [n for n, m in stage_of.items() if not n.startswith(APE_PREFIX) and (m is None or int(m.group(2)) == last[m.group(1)])]

    def rng_state(self):
        return runtime.rng_state(next(self.parameters()).device)

    def _anchor(self, device):
        # torch.autograd only schedules a node whose inputs need grad; parameter gradients are written straight into
        # the arena by the HIP kernels, so a dummy differentiable input keeps each encoder node alive.
        return runtime.anchor(device)  # (one cached leaf per device: a fresh torch.zeros per stage call was a fill launch in the step)

    # ------------------------------------------------------------------------------------------------ the pass protocol
    # What FOCAL.forward and the training loops call.  A model supplies `_run_encoders` (which stream an encoder gets, what it is fed),
    # `_join_features` (how the classifier head reads the modality features), `views_share_pass` and, where it has any, `_before_fork`
    # and `finish_views`.
    def forward(self, freq_x, class_head=True, proj_head=False, defer_join=False, view_index=None, views_in_batch=1):
        """`view_index`: FOCAL.forward numbers its two backbone calls 0 / 1; `views_in_batch`: both views in this one pass.  Only a
        backbone with batch statistics (DeepSense) reads either."""
        if class_head:
            return self.forward_classifier(freq_x)
        return self.forward_encoder(freq_x, proj_head, defer_join, view_index, views_in_batch)

    def forward_encoder(self, freq_x, proj_head=False, defer_join=False, view_index=None, views_in_batch=1):
        view = self._fwd_calls
        self._fwd_calls = (self._fwd_calls + 1) & 0xFFFF
        # one HIP stream per modality encoder (see focal_amd/runtime.py: side streams); joined before returning
        dev = next(self.parameters()).device
        if dev.type != "cuda":
            raise FocalHipError("the FOCAL HIP path needs the model on a ROCm device (no CPU fallback)")
        cur = torch.cuda.current_stream(dev)
        # The parameter arena (and its bf16 shadow) must exist BEFORE the fork point: built lazily inside the first encoder's pass it was
        # filled on that encoder's stream AFTER the point the other encoders start from, and on a fresh model they could read a zero arena
        # (round 5: test_train_step_loss_and_gradients[bf16] saw an all-zero seismic embedding in 2 of 16 fresh processes).
        self.arena()
        self._before_fork(view_index)
        point = runtime.fork_point(dev)  # every encoder starts from here: none waits for the one launched before it
        out = self._run_encoders(freq_x, proj_head, view, dev, cur, point, view_index, views_in_batch)
        if not defer_join:  # FOCAL.forward joins once after both views so that their encoders overlap
            runtime.join_all(dev)
        return {mod: out[mod] for mod in self.modalities}

    def _before_fork(self, view_index):
        """Launches of the caller's stream that every encoder's pass reads (DeepSense: the re-ordered weights)."""

    def finish_views(self):
        """After both views' passes of a step (FOCAL.forward); DeepSense applies its BatchNorm running-buffer updates here."""

    def forward_classifier(self, freq_x):
        """`backbone(freq_x, class_head=True)` -> logits (reference: models/SW_Transformer.py:269-276, models/DeepSense.py:154-157).  This is
        the finetuning path: the encoders in front run forward-only (finetuning freezes them, general_utils/weight_utils.py:61-80), the
        head -- modality fusion (SW_Transformer) + class layer -- is one differentiable node (focal_amd/head_engine.py)."""
        if not self._hot.has_head:
            raise NotImplementedError("class_head=True needs the classifier head in the parameter arena: build the model with "
                                      "args.stage = 'finetune' (or supervised train_mode)")
        # supervised training from scratch (train_utils/supervised_train.py): the gradient flows on into the encoders
        with torch.set_grad_enabled(self.supervised and torch.is_grad_enabled()):
            feats = self.forward_encoder(freq_x)
        return run_stage(self, self._class_head, self._join_features([feats[m] for m in self.modalities]), self.training)


def _join_after_backward(device):
    """When the autograd engine has run every node of this backward pass, the thread that called backward() makes its current stream
    wait for all encoder side streams (runtime.join_all: event waits).  Queued by every stage node: a few redundant waits per pass, no
    state that an exception inside a backward pass could leave behind."""
    key = torch.device(device)
    torch.autograd.Variable._execution_engine.queue_callback(lambda: runtime.join_all(key))




class StageFn(torch.autograd.Function):
    """One autograd node around an engine object exposing forward(x | [x, ...], *args) -> (y, saved) / backward(saved, dy) -> the input
    gradient(s): None (the inputs are leaves of the step: spectra), one tensor, or a list with one per input (the location stage)."""

    @staticmethod
    def forward(ctx, anchor, engine, args, as_list, *xs):
        # the inputs may have been produced on other streams (encoders run on side streams): keep their blocks alive for this one
        cur = torch.cuda.current_stream(xs[0].device)
        for x in xs:
            x.record_stream(cur)
        y, saved = engine.forward(list(xs) if as_list else xs[0], *args)
        ctx.engine, ctx.saved, ctx.n = engine, saved, len(xs)
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = dy.contiguous()
        dy.record_stream(torch.cuda.current_stream(dy.device))  # produced by the loss head on the caller's stream
        dxs = ctx.engine.backward(ctx.saved, dy)
        ctx.saved = None
        # The parameter gradients were written straight into the arena on THIS stream (the stage's forward stream).  Autograd orders the
        # caller's stream behind the streams of the leaves that received a gradient through it -- none here (the anchor gets None) -- so a
        # caller that reads p.grad right after backward() raced the last kernels of a side-stream encoder (round 5).  The optimizer joins
        # every side stream itself; a callback at the END of the backward pass does it for everybody else: an event wait, no kernel.  (Not
        # a wait per stage: the caller's stream carries the first modality's own backward pass, which would then queue behind every other
        # modality's -- measured -7 % on the four-modality HAR4 step.)
        _join_after_backward(dy.device)
        if dxs is None:
            dxs = (None,) * ctx.n
        elif torch.is_tensor(dxs):
            dxs = (dxs,)
        return (None, None, None, None, *dxs)


def run_stage(backbone, engine, x, *args, input_grads=False):
    """engine.forward(x, *args) as one autograd node; x is one tensor or a list of them (the engine is handed what it was given).  The
    node exists when grad is enabled -- with `input_grads` (a stage behind other nodes, which trains only with them: the location fusion
    over a modality's L encoder outputs; autograd hands each encoder its gradient on the stream its forward ran on) only when some input
    requires grad.  Otherwise the engine's forward runs directly."""
    xs = x if isinstance(x, (list, tuple)) else (x,)
    if torch.is_grad_enabled() and (not input_grads or any(t.requires_grad for t in xs)):
        return StageFn.apply(backbone._anchor(xs[0].device), engine, args, x is xs, *xs)
    cur = torch.cuda.current_stream(xs[0].device)
    for t in xs:
        t.record_stream(cur)
    y, _ = engine.forward(list(xs) if x is xs else x, *args)
    return y
