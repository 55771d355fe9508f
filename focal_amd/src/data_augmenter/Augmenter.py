"""View generation in front of the encoders (reference: data_augmenter/Augmenter.py:25-227).

`forward("random", time_loc_inputs)` draws ONE augmenter from the configured pool per call, flips a coin per
(location, modality) as the reference's augmenter classes do, and always ends with the time->frequency transform,
which runs on the HIP DFT kernel.  The augmentation arithmetic (negation, scaling, horizontal flip, interval
permutation, phase shift) is folded into that kernel (`focal_augment_fft_fwd`); in this form the random draws are made on the
host, unseeded as in the reference.
`forward_random_pair(time_loc_inputs)` (round 5) is what the training loop uses: BOTH views of a step with every draw made on the
DEVICE (`focal_view_draw`: the augmenter of each view, the per-(location, modality) coins, scale factors, interval orders, phase
angles, warp knots), the warp tables built on the device (`focal_warp_plan_multi`) and the transforms reading their augmentation
from the drawn records -- launches of fixed shape, so the views are part of the captured step and a replay draws fresh ones.
`forward_fixed_device(time_loc_inputs)` is the same for the supervised `fixed` pipeline: Mixup's draws (`focal_mixup_draw`), the mix of
all modalities (`focal_mixup_multi`), the phase-shift draw and one transform call, a fixed launch sequence inside the captured
classifier step; `forward_fixed` keeps the host-drawn form.
`time_warp` / `mag_warp` wrap tsai's random-spline transforms, whose source is not available in this build environment: they
are restated from tsai's published algorithm in focal_amd/warp.py (the curve, drawn on the host like every other augmenter's
randomness) and run as one device pass in front of the transform (focal_warp_fwd); see that module for the one documented
deviation (cardinal-form signal spline with clamped ends).
"""
import logging
import math
import os
import sys
from math import floor
from random import randint, random

import numpy as np
import torch

_ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "..", ".."))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

from focal_amd import ops  # noqa: E402


# Every augmenter is a host-side DRAW (what the reference's classes do with `random()` / `torch.normal` / `torch.randperm`)
# returning keyword arguments of `ops.fft_realpack`: the arithmetic itself is folded into the DFT kernel
# (focal_augment_fft_fwd), so a view costs one pass over the window instead of an augmentation pass plus a transform pass.
def _negation(x, cfg):  # NegationAugmenter.py:34
    return dict(scale=-1.0)


def _scaling(x, cfg):  # ScalingAugmenter.py:35-36: one N(1, std) factor per (loc, mod)
    return dict(scale=float(np.random.normal(1.0, cfg["std"])))


def _horizontal_flip(x, cfg):  # HorizontalFlipAugmenter.py:34: flip intervals and samples
    return dict(flip=True)


def _permutation(x, cfg):  # PermutationAugmenter.py:35-36: one random interval order for the whole batch
    return dict(perm=torch.randperm(x.shape[2]).tolist())


def _time_warp(x, cfg):  # TimeWarpAugmenter.py:18,44 -> tsai TSTimeWarp (restated in focal_amd/warp.py): one curve per (loc, mod)
    from focal_amd import warp
    L = x.shape[2] * x.shape[3]
    k0, w = warp.time_warp_tables(warp.warp_positions(L, warp.draw_knots(cfg["order"], cfg["magnitude"]), cfg["order"]))
    return dict(pre=lambda t: ops.time_warp(t, torch.from_numpy(k0).to(t.device), torch.from_numpy(w).to(t.device)))


def _mag_warp(x, cfg):  # MagWarpAugmenter.py:18,44 -> tsai TSMagWarp
    from focal_amd import warp
    L = x.shape[2] * x.shape[3]
    mult = warp.random_curve(L, warp.draw_knots(cfg["order"], cfg["magnitude"]), cfg["order"]).astype(np.float32)
    return dict(pre=lambda t: ops.mag_warp(t, torch.from_numpy(mult).to(t.device)))


def _phase_shift(x, cfg):  # PhaseShiftAugmenter.py:39-54: rotate every complex bin by one random angle
    return dict(phase=(random() - 0.5) * 2 * math.pi)


# The four augmenters whose parameters travel in a focal_view_extra (include/focal_hip.h).  Beside the dataset's own section `cfg` carries
# what Augmenter.__init__ derived for the (location, modality) at hand: jitter "std", time_mask "max_duration", freq_mask "max_band_width".
def _jitter(x, cfg):  # JitterAugmenter.py:37-40: x + N(0, 1) * std.  The reference draws the noise tensor; here one key, and the kernel the noise
    return dict(jitter=(float(cfg["std"]), int(torch.randint(0, 2 ** 32, (1,), dtype=torch.int64).item())))


def _channel_shuffle(x, cfg):  # ChannelShuffleAugmenter.py:34-37: one channel order for the whole batch
    return dict(chan=torch.randperm(x.shape[1]).tolist())


def _time_mask(x, cfg):  # TimeMaskAugmenter.py:37-41: interval-sized numbers, applied to the SAMPLE axis (sic); the slice clips at n
    duration = randint(1, cfg["max_duration"])
    start = torch.randint(0, x.shape[2] - duration, (1,)).item()
    n = x.shape[3]
    return dict(time_mask=(min(start, n), min(start + duration, n) - min(start, n)))


def _freq_mask(x, cfg):  # FreqMaskAugmenter.py:44-48: a band of bins of all 2C channels, no mirror bin
    band = randint(1, cfg["max_band_width"])
    start = torch.randint(0, x.shape[-1] - band, (1,)).item()
    return dict(freq_mask=(start, band))


def _mixup_in_random_pool(x, cfg):  # MixupAugmenter mixes samples AND labels: it belongs to the supervised `fixed` pipeline
    raise NotImplementedError("mixup is a `fixed`-pipeline augmenter (supervised training); it is not drawn as a FOCAL view")


def draw_mixup(cfg, shapes):
    """The host draws of one Mixup call in mode "random_batch" (input_utils/mixup_utils.py:154-176 `_params_per_batch`, :252-281
    `_mix_batch_random`, :32-54 `rand_bbox`), in the reference's order: apply?, cutmix?, lambda, one batch permutation, and for
    CutMix one box centre per (location, modality) tensor.  shapes = {(loc, mod): (B, C, I, S)} in iteration order.
    Returns None (no mixing) or dict(lam=, cut=, perm=, boxes={(loc, mod): (yl, yh, xl, xh)})."""
    if cfg.get("mode", "batch") != "random_batch" or cfg.get("cutmix_minmax") is not None:
        raise NotImplementedError("Mixup: only mode 'random_batch' without cutmix_minmax (the shipped configuration) is built")
    if not (np.random.rand() < cfg["prob"]):
        return None
    ma, ca = cfg["mixup_alpha"], cfg["cutmix_alpha"]
    cut = False
    if ma > 0.0 and ca > 0.0:
        cut = bool(np.random.rand() < cfg["switch_prob"])
        lam = np.random.beta(ca, ca) if cut else np.random.beta(ma, ma)
    elif ma > 0.0:
        lam = np.random.beta(ma, ma)
    elif ca > 0.0:
        cut, lam = True, np.random.beta(ca, ca)
    else:
        raise AssertionError("One of mixup_alpha > 0., cutmix_alpha > 0. should be true.")
    lam = float(lam)
    if lam == 1:
        return None
    B = next(iter(shapes.values()))[0]
    out = dict(lam=lam, cut=cut, perm=torch.randperm(B), boxes={})
    if cut:
        for key, (_, _, I, S) in shapes.items():
            ratio = np.sqrt(1 - lam)
            cut_h, cut_w = int(I * ratio), int(S * ratio)
            cy, cx = np.random.randint(0, I), np.random.randint(0, S)
            out["boxes"][key] = (int(np.clip(cy - cut_h // 2, 0, I)), int(np.clip(cy + cut_h // 2, 0, I)),
                                 int(np.clip(cx - cut_w // 2, 0, S)), int(np.clip(cx + cut_w // 2, 0, S)))
    return out


TIME_AUGMENTERS = {"no": None, "mixup": _mixup_in_random_pool, "negation": _negation, "scaling": _scaling, "horizontal_flip": _horizontal_flip,
                   "permutation": _permutation, "time_warp": _time_warp, "mag_warp": _mag_warp, "jitter": _jitter,
                   "channel_shuffle": _channel_shuffle, "time_mask": _time_mask}
FREQ_AUGMENTERS = {"no": None, "phase_shift": _phase_shift, "freq_mask": _freq_mask}


def _transform_all(items):
    """{loc: {mod: fft_realpack keyword arguments}} -> {loc: {mod: spectrum}}: every (location, modality) of a view in ONE call
    (ops.fft_realpack_multi: the short-row sensor modalities share a launch instead of one launch each)."""
    flat = [(loc, mod) for loc, mods in items.items() for mod in mods]
    outs = ops.fft_realpack_multi([items[loc][mod] for loc, mod in flat])
    res = {loc: {} for loc in items}
    for (loc, mod), o in zip(flat, outs):
        res[loc][mod] = o
    return res


class Augmenter:
    def __init__(self, args) -> None:
        self.args = args
        self.modalities = args.dataset_config["modality_names"]
        self.locations = args.dataset_config["location_names"]
        if args.train_mode != "supervised" and args.stage == "pretrain":
            pool = args.dataset_config[args.learn_framework]["random_augmenters"]
        else:
            pool = args.dataset_config[args.model]["fixed_augmenters"]
        self.time_aug_names, self.freq_aug_names = list(pool["time_augmenters"]), list(pool["freq_augmenters"])
        for n in self.time_aug_names:
            if n not in TIME_AUGMENTERS:
                raise Exception(f"Invalid augmenter provided: {n}")
        for n in self.freq_aug_names:
            if n not in FREQ_AUGMENTERS:
                raise Exception(f"Invalid augmenter provided: {n}")
        self.aug_names = self.time_aug_names + self.freq_aug_names
        self._derived = self._derive_extended(args.dataset_config)

    def _derive_extended(self, cfg):
        """Per-(location, modality) parameters of jitter / channel_shuffle / time_mask / freq_mask as the reference's classes derive them at
        construction, for the ones the pool names; an impossible configuration is refused here, with the key to fix."""
        out = {}
        slots = [(loc, mod) for loc in self.locations for mod in self.modalities]
        if "jitter" in self.aug_names:  # JitterAugmenter.init_value_range: value_range[mod] / 100 * std_in_percent
            sec = cfg.get("jitter", {})
            vr = sec.get("value_range")
            if not isinstance(vr, dict) or any(mod not in vr for mod in self.modalities):
                raise ValueError("jitter is in the augmenter pool but `jitter.value_range` does not give every modality's range: add "
                                 "`value_range: {<modality>: <largest absolute time-domain sample>, ...}` for " + ", ".join(self.modalities)
                                 + " to the dataset config's `jitter` section")
            out["jitter"] = {k: {"std": float(vr[k[1]]) / 100 * sec["std_in_percent"]} for k in slots}
        if "channel_shuffle" in self.aug_names:
            ch = cfg.get("loc_mod_in_time_channels", {})
            for loc, mod in slots:
                c = ch.get(loc, {}).get(mod)
                if c is not None and c > ops._lib.VIEW_MAX_CHANNELS:
                    raise ValueError(f"channel_shuffle: `loc_mod_in_time_channels.{loc}.{mod}` = {c} exceeds the {ops._lib.VIEW_MAX_CHANNELS} "
                                     "channels the shuffle is built for")
            out["channel_shuffle"] = {k: {} for k in slots}
        if "time_mask" in self.aug_names:  # TimeMaskAugmenter.py:17
            d = floor(cfg["num_segments"] * cfg["time_mask"]["mask_ratio"])
            if d < 1:
                raise ValueError(f"time_mask: floor(num_segments * `time_mask.mask_ratio`) = {d}: the longest mask must be at least 1")
            out["time_mask"] = {k: {"max_duration": d} for k in slots}
        if "freq_mask" in self.aug_names:  # FreqMaskAugmenter.py:17-24: per modality, from the first location that has it
            widths = {}
            for loc, mod in slots:
                if mod not in widths:
                    widths[mod] = floor(cfg["loc_mod_spectrum_len"][loc][mod] * cfg["freq_mask"]["mask_ratio"])
                    if widths[mod] <= 1:
                        raise ValueError(f"freq_mask: floor(loc_mod_spectrum_len.{loc}.{mod} * `freq_mask.mask_ratio`) = {widths[mod]}: "
                                         "the widest band must exceed 1 (the reference asserts it)")
            out["freq_mask"] = {k: {"max_band_width": widths[k[1]]} for k in slots}
        return out

    def to(self, device):
        return self

    def forward(self, option, time_loc_inputs, labels=None, return_aug_id=False, return_aug_mods=False):
        time_loc_inputs, labels = self.move_to_target_device(time_loc_inputs, labels)
        if option == "random":
            out = self.forward_random(time_loc_inputs)
        elif option == "fixed":
            out = self.forward_fixed(time_loc_inputs, labels)
        elif option == "no":
            out = self.fft_preprocess(time_loc_inputs)
        else:
            raise Exception(f"Invalid augmentation option: {option}")
        return out if labels is None else (out, labels)

    def _draw(self, fn, name, inputs):
        """Per (location, modality): the reference's coin flip, then the augmenter's own draw -> fft_realpack keyword arguments."""
        out = {}
        for loc in self.locations:
            out[loc] = {}
            for mod in self.modalities:
                hit = fn is not None and random() < self.args.dataset_config[name]["prob"]
                if hit:
                    sec = self.args.dataset_config.get(name, {})
                    extra = self._derived.get(name, {}).get((loc, mod))
                    out[loc][mod] = fn(inputs[loc][mod], dict(sec, **extra) if extra else sec)
                else:
                    out[loc][mod] = {}
        return out

    def forward_fixed(self, time_loc_inputs, labels=None):
        """The supervised pipeline (reference :52-74): every configured time augmenter in order, the transform, every configured
        frequency augmenter.  Built: `mixup` (focal_mixup_fwd) / `no` in the time domain, `phase_shift` (folded into the DFT) /
        `no` in the frequency domain -- the shipped `fixed_augmenters`.
        Reference quirk, reproduced: forward_fixed resets the labels to the ORIGINAL ones before the frequency stage (:66
        `augmented_freq_loc_inputs, augmented_labels = freq_loc_inputs, labels`), so Mixup's mixed soft targets never reach the
        loss -- the samples are mixed, the labels are not; this returns nothing but the spectra (the caller keeps its labels)."""
        x = time_loc_inputs
        for name in self.time_aug_names:
            if name == "no":
                continue
            if name != "mixup":
                raise NotImplementedError(f"fixed-pipeline time augmenter {name!r} is not built (shipped configs use mixup / no)")
            draw = draw_mixup(self.args.dataset_config["mixup"], {(loc, mod): tuple(t.shape) for loc, mods in x.items() for mod, t in mods.items()})
            if draw is not None:
                perm = draw["perm"].to(torch.int32).to(self.args.device)
                x = {loc: {mod: ops.mixup(t.contiguous(), perm, draw["lam"], draw["boxes"].get((loc, mod)) if draw["cut"] else None)
                           for mod, t in mods.items()} for loc, mods in x.items()}
        kw = {loc: {mod: {} for mod in mods} for loc, mods in x.items()}
        for name in self.freq_aug_names:
            if name == "no":
                continue
            if name != "phase_shift":
                raise NotImplementedError(f"fixed-pipeline frequency augmenter {name!r} is not built (shipped configs use phase_shift / no)")
            d = self._draw(FREQ_AUGMENTERS[name], name, x)
            for loc in d:
                for mod in d[loc]:
                    kw[loc][mod].update(d[loc][mod])
        return _transform_all({loc: {mod: dict(x=t.contiguous(), out=self._static_out(loc, mod, t), **kw[loc][mod]) for mod, t in mods.items()}
                               for loc, mods in x.items()})

    def forward_random(self, time_loc_inputs):
        """ONE augmenter from the (time + freq) pool per call (reference :76-113); its arithmetic runs inside the DFT kernel."""
        k = np.random.randint(len(self.aug_names))
        name = self.aug_names[k]
        fn = TIME_AUGMENTERS[name] if k < len(self.time_aug_names) else FREQ_AUGMENTERS[name]
        kw = self._draw(fn, name, time_loc_inputs)
        items = {}
        for loc, mods in time_loc_inputs.items():
            items[loc] = {}
            for mod, x in mods.items():
                k = dict(kw[loc][mod])
                pre = k.pop("pre", None)  # the spline warps are a pass of their own in front of the transform
                src = pre(x.contiguous()) if pre is not None else x.contiguous()
                items[loc][mod] = dict(x=src, out=self._view_slot(loc, mod, x), **k)
        return _transform_all(items)

    # ------------------------------------------------------------------------------------------ random views, drawn on the device
    def device_draws_supported(self):
        """The pool is made of augmenters focal_view_draw knows (every shipped `random_augmenters` pool is)."""
        cfg = self.args.dataset_config
        n_slots = sum(len(cfg["modality_names"]) for _ in cfg["location_names"])
        return (all(n in ops.VIEW_KINDS for n in self.aug_names) and 1 <= len(self.aug_names) <= ops._lib.VIEW_MAX_POOL
                and n_slots <= ops._lib.VIEW_MAX_SLOTS)

    def _device_state(self, inputs):
        flat = [(loc, mod) for loc in inputs for mod in inputs[loc]]
        key = tuple((loc, mod, tuple(inputs[loc][mod].shape), inputs[loc][mod].device) for loc, mod in flat)
        # one state PER batch shape, never dropped: a captured step graph holds the addresses of its plans / views / warp tables, and the
        # last batch of an epoch (no drop_last) is smaller -- replacing the state would hand those blocks back to the allocator while the
        # graph keeps writing into them from the next epoch on
        states = self.__dict__.setdefault("_dev_states", {})
        st = states.get(key)
        if st is not None:
            return st
        cfg = self.args.dataset_config
        dv, shape = self._derived, lambda k: inputs[k[0]][k[1]].shape
        pool = ops.view_pool([(n, cfg[n]["prob"] if n != "no" else 0.0) for n in self.aug_names],
                             [inputs[loc][mod].shape[2] for loc, mod in flat],
                             scaling_std=cfg.get("scaling", {}).get("std", 0.2),
                             mag_warp=(cfg.get("mag_warp", {}).get("magnitude", 0.05), cfg.get("mag_warp", {}).get("order", 4)),
                             time_warp=(cfg.get("time_warp", {}).get("magnitude", 0.2), cfg.get("time_warp", {}).get("order", 6)),
                             jitter_std=[dv["jitter"][k]["std"] for k in flat] if "jitter" in dv else None,
                             channels=[shape(k)[1] for k in flat] if "channel_shuffle" in dv else None,
                             time_mask=[(dv["time_mask"][k]["max_duration"], shape(k)[2]) for k in flat] if "time_mask" in dv else None,
                             freq_mask=[(dv["freq_mask"][k]["max_band_width"], shape(k)[3]) for k in flat] if "freq_mask" in dv else None)
        dev = inputs[flat[0][0]][flat[0][1]].device
        n = len(flat)
        warps = any(k in ("mag_warp", "time_warp") for k in self.aug_names)
        # (a pool that names jitter / channel_shuffle / time_mask / freq_mask draws an extra record beside each plan)
        extras = ops.new_view_extras(2, n, dev) if any(k in ops.VIEW_KINDS_EX for k in self.aug_names) else None
        st = {"key": key, "flat": flat, "pool": pool, "plans": ops.new_view_plans(2, n, dev), "extras": extras, "warps": warps,
              "both": {k: torch.empty((2 * inputs[k[0]][k[1]].shape[0], 2 * inputs[k[0]][k[1]].shape[1]) + tuple(inputs[k[0]][k[1]].shape[2:]),
                                      dtype=torch.float32, device=dev) for k in flat},
              # the warped copies and the tables of (view, slot): written only when the plan drew a warp
              "warped": [{k: torch.empty_like(inputs[k[0]][k[1]], dtype=torch.float32) for k in flat} for _ in range(2)] if warps else None,
              "tables": [{k: torch.empty(2 * inputs[k[0]][k[1]].shape[2] * inputs[k[0]][k[1]].shape[3], dtype=torch.float32, device=dev)
                          for k in flat} for _ in range(2)] if warps else None}
        from focal_amd import runtime
        st["view_state"] = runtime.view_state(dev)  # (may broadcast the job's draw seed: eager, first step, every rank at the same point)
        states[key] = st
        return st

    def forward_random_pair(self, time_loc_inputs, stream_id=None):
        """(view 1, view 2) of the same windows with every random draw made on the device (reference: two calls of forward("random"),
        data_augmenter/Augmenter.py:76-113): one draw launch, two warp launches (they return at once unless a plan drew a warp), one
        transform call for all (view, location, modality).  Inputs: fp32 [B, C, I, S] device tensors.  The two views of a modality are
        the halves of one [2B, 2C, I, S] tensor, as forward("random") arranges them."""
        from focal_amd import distributed, runtime
        x = {loc: {mod: t.contiguous() for mod, t in mods.items()} for loc, mods in time_loc_inputs.items()}
        st = self._device_state(x)
        flat, n = st["flat"], len(st["flat"])
        dev = x[flat[0][0]][flat[0][1]].device
        if stream_id is None:
            stream_id = 0x56494557   # ("VIEW")
        # the draw's own state, started from one seed on every data-parallel rank: identical plans on all ranks (the reference draws once
        # per batch; the global batch is the batch), different dropout masks (runtime.rng_state stays per rank)
        ops.view_draw_shared(st["pool"], 2, n, st["view_state"], stream_id, st["plans"], extras=st["extras"])
        if st["warps"]:
            ops.warp_plan_multi([dict(x=x[l][m], plan=st["plans"][v * n + i], tables=st["tables"][v][(l, m)], y=st["warped"][v][(l, m)])
                                 for v in range(2) for i, (l, m) in enumerate(flat)])
        items = []
        for v in range(2):
            for i, (l, m) in enumerate(flat):
                B = x[l][m].shape[0]
                items.append(dict(x=x[l][m], plan=st["plans"][v * n + i], x_warped=st["warped"][v][(l, m)] if st["warps"] else x[l][m],
                                  out=st["both"][(l, m)][v * B:(v + 1) * B]))
                if st["extras"] is not None:  # every rank draws the same jitter key: the rank salts the noise (independent per sample of the global batch)
                    items[-1].update(extra=st["extras"][v * n + i], noise_salt=distributed.rank())
        outs = ops.fft_realpack_multi(items)
        views = ({loc: {} for loc in x}, {loc: {} for loc in x})
        for v in range(2):
            for i, (l, m) in enumerate(flat):
                views[v][l][m] = outs[v * n + i]
        return views

    # ------------------------------------------------------------------------------------------ the fixed pipeline, drawn on the device
    FIXED_MIX_STREAM, FIXED_VIEW_STREAM = 0x4D495846, 0x46495856   # ("MIXF", "FIXV": apart from the random views' 0x56494557)

    def fixed_device_draws_supported(self):
        """The `fixed` pipeline is made of what focal_mixup_draw / focal_view_draw know (every shipped `fixed_augmenters` is):
        mixup / no in the time domain, phase_shift / no after the transform, Mixup in mode "random_batch" without cutmix_minmax."""
        cfg = self.args.dataset_config
        if not (set(self.time_aug_names) <= {"no", "mixup"} and set(self.freq_aug_names) <= {"no", "phase_shift"}):
            return False
        if "mixup" in self.time_aug_names:
            mc = cfg.get("mixup", {})
            if mc.get("mode", "batch") != "random_batch" or mc.get("cutmix_minmax") is not None:
                return False
        return len(cfg["location_names"]) * len(cfg["modality_names"]) <= ops._lib.VIEW_MAX_SLOTS

    def _fixed_state(self, inputs):
        """What forward_fixed_device writes, ONE state per batch shape and never dropped, for the reason _device_state gives: a captured
        step holds the addresses of the record, the permutation, the plans, the mixed windows and the spectra."""
        flat = [(loc, mod) for loc in inputs for mod in inputs[loc]]
        key = tuple((loc, mod, tuple(inputs[loc][mod].shape), inputs[loc][mod].device) for loc, mod in flat)
        states = self.__dict__.setdefault("_fixed_states", {})
        st = states.get(key)
        if st is not None:
            return st
        from focal_amd import runtime
        cfg = self.args.dataset_config
        dev = inputs[flat[0][0]][flat[0][1]].device
        shape = lambda k: tuple(inputs[k[0]][k[1]].shape)
        phase = "phase_shift" in self.freq_aug_names
        st = {"key": key, "flat": flat, "mix": "mixup" in self.time_aug_names, "B": shape(flat[0])[0],
              "rec": ops.new_mix_record(dev), "perm": torch.zeros(shape(flat[0])[0], dtype=torch.int32, device=dev),
              "mixed": {k: torch.empty(shape(k), dtype=torch.float32, device=dev) for k in flat},
              # a one-entry pool: the view draw's per-slot coin is the augmenter's own (PhaseShiftAugmenter.py: random() < prob)
              "pool": ops.view_pool([("phase_shift", cfg["phase_shift"]["prob"])] if phase else [("no", 0.0)], [shape(k)[2] for k in flat]),
              "plans": ops.new_view_plans(1, len(flat), dev),
              "out": {k: torch.empty((shape(k)[0], 2 * shape(k)[1]) + shape(k)[2:], dtype=torch.float32, device=dev) for k in flat},
              "draw_state": runtime.view_state(dev)}
        states[key] = st
        return st

    def forward_fixed_device(self, time_loc_inputs):
        """forward_fixed with every draw made on the DEVICE, as one fixed sequence of launches (so the pipeline sits inside a captured
        step and a replay draws anew): the mix draw (focal_mixup_draw), the mix pass of all slots (focal_mixup_multi; when `mixup` is
        configured), the phase draw (focal_view_draw over a one-entry pool, one view), ONE transform call over all slots that reads the
        drawn plans.  Inputs: fp32 [B, C, I, S] device tensors; returns address-stable spectra.  Labels are not touched: the reference
        resets them before the frequency stage (see forward_fixed)."""
        x = {loc: {mod: t.contiguous() for mod, t in mods.items()} for loc, mods in time_loc_inputs.items()}
        st = self._fixed_state(x)
        flat, n = st["flat"], len(st["flat"])
        src = {k: x[k[0]][k[1]] for k in flat}
        if st["mix"]:
            ops.mixup_draw(self.args.dataset_config["mixup"], st["B"], [src[k].shape[2:] for k in flat], st["draw_state"],
                           self.FIXED_MIX_STREAM, st["rec"], st["perm"])
            ops.mixup_multi([dict(x=src[k], y=st["mixed"][k], slot=i) for i, k in enumerate(flat)], st["rec"], st["perm"])
            src = st["mixed"]
        ops.view_draw_shared(st["pool"], 1, n, st["draw_state"], self.FIXED_VIEW_STREAM, st["plans"])
        outs = ops.fft_realpack_multi([dict(x=src[k], plan=st["plans"][i], x_warped=src[k], out=st["out"][k]) for i, k in enumerate(flat)])
        res = {loc: {} for loc in x}
        for (loc, mod), o in zip(flat, outs):
            res[loc][mod] = o
        return res

    def _static_out(self, loc, mod, x):
        """`static_fixed` (set by a loop that replays the classifier step behind host-drawn spectra): the spectrum of a (location,
        modality) keeps its address per batch shape, so the captured step can read it.  Off (the default): a fresh tensor per call."""
        if not getattr(self, "static_fixed", False):
            return None
        pool = self.__dict__.setdefault("_static_fixed_out", {})
        shape = (x.shape[0], 2 * x.shape[1], x.shape[2], x.shape[3])
        key = (loc, mod, shape, x.device)
        if key not in pool:
            pool[key] = torch.empty(shape, dtype=torch.float32, device=x.device)
        return pool[key]

    def begin_step(self):
        """Called by the training loop before the first of a step's two draws (static_views): the next draw of every tensor gets the FIRST
        half again.  Without it an odd number of draws on a training-shaped batch -- an exception between the two draws, a caller that
        draws one view, a resume in mid-pair -- slipped the parity for good: view 1 in the second half, the captured step never matched
        again and the job silently ran eagerly."""
        for ent in self.__dict__.get("_static_pairs", {}).values():
            ent[1] = 0

    def _view_slot(self, loc, mod, x):
        """Where this view's spectrum goes: the pretraining loop draws two views of the same windows back to back
        (train_utils/pretrain.py), so the first call gets the first half of a fresh [2B, 2C, I, n] tensor and the second call (same
        input tensor) the second half -- a backbone that runs both views as one batch then needs no concatenation."""
        key = (loc, mod)
        B = x.shape[0]
        # `static_views` (set by the graph-replaying training loop): the two-view tensor of a (location, modality) keeps its address
        # from step to step, so a captured step can read it; the loop guarantees a step has finished reading before the next writes.
        # The halves are handed out strictly in turn (first, second, first, ...) per tensor: pairing by the input's address, as the
        # non-static path below does, would hand the FIRST half out twice whenever a loader that sources its batches on the host
        # makes `move_to_target_device` allocate a new device tensor per call -- view 2 would silently overwrite view 1.
        if getattr(self, "static_views", False):
            pool = self.__dict__.setdefault("_static_pairs", {})
            shape = (2 * B, 2 * x.shape[1], x.shape[2], x.shape[3])
            ent = pool.get((key, shape, x.device))
            if ent is None:
                ent = pool[(key, shape, x.device)] = [torch.empty(shape, dtype=torch.float32, device=x.device), 0]
            ent[1] += 1
            return ent[0][:B] if ent[1] % 2 == 1 else ent[0][B:]
        pend = self.__dict__.setdefault("_pending_pairs", {})
        tag = (x.data_ptr(), tuple(x.shape), x.device)
        hit = pend.pop(key, None)
        if hit is not None and hit[0] == tag:
            return hit[1][B:]
        base = torch.empty(2 * B, 2 * x.shape[1], x.shape[2], x.shape[3], dtype=torch.float32, device=x.device)
        pend[key] = (tag, base)
        return base[:B]

    def move_to_target_device(self, time_loc_inputs, labels):
        dev = self.args.device
        out = {loc: {mod: t.float().to(dev) for mod, t in mods.items()} for loc, mods in time_loc_inputs.items()}
        return out, (labels.to(dev) if labels is not None else None)

    def fft_preprocess(self, time_loc_inputs):
        """[b, c, i, s] real -> [b, 2c, i, s] packed spectrum (reference :141-158), on the HIP DFT kernel."""
        return _transform_all({loc: {mod: dict(x=x.contiguous(), out=self._static_out(loc, mod, x)) for mod, x in mods.items()}
                               for loc, mods in time_loc_inputs.items()})
