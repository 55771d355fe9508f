"""Tensor-level wrappers over the libfocal_hip C ABI.

PyTorch is plumbing here: it owns device memory (torch.empty), the current HIP stream and autograd bookkeeping; all
arithmetic happens in the HIP kernels.  Every function enqueues on `torch.cuda.current_stream()` and returns
immediately; none of them has a CPU implementation.
"""
import ctypes as C
import math
import os

import torch

from . import _lib
from ._lib import (ACT_GELU, ACT_NONE, ACT_RELU_OUT, EPI_GELU, EPI_NONE, EPI_RELU, EPI_RESIDUAL, FOCAL_BF16, FOCAL_F32,
                   AdamWDesc, AttnDesc, BNDesc, ConvDesc, ConvInDesc, DropDesc, Embed2Desc, EmbedDesc, FFTDesc, GRUDesc, LinearDesc,
                   LNDesc, LossDesc, MlpDesc, check)

_TORCH2CODE = {torch.float32: FOCAL_F32, torch.bfloat16: FOCAL_BF16}
_CODE2TORCH = {v: k for k, v in _TORCH2CODE.items()}


def code(dtype):
    return _TORCH2CODE[dtype]


def torch_dtype(c):
    return _CODE2TORCH[c]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


# ------------------------------------------------------------------------------------------------ per-step zero pool
# Many kernels accumulate with atomics into small buffers that must start at zero (BatchNorm channel sums, split weight
# gradients).  One memset per buffer is one graph node each (~100 per DeepSense step); instead they are slices of ONE fp32
# pool that `zero_pool_reset` (called by the optimizer's zero_grad, after the side streams are joined) zeroes with a single
# launch.  A slice is handed out once between two resets, so correctness never depends on the reset being called: without it
# the pool simply runs out and callers fall back to their own zero-fill.
_ZERO_POOL = {}
_ZERO_POOL_FLOATS = 4 << 20


def zero_pool_reset(device):
    st = _ZERO_POOL.get(torch.device(device))
    if st is None:
        return
    if st["ptr"] > 0:
        st["buf"][:st["ptr"]].zero_()
    st["ptr"] = 0


def pool_zeros(n, device):
    """n zero fp32 values from the pool, or None when the pool cannot serve them (caller then zero-fills itself)."""
    dev = torch.device(device)
    if dev.type != "cuda":
        return None
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    st = _ZERO_POOL.get(dev)
    if st is None:
        if torch.cuda.is_current_stream_capturing():
            return None  # never create the pool inside a graph capture
        st = _ZERO_POOL[dev] = {"buf": torch.zeros(_ZERO_POOL_FLOATS, dtype=torch.float32, device=dev), "ptr": 0}
        torch.cuda.current_stream(dev).synchronize()  # created on whichever stream asked first; every stream must see the zeros
    need = (n + 63) // 64 * 64
    if st["ptr"] + need > _ZERO_POOL_FLOATS:
        return None
    out = st["buf"][st["ptr"]:st["ptr"] + n]
    st["ptr"] += need
    return out


def zeros(shape, device):
    """fp32 zeros of `shape`: a pool slice when possible, else torch.zeros."""
    n = 1
    for v in shape:
        n *= int(v)
    t = pool_zeros(n, device)
    return t.view(*shape) if t is not None else torch.zeros(*shape, dtype=torch.float32, device=device)


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _lib.FocalHipError("libfocal_hip operates on device tensors only (no CPU fallback)")
        if t is not None and not t.is_contiguous():
            raise _lib.FocalHipError("libfocal_hip needs contiguous tensors")


def drop_desc(rng=None, stream_elem=0, p_elem=0.0, stream_path=0, p_path=0.0, rows_per_sample=1):
    return DropDesc(_p(rng), stream_elem, p_elem, stream_path, p_path, rows_per_sample)


NO_DROP = drop_desc()


# ------------------------------------------------------------------------------------------------ RNG / optimizer
def new_rng_state(seed, device):
    return torch.tensor([seed & 0xFFFFFFFF, 0, 0, 0], dtype=torch.int64, device=device).to(torch.int32)


def new_step_state(device, count=0):
    """The optimizer's device-side step state for adamw_multi(advance=True): {seed, step count, tickets ...} (FOCAL_STEP_STATE_WORDS)."""
    st = torch.zeros(40, dtype=torch.int32, device=device)
    if count:
        st[1] = int(count)
    return st


def mark(slots, index):
    """Diagnostic: slots[index] (int64 device tensor) = device wall clock, 100 MHz ticks, when the launch runs on the current stream."""
    check(_lib.load().focal_mark(_p(slots), int(index), _stream()))


def rng_advance(state):
    check(_lib.load().focal_rng_advance(_p(state), _stream()))


def cast_bf16(src, dst):
    _need_cuda(src, dst)
    check(_lib.load().focal_cast_bf16(_p(src), _p(dst), src.numel(), _stream()))


def new_clip_state(device):
    """Device state of gradient clipping: (partial row of CLIP_SCRATCH_WORDS fp32 sums of squares, record of CLIP_RECORD_WORDS words)."""
    return (torch.zeros(_lib.CLIP_SCRATCH_WORDS, dtype=torch.float32, device=device),
            torch.zeros(_lib.CLIP_RECORD_WORDS, dtype=torch.int32, device=device))


def grad_norm(segs, clip_state):
    """The norm pass: per-workgroup sums of squares of the flat fp32 gradient tensors `segs` (lengths multiples of 4) into clip_state's
    partial row, one launch; adamw_multi(..., clip=(clip_state, max_norm)) behind it turns the row into the norm and the coefficient."""
    _need_cuda(*segs)
    n = len(segs)
    if any(g.dtype != torch.float32 for g in segs):
        raise _lib.FocalHipError("grad_norm: gradients are fp32")
    check(_lib.load().focal_grad_norm_multi(n, (C.c_void_p * max(n, 1))(*[_p(g) for g in segs]), (C.c_long * max(n, 1))(*[g.numel() for g in segs]),
                                            _p(clip_state[0]), clip_state[0].numel(), _stream()))


def read_clip_stats(clip_state):
    """One device-to-host copy of the record, as a dict; the record is reset (call outside graph capture, e.g. once per epoch)."""
    rec = clip_state[1].cpu()
    clip_state[1].zero_()
    f = rec.view(torch.float32)
    steps, clipped, skipped = (int(v) for v in rec[:3])
    return {"steps": steps, "clipped": clipped, "skipped": skipped, "norm_sum": float(f[3]), "norm_max": float(f[4]),
            "norm_mean": float(f[3]) / max(steps - skipped, 1), "last_norm": float(f[5]), "last_sq": float(f[6]), "last_coef": float(f[7])}


def adamw_multi(segments, lr_dev, rng_state, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.05, l2_decay=False, advance=False, seed_state=None,
                clip=None):
    """segments: list of (p, g, m, v, shadow_or_None) flat tensors (lengths multiples of 4).  rng_state[1] is the step count the update
    uses; advance=True: the count used is rng_state[1] + 1 and the kernel itself then advances rng_state and (if given) seed_state
    (focal_adamw_multi_advance: what two focal_rng_advance launches in front of the call would have done).
    clip=(clip_state, max_norm): the update on g * min(1, max_norm / (norm + 1e-6)), the norm from the partial row grad_norm() left in
    clip_state; a non-finite norm skips the step (focal_adamw_clip_multi / _advance)."""
    n = len(segments)
    arr = lambda i: (C.c_void_p * n)(*[_p(s[i]) for s in segments])
    has_shadow = any(s[4] is not None for s in segments)
    lens = (C.c_long * n)(*[s[0].numel() for s in segments])
    d = AdamWDesc(beta1, beta2, eps, weight_decay, int(l2_decay))
    if clip is not None:
        (row, rec), max_norm = clip
        max_norm = float(max_norm)
        if not max_norm > 0.0:  # refused here as well: a NaN or non-positive bound never reaches a launch
            raise ValueError(f"adamw_multi: max_norm = {max_norm} must be positive (inf: clip nothing, record the norms)")
        tail = (_p(row), row.numel(), _p(rec), rec.numel(), max_norm, _stream())
        if advance:
            check(_lib.load().focal_adamw_clip_multi_advance(C.byref(d), n, arr(0), arr(1), arr(2), arr(3), arr(4) if has_shadow else None,
                                                             lens, _p(lr_dev), _p(rng_state), rng_state.numel(), _p(seed_state), *tail))
            return
        check(_lib.load().focal_adamw_clip_multi(C.byref(d), n, arr(0), arr(1), arr(2), arr(3), arr(4) if has_shadow else None,
                                                 lens, _p(lr_dev), _p(rng_state), *tail))
        return
    if advance:
        check(_lib.load().focal_adamw_multi_advance(C.byref(d), n, arr(0), arr(1), arr(2), arr(3), arr(4) if has_shadow else None,
                                                    lens, _p(lr_dev), _p(rng_state), rng_state.numel(), _p(seed_state), _stream()))
        return
    check(_lib.load().focal_adamw_multi(C.byref(d), n, arr(0), arr(1), arr(2), arr(3), arr(4) if has_shadow else None,
                                        lens, _p(lr_dev), _p(rng_state), _stream()))


def lamb_table(index_rows, lo, hi, exclude_1d=True):
    """The piece table of LAMB over the arena span [lo, hi), host side (pure Python).  index_rows: the (offset, numel, shape) rows of
    ParamArena.index in arena order.  Every tensor whose offset lies in the span is cut into pieces of at most _lib.LAMB_PIECE elements
    that tile its ALIGN-padded extent (the pad elements are zero and stay zero); offsets count from `lo`.  exclude_1d: a tensor with
    ndim <= 1 is neither adapted nor decayed.  Returns {"n", "pieces": [(offset, length, tensor)], "tensors": [(first piece, last piece,
    flags)], "rows": [the index row of each tensor]} -- tensors without elements own no piece and are left out."""
    rows = [(int(o), int(k), tuple(shp)) for o, k, shp in index_rows]
    inside = [(i, r) for i, r in enumerate(rows) if lo <= r[0] < hi and r[1] > 0]
    pieces, tensors, which = [], [], []
    for j, (i, (o, k, shp)) in enumerate(inside):
        end = inside[j + 1][1][0] if j + 1 < len(inside) else hi  # the padded extent ends where the next tensor starts
        if not (o + k <= end <= hi and (o - lo) % 4 == 0 and (end - o) % 4 == 0):
            raise ValueError(f"lamb_table: tensor {i} at [{o}, {o + k}) does not fit a padded extent ending at {end} inside [{lo}, {hi})")
        flags = 0 if (exclude_1d and len(shp) <= 1) else (_lib.LAMB_ADAPT | _lib.LAMB_DECAY)
        first = len(pieces)
        for a in range(o, end, _lib.LAMB_PIECE):
            pieces.append((a - lo, min(_lib.LAMB_PIECE, end - a), len(tensors)))
        tensors.append((first, len(pieces), flags))
        which.append(i)
    return {"n": hi - lo, "pieces": pieces, "tensors": tensors, "rows": which}


def lamb_table_upload(table, device):
    """The device side of a lamb_table(): the table's words, the partial row and the per-tensor record (call outside graph capture)."""
    words = [w for o, k, t in table["pieces"] for w in (o, k, t, 0)] + [w for a, b, f in table["tensors"] for w in (a, b, f, 0)]
    out = dict(table)
    out["host"] = (C.c_int32 * max(len(words), 1))(*words)
    out["dev"] = torch.tensor(words, dtype=torch.int32).to(device)
    out["partials"] = torch.zeros(2 * max(len(table["pieces"]), 1), dtype=torch.float32, device=device)
    out["record"] = torch.zeros(_lib.LAMB_RECORD_WORDS * max(len(table["tensors"]), 1), dtype=torch.float32, device=device)
    return out


def lamb_multi(segments, tables, lr_dev, rng_state, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.05, max_trust=math.inf, advance=False,
               seed_state=None, clip=None):
    """LAMB over `segments` (as adamw_multi: (p, g, m, v, shadow_or_None) flat tensors), tables[i] the uploaded lamb_table of segment i
    (its offsets count from the segment's start).  Two launches per segment: moments + per-piece sums of squares, then the trust ratio
    and the weights; the per-tensor {phi, |w|, |u|} lands in tables[i]["record"].  advance / seed_state / clip: as adamw_multi."""
    n = len(segments)
    max_trust = float(max_trust)
    if not max_trust > 0.0:
        raise ValueError(f"lamb_multi: max_trust = {max_trust} must be positive (inf: no clamp)")
    if len(tables) != n:
        raise ValueError(f"lamb_multi: {len(tables)} tables for {n} segments")
    arr = lambda i: (C.c_void_p * max(n, 1))(*[_p(s[i]) for s in segments])
    has_shadow = any(s[4] is not None for s in segments)
    lens = (C.c_long * max(n, 1))(*[s[0].numel() for s in segments])
    tabs = (_lib.LambTable * max(n, 1))(*[_lib.LambTable(C.cast(t["host"], C.c_void_p), _p(t["dev"]), len(t["pieces"]), len(t["tensors"]),
                                                        _p(t["partials"]), t["partials"].numel(), _p(t["record"]), t["record"].numel())
                                          for t in tables])
    d = AdamWDesc(beta1, beta2, eps, weight_decay, 0)
    if clip is not None:
        (row, rec), max_norm = clip
        max_norm = float(max_norm)
        if not max_norm > 0.0:
            raise ValueError(f"lamb_multi: max_norm = {max_norm} must be positive (inf: clip nothing, record the norms)")
        tail = (_p(row), row.numel(), _p(rec), rec.numel(), max_norm, _stream())
    else:
        tail = (None, 0, None, 0, 0.0, _stream())
    head = (C.byref(d), n, arr(0), arr(1), arr(2), arr(3), arr(4) if has_shadow else None, lens, tabs, max_trust, _p(lr_dev), _p(rng_state))
    if advance:
        check(_lib.load().focal_lamb_multi_advance(*head, rng_state.numel(), _p(seed_state), *tail))
        return
    check(_lib.load().focal_lamb_multi(*head, *tail))


# ------------------------------------------------------------------------------------------------ row 3
_TWIDDLES = {}


def _factor(n):
    """n = n1 * n2 with n1 as close to sqrt(n) as possible (n2 = 1 -> direct DFT for short rows)."""
    if n <= 64:
        return n, 1
    best = 1
    for a in range(1, int(math.isqrt(n)) + 1):
        if n % a == 0:
            best = a
    return n // best, best


def _fft_problem(x, scale=1.0, flip=False, perm=None, phase=0.0, out=None, plan=None, x_warped=None):
    """(descriptor, augmentation descriptor | None, x, twiddle table, out) of one transform.  plan (a row of ops.view_draw's tensor) /
    x_warped are bound by fft_realpack_multi."""
    _need_cuda(x)
    B, Cc, I, n = x.shape
    key = (n, x.device)
    if key not in _TWIDDLES:
        k = torch.arange(n, dtype=torch.float64)
        ang = 2.0 * math.pi * k / n
        _TWIDDLES[key] = torch.stack([torch.cos(ang), -torch.sin(ang)], 1).to(torch.float32).contiguous().to(x.device)
    n1, n2 = _factor(n)
    if out is None:
        out = torch.empty(B, 2 * Cc, I, n, dtype=torch.float32, device=x.device)
    elif tuple(out.shape) != (B, 2 * Cc, I, n) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != x.device:
        raise ValueError("fft_realpack: `out` must be a contiguous fp32 [B, 2C, I, n] tensor on x's device")
    d = FFTDesc(B, Cc, I, n, n1, n2)
    if scale == 1.0 and not flip and perm is None and phase == 0.0:
        return d, None, x, _TWIDDLES[key], out
    a = _lib.AugDesc()
    a.scale, a.flip, a.use_perm = float(scale), int(bool(flip)), int(perm is not None)
    a.phase_cos, a.phase_sin = math.cos(phase), math.sin(phase)
    if perm is not None:
        perm = [int(v) for v in perm]
        if sorted(perm) != list(range(I)):
            raise ValueError(f"perm must be a permutation of range({I})")
        for i, v in enumerate(perm):
            a.perm[i] = v
    return d, a, x, _TWIDDLES[key], out


_EXTRA_KEYS = ("jitter", "chan", "time_mask", "freq_mask", "extra", "noise_salt")


def _host_extra(x, jitter=None, chan=None, time_mask=None, freq_mask=None):
    """The focal_view_extra of one transform from its keywords: jitter=(std, key), chan=channel order, time_mask / freq_mask=(lo, n)."""
    e = _lib.ViewExtra()
    Cc, n = x.shape[1], x.shape[3]
    if jitter is not None:
        if float(jitter[0]) < 0:
            raise ValueError("jitter: the standard deviation must not be negative")
        e.jitter_std, e.jitter_key = float(jitter[0]), int(jitter[1]) & 0xFFFFFFFF
    if chan is not None:
        chan = [int(v) for v in chan]
        if Cc > _lib.VIEW_MAX_CHANNELS or sorted(chan) != list(range(Cc)):
            raise ValueError(f"chan must be a permutation of range({Cc}), at most {_lib.VIEW_MAX_CHANNELS} channels")
        e.use_chan = 1
        for i, v in enumerate(chan):
            e.chan[i] = v
    for name, val in (("tmask", time_mask), ("fmask", freq_mask)):
        if val is not None:
            lo, cnt = int(val[0]), int(val[1])
            if lo < 0 or cnt < 0 or lo + cnt > n:
                raise ValueError(f"{name}: [{lo}, {lo + cnt}) leaves [0, {n}]")
            setattr(e, name + "_lo", lo)
            setattr(e, name + "_n", cnt)
    return e


def fft_realpack(x, scale=1.0, flip=False, perm=None, phase=0.0, out=None, **extra):
    """[B, C, I, n] real fp32 -> [B, 2C, I, n] (Re/Im channel pairs of the full two-sided spectrum).

    Optional view augmentation folded into the transform (focal_augment_fft_fwd): x * scale, horizontal flip (intervals and
    samples reversed), interval order `perm` (sequence of I ints), and a rotation of every bin by `phase` radians.
    `out`: write into this contiguous [B, 2C, I, n] fp32 tensor (e.g. one half of a two-view batch) instead of allocating.
    jitter=(std, key) / chan=order / time_mask=(lo, n) / freq_mask=(lo, n) / extra=device record / noise_salt=: the augmenters that
    travel in a focal_view_extra (focal_fft_realpack_multi)."""
    if extra:
        return fft_realpack_multi([dict(x=x, scale=scale, flip=flip, perm=perm, phase=phase, out=out, **extra)])[0]
    d, a, x, tw, out = _fft_problem(x, scale, flip, perm, phase, out)
    if a is None:
        check(_lib.load().focal_fft_realpack_fwd(C.byref(d), _p(x), _p(tw), _p(out), _stream()))
    else:
        check(_lib.load().focal_augment_fft_fwd(C.byref(d), C.byref(a), _p(x), _p(tw), _p(out), _stream()))
    return out


def fft_realpack_multi(items):
    """items: [dict(x=..., scale=, flip=, perm=, phase=, out=)] -- the keyword arguments of fft_realpack, one dict per transform (the
    modalities of a view, or of both views) -> list of outputs.  One call (focal_fft_realpack_multi): the short-row transforms (the
    20-sample sensor modalities) share one launch, the others are launched as fft_realpack would.
    An item may also carry jitter= / chan= / time_mask= / freq_mask= (host values), extra= (a row of new_view_extras: read on the device
    when the kernel runs) and noise_salt=.  The library, not this function, decides which kernels a call runs: the plain ones unless some
    item carries an extra."""
    probs = [_fft_problem(**{k: v for k, v in it.items() if k not in _EXTRA_KEYS}) for it in items]
    arr = (_lib.FftProblem * len(probs))()
    for q, it, (d, a, x, tw, out) in zip(arr, items, probs):
        q.d = d
        q.has_aug = int(a is not None)
        if a is not None:
            q.aug = a
        q.x, q.twiddle, q.out = _p(x), _p(tw), _p(out)
        plan = it.get("plan")
        if plan is not None:  # the augmentation is read from the device record when the kernel runs (view draws inside the captured step)
            _need_cuda(plan, it["x_warped"])
            q.plan, q.x_warped = _p(plan), _p(it["x_warped"])
        q.noise_salt = int(it.get("noise_salt") or 0) & 0xFFFFFFFF
        if it.get("extra") is not None:
            rec = it["extra"]
            _need_cuda(rec)
            assert rec.dtype == torch.uint8 and rec.numel() == VIEW_EXTRA_BYTES and rec.is_contiguous()
            q.extra_dev = _p(rec)
        elif any(it.get(k) is not None for k in ("jitter", "chan", "time_mask", "freq_mask")):
            q.has_extra = 1
            q.extra = _host_extra(x, it.get("jitter"), it.get("chan"), it.get("time_mask"), it.get("freq_mask"))
    check(_lib.load().focal_fft_realpack_multi(len(probs), arr, _stream()))
    return [p[4] for p in probs]


# ---- view draws on the device (focal_view_draw / focal_warp_plan_multi: include/focal_hip.h)
VIEW_KINDS = {"no": _lib.VIEW_NONE, "negation": _lib.VIEW_NEGATION, "scaling": _lib.VIEW_SCALING, "horizontal_flip": _lib.VIEW_HFLIP,
              "permutation": _lib.VIEW_PERMUTATION, "phase_shift": _lib.VIEW_PHASE_SHIFT, "mag_warp": _lib.VIEW_MAG_WARP,
              "time_warp": _lib.VIEW_TIME_WARP, "jitter": _lib.VIEW_JITTER, "channel_shuffle": _lib.VIEW_CHANNEL_SHUFFLE,
              "time_mask": _lib.VIEW_TIME_MASK, "freq_mask": _lib.VIEW_FREQ_MASK}
VIEW_KINDS_EX = ("jitter", "channel_shuffle", "time_mask", "freq_mask")   # the kinds that travel in a focal_view_extra
VIEW_PLAN_BYTES = C.sizeof(_lib.ViewPlan)
VIEW_EXTRA_BYTES = C.sizeof(_lib.ViewExtra)


def view_pool(entries, intervals, scaling_std=0.2, mag_warp=(0.05, 4), time_warp=(0.2, 6), jitter_std=None, channels=None, time_mask=None,
              freq_mask=None):
    """entries: [(augmenter name, coin probability)] -- the pool (1 .. 16 entries) ONE entry of which is drawn per view; intervals: per slot
    ((location, modality) pair) the interval count a permutation shuffles; the two warps' (magnitude, spline ord).  A pool that names
    jitter / channel_shuffle / time_mask / freq_mask needs that kind's per-slot list: jitter_std [std], channels [C], time_mask [(D, I)],
    freq_mask [(W, n)]."""
    if not 1 <= len(entries) <= _lib.VIEW_MAX_POOL or not 1 <= len(intervals) <= _lib.VIEW_MAX_SLOTS:
        raise ValueError(f"view_pool: 1 .. {_lib.VIEW_MAX_POOL} pool entries, 1 .. {_lib.VIEW_MAX_SLOTS} slots")
    pool = _lib.ViewPool()
    names = {name for name, _ in entries}
    ns = len(intervals)
    for need, arg, label in zip(VIEW_KINDS_EX, (jitter_std, channels, time_mask, freq_mask), ("jitter_std", "channels", "time_mask", "freq_mask")):
        if need in names and (arg is None or len(arg) != ns):
            raise ValueError(f"view_pool: a pool with {need} needs {label}= with one entry per slot")
    for i in range(ns):
        if jitter_std is not None:
            pool.jitter_std[i] = float(jitter_std[i])
        if channels is not None:
            pool.channels[i] = int(channels[i])
        if time_mask is not None:
            pool.tmask_d[i], pool.tmask_i[i] = int(time_mask[i][0]), int(time_mask[i][1])
        if freq_mask is not None:
            pool.fmask_w[i], pool.fmask_n[i] = int(freq_mask[i][0]), int(freq_mask[i][1])
    pool.n_aug = len(entries)
    for i, (name, prob) in enumerate(entries):
        pool.kind[i], pool.prob[i] = VIEW_KINDS[name], float(prob)
    pool.scaling_std = float(scaling_std)
    pool.mag_magnitude, pool.mag_order = float(mag_warp[0]), int(mag_warp[1])
    pool.time_magnitude, pool.time_order = float(time_warp[0]), int(time_warp[1])
    for i, n in enumerate(intervals):
        pool.intervals[i] = int(n)
    return pool


def new_view_plans(n_views, n_slots, device):
    """uint8 [n_views * n_slots, sizeof(focal_view_plan)]: row v * n_slots + s is the plan of (view v, slot s)."""
    return torch.zeros(n_views * n_slots, VIEW_PLAN_BYTES, dtype=torch.uint8, device=device)


def new_view_extras(n_views, n_slots, device):
    """uint8 [n_views * n_slots, sizeof(focal_view_extra)] beside new_view_plans; zero = the identity."""
    return torch.zeros(n_views * n_slots, VIEW_EXTRA_BYTES, dtype=torch.uint8, device=device)


def read_view_extras(extras):
    """Host copies of the extra records (tests, diagnostics): a list of _lib.ViewExtra."""
    raw = extras.cpu().numpy().tobytes()
    return [_lib.ViewExtra.from_buffer_copy(raw[i * VIEW_EXTRA_BYTES:(i + 1) * VIEW_EXTRA_BYTES]) for i in range(extras.shape[0])]


def write_view_extra(extras, index, jitter=None, chan=None, time_mask=None, freq_mask=None, like=None):
    """Force one extra record (tests); `like` = the [B, C, I, n] tensor it will be applied to (for the checks of _host_extra)."""
    e = _host_extra(like, jitter, chan, time_mask, freq_mask)
    extras[index].copy_(torch.frombuffer(bytearray(bytes(e)), dtype=torch.uint8))


def _view_draw(pool, n_views, n_slots, state, advance, stream_id, plans, extras):
    _need_cuda(plans, state)
    assert plans.shape == (n_views * n_slots, VIEW_PLAN_BYTES) and plans.dtype == torch.uint8 and plans.is_contiguous()
    if extras is None:
        if any(pool.kind[i] >= _lib.VIEW_JITTER for i in range(pool.n_aug)):
            raise ValueError("view_draw: a pool that names jitter / channel_shuffle / time_mask / freq_mask needs extras=new_view_extras(...)")
    else:
        _need_cuda(extras)
        assert extras.shape == (n_views * n_slots, VIEW_EXTRA_BYTES) and extras.dtype == torch.uint8 and extras.is_contiguous()
    check(_lib.load().focal_view_draw(C.byref(pool), n_views, n_slots, _p(state), advance, int(stream_id) & 0xFFFFFFFF, _p(plans),
                                      _p(extras), _stream()))
    return plans


def view_draw(pool, n_views, n_slots, seed_state, stream_id, plans, extras=None):
    """The draws of n_views views over n_slots slots into `plans` (new_view_plans), keyed by seed_state[0] (the device seed word the
    optimizer advances every step) and stream_id; with extras= (new_view_extras) also the records of jitter / channel_shuffle / time_mask /
    freq_mask, which a pool that names one of them needs."""
    return _view_draw(pool, n_views, n_slots, seed_state, 0, stream_id, plans, extras)


def view_draw_shared(pool, n_views, n_slots, view_state, stream_id, plans, extras=None):
    """view_draw from the draw's own device state (runtime.view_state: one seed broadcast to every data-parallel rank), which the kernel
    advances itself: every rank draws the same plans, replay after replay."""
    assert view_state.dtype == torch.int32 and view_state.numel() >= 4
    return _view_draw(pool, n_views, n_slots, view_state, 1, stream_id, plans, extras)


def read_view_plans(plans):
    """Host copies of the plan records (tests, diagnostics): a list of _lib.ViewPlan."""
    raw = plans.cpu().numpy().tobytes()
    return [_lib.ViewPlan.from_buffer_copy(raw[i * VIEW_PLAN_BYTES:(i + 1) * VIEW_PLAN_BYTES]) for i in range(plans.shape[0])]


def write_view_plan(plans, index, scale=1.0, flip=False, perm=None, phase=0.0, warp=0, knots=None, kind=0):
    """Force one plan record (tests: the reference fixtures' forced draws through the device-plan path)."""
    pl = _lib.ViewPlan()
    pl.aug.scale, pl.aug.flip, pl.aug.use_perm = float(scale), int(bool(flip)), int(perm is not None)
    pl.aug.phase_cos, pl.aug.phase_sin = math.cos(phase), math.sin(phase)
    for i in range(32):
        pl.aug.perm[i] = int(perm[i]) if perm is not None and i < len(perm) else i
    pl.kind, pl.warp = int(kind), int(warp)
    if int(warp) != 0 and (knots is None or not 4 <= len(knots) <= _lib.VIEW_MAX_KNOTS):
        raise ValueError(f"write_view_plan: a warp needs 4 .. {_lib.VIEW_MAX_KNOTS} knots")
    if knots is not None:
        pl.nknots = len(knots)
        for i, v in enumerate(knots):
            pl.knots[i] = float(v)
    buf = torch.frombuffer(bytearray(bytes(pl)), dtype=torch.uint8)
    plans[index].copy_(buf)


_END_COEF = {}


def warp_end_coefficients(device):
    """Device fp32 [47][4][48]: the end-window basis splines of the time warp (focal_amd.warp.end_window_coefficients), once per device."""
    key = torch.device(device)
    if key not in _END_COEF:
        from . import warp
        _END_COEF[key] = torch.from_numpy(warp.end_window_coefficients()).to(device)
    return _END_COEF[key]


def warp_plan_multi(problems):
    """problems: [dict(x=[B, C, I, S] fp32, plan=row of the plan tensor, tables=fp32 [2 * I * S] workspace, y=like x)]: the warps the
    plans ask for (focal_warp_plan_multi: two launches whatever they ask)."""
    if len(problems) > 8:  # (the launch table holds 8 problems: a dataset with 5 .. 8 (location, modality) slots asks for 10 .. 16)
        for k in range(0, len(problems), 8):
            warp_plan_multi(problems[k:k + 8])
        return
    arr = (_lib.WarpProblem * len(problems))()
    for i, q in enumerate(problems):
        x, y = q["x"], q["y"]
        _need_cuda(x, y, q["plan"], q["tables"])
        B, Cc, I, S = x.shape
        assert y.shape == x.shape and x.is_contiguous() and y.is_contiguous() and q["tables"].numel() >= 2 * I * S
        arr[i].rows, arr[i].L = B * Cc, I * S
        arr[i].x, arr[i].plan, arr[i].tables, arr[i].y = _p(x), _p(q["plan"]), _p(q["tables"]), _p(y)
    check(_lib.load().focal_warp_plan_multi(len(problems), arr, _p(warp_end_coefficients(problems[0]["x"].device)), _stream()))


def mag_warp(x, mult):
    """[B, C, I, S] fp32 x mult [I*S] (device fp32): the magnitude warp of focal_warp_fwd."""
    _need_cuda(x, mult)
    B, Cc, I, S = x.shape
    y = torch.empty_like(x)
    check(_lib.load().focal_warp_fwd(B * Cc, I * S, _p(x), _p(mult), None, None, 0, _p(y), _stream()))
    return y


def time_warp(x, k0, w):
    """[B, C, I, S] fp32 resampled along the flattened (I, S) axis with the tables of focal_amd.warp.time_warp_tables (device)."""
    _need_cuda(x, k0, w)
    B, Cc, I, S = x.shape
    y = torch.empty_like(x)
    check(_lib.load().focal_warp_fwd(B * Cc, I * S, _p(x), None, _p(k0), _p(w), w.shape[1], _p(y), _stream()))
    return y


def mixup(x, perm, lam=1.0, box=None):
    """focal_mixup_fwd: x fp32 [B, C, I, S], perm int32 [B] (device).  box = (yl, yh, xl, xh) -> CutMix paste, else lam-blend."""
    _need_cuda(x, perm)
    B, Cc, I, S = x.shape
    y = torch.empty_like(x)
    yl, yh, xl, xh = box if box is not None else (0, 0, 0, 0)
    check(_lib.load().focal_mixup_fwd(B, Cc, I, S, _p(x), _p(perm), float(lam), int(box is not None), int(yl), int(yh), int(xl), int(xh),
                                      _p(y), _stream()))
    return y


# ---- Mixup drawn on the device (focal_mixup_draw / focal_mixup_multi: include/focal_hip.h)
MIX_RECORD_BYTES = C.sizeof(_lib.MixRecord)


def new_mix_record(device):
    """uint8 [sizeof(focal_mix_record)]; zero = apply 0, which focal_mixup_multi copies through."""
    return torch.zeros(MIX_RECORD_BYTES, dtype=torch.uint8, device=device)


def read_mix_record(rec):
    """Host copy of the record (tests, diagnostics): a _lib.MixRecord."""
    return _lib.MixRecord.from_buffer_copy(rec.cpu().numpy().tobytes())


def write_mix_record(rec, apply=1, cut=0, lam=1.0, boxes=()):
    """Force a record (tests); boxes = [(yl, yh, xl, xh)] per slot."""
    r = _lib.MixRecord()
    r.apply, r.cut, r.lam = int(apply), int(cut), float(lam)
    for q, box in enumerate(boxes):
        for k in range(4):
            r.box[q][k] = int(box[k])
    rec.copy_(torch.frombuffer(bytearray(bytes(r)), dtype=torch.uint8))


def mixup_draw(cfg, B, slots, state, stream_id, rec, perm, advance=True):
    """The draws of one Mixup call in mode "random_batch" on the device: cfg = the dataset config's `mixup` section (prob, switch_prob,
    mixup_alpha, cutmix_alpha), slots = [(I, S)] of the (location, modality) tensors, state = 4 int32 device words {seed, draw count, 0, 0}
    (advance: the kernel moves them on), rec = new_mix_record, perm = int32 [B] device."""
    _need_cuda(rec, perm, state)
    assert rec.dtype == torch.uint8 and rec.numel() == MIX_RECORD_BYTES and perm.dtype == torch.int32 and perm.numel() >= B
    assert state is None or (state.dtype == torch.int32 and state.numel() >= 4)
    n = len(slots)
    Is, Ss = (C.c_int * max(n, 1))(*[int(s[0]) for s in slots]), (C.c_int * max(n, 1))(*[int(s[1]) for s in slots])
    check(_lib.load().focal_mixup_draw(float(cfg["prob"]), float(cfg["switch_prob"]), float(cfg["mixup_alpha"]), float(cfg["cutmix_alpha"]),
                                       int(B), n, Is, Ss, _p(state), int(bool(advance)), int(stream_id) & 0xFFFFFFFF, _p(rec), _p(perm),
                                       _stream()))


def mixup_multi(items, rec, perm):
    """items: [dict(x=fp32 [B, C, I, S], y=like x | None, slot=)] -- every (location, modality) tensor of a step mixed in ONE launch as the
    device record and permutation say when the kernel runs (focal_mixup_multi) -> the list of outputs."""
    _need_cuda(rec, perm)
    assert rec.dtype == torch.uint8 and rec.numel() == MIX_RECORD_BYTES and perm.dtype == torch.int32
    arr = (_lib.MixProblem * max(len(items), 1))()
    outs = []
    for q, it in zip(arr, items):
        x = it["x"]
        y = it.get("y")
        if y is None:
            y = torch.empty_like(x)
        _need_cuda(x, y)
        assert x.dtype == torch.float32 and y.dtype == torch.float32 and y.shape == x.shape and x.dim() == 4 and perm.numel() >= x.shape[0]
        q.B, q.C, q.I, q.S = x.shape
        q.x, q.y, q.slot = _p(x), _p(y), int(it.get("slot", 0))
        outs.append(y)
    check(_lib.load().focal_mixup_multi(len(items), arr, _p(rec), _p(perm), _stream()))
    return outs


# ------------------------------------------------------------------------------------------------ row 8
def pad_patch_embed_ln(x, w, b, gamma, beta, Hp, Wp, pw, eps=1e-5, next_ln=None):
    """next_ln = (gamma2, beta2, out_dtype): also return (LayerNorm(tokens), stats) of the LayerNorm that follows (C0 == 64)."""
    _need_cuda(x, w, b, gamma, beta)
    B, cin, I, S = x.shape
    C0 = w.shape[0]
    out = torch.empty(B * Hp * Wp, C0, dtype=torch.float32, device=x.device)
    d = EmbedDesc(B, cin, I, S, Hp, Wp, pw, C0, eps)
    if next_ln is None:
        check(_lib.load().focal_pad_patch_embed_ln_fwd(C.byref(d), _p(x), _p(w), _p(b), _p(gamma), _p(beta), _p(out), _stream()))
        return out
    g2, b2, dt = next_ln
    y_ln = torch.empty(B * Hp * Wp, C0, dtype=dt, device=x.device)
    stats = torch.empty(B * Hp * Wp, 2, dtype=torch.float32, device=x.device)
    check(_lib.load().focal_pad_patch_embed_ln2_fwd(C.byref(d), _p(x), _p(w), _p(b), _p(gamma), _p(beta), _p(out), _p(g2), _p(b2),
                                                    1e-5, code(dt), _p(y_ln), _p(stats), _stream()))
    return out, y_ln, stats


def pad_patch_embed_ape_ln(x, w, b, gamma, beta, Hp, Wp, pw, stride=1, ape=None, eps=1e-5, next_ln=None):
    """pad_patch_embed_ln on the RAW input [B, cin, I, S] with the reference's in_stride folded into the patch gather (w is
    [C0, cin * stride, 1, pw]) and the absolute position embedding `ape` ([Hp * Wp, C0] values, or None) added to the tokens;
    with next_ln the second LayerNorm reads the position-embedded tokens."""
    _need_cuda(x, w, b, gamma, beta, ape)
    B, cin, I, S = x.shape
    C0 = w.shape[0]
    if ape is not None and ape.numel() != Hp * Wp * C0:
        raise _lib.FocalHipError(f"absolute position embedding of {ape.numel()} values on a {Hp} x {Wp} x {C0} token grid")
    out = torch.empty(B * Hp * Wp, C0, dtype=torch.float32, device=x.device)
    d = Embed2Desc(B, cin, I, S, Hp, Wp, pw, C0, stride, eps)
    if next_ln is None:
        check(_lib.load().focal_pad_patch_embed_ape_ln_fwd(C.byref(d), _p(x), _p(w), _p(b), _p(gamma), _p(beta), _p(ape), _p(out), _stream()))
        return out
    g2, b2, dt = next_ln
    y_ln = torch.empty(B * Hp * Wp, C0, dtype=dt, device=x.device)
    stats = torch.empty(B * Hp * Wp, 2, dtype=torch.float32, device=x.device)
    check(_lib.load().focal_pad_patch_embed_ape_ln2_fwd(C.byref(d), _p(x), _p(w), _p(b), _p(gamma), _p(beta), _p(ape), _p(out), _p(g2), _p(b2),
                                                        1e-5, code(dt), _p(y_ln), _p(stats), _stream()))
    return out, y_ln, stats


def ape_add(x, ape):
    """x (fp32 [N * HW, C0]) += ape (HW * C0 values) per sample, in place."""
    _need_cuda(x, ape)
    cols = ape.numel()
    check(_lib.load().focal_ape_add_fwd(x.numel() // cols, cols, _p(x), _p(ape), _stream()))


def ape_bwd(g, dape):
    """dape (fp32, HW * C0 values) += the sum over the N samples of g (fp32 [N * HW, C0]): the absolute position embedding's gradient."""
    _need_cuda(g, dape)
    cols = dape.numel()
    check(_lib.load().focal_ape_bwd(g.numel() // cols, cols, _p(g), _p(dape), _stream()))


# ------------------------------------------------------------------------------------------------ LayerNorm
def ln_desc(dtype_code, rows, Cc, eps=1e-5, gather=None):
    if gather is None:
        return LNDesc(dtype_code, rows, Cc, eps, 0, 0, 0, 0, 0)
    B, H, W, Cin = gather
    return LNDesc(dtype_code, rows, Cc, eps, 1, B, H, W, Cin)


def layernorm_fwd(x, gamma, beta, out_dtype, gather=None, desc=None):
    """x fp32 [rows, C] (or [B, H, W, Cin] with gather=(B, H, W, Cin)) -> (y [rows, C] out_dtype, stats [rows, 2])."""
    _need_cuda(x, gamma, beta)
    if gather is None:
        rows, Cc = x.shape
    else:
        B, H, W, Cin = gather
        rows, Cc = B * (H // 2) * (W // 2), 4 * Cin
    d = desc or ln_desc(code(out_dtype), rows, Cc, gather=gather)
    y = torch.empty(rows, Cc, dtype=out_dtype, device=x.device)
    stats = torch.empty(rows, 2, dtype=torch.float32, device=x.device)
    check(_lib.load().focal_layernorm_fwd(C.byref(d), _p(x), _p(gamma), _p(beta), _p(y), _p(stats), _stream()))
    return y, stats


def layernorm_bwd(dy, x, stats, gamma, dx, accumulate, dgamma, dbeta, gather=None, desc=None, dx_masked=None, mask=None):
    """dx_masked (dy.dtype, same shape as dx) <- dx * mask for the residual branch that consumes dx next (mask=None: a
    plain dtype copy)."""
    _need_cuda(dy, x, stats, gamma, dx, dgamma, dbeta)
    rows, Cc = dy.shape
    d = desc or ln_desc(code(dy.dtype), rows, Cc, gather=gather)
    if dx_masked is not None:
        assert dx_masked.dtype == dy.dtype and dx_masked.numel() == dx.numel()
        mask = mask or NO_DROP
    check(_lib.load().focal_layernorm_bwd(C.byref(d), _p(dy), _p(x), _p(stats), _p(gamma), _p(dx), int(accumulate),
                                          _p(dgamma), _p(dbeta), _p(dx_masked), C.byref(mask) if mask is not None else None,
                                          _stream()))


def mask_cast(g, mask, dtype):
    """dtype(g * mask) for an fp32 [rows, C] gradient (see focal_mask_cast)."""
    _need_cuda(g)
    rows, Cc = g.shape
    out = torch.empty(rows, Cc, dtype=dtype, device=g.device)
    check(_lib.load().focal_mask_cast(code(dtype), rows, Cc, _p(g), C.byref(mask or NO_DROP), _p(out), _stream()))
    return out


# ------------------------------------------------------------------------------------------------ Linear family
def linear_desc(dtype_code, M, N, K, x_dtype, y_dtype, act_in=ACT_NONE, epilogue=EPI_NONE, splits=1, out_drop=None, dw_workgroups=0):
    return LinearDesc(dtype_code, M, N, K, x_dtype, y_dtype, act_in, epilogue, splits, out_drop or NO_DROP, dw_workgroups)


def linear_fwd(d, x, w, bias, resid, y, act_grad=None):
    check(_lib.load().focal_linear_fwd(C.byref(d), _p(x), _p(w), _p(bias), _p(resid), _p(y), _p(act_grad), _stream()))


def linear_resid_ln_fwd(d, x, w, bias, resid, y, gamma, beta, out_dtype, eps=1e-5):
    """y = resid + drop(x w^T + bias) and, from the same kernel, (LayerNorm(y), stats) of the Swin LayerNorm that follows
    (N == 64; N == 128 / 256 in bf16: ops.resid_ln_supported).  Returns (y_ln [M, N] out_dtype, stats [M, 2])."""
    y_ln = torch.empty(d.M, d.N, dtype=out_dtype, device=y.device)
    stats = torch.empty(d.M, 2, dtype=torch.float32, device=y.device)
    check(_lib.load().focal_linear_resid_ln_fwd(C.byref(d), _p(x), _p(w), _p(bias), _p(resid), _p(y), _p(gamma), _p(beta), eps,
                                                _p(y_ln), _p(stats), _stream()))
    return y_ln, stats


def resid_ln_supported(dtype_code, N, K):
    return bool(_lib.load().focal_linear_resid_ln_supported(dtype_code, N, K))


def linear_bwd_data(d, dy, w, x, dx):
    check(_lib.load().focal_linear_bwd_data(C.byref(d), _p(dy), _p(w), _p(x), _p(dx), _stream()))


def bwd_data_ln_supported(dtype_code, N, K):
    return bool(_lib.load().focal_linear_bwd_data_ln_supported(dtype_code, N, K))


def linear_bwd_data_ln(d, dy, w, ln_x, ln_stats, ln_gamma, g, dgamma, dbeta, g_masked=None, mask=None):
    """dX of the linear layer `d` and the backward of the LayerNorm that produced its input, in one kernel: g += dLN(dy . w); dgamma / dbeta
    accumulate; g_masked (dy.dtype) <- g * mask for the residual branch that consumes g next (mask=None: a plain cast)."""
    _need_cuda(dy, w, ln_x, ln_stats, ln_gamma, g, dgamma, dbeta, g_masked)
    if g_masked is not None:
        mask = mask or NO_DROP
    check(_lib.load().focal_linear_bwd_data_ln(C.byref(d), _p(dy), _p(w), _p(ln_x), _p(ln_stats), _p(ln_gamma), _p(g), _p(dgamma), _p(dbeta),
                                               _p(g_masked), C.byref(mask) if mask is not None else None, _stream()))


def linear_bwd_weight(d, dy, x, dw, dbias):
    check(_lib.load().focal_linear_bwd_weight(C.byref(d), _p(dy), _p(x), _p(dw), _p(dbias), _stream()))


def dw_group_supported(dtype_code, M, N, K):
    return bool(_lib.load().focal_linear_bwd_weight_group_supported(dtype_code, M, N, K))


def dw_group_kind(dtype_code, M, N, K):
    """2: a shape for the 128 x 128 grouped weight-gradient launch, 1: for the 64-tile group only (at most 4 problems), 0: neither."""
    return int(_lib.load().focal_linear_bwd_weight_group_kind(dtype_code, M, N, K))


def _dw_problems(items, exclusive):
    arr = (_lib.DwProblem * len(items))()
    for i, (dy, x, dw, db) in enumerate(items):
        _need_cuda(dy, x, dw, db)
        arr[i] = _lib.DwProblem(_p(dy), _p(x), _p(dw), _p(db), dy.shape[0], dy.shape[1], x.shape[1], 1 if exclusive else 0)
    return arr


DW_GROUP_MAX_PROBLEMS = 20  # FOCAL_DW_GROUP_MAX_PROBLEMS (include/focal_hip.h)


def linear_bwd_weight_group(dtype_code, items, exclusive=True):
    """items: [(dy [M, N], x [M, K], dw [N, K] fp32, dbias [N] fp32 | None)] -- the weight gradients of several linear layers as ONE
    launch (focal_linear_bwd_weight_group).  exclusive: nothing else adds to these dw while the launch runs."""
    arr = _dw_problems(items, exclusive)
    check(_lib.load().focal_linear_bwd_weight_group(dtype_code, len(items), arr, _stream()))


DW_TAIL_MAX = 8


def linear_bwd_weight_group_f32(compute_code, items, workgroups=0):
    """items: [(dy [M, N] fp32, x [M, K] fp32, dw [N, K] fp32, dbias [N] fp32 | None)], at most 8 -- weight gradients whose operands are fp32
    tensors (DeepSense's GRU) as ONE launch (focal_linear_bwd_weight_group_f32); `compute_code`: the matrix cores' operand type."""
    for dy, x, dw, db in items:
        if dy.dtype != torch.float32 or x.dtype != torch.float32 or dy.dim() != 2 or x.dim() != 2 or not (dy.is_contiguous() and x.is_contiguous()):
            raise _lib.FocalHipError("linear_bwd_weight_group_f32: dy and x must be contiguous fp32 matrices")
    check(_lib.load().focal_linear_bwd_weight_group_f32(compute_code, len(items), _dw_problems(items, False), workgroups, _stream()))


def linear_bwd_weight_group_workgroups(dtype_code, items, exclusive=True):
    return _lib.load().focal_linear_bwd_weight_group_workgroups(dtype_code, len(items), _dw_problems(items, exclusive))


def linear(x, w, bias=None, *, compute, y_dtype=None, resid=None, act_in=ACT_NONE, epilogue=EPI_NONE, splits=1,
           out_drop=None, act_grad=None):
    """Convenience forward: allocates y.  `compute` is the matrix-core operand dtype (torch.float32 / bfloat16)."""
    _need_cuda(x, w, bias, resid)
    M, K = x.shape
    N = w.shape[0]
    y_dtype = y_dtype or compute
    d = linear_desc(code(compute), M, N, K, code(x.dtype), code(y_dtype), act_in, epilogue, splits, out_drop)
    y = (torch.zeros if splits > 1 else torch.empty)(M, N, dtype=y_dtype, device=x.device)
    linear_fwd(d, x, w, bias, resid, y, act_grad)
    return y, d


# ------------------------------------------------------------------------------------------------ fused MLP branch
def mlp_supported(dtype, Cc, hidden):
    return bool(_lib.load().focal_mlp_supported(code(dtype), Cc, hidden))


def mlp_desc(dtype_code, M, Cc, hidden, drop_hidden=None, drop_out=None, ln_eps=1e-5):
    return MlpDesc(dtype_code, M, Cc, hidden, drop_hidden or NO_DROP, drop_out or NO_DROP, ln_eps)


def mlp_mask_bits(d, device):
    """The hidden-dropout keep bits of one fused-MLP call (int32 [M, 8]; None when the descriptor has no hidden dropout): filled by
    mlp_fwd, read by mlp_bwd -- together with `a` the saved state of the branch."""
    if d.drop_hidden.p_elem <= 0.0:
        return None
    return torch.empty(d.M, 8, dtype=torch.int32, device=device)


def _next_ln(d, like, next_ln):
    """The `next_ln` epilogue of the MLP forwards: the kernel's four pointers (gamma, beta, y_ln, stats) and what the wrapper returns for it,
    (y_ln, stats) allocated here -- or four nulls and None when the caller asked for no LayerNorm."""
    if next_ln is None:
        return (None,) * 4, None
    y_ln = torch.empty(d.M, d.C, dtype=like.dtype, device=like.device)
    stats = torch.empty(d.M, 2, dtype=torch.float32, device=like.device)
    return (_p(next_ln[0]), _p(next_ln[1]), _p(y_ln), _p(stats)), (y_ln, stats)


def _ln_mask(ln, key):
    """The mask pointer of the MLP backwards' fused LayerNorm backward: null without `ln`, else the mask under `key` (no dropout when absent)."""
    return None if ln is None else C.byref(ln.get(key) or NO_DROP)


def mlp_fwd(d, a, resid, w1, b1, w2, b2, y, next_ln=None, mask_bits=None):
    """y = resid + drop_out(drop_hidden(gelu(a w1^T + b1)) w2^T + b2) (focal_mlp_fwd); next_ln = (gamma, beta) also returns
    (LayerNorm(y) in a's dtype, stats) of the LayerNorm that reads y next.  mask_bits (ops.mlp_mask_bits) receives the hidden
    dropout's keep bits for mlp_bwd."""
    _need_cuda(a, resid, w1, b1, w2, b2, y, mask_bits)
    ln_ptrs, out = _next_ln(d, a, next_ln)
    check(_lib.load().focal_mlp_fwd(C.byref(d), _p(a), _p(resid), _p(w1), _p(b1), _p(w2), _p(b2), _p(y), *ln_ptrs, _p(mask_bits), _stream()))
    return out


def mlp_proj_supported(dtype, Cc, hidden):
    return bool(_lib.load().focal_mlp_proj_supported(code(dtype), Cc, hidden))


def mlp_proj_fwd(d, o, x, wp, bp, drop_proj, g2, bt2, x_mid, w1, b1, w2, b2, y, next_ln=None, mask_bits=None):
    """The attention branch's tail and the MLP branch of a 64-channel block in one launch (focal_mlp_proj_fwd): x_mid = x + drop_proj(o wp^T +
    bp) (written to `x_mid`), a2 = LayerNorm(x_mid; g2, bt2), then mlp_fwd.  Returns (a2, st2) and, with next_ln, (y_ln, stats) of the
    LayerNorm that reads y next."""
    _need_cuda(o, x, wp, bp, g2, bt2, x_mid, w1, b1, w2, b2, y, mask_bits)
    a2 = torch.empty(d.M, d.C, dtype=o.dtype, device=o.device)
    st2 = torch.empty(d.M, 2, dtype=torch.float32, device=o.device)
    mask = drop_proj or NO_DROP
    ln_ptrs, out = _next_ln(d, o, next_ln)
    check(_lib.load().focal_mlp_proj_fwd(C.byref(d), _p(o), _p(x), _p(wp), _p(bp), C.byref(mask), _p(g2), _p(bt2), _p(x_mid), _p(a2), _p(st2), _p(w1), _p(b1),
                                         _p(w2), _p(b2), _p(y), *ln_ptrs, _p(mask_bits), _stream()))
    return (a2, st2), out


def mlp_wide_supported(dtype, Cc, hidden):
    return bool(_lib.load().focal_mlp_wide_supported(code(dtype), Cc, hidden))


def mlp_wide_fwd(d, a, resid, w1, b1, w2, b2, y, h, hg, next_ln=None):
    """The MLP branch at 128 / 256 channels as one launch (focal_mlp_wide_fwd): h, hg = drop_hidden(gelu(a w1^T + b1)) and its derivative
    x mask ([M, hidden], written for the backward pass), y = resid + drop_out(h w2^T + b2); next_ln = (gamma, beta) (128 channels) also
    returns (LayerNorm(y) in a's dtype, stats).  Bit-identical to linear_fwd(GELU) + linear_fwd / linear_resid_ln_fwd."""
    _need_cuda(a, resid, w1, b1, w2, b2, y, h, hg)
    assert h.shape == (d.M, d.hidden) and hg.shape == h.shape and h.dtype == a.dtype and hg.dtype == a.dtype and h.is_contiguous() and hg.is_contiguous()
    ln_ptrs, out = _next_ln(d, a, next_ln)
    check(_lib.load().focal_mlp_wide_fwd(C.byref(d), _p(a), _p(resid), _p(w1), _p(b1), _p(w2), _p(b2), _p(y), _p(h), _p(hg), *ln_ptrs, _stream()))
    return out


def mlp_wide_proj_supported(dtype, Cc, hidden):
    return bool(_lib.load().focal_mlp_wide_proj_supported(code(dtype), Cc, hidden))


def mlp_wide_proj_fwd(d, o, x, wp, bp, drop_proj, g2, bt2, x_mid, w1, b1, w2, b2, y, h, hg, next_ln=None):
    """mlp_proj_fwd's form at 128 / 256 channels (focal_mlp_wide_proj_fwd): x_mid = x + drop_proj(o wp^T + bp) (written to `x_mid`),
    a2 = LayerNorm(x_mid; g2, bt2), then mlp_wide_fwd.  Returns (a2, st2), (y_ln, stats) | None."""
    _need_cuda(o, x, wp, bp, g2, bt2, x_mid, w1, b1, w2, b2, y, h, hg)
    a2 = torch.empty(d.M, d.C, dtype=o.dtype, device=o.device)
    st2 = torch.empty(d.M, 2, dtype=torch.float32, device=o.device)
    mask = drop_proj or NO_DROP
    ln_ptrs, out = _next_ln(d, o, next_ln)
    check(_lib.load().focal_mlp_wide_proj_fwd(C.byref(d), _p(o), _p(x), _p(wp), _p(bp), C.byref(mask), _p(g2), _p(bt2), _p(x_mid), _p(a2), _p(st2), _p(w1), _p(b1),
                                              _p(w2), _p(b2), _p(y), _p(h), _p(hg), *ln_ptrs, _stream()))
    return (a2, st2), out


def mlp_wide_bwd_supported(dtype, Cc, hidden):
    return bool(_lib.load().focal_mlp_wide_bwd_supported(code(dtype), Cc, hidden))


def mlp_wide_bwd_data(d, gm, hg, w1, w2, du, dc=None, ln=None):
    """du = (gm w2) x hg and dc = du w1 in one launch (focal_mlp_wide_bwd_data).  dc: the [M, C] output; or ln = dict(x=, stats=, gamma=, g=,
    g_masked=, mask=, dgamma=, dbeta=) (128 channels): norm2's backward finished on the row as linear_bwd_data_ln does."""
    _need_cuda(gm, hg, w1, w2, du, dc)
    assert du.shape == (d.M, d.hidden) and du.dtype == gm.dtype and du.is_contiguous() and hg.shape == du.shape
    if ln is None:
        assert dc is not None and dc.shape == (d.M, d.C) and dc.dtype == gm.dtype and dc.is_contiguous()
    L = ln or {}  # (with ln the row's LayerNorm backward replaces dc: the kernel gets no dc pointer; without it no mask pointer)
    check(_lib.load().focal_mlp_wide_bwd_data(C.byref(d), _p(gm), _p(hg), _p(w1), _p(w2), _p(du), _p(dc if ln is None else None), _p(L.get("x")), _p(L.get("stats")),
                                              _p(L.get("gamma")), _p(L.get("g")), _p(L.get("g_masked")), _ln_mask(ln, "mask"), _p(L.get("dgamma")),
                                              _p(L.get("dbeta")), _stream()))


def mlp_bwd_partials_floats(d):
    return int(_lib.load().focal_mlp_bwd_partials_floats(C.byref(d)))


def mlp_bwd_partials(d, device):
    """The workspace focal_mlp_bwd sums its workgroups' weight-gradient images through (instead of fp32 atomics): fp32 [workgroups * 32768]."""
    return torch.empty(int(_lib.load().focal_mlp_bwd_partials_floats(C.byref(d))), dtype=torch.float32, device=device)


def mlp_bwd(d, gm, a, w1, b1, w2, da, dw1, db1, dw2, db2, ln=None, mask_bits=None, partials=None):
    """focal_mlp_bwd.  mask_bits: what mlp_fwd filled (required when the descriptor has hidden dropout).  ln = dict(x=, stats=, gamma=,
    g=, gm_next=, next_mask=, dgamma=, dbeta=) fuses the backward of the LayerNorm that produced `a` (norm2) into the kernel: g += dLN,
    gm_next = dtype(g x next_mask), dgamma / dbeta accumulate, and `da` is neither needed nor written (pass None) -- what the Swin engine
    always does.  partials (mlp_bwd_partials): the weight gradients leave through a workspace + a reduce launch instead of atomics."""
    _need_cuda(gm, a, w1, b1, w2, da, dw1, db1, dw2, db2, mask_bits, partials)
    L = ln or {}
    check(_lib.load().focal_mlp_bwd(C.byref(d), _p(gm), _p(a), _p(w1), _p(b1), _p(w2), _p(da), _p(dw1), _p(db1), _p(dw2), _p(db2),
                                    _p(L.get("x")), _p(L.get("stats")), _p(L.get("gamma")), _p(L.get("g")), _p(L.get("gm_next")), _ln_mask(ln, "next_mask"),
                                    _p(L.get("dgamma")), _p(L.get("dbeta")), _p(mask_bits), _p(partials), _stream()))


# ------------------------------------------------------------------------------------------------ row 10
def attn_desc(dtype_code, B, H, W, Cc, heads, wh, ww, sh, sw, p_attn=0.0, rng=None, stream=0):
    return AttnDesc(dtype_code, B, H, W, Cc, heads, wh, ww, sh, sw, p_attn, _p(rng), stream)


def window_attn_fwd(d, qkv, bias_table, out):
    check(_lib.load().focal_window_attn_fwd(C.byref(d), _p(qkv), _p(bias_table), _p(out), _stream()))


def window_attn_bwd(d, qkv, bias_table, dout, dqkv, dbias_table):
    check(_lib.load().focal_window_attn_bwd(C.byref(d), _p(qkv), _p(bias_table), _p(dout), _p(dqkv), _p(dbias_table),
                                            _stream()))


def attn_qkv_supported(dtype_code, Cc, heads, window_tokens):
    return bool(_lib.load().focal_window_attn_qkv_supported(dtype_code, Cc, heads, window_tokens))


def window_attn_qkv_fwd(d, a1, wqkv, bqkv, bias_table, out):
    """W-MSA with the qkv Linear folded in (64-channel blocks): a1 [M, C] -> out [M, C]; no [M, 3C] tensor."""
    _need_cuda(a1, wqkv, bqkv, bias_table, out)
    check(_lib.load().focal_window_attn_qkv_fwd(C.byref(d), _p(a1), _p(wqkv), _p(bqkv), _p(bias_table), _p(out), _stream()))


def window_attn_qkv_bwd(d, a1, wqkv, bqkv, bias_table, dout, dqkv, dbias_table, wproj=None):
    """wproj given: `dout` is the gradient w.r.t. the proj Linear's OUTPUT (masked, operand dtype) and the kernel forms dout . wproj itself."""
    _need_cuda(a1, wqkv, bqkv, bias_table, dout, dqkv, dbias_table, wproj)
    check(_lib.load().focal_window_attn_qkv_bwd(C.byref(d), _p(a1), _p(wqkv), _p(bqkv), _p(bias_table), _p(dout), _p(wproj), _p(dqkv),
                                                _p(dbias_table), _stream()))


# ------------------------------------------------------------------------------------------------ rows 11-13
_LOSS_WS = {}


def _loss_setup(feats1, feats2, temperature, margin, weights, seq, no_private):
    feats = list(feats1) + list(feats2)
    _need_cuda(*feats)
    M = len(feats1)
    B, dim = feats[0].shape
    dev = feats[0].device
    d = LossDesc(M, B, dim, seq, temperature, margin, weights[0], weights[1], weights[2], weights[3], int(no_private))
    lib = _lib.load()
    need = lib.focal_loss_head_workspace(C.byref(d))
    if need == 0:
        raise _lib.FocalHipError(f"loss_head: {lib.focal_last_error().decode()}")
    key = (dev, torch.cuda.current_stream().cuda_stream)
    ws = _LOSS_WS.get(key)
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        _LOSS_WS[key] = ws
    # one allocation [2M gradients | terms(5) + pad]: the library zeroes it with one memset, the autograd node scales it with one launch
    n = B * dim
    flat = torch.empty(2 * M * n + 8, dtype=torch.float32, device=dev)
    # ABI order is view-major (index v * M + m); memory order is modality-major, so a modality's two view gradients are the
    # two halves of one [2B, dim] block (what a backbone that ran both views as one batch wants back, without a concatenation)
    grads = [flat[(m * 2 + v) * n:(m * 2 + v + 1) * n].view(B, dim) for v in range(2) for m in range(M)]
    terms = flat[2 * M * n:2 * M * n + 5]
    fa = (C.c_void_p * (2 * M))(*[_p(f) for f in feats])
    ga = (C.c_void_p * (2 * M))(*[_p(g) for g in grads])
    return lib, d, M, n, feats, flat, grads, terms, fa, ga, ws


def loss_head(feats1, feats2, temperature, margin, weights, seq=4, no_private=False, return_flat=False):
    """feats{1,2}: lists (modality order) of fp32 [B, dim].  Returns (terms[5] device tensor, grads1, grads2)."""
    lib, d, M, n, feats, flat, grads, terms, fa, ga, ws = _loss_setup(feats1, feats2, temperature, margin, weights, seq, no_private)
    check(lib.focal_loss_head(C.byref(d), fa, _p(terms), ga, _p(ws), ws.numel(), _stream()))
    if return_flat:  # the gradients as ONE tensor (they are views of it)
        return terms, grads[:M], grads[M:], flat[:2 * M * n]
    return terms, grads[:M], grads[M:]


class ShardedLossHead:
    """The loss head of `world` data-parallel ranks, each over the rows of its own samples (focal_loss_head_shard_a / _b).
    `phase_a(...)` fills the persistent `send` buffer [n]; the caller all-gathers it into `chunks` [world, n];
    `phase_b()` returns what `loss_head(..., return_flat=True)` returns; only the rank's own rows of the gradients are non-zero."""

    _BUF = {}

    def __init__(self, rank, world):
        self.rank, self.world = rank, world
        self.state = None

    def exchange_buffers(self, d, dev):
        n = _lib.load().focal_loss_head_exchange_floats(C.byref(d), self.world)
        if n == 0:
            raise _lib.FocalHipError(f"loss_head (sharded): {_lib.load().focal_last_error().decode()}")
        key = (dev, self.world, n)
        if key not in self._BUF:  # address-stable: captured graph segments write / read them, the collective between them is eager
            self._BUF[key] = (torch.zeros(n, dtype=torch.float32, device=dev), torch.zeros(self.world, n, dtype=torch.float32, device=dev))
        return self._BUF[key]

    def phase_a(self, feats1, feats2, temperature, margin, weights, seq=4, no_private=False):
        lib, d, M, n, feats, flat, grads, terms, fa, ga, ws = _loss_setup(feats1, feats2, temperature, margin, weights, seq, no_private)
        self.send, self.chunks = self.exchange_buffers(d, feats[0].device)
        check(lib.focal_loss_head_shard_a(C.byref(d), self.rank, self.world, fa, _p(terms), ga, _p(self.send), _p(ws), ws.numel(), _stream()))
        self.state = (lib, d, M, n, feats, flat, grads, terms, fa, ga, ws)
        return self.send, self.chunks

    def phase_b(self):
        lib, d, M, n, feats, flat, grads, terms, fa, ga, ws = self.state
        self.state = None
        check(lib.focal_loss_head_shard_b(C.byref(d), self.rank, self.world, fa, _p(terms), ga, _p(self.chunks), _p(ws), ws.numel(), _stream()))
        return terms, grads[:M], grads[M:], flat[:2 * M * n]


# ------------------------------------------------------------------------------------------------ rows 5-6 (DeepSense)
def conv_in_desc(B, cin, I, S_in, S_out, k, stride, pad_left, Cc):
    return ConvInDesc(B, cin, I, S_in, S_out, k, stride, pad_left, Cc)


def conv_in_fwd(d, x, w, bias):
    z = torch.empty(d.B * d.I * d.S_out, d.C, dtype=torch.float32, device=x.device)
    check(_lib.load().focal_conv_in_fwd(C.byref(d), _p(x), _p(w), _p(bias), _p(z), _stream()))
    return z


def conv_in_bwd_weight(d, x, dz, dw, dbias):
    check(_lib.load().focal_conv_in_bwd_weight(C.byref(d), _p(x), _p(dz), code(dz.dtype), _p(dw), _p(dbias), _stream()))


def conv_in_bwd_data(d, dz, w, scale=1.0, out=None):
    """dx [B*I, S] fp32 = scale * conv_in^T(dz): the in-conv's input gradient where its input is not a leaf (cin = 1, stride 1 only)."""
    _need_cuda(dz, w)
    if not dz.is_contiguous() or dz.numel() != d.B * d.I * d.S_out * d.C:
        raise _lib.FocalHipError(f"conv_in_bwd_data: dz must be a contiguous [{d.B * d.I * d.S_out}, {d.C}] tensor")
    if w.dtype != torch.float32 or not w.is_contiguous() or w.numel() != d.C * d.cin * d.k:
        raise _lib.FocalHipError("conv_in_bwd_data: w must be the contiguous fp32 [C, cin, 1, k] filter")
    dx = torch.empty(d.B * d.I, d.S_in, dtype=torch.float32, device=dz.device) if out is None else out
    if dx.dtype != torch.float32 or not dx.is_contiguous() or dx.numel() != d.B * d.I * d.S_in:
        raise _lib.FocalHipError("conv_in_bwd_data: out must be a contiguous fp32 [B*I, S] tensor")
    check(_lib.load().focal_conv_in_bwd_data(C.byref(d), _p(dz), code(dz.dtype), _p(w), float(scale), _p(dx), _stream()))
    return dx


def rows_mean(xs, out=None):
    """y = (xs[0] + ... + xs[L-1]) / L for 2 <= L <= 8 equal-shaped contiguous fp32 tensors: one launch, the pointers travel by value."""
    _need_cuda(*xs)
    L, n = len(xs), xs[0].numel()
    if not 2 <= L <= 8:
        raise _lib.FocalHipError(f"rows_mean: 2 .. 8 inputs (got {L})")
    if any(x.dtype != torch.float32 or not x.is_contiguous() or x.numel() != n for x in xs):
        raise _lib.FocalHipError("rows_mean: inputs must be contiguous fp32 tensors of one size")
    y = torch.empty_like(xs[0]) if out is None else out
    ptrs = _lib.Ptr8()
    for i, x in enumerate(xs):
        ptrs.p[i] = x.data_ptr()
    check(_lib.load().focal_rows_mean(n, L, ptrs, _p(y), _stream()))
    return y


def permute_pack(src, A, Bd, Cd, dtype):
    """dst[a][c][b] = src[a][b][c], cast to `dtype`."""
    dst = torch.empty(A, Cd, Bd, dtype=dtype, device=src.device)
    check(_lib.load().focal_permute_pack(A, Bd, Cd, _p(src), _p(dst), code(dtype), _stream()))
    return dst


def permute_unpack_add(src, dst, A, Bd, Cd):
    """dst[a][b][c] += src[a][c][b] (fp32)."""
    check(_lib.load().focal_permute_unpack_add(A, Bd, Cd, _p(src), _p(dst), _stream()))


PACK_PERMUTE, PACK_CONV_BWD, PACK_FRAG, PACK_FRAG_T = 0, 1, 2, 3
PACK_MAX = 24


def pack_multi(entries, dtype):
    """entries: [(src fp32, dst `dtype`, A, B, C, kind)] -- every re-ordering of an encoder's weights in one launch."""
    arr = (_lib.PackEntry * len(entries))()
    for i, (src, dst, A, Bd, Cd, kind) in enumerate(entries):
        _need_cuda(src, dst)
        arr[i] = _lib.PackEntry(_p(src), _p(dst), A, Bd, Cd, kind)
    check(_lib.load().focal_pack_multi(code(dtype), len(entries), arr, _stream()))


def unpack_add_multi(entries):
    """entries: [(src packed fp32 [A][C][B], dst fp32 [A][B][C], A, B, C)]: dst += unpacked src, one launch."""
    arr = (_lib.PackEntry * len(entries))()
    for i, (src, dst, A, Bd, Cd) in enumerate(entries):
        _need_cuda(src, dst)
        arr[i] = _lib.PackEntry(_p(src), _p(dst), A, Bd, Cd, PACK_PERMUTE)
    check(_lib.load().focal_unpack_add_multi(len(entries), arr, _stream()))


def conv_desc(dtype_code, rows, S, C_in, C_out, k, dw_workgroups=0):
    return ConvDesc(dtype_code, rows, S, C_in, C_out, k, dw_workgroups)


def conv_pack_bwd(d, w, dtype):
    dst = torch.empty(d.C_in, d.k, d.C_out, dtype=dtype, device=w.device)
    check(_lib.load().focal_conv_pack_bwd(C.byref(d), _p(w), _p(dst), _stream()))
    return dst


def conv_fwd(d, x, w_fwd, bias):
    z = torch.empty(d.rows, d.C_out, dtype=torch.float32, device=x.device)
    check(_lib.load().focal_conv_fwd(C.byref(d), _p(x), _p(w_fwd), _p(bias), _p(z), _stream()))
    return z


def conv_fwd_bn_sums_supported(d, d_bn, x, w_fwd):
    return bool(_lib.load().focal_conv_fwd_bn_sums_supported(C.byref(d), C.byref(d_bn), _p(x), _p(w_fwd)))


def conv_fwd_bn_sums(d, x, w_fwd, bias, d_bn):
    """focal_conv_fwd_bn in its sums-only form (round 6): -> (z, sums); bn_act_fwd_sums finishes the statistics."""
    dev = x.device
    z = torch.empty(d.rows, d.C_out, dtype=torch.float32, device=dev)
    n = _bn_groups(d_bn) * (_lib.BN_STAT_SLOTS * 2 * d_bn.C + 1)
    scratch = pool_zeros(n, dev)
    if scratch is None:
        scratch = torch.zeros(n, dtype=torch.float32, device=dev)
    check(_lib.load().focal_conv_fwd_bn(C.byref(d), _p(x), _p(w_fwd), _p(bias), _p(z), C.byref(d_bn), _p(scratch), None, None, None, _stream()))
    return z, scratch


def bn_act_fwd_sums(d, z, sums, running_mean, running_var, gamma, beta, resid, cast_dtype=None):
    """bn_act_fwd on a convolution's per-channel sums (conv_fwd_bn_sums): -> (y, y_cast, mean_rstd)."""
    y = torch.empty_like(z)
    ya = torch.empty(z.shape, dtype=cast_dtype, device=z.device) if cast_dtype not in (None, torch.float32) else None
    mean_rstd = torch.empty(_bn_groups(d) * 2 * d.C, dtype=torch.float32, device=z.device)
    check(_lib.load().focal_bn_act_fwd_sums(C.byref(d), _p(z), _p(sums), _p(mean_rstd), _p(running_mean), _p(running_var), _p(gamma), _p(beta),
                                            _p(resid), _p(y), _p(ya), _stream()))
    return y, (ya if ya is not None else y), mean_rstd


def conv_fwd_bn(d, x, w_fwd, bias, d_bn, running_mean, running_var):
    """conv_fwd + the training-mode statistics of the BatchNorm behind it in one launch (focal_conv_fwd_bn): -> (z, mean_rstd).  One rank /
    no sync_bn (the global-batch form all-reduces the sums between two kernels: conv_fwd + bn_stats)."""
    dev = x.device
    z = torch.empty(d.rows, d.C_out, dtype=torch.float32, device=dev)
    G = _bn_groups(d_bn)
    n = G * (_lib.BN_STAT_SLOTS * 2 * d_bn.C + 1)
    scratch = pool_zeros(n, dev)
    if scratch is None:
        scratch = torch.zeros(n, dtype=torch.float32, device=dev)
    mean_rstd = torch.empty(G * 2 * d_bn.C, dtype=torch.float32, device=dev)
    check(_lib.load().focal_conv_fwd_bn(C.byref(d), _p(x), _p(w_fwd), _p(bias), _p(z), C.byref(d_bn), _p(scratch), _p(mean_rstd),
                                        _p(running_mean), _p(running_var), _stream()))
    return z, mean_rstd


def conv_bwd_data(d, dz, w_bwd, g_in, g_out):
    check(_lib.load().focal_conv_bwd_data(C.byref(d), _p(dz), _p(w_bwd), _p(g_in), _p(g_out), _stream()))


def conv_bwd_weight(d, dz, x, dw_packed, dbias):
    check(_lib.load().focal_conv_bwd_weight(C.byref(d), _p(dz), _p(x), _p(dw_packed), _p(dbias), _stream()))


def bn_desc(dtype_code, rows, Cc, rows_per_sample, p_drop=0.0, rng=None, stream=0, eps=1e-5, momentum=0.1, stat_rows=0, groups=1):
    """groups > 1: the rows are `groups` equal consecutive ranges with batch statistics of their own (the two views of a FOCAL step as
    one batch): mean_rstd [groups, 2C], the running buffers handed to bn_stats / conv_fwd_bn are per-group sinks [groups, C]."""
    return BNDesc(dtype_code, rows, Cc, rows_per_sample, eps, momentum, p_drop, _p(rng), stream, stat_rows, groups)


def _bn_groups(d):
    return d.groups if d.groups > 1 else 1


def _sync_world():
    import torch.distributed as dist
    return dist.get_world_size() if (dist.is_available() and dist.is_initialized()) else 1


def bn_stats(d, z, running_mean, running_var, training, sync=False):
    """mean / rstd of z [rows, C].  sync=True under torch.distributed: the 2C per-channel sums are all-reduced between the
    partial and the finalize kernels, so every rank normalises with the statistics of the GLOBAL batch (equal shards)."""
    dev = running_mean.device
    G = _bn_groups(d)
    scratch = pool_zeros(G * (2 * d.C + 1), dev) if training else None  # {sum, sum of squares} + the statistics kernel's arrival counter
    pre = _lib.BN_SCRATCH_ZEROED if scratch is not None else 0
    if scratch is None:
        scratch = torch.empty(G * (2 * d.C + 1), dtype=torch.float32, device=dev)
    mean_rstd = torch.empty(G * 2 * d.C, dtype=torch.float32, device=dev)
    lib = _lib.load()
    args = (_p(z), _p(scratch), _p(mean_rstd), _p(running_mean), _p(running_var))
    world = _sync_world() if (sync and training) else 1
    if world > 1:
        import torch.distributed as dist
        check(lib.focal_bn_stats(C.byref(d), *args, _lib.BN_PARTIAL | pre, _stream()))
        dist.all_reduce(scratch[:2 * d.C], op=dist.ReduceOp.SUM)
        d.stat_rows = d.rows * world
        check(lib.focal_bn_stats(C.byref(d), *args, _lib.BN_FINALIZE, _stream()))
    else:
        check(lib.focal_bn_stats(C.byref(d), *args, (_lib.BN_TRAIN | pre) if training else _lib.BN_EVAL, _stream()))
    return mean_rstd


def bn_running_combine(running, view1, view2, momentum=0.1):
    """running[i] <- (1 - m) ((1 - m) running[i] + m view1[i]) + m view2[i] for n same-sized fp32 buffers, one launch."""
    _need_cuda(*running, *view1, *view2)
    check(_lib.load().focal_bn_running_combine(len(running), _parr(running), _parr(view1), _parr(view2), running[0].numel(), momentum, _stream()))


def bn_act_fwd(d, z, mean_rstd, gamma, beta, resid, cast_dtype=None):
    y = torch.empty_like(z)
    ya = torch.empty(z.shape, dtype=cast_dtype, device=z.device) if cast_dtype not in (None, torch.float32) else None
    check(_lib.load().focal_bn_act_fwd(C.byref(d), _p(z), _p(mean_rstd), _p(gamma), _p(beta), _p(resid), _p(y), _p(ya), _stream()))
    return y, (ya if ya is not None else y)


def bn_act_bwd(d, z, g, mean_rstd, gamma, beta, dgamma, dbeta, out_dtype, sync=False):
    G = _bn_groups(d)
    scratch = pool_zeros(G * (2 * d.C + 1), z.device)
    pre = _lib.BN_SCRATCH_ZEROED if scratch is not None else 0
    if scratch is None:
        scratch = torch.empty(G * (2 * d.C + 1), dtype=torch.float32, device=z.device)
    dz = torch.empty(z.shape, dtype=out_dtype, device=z.device)
    lib = _lib.load()
    args = (_p(z), _p(g), _p(mean_rstd), _p(gamma), _p(beta), _p(scratch), _p(dz), _p(dgamma), _p(dbeta))
    world = _sync_world() if sync else 1
    if world > 1:
        import torch.distributed as dist
        check(lib.focal_bn_act_bwd(C.byref(d), *args, _lib.BN_PARTIAL | pre, _stream()))
        dist.all_reduce(scratch[:2 * d.C], op=dist.ReduceOp.SUM)
        d.stat_rows = d.rows * world
        check(lib.focal_bn_act_bwd(C.byref(d), *args, _lib.BN_FINALIZE, _stream()))
    else:
        check(lib.focal_bn_act_bwd(C.byref(d), *args, _lib.BN_TRAIN | pre, _stream()))
    return dz


def gru_gate_fwd(d, t, dir_off, gi, gh, h_prev, h_new, out, save):
    check(_lib.load().focal_gru_gate_fwd(C.byref(d), t, dir_off, _p(gi), _p(gh), _p(h_prev), _p(h_new), _p(out), _p(save), _stream()))


def gru_gate_bwd(d, t, dir_off, dout, ld_b, ld_t, scale, dh_rec, dhz_in, save, h_prev, dgi, dgh, dhz_out):
    check(_lib.load().focal_gru_gate_bwd(C.byref(d), t, dir_off, _p(dout), ld_b, ld_t, scale, _p(dh_rec), _p(dhz_in), _p(save),
                                         _p(h_prev), _p(dgi), _p(dgh), _p(dhz_out), _stream()))


def _parr(tensors):
    return (C.c_void_p * len(tensors))(*[_p(t) for t in tensors])


def gru_seq_fwd(d, gi, whh, bhh, hs, save, out):
    """Whole-sequence GRU layer, one launch for len(gi) directions (lists of per-direction tensors)."""
    check(_lib.load().focal_gru_seq_fwd(C.byref(d), len(gi), _parr(gi), _parr(whh), _parr(bhh), _parr(hs), _parr(save), _p(out), _stream()))


def gru_seq_bwd(d, dout, ld_b, ld_t, scale, whh_t, hs, save, dgi, dgh):
    check(_lib.load().focal_gru_seq_bwd(C.byref(d), len(hs), _p(dout), ld_b, ld_t, scale, _parr(whh_t), _parr(hs), _parr(save), _parr(dgi),
                                        _parr(dgh), _stream()))


def fusion_attn_fwd(B, M, E, heads, q, kv, out, probs, weights, rng, stream_id, p_drop):
    check(_lib.load().focal_fusion_attn_fwd(B, M, E, heads, _p(q), _p(kv), _p(out), _p(probs), _p(weights), _p(rng), stream_id, p_drop, _stream()))


def fusion_attn_bwd(B, M, E, heads, q, kv, probs, weights, dout, dq, dkv):
    check(_lib.load().focal_fusion_attn_bwd(B, M, E, heads, _p(q), _p(kv), _p(probs), _p(weights), _p(dout), _p(dq), _p(dkv), _stream()))


def loc_attn_fwd(N, L, E, heads, qkv, out, probs, weights, rng, stream_id, p_drop):
    _need_cuda(qkv, out, probs, weights)
    check(_lib.load().focal_loc_attn_fwd(N, L, E, heads, _p(qkv), _p(out), _p(probs), _p(weights), _p(rng), stream_id, p_drop, _stream()))


def loc_attn_bwd(N, L, E, heads, qkv, probs, weights, dout, dqkv):
    _need_cuda(qkv, probs, weights, dout, dqkv)
    check(_lib.load().focal_loc_attn_bwd(N, L, E, heads, _p(qkv), _p(probs), _p(weights), _p(dout), _p(dqkv), _stream()))


def loc_stack(feats, out):
    """out [N, L, E] <- the L location features [N, E] (one launch)."""
    _need_cuda(out, *feats)
    N, L, E = out.shape
    ptrs = (C.c_void_p * L)(*[f.data_ptr() for f in feats])
    check(_lib.load().focal_loc_stack(N, L, E, ptrs, _p(out), _stream()))


def loc_unstack_add(a, b, dst):
    """dst[l] [N, E] <- a[:, l] + b[:, l] for a, b [N, L, E]."""
    _need_cuda(a, b, *dst)
    N, L, E = a.shape
    ptrs = (C.c_void_p * L)(*[d.data_ptr() for d in dst])
    check(_lib.load().focal_loc_unstack_add(N, L, E, _p(a), _p(b), ptrs, _stream()))


def loc_mean_bwd_add(dq, dx):
    """dx [N, L, E] += dq [N, E] / L (the gradient of a mean over the L tokens)."""
    _need_cuda(dq, dx)
    N, L, E = dx.shape
    check(_lib.load().focal_loc_mean_bwd_add(N, L, E, _p(dq), _p(dx), _stream()))


def small_linear_fwd(x, w, bias):
    B, K = x.shape
    y = torch.empty(B, w.shape[0], dtype=torch.float32, device=x.device)
    check(_lib.load().focal_small_linear_fwd(B, w.shape[0], K, _p(x), _p(w), _p(bias), _p(y), _stream()))
    return y


def small_linear_bwd(dy, x, w, dw, dbias, need_dx=True):
    B, K = x.shape
    dx = torch.empty_like(x) if need_dx else None
    check(_lib.load().focal_small_linear_bwd(B, w.shape[0], K, _p(dy), _p(x), _p(w), _p(dw), _p(dbias), _p(dx), _stream()))
    return dx


def cross_entropy(logits, labels):
    """nn.CrossEntropyLoss() (mean): returns (loss [1] fp32, dlogits [B, C])."""
    _need_cuda(logits, labels)
    B, Cn = logits.shape
    logits = logits.float().contiguous()
    labels = labels.long().contiguous()
    loss = torch.empty(1, dtype=torch.float32, device=logits.device)
    dlogits = torch.empty_like(logits)
    check(_lib.load().focal_cross_entropy(B, Cn, _p(logits), _p(labels), _p(loss), _p(dlogits), _stream()))
    return loss, dlogits


def eval_accumulate(acc, conf, labels, logits=None, preds=None, preds_out=None):
    """One batch into the evaluation accumulators (focal_eval_accumulate), no host read.  Caller-owned: acc fp64 [2] = {sum of the
    per-batch mean losses, batches}, conf int32 [C*C + 1] = the confusion matrix conf[label * C + pred] and, last, the count of rows
    whose label or prediction lies outside [0, C).  Exactly one of logits (fp32 [B, C]; the loss and the argmax are taken in the
    kernel) and preds ([B] class indices; the matrix alone).  preds_out (int64 [B]) receives the predictions.  The inputs (labels,
    logits, preds) are converted to int64 / fp32 and copied when they are strided; acc, conf and preds_out are written in place and
    must be contiguous."""
    labels = labels.long().contiguous()
    logits = None if logits is None else logits.float().contiguous()
    preds = None if preds is None else preds.long().contiguous()
    _need_cuda(acc, conf, labels, logits, preds, preds_out)
    if acc.dtype != torch.float64 or acc.numel() != 2 or conf.dtype != torch.int32:
        raise _lib.FocalHipError("eval_accumulate: acc must be fp64 [2] and conf int32 [C*C + 1]")
    Cn = math.isqrt(max(conf.numel() - 1, 0))
    if Cn * Cn + 1 != conf.numel():
        raise _lib.FocalHipError(f"eval_accumulate: conf holds {conf.numel()} words, which is not C*C + 1 for any C")
    B = labels.numel()
    if logits is not None and tuple(logits.shape) != (B, Cn):
        raise _lib.FocalHipError(f"eval_accumulate: logits {tuple(logits.shape)} against {B} labels and a {Cn} x {Cn} matrix")
    if preds is not None and preds.numel() != B:
        raise _lib.FocalHipError(f"eval_accumulate: {preds.numel()} predictions against {B} labels")
    if preds_out is not None and (preds_out.dtype != torch.int64 or preds_out.numel() != B):
        raise _lib.FocalHipError("eval_accumulate: preds_out must be int64 [B]")
    check(_lib.load().focal_eval_accumulate(B, Cn, _p(logits), _p(preds), _p(labels), _p(acc), _p(conf), _p(preds_out), _stream()))


class EvalState:
    """Loss and confusion matrix of one evaluation pass, kept on the device: `add` is one launch per batch, `read` the pass's one
    synchronising call."""

    def __init__(self, num_classes, device):
        self.C = int(num_classes)
        self.acc = torch.zeros(2, dtype=torch.float64, device=device)
        self.conf = torch.zeros(self.C * self.C + 1, dtype=torch.int32, device=device)

    def add(self, labels, logits=None, preds=None, preds_out=None):
        eval_accumulate(self.acc, self.conf, labels, logits=logits, preds=preds, preds_out=preds_out)

    def read(self):
        """(sum of the per-batch mean losses, number of batches, confusion matrix as int64 numpy [C, C]); one device-to-host copy."""
        words = torch.cat([self.acc.view(torch.int32), self.conf]).cpu().numpy()
        loss_sum, n_batches = words[:4].view("float64")
        rejected, cells = int(words[-1]), self.C * self.C
        if rejected:
            raise ValueError(f"{rejected} evaluated rows carry a label or a prediction outside [0, {self.C})")
        return float(loss_sum), int(n_batches), words[4:4 + cells].astype("int64").reshape(self.C, self.C)


def knn_check_limits(D, k, n_classes):
    """The limits of focal_knn_search / focal_knn_vote on the feature width, k and the class count, refused here with the limit named
    (the library refuses them too, before any launch)."""
    if not 1 <= k <= _lib.KNN_MAX_K:
        raise _lib.FocalHipError(f"knn: need 1 <= k <= {_lib.KNN_MAX_K} (got k={k})")
    if not 1 <= n_classes <= _lib.KNN_MAX_CLASSES:
        raise _lib.FocalHipError(f"knn: need 1 <= n_classes <= {_lib.KNN_MAX_CLASSES} (got n_classes={n_classes})")
    if D < 4 or D % 4:
        raise _lib.FocalHipError(f"knn: need a feature width D >= 4 with D % 4 == 0 (got D={D})")


def knn_default_slices(nq, nt, device):
    """Slices of the training rows so that the search launches about two workgroups per CU, never more than there are training tiles."""
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    q_tiles = -(-nq // _lib.KNN_QUERY_TILE)
    return max(1, min(-(-nt // _lib.KNN_TRAIN_TILE), round(2 * cus / q_tiles)))


def knn_search_vote(q, t, t_sq, t_labels, k, n_classes, q_labels=None, conf=None, want_neighbours=False, slices=None):
    """The k nearest rows of t (fp32 [nt, D], squared norms t_sq [nt], labels t_labels int64 [nt]) for every row of q (fp32 [nq, D]) and
    their vote (focal_knn_search + focal_knn_vote: two launches, no host read).  Returns preds (int64 [nq]) and, with want_neighbours,
    also nbr_idx (int32 [nq, k]) and nbr_d2 (fp32 [nq, k]), sorted by (d2, index); columns from min(k, nt) on hold -1 / +inf.  conf
    (int32 [C*C + 1], with q_labels) accumulates the confusion matrix as eval_accumulate's prediction mode does.  The results do not
    depend on `slices` (None: knn_default_slices)."""
    _need_cuda(q, t, t_sq, t_labels, q_labels, conf)
    if q.dtype != torch.float32 or t.dtype != torch.float32 or t_sq.dtype != torch.float32 or q.dim() != 2 or t.dim() != 2:
        raise _lib.FocalHipError("knn_search_vote: q, t and t_sq are fp32, q and t matrices")
    nq, D = q.shape
    nt = t.shape[0]
    if t.shape[1] != D or t_sq.numel() != nt or t_labels.dtype != torch.int64 or t_labels.numel() != nt:
        raise _lib.FocalHipError(f"knn_search_vote: q {tuple(q.shape)} against t {tuple(t.shape)}, {t_sq.numel()} norms and "
                                 f"{t_labels.numel()} int64 labels")
    if nq < 1 or nt < 1:
        raise _lib.FocalHipError(f"knn_search_vote: need nq >= 1 and nt >= 1 (got nq={nq} nt={nt})")
    k, n_classes = int(k), int(n_classes)
    knn_check_limits(D, k, n_classes)
    if conf is not None:
        if conf.dtype != torch.int32 or conf.numel() != n_classes * n_classes + 1:
            raise _lib.FocalHipError(f"knn_search_vote: conf must be int32 [{n_classes * n_classes + 1}]")
        if q_labels is None or q_labels.dtype != torch.int64 or q_labels.numel() != nq:
            raise _lib.FocalHipError("knn_search_vote: a confusion matrix needs q_labels int64 [nq]")
    slices = knn_default_slices(nq, nt, q.device) if slices is None else int(slices)
    if slices < 1:
        raise _lib.FocalHipError(f"knn_search_vote: need slices >= 1 (got {slices})")
    d = _lib.KnnDesc(nq, nt, D, k, n_classes, slices)
    lib = _lib.load()
    part_d2 = torch.empty(nq, slices, k, dtype=torch.float32, device=q.device)
    part_idx = torch.empty(nq, slices, k, dtype=torch.int32, device=q.device)
    check(lib.focal_knn_search(C.byref(d), _p(q), _p(t), _p(t_sq), _p(part_d2), _p(part_idx), _stream()))
    preds = torch.empty(nq, dtype=torch.int64, device=q.device)
    nbr_idx = torch.empty(nq, k, dtype=torch.int32, device=q.device) if want_neighbours else None
    nbr_d2 = torch.empty(nq, k, dtype=torch.float32, device=q.device) if want_neighbours else None
    check(lib.focal_knn_vote(C.byref(d), _p(part_d2), _p(part_idx), _p(t_labels), _p(q_labels), _p(preds), _p(nbr_idx), _p(nbr_d2),
                             _p(conf), _stream()))
    return (preds, nbr_idx, nbr_d2) if want_neighbours else preds


def rank_check_limits(D, nq, nt, slices):
    """The limits of focal_rank_positive on the feature width, the row counts and the slices, refused here with the library's own text
    (it refuses them too, before any launch)."""
    if D < 4 or D % 4:
        raise _lib.FocalHipError(f"rank_positive: need D >= 4 and D % 4 == 0 (got D={D})")
    if nq < 1 or nt < 1:
        raise _lib.FocalHipError(f"rank_positive: need nq >= 1 and nt >= 1 (got nq={nq} nt={nt})")
    if not 1 <= slices <= _lib.RANK_MAX_SLICES:
        raise _lib.FocalHipError(f"rank_positive: need 1 <= slices <= {_lib.RANK_MAX_SLICES} (got slices={slices})")


def rank_positive(q, t, t_sq, pos, slices=None, want_d2=False):
    """Where row pos[i] of t (fp32 [nt, D], squared norms t_sq [nt]) lands among all rows of t ranked for query q[i] (fp32 [nq, D]) under
    focal_knn_search's distance and (d2, index) order (focal_rank_positive: two launches, no host read, no [nq, nt] tensor).  Returns
    before (int32 [nq], the rows ordering before the positive: its rank is before + 1) and tied (int32 [nq], the other rows at exactly the
    positive's distance); with want_d2 also pos_d2 (fp32 [nq]), the bits the search gives that pair.  A pos outside [0, nt) gives
    -1 / -1 / NaN.  The results do not depend on `slices` (None: knn_default_slices)."""
    _need_cuda(q, t, t_sq, pos)
    if q.dtype != torch.float32 or t.dtype != torch.float32 or t_sq.dtype != torch.float32 or q.dim() != 2 or t.dim() != 2:
        raise _lib.FocalHipError("rank_positive: q, t and t_sq are fp32, q and t matrices")
    nq, D = q.shape
    nt = t.shape[0]
    if t.shape[1] != D or t_sq.numel() != nt or pos.dtype != torch.int32 or pos.numel() != nq:
        raise _lib.FocalHipError(f"rank_positive: q {tuple(q.shape)} against t {tuple(t.shape)}, {t_sq.numel()} norms and "
                                 f"{pos.numel()} {pos.dtype} positives (need int32 [nq])")
    if not (q.is_contiguous() and t.is_contiguous() and t_sq.is_contiguous() and pos.is_contiguous()):
        raise _lib.FocalHipError("rank_positive: q, t, t_sq and pos must be contiguous")
    if nq >= 1 and nt >= 1 and D >= 4 and D % 4 == 0 and slices is None:
        slices = knn_default_slices(nq, nt, q.device)
    slices = 1 if slices is None else int(slices)
    rank_check_limits(D, nq, nt, slices)
    if q.data_ptr() % 16 or t.data_ptr() % 16:
        raise _lib.FocalHipError("rank_positive: q and t must be 16-byte aligned")
    d = _lib.RankDesc(nq, nt, D, slices)
    lib = _lib.load()
    before = torch.empty(nq, dtype=torch.int32, device=q.device)
    tied = torch.empty(nq, dtype=torch.int32, device=q.device)
    pos_d2 = torch.empty(nq, dtype=torch.float32, device=q.device)
    ws_bytes = int(lib.focal_rank_workspace(C.byref(d)))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=q.device)
    check(lib.focal_rank_positive(C.byref(d), _p(q), _p(t), _p(t_sq), _p(pos), _p(before), _p(tied), _p(pos_d2), _p(ws), ws_bytes,
                                  _stream()))
    return (before, tied, pos_d2) if want_d2 else (before, tied)


_PAIR_WS = {}


def pair_sums_check_limits(D, nq, nt, G, slices, fn, scale, self_offset):
    """The limits of focal_pair_sums on the feature width, the row counts, the groups, the slices, the function and its scale, refused
    here with the library's own text (it refuses them too, before any launch).  Returns the function's code."""
    if D < 4 or D % 4:
        raise _lib.FocalHipError(f"pair_sums: need D >= 4 and D % 4 == 0 (got D={D})")
    if nq < 1 or nt < 1:
        raise _lib.FocalHipError(f"pair_sums: need nq >= 1 and nt >= 1 (got nq={nq} nt={nt})")
    if not 1 <= G <= _lib.PAIR_MAX_GROUPS:
        raise _lib.FocalHipError(f"pair_sums: need 1 <= G <= {_lib.PAIR_MAX_GROUPS} (got G={G})")
    if not 1 <= slices <= _lib.PAIR_MAX_SLICES:
        raise _lib.FocalHipError(f"pair_sums: need 1 <= slices <= {_lib.PAIR_MAX_SLICES} (got slices={slices})")
    code = _lib.PAIR_FNS.get(fn, fn if isinstance(fn, int) else -1)
    if code not in _lib.PAIR_FNS.values():
        raise _lib.FocalHipError(f"pair_sums: need fn in 0 .. 2 (sqdist, dist, gauss; got fn={fn})")
    if not (math.isfinite(scale) and scale >= 0):
        raise _lib.FocalHipError(f"pair_sums: need a finite scale >= 0 (got scale={scale:g})")
    if self_offset < -1:
        raise _lib.FocalHipError(f"pair_sums: need self_offset >= -1 (got self_offset={self_offset})")
    return code


def pair_sums(q, t, t_sq, group=None, G=1, fn="dist", scale=1.0, self_offset=None, slices=None):
    """S fp32 [nq, G]: S[i, g] = the sum over the rows j of t (fp32 [nt, D], squared norms t_sq [nt]) with group[j] == g of
    f(max(d2(q_i, t_j), 0)) under focal_knn_search's distance (focal_pair_sums: one or two launches, no host read, no [nq, nt] tensor).
    fn: "sqdist" (f = x), "dist" (sqrt x) or "gauss" (exp(-scale x)).  group: int32 [nt], ids outside [0, G) are not counted; None with
    G = 1 puts every row in group 0.  self_offset = o says that q[i] is t[o + i] and leaves that one candidate out (None: nothing).
    Equal arguments give equal bits; `slices` (None: knn_default_slices) fixes the order of the sums, so another value may differ in
    the last bits."""
    _need_cuda(q, t, t_sq, group)
    if q.dtype != torch.float32 or t.dtype != torch.float32 or t_sq.dtype != torch.float32 or q.dim() != 2 or t.dim() != 2:
        raise _lib.FocalHipError("pair_sums: q, t and t_sq are fp32, q and t matrices")
    nq, D = q.shape
    nt = t.shape[0]
    if t.shape[1] != D or t_sq.numel() != nt:
        raise _lib.FocalHipError(f"pair_sums: q {tuple(q.shape)} against t {tuple(t.shape)} and {t_sq.numel()} norms")
    if group is not None and (group.dtype != torch.int32 or group.numel() != nt):
        raise _lib.FocalHipError(f"pair_sums: {group.numel()} {group.dtype} group ids for {nt} rows (need int32 [nt])")
    if not (q.is_contiguous() and t.is_contiguous() and t_sq.is_contiguous() and (group is None or group.is_contiguous())):
        raise _lib.FocalHipError("pair_sums: q, t, t_sq and group must be contiguous")
    G = int(G)
    if group is None and G != 1:
        raise _lib.FocalHipError(f"pair_sums: G={G} groups need the group ids (group may be None for G = 1 only)")
    if nq >= 1 and nt >= 1 and slices is None:
        slices = knn_default_slices(nq, nt, q.device)
    slices = 1 if slices is None else int(slices)
    self_offset = -1 if self_offset is None else int(self_offset)
    code = pair_sums_check_limits(D, nq, nt, G, slices, fn, float(scale), self_offset)
    if q.data_ptr() % 16 or t.data_ptr() % 16:
        raise _lib.FocalHipError("pair_sums: q and t must be 16-byte aligned")
    d = _lib.PairSumDesc(nq, nt, D, G, slices, code, self_offset, float(scale))
    lib = _lib.load()
    need = int(lib.focal_pair_sums_workspace(C.byref(d)))
    if need == 0:
        raise _lib.FocalHipError(f"pair_sums: {lib.focal_last_error().decode()}")
    key = (q.device, torch.cuda.current_stream().cuda_stream)
    ws = _PAIR_WS.get(key)
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, dtype=torch.uint8, device=q.device)
        _PAIR_WS[key] = ws
    S = torch.empty(nq, G, dtype=torch.float32, device=q.device)
    check(lib.focal_pair_sums(C.byref(d), _p(q), _p(t), _p(t_sq), _p(group), _p(S), _p(ws), ws.numel(), _stream()))
    return S


def seq_rank_check_limits(D, n, L, slices, fn, margin):
    """The limits of focal_seq_rank on the feature width, the sequence length, the row count, the slices, the function and the margin,
    refused here with the library's own text (it refuses them too, before any launch).  Returns the function's code."""
    if D < 4 or D % 4:
        raise _lib.FocalHipError(f"seq_rank: need D >= 4 and D % 4 == 0 (got D={D})")
    if L not in _lib.SEQRANK_LENGTHS:
        raise _lib.FocalHipError(f"seq_rank: need L in {{2, 4, 8, 16}} (got L={L})")
    if n < 1 or n % L:
        raise _lib.FocalHipError(f"seq_rank: need n % L == 0 (got n={n} L={L})")
    if n // L < 2:
        raise _lib.FocalHipError(f"seq_rank: need S = n / L >= 2 sequences (got n={n} L={L})")
    if not 1 <= slices <= _lib.SEQRANK_MAX_SLICES:
        raise _lib.FocalHipError(f"seq_rank: need 1 <= slices <= {_lib.SEQRANK_MAX_SLICES} (got slices={slices})")
    if -(-n // _lib.KNN_QUERY_TILE) * slices >= 1 << 31:
        raise _lib.FocalHipError(f"seq_rank: n / {_lib.KNN_QUERY_TILE} * slices exceeds the launch grid (n={n} slices={slices})")
    code = _lib.SEQRANK_FNS.get(fn, fn if isinstance(fn, int) else -1)
    if code not in _lib.SEQRANK_FNS.values():
        raise _lib.FocalHipError(f"seq_rank: need fn in 0 .. 1 (sqdist, dist; got fn={fn})")
    if not math.isfinite(margin):
        raise _lib.FocalHipError(f"seq_rank: need a finite margin (got margin={margin:g})")
    return code


def seq_rank(z, z_sq, L, margin, fn="dist", slices=None):
    """The sequence ranking counts of z (fp32 [n, D], rows a L .. a L + L - 1 = sequence a, squared norms z_sq [n]) under
    focal_knn_search's distance (focal_seq_rank: two or three launches, no host read, no [n, n] and no [S, S] tensor).  Returns the dict
    intra_d2 (fp32 [n, L]), intra_sum, hinge_sum, inter_sum (fp32 [S]), before, viol (int32 [S]) of include/focal_hip.h.  fn: "sqdist"
    (f = x) or "dist" (sqrt x).  The integer counts do not depend on `slices` (None: knn_default_slices); it fixes the order of the float
    sums, so another value may differ in their last bits."""
    _need_cuda(z, z_sq)
    if z.dtype != torch.float32 or z_sq.dtype != torch.float32 or z.dim() != 2:
        raise _lib.FocalHipError("seq_rank: z and z_sq are fp32, z a matrix")
    n, D = z.shape
    if z_sq.numel() != n:
        raise _lib.FocalHipError(f"seq_rank: z {tuple(z.shape)} and {z_sq.numel()} norms")
    if not (z.is_contiguous() and z_sq.is_contiguous()):
        raise _lib.FocalHipError("seq_rank: z and z_sq must be contiguous")
    L = int(L)
    if n >= 1 and slices is None:
        slices = knn_default_slices(n, n, z.device)
    slices = 1 if slices is None else int(slices)
    code = seq_rank_check_limits(D, n, L, slices, fn, float(margin))
    if z.data_ptr() % 16:
        raise _lib.FocalHipError("seq_rank: z must be 16-byte aligned")
    d = _lib.SeqRankDesc(n, D, L, slices, code, float(margin))
    lib = _lib.load()
    need = int(lib.focal_seq_rank_workspace(C.byref(d)))
    if need == 0:
        raise _lib.FocalHipError(f"seq_rank: {lib.focal_last_error().decode()}")
    S = n // L
    out = {"intra_d2": torch.empty(n, L, dtype=torch.float32, device=z.device)}
    for name in ("intra_sum", "hinge_sum", "inter_sum"):
        out[name] = torch.empty(S, dtype=torch.float32, device=z.device)
    for name in ("before", "viol"):
        out[name] = torch.empty(S, dtype=torch.int32, device=z.device)
    ws = torch.empty(need, dtype=torch.uint8, device=z.device)
    check(lib.focal_seq_rank(C.byref(d), _p(z), _p(z_sq), _p(out["intra_d2"]), _p(out["intra_sum"]), _p(out["before"]), _p(out["viol"]),
                             _p(out["hinge_sum"]), _p(out["inter_sum"]), _p(ws), need, _stream()))
    return out


def kmeans_check_limits(D, K, R):
    """The limits of focal_kmeans_assign / focal_kmeans_update on the feature width, the clusters per restart and the restarts, refused
    here with the limit named (the library refuses them too, before any launch)."""
    if D < 4 or D % 4:
        raise _lib.FocalHipError(f"kmeans: need a feature width D >= 4 with D % 4 == 0 (got D={D})")
    if not 1 <= K <= _lib.KMEANS_MAX_K:
        raise _lib.FocalHipError(f"kmeans: need 1 <= K <= {_lib.KMEANS_MAX_K} (got K={K})")
    if R < 1 or R * K > _lib.KMEANS_MAX_CENTROIDS:
        raise _lib.FocalHipError(f"kmeans: need R >= 1 and R * K <= {_lib.KMEANS_MAX_CENTROIDS} (got R={R} K={K})")


def kmeans_default_slices(n, D, device):
    """Row slices of focal_kmeans_update: knn_default_slices' rule (about two workgroups per CU) with the update's 64-column chunks in the
    place of the query tiles, never more than there are 64-row blocks."""
    return knn_default_slices(-(-D // 64) * _lib.KNN_QUERY_TILE, n, device)


def _kmeans_args(who, x, c, c_sq, K):
    _need_cuda(x, c, c_sq)
    if x.dtype != torch.float32 or c.dtype != torch.float32 or c_sq.dtype != torch.float32 or x.dim() != 2 or c.dim() != 2:
        raise _lib.FocalHipError(f"{who}: x, c and c_sq are fp32, x and c matrices")
    if not (x.is_contiguous() and c.is_contiguous() and c_sq.is_contiguous()):
        raise _lib.FocalHipError(f"{who}: x, c and c_sq must be contiguous")
    n, D = x.shape
    K = int(K)
    if K < 1 or c.shape[0] % K or c.shape[1] != D or c_sq.numel() != c.shape[0]:
        raise _lib.FocalHipError(f"{who}: x {tuple(x.shape)} against c {tuple(c.shape)}, {c_sq.numel()} norms and K={K} "
                                 f"(need 1 <= K <= {_lib.KMEANS_MAX_K} and c [R * K, D])")
    R = c.shape[0] // K
    if n < 1:
        raise _lib.FocalHipError(f"{who}: need n >= 1 (got n={n})")
    kmeans_check_limits(D, K, R)
    return n, D, K, R


def kmeans_assign(x, c, c_sq, K, labels=None, min_d2=None, changed=None, want_min_d2=False):
    """labels[r, i] = the nearest of restart r's K centroids (c fp32 [R * K, D], squared norms c_sq) to row i of x (fp32 [n, D]) under
    focal_knn_search's distance, ordered by (d2, k) (focal_kmeans_assign: one launch, no host read).  labels (int32 [R, n]) is written in
    place when given; min_d2 (fp32 [R, n], or want_min_d2) receives the chosen distance; changed (int32 [R]) += the rows whose label
    differs from the one `labels` held on entry.  Returns labels, or (labels, min_d2) when min_d2 was asked for."""
    n, D, K, R = _kmeans_args("kmeans_assign", x, c, c_sq, K)
    _need_cuda(labels, min_d2, changed)
    if labels is None:
        labels = torch.full((R, n), -1, dtype=torch.int32, device=x.device)
    if min_d2 is None and want_min_d2:
        min_d2 = torch.empty(R, n, dtype=torch.float32, device=x.device)
    if labels.dtype != torch.int32 or labels.numel() != R * n or not labels.is_contiguous():
        raise _lib.FocalHipError(f"kmeans_assign: labels must be contiguous int32 [{R}, {n}]")
    if min_d2 is not None and (min_d2.dtype != torch.float32 or min_d2.numel() != R * n or not min_d2.is_contiguous()):
        raise _lib.FocalHipError(f"kmeans_assign: min_d2 must be contiguous fp32 [{R}, {n}]")
    if changed is not None and (changed.dtype != torch.int32 or changed.numel() != R or not changed.is_contiguous()):
        raise _lib.FocalHipError(f"kmeans_assign: changed must be contiguous int32 [{R}]")
    d = _lib.KMeansDesc(n, D, K, R, 1)
    check(_lib.load().focal_kmeans_assign(C.byref(d), _p(x), _p(c), _p(c_sq), _p(labels), _p(min_d2), _p(changed), _stream()))
    return labels if min_d2 is None else (labels, min_d2)


def kmeans_workspace(n, D, K, R, slices, device):
    """The workspace of kmeans_update for these sizes (uint8; reusable across calls)."""
    kmeans_check_limits(D, K, R)
    d = _lib.KMeansDesc(n, D, K, R, slices)
    return torch.empty(_lib.load().focal_kmeans_update_workspace(C.byref(d)), dtype=torch.uint8, device=device)


def kmeans_update(x, labels, c, c_sq, K, min_d2=None, counts=None, inertia=None, slices=None, workspace=None):
    """c[r * K + k] <- the mean of the rows of x labelled k in restart r, c_sq its squared norm, both IN PLACE; an empty cluster keeps
    its centroid, bits unchanged (focal_kmeans_update: two launches, no floating-point atomics, no host read).  Returns (counts int32
    [R, K], inertia fp32 [R] = the sums of min_d2's rows, or None without min_d2).  The results are bit-identical for equal arguments;
    they depend on `slices` (None: kmeans_default_slices), which fixes the order of the sums.  workspace: kmeans_workspace(...), so
    that repeated calls allocate nothing."""
    n, D, K, R = _kmeans_args("kmeans_update", x, c, c_sq, K)
    _need_cuda(labels, min_d2, counts, inertia, workspace)
    if labels.dtype != torch.int32 or labels.numel() != R * n or not labels.is_contiguous():
        raise _lib.FocalHipError(f"kmeans_update: labels must be contiguous int32 [{R}, {n}]")
    if min_d2 is not None and (min_d2.dtype != torch.float32 or min_d2.numel() != R * n or not min_d2.is_contiguous()):
        raise _lib.FocalHipError(f"kmeans_update: min_d2 must be contiguous fp32 [{R}, {n}]")
    slices = kmeans_default_slices(n, D, x.device) if slices is None else int(slices)
    if not 1 <= slices <= 65535:
        raise _lib.FocalHipError(f"kmeans_update: need 1 <= slices <= 65535 (got {slices})")
    if counts is None:
        counts = torch.empty(R, K, dtype=torch.int32, device=x.device)
    if inertia is None and min_d2 is not None:
        inertia = torch.empty(R, dtype=torch.float32, device=x.device)
    if counts.dtype != torch.int32 or counts.numel() != R * K or not counts.is_contiguous():
        raise _lib.FocalHipError(f"kmeans_update: counts must be contiguous int32 [{R}, {K}]")
    if inertia is not None and (min_d2 is None or inertia.dtype != torch.float32 or inertia.numel() != R or not inertia.is_contiguous()):
        raise _lib.FocalHipError(f"kmeans_update: inertia must be contiguous fp32 [{R}] and needs min_d2")
    if workspace is None:
        workspace = kmeans_workspace(n, D, K, R, slices, x.device)
    d = _lib.KMeansDesc(n, D, K, R, slices)
    check(_lib.load().focal_kmeans_update(C.byref(d), _p(x), _p(labels), _p(min_d2), _p(c), _p(c_sq), _p(counts), _p(inertia), _p(workspace),
                                          workspace.numel() * workspace.element_size(), _stream()))
    return counts, inertia


def probe_check_limits(D, C_, R):
    """The limits of focal_probe_forward / focal_probe_grad on the feature width, the classes per problem and the problems, refused here
    with the limit named (the library refuses them too, before any launch)."""
    if D < 4 or D % 4:
        raise _lib.FocalHipError(f"probe: need a feature width D >= 4 with D % 4 == 0 (got D={D})")
    if not 2 <= C_ <= _lib.PROBE_MAX_C:
        raise _lib.FocalHipError(f"probe: need 2 <= C <= {_lib.PROBE_MAX_C} (got C={C_})")
    if R < 1 or R * C_ > _lib.PROBE_MAX_ROWS:
        raise _lib.FocalHipError(f"probe: need R >= 1 and R * C <= {_lib.PROBE_MAX_ROWS} (got R={R} C={C_})")


def probe_default_slices(n, D, device):
    """Row slices of focal_probe_grad: kmeans_default_slices' rule (about two workgroups per CU over the 64-column chunks of D), never
    more than there are 64-row blocks."""
    return kmeans_default_slices(n, D, device)


def _probe_args(who, x, w, b, num_classes):
    _need_cuda(x, w, b)
    if x.dtype != torch.float32 or w.dtype != torch.float32 or b.dtype != torch.float32 or x.dim() != 2 or w.dim() != 2:
        raise _lib.FocalHipError(f"{who}: x, w and b are fp32, x and w matrices")
    if not (x.is_contiguous() and w.is_contiguous() and b.is_contiguous()):
        raise _lib.FocalHipError(f"{who}: x, w and b must be contiguous")
    n, D = x.shape
    Cn = int(num_classes)
    if Cn < 1 or w.shape[0] % Cn or w.shape[1] != D or b.numel() != w.shape[0]:
        raise _lib.FocalHipError(f"{who}: x {tuple(x.shape)} against w {tuple(w.shape)}, {b.numel()} biases and C={Cn} "
                                 f"(need 2 <= C <= {_lib.PROBE_MAX_C} and w [R * C, D])")
    R = w.shape[0] // Cn
    if n < 1:
        raise _lib.FocalHipError(f"{who}: need n >= 1 (got n={n})")
    probe_check_limits(D, Cn, R)
    return n, D, Cn, R


def probe_forward(x, w, b, num_classes, y=None, ce=None, g=None, preds=None, want_ce=False, want_g=False, want_preds=False,
                  check_labels=True):
    """The softmax pass of R problems (w fp32 [R * C, D], b fp32 [R * C]) over x (fp32 [n, D]) with labels y (int32 [n])
    (focal_probe_forward: one launch).  Returns (ce fp32 [R, n], g fp32 [n, R * C] = softmax - onehot, preds int32 [R, n]), each None
    unless given or asked for with want_*; a predict-only call needs no y.  check_labels refuses a label outside [0, C) before the
    launch -- the pass's one host read: a caller that has checked its labels once (or captures the call) passes False."""
    n, D, Cn, R = _probe_args("probe_forward", x, w, b, num_classes)
    _need_cuda(y, ce, g, preds)
    if ce is None and want_ce:
        ce = torch.empty(R, n, dtype=torch.float32, device=x.device)
    if g is None and want_g:
        g = torch.empty(n, R * Cn, dtype=torch.float32, device=x.device)
    if preds is None and want_preds:
        preds = torch.empty(R, n, dtype=torch.int32, device=x.device)
    if ce is None and g is None and preds is None:
        raise _lib.FocalHipError("probe_forward: no output asked for (ce, g or preds)")
    if ce is not None or g is not None:
        if y is None or y.dtype != torch.int32 or y.numel() != n or not y.is_contiguous():
            raise _lib.FocalHipError(f"probe_forward: ce and g need the labels y, contiguous int32 [{n}]")
        if check_labels:
            low, high = (int(v) for v in torch.stack([y.min(), y.max()]).cpu())
            if low < 0 or high >= Cn:
                raise _lib.FocalHipError(f"probe_forward: labels must lie in [0, {Cn}) (got {low} .. {high})")
    else:
        y = None
    if ce is not None and (ce.dtype != torch.float32 or ce.numel() != R * n or not ce.is_contiguous()):
        raise _lib.FocalHipError(f"probe_forward: ce must be contiguous fp32 [{R}, {n}]")
    if g is not None and (g.dtype != torch.float32 or g.numel() != n * R * Cn or not g.is_contiguous()):
        raise _lib.FocalHipError(f"probe_forward: g must be contiguous fp32 [{n}, {R * Cn}]")
    if preds is not None and (preds.dtype != torch.int32 or preds.numel() != R * n or not preds.is_contiguous()):
        raise _lib.FocalHipError(f"probe_forward: preds must be contiguous int32 [{R}, {n}]")
    d = _lib.ProbeDesc(n, D, Cn, R, 1)
    check(_lib.load().focal_probe_forward(C.byref(d), _p(x), _p(w), _p(b), _p(y), _p(ce), _p(g), _p(preds), _stream()))
    return ce, g, preds


def probe_workspace(n, D, num_classes, R, slices, device):
    """The workspace of probe_grad for these sizes (uint8; reusable across calls)."""
    probe_check_limits(D, num_classes, R)
    d = _lib.ProbeDesc(n, D, num_classes, R, slices)
    return torch.empty(_lib.load().focal_probe_grad_workspace(C.byref(d)), dtype=torch.uint8, device=device)


def probe_grad(x, g, ce, w, lam, num_classes, gw=None, gb=None, f=None, slices=None, workspace=None):
    """gw [R * C, D] = g^T x / n + lam_r W_r, gb [R * C] = the column means of g, f fp64 [R] = mean(ce_r) + lam_r / 2 |W_r|^2, from
    probe_forward's g (fp32 [n, R * C]) and ce (fp32 [R, n]) (focal_probe_grad: two launches, no floating-point atomics, no host read).
    lam: fp32 [R].  Returns (f, gw, gb), written in place when given.  The results are bit-identical for equal arguments; gw and gb
    depend on `slices` (None: probe_default_slices), which fixes the order of the sums.  workspace: probe_workspace(...), so that
    repeated calls allocate nothing."""
    _need_cuda(x, g, ce, w, lam, gw, gb, f, workspace)
    if any(t.dtype != torch.float32 for t in (x, g, ce, w, lam)) or x.dim() != 2 or w.dim() != 2:
        raise _lib.FocalHipError("probe_grad: x, g, ce, w and lam are fp32, x and w matrices")
    if not all(t.is_contiguous() for t in (x, g, ce, w, lam)):
        raise _lib.FocalHipError("probe_grad: x, g, ce, w and lam must be contiguous")
    n, D = x.shape
    Cn = int(num_classes)
    if Cn < 1 or w.shape[0] % Cn or w.shape[1] != D:
        raise _lib.FocalHipError(f"probe_grad: x {tuple(x.shape)} against w {tuple(w.shape)} and C={Cn} (need w [R * C, D])")
    R = w.shape[0] // Cn
    if n < 1:
        raise _lib.FocalHipError(f"probe_grad: need n >= 1 (got n={n})")
    probe_check_limits(D, Cn, R)
    if g.numel() != n * R * Cn or ce.numel() != R * n or lam.numel() != R:
        raise _lib.FocalHipError(f"probe_grad: need g [{n}, {R * Cn}], ce [{R}, {n}] and lam [{R}]")
    slices = probe_default_slices(n, D, x.device) if slices is None else int(slices)
    if not 1 <= slices <= 65535:
        raise _lib.FocalHipError(f"probe_grad: need 1 <= slices <= 65535 (got {slices})")
    if gw is None:
        gw = torch.empty(R * Cn, D, dtype=torch.float32, device=x.device)
    if gb is None:
        gb = torch.empty(R * Cn, dtype=torch.float32, device=x.device)
    if f is None:
        f = torch.empty(R, dtype=torch.float64, device=x.device)
    if gw.dtype != torch.float32 or gw.numel() != R * Cn * D or not gw.is_contiguous():
        raise _lib.FocalHipError(f"probe_grad: gw must be contiguous fp32 [{R * Cn}, {D}]")
    if gb.dtype != torch.float32 or gb.numel() != R * Cn or not gb.is_contiguous():
        raise _lib.FocalHipError(f"probe_grad: gb must be contiguous fp32 [{R * Cn}]")
    if f.dtype != torch.float64 or f.numel() != R or not f.is_contiguous():
        raise _lib.FocalHipError(f"probe_grad: f must be contiguous fp64 [{R}]")
    if workspace is None:
        workspace = probe_workspace(n, D, Cn, R, slices, x.device)
    d = _lib.ProbeDesc(n, D, Cn, R, slices)
    check(_lib.load().focal_probe_grad(C.byref(d), _p(x), _p(g), _p(ce), _p(w), _p(lam), _p(gw), _p(gb), _p(f), _p(workspace),
                                       workspace.numel() * workspace.element_size(), _stream()))
    return f, gw, gb


def tsne_check_limits(n, D, perplexity=None):
    """The limits of the focal_tsne_* exports on the row count, the feature width and the perplexity, refused here with the limit named
    (the library refuses them too, before any launch)."""
    if D < 4 or D % 4:
        raise _lib.FocalHipError(f"tsne: need a feature width D >= 4 with D % 4 == 0 (got D={D})")
    if not 2 <= n <= _lib.TSNE_MAX_N:
        raise _lib.FocalHipError(f"tsne: need 2 <= n <= {_lib.TSNE_MAX_N} (got n={n}): a row of the distance matrix is held in LDS")
    if perplexity is not None and not 1 <= float(perplexity) < n:
        raise _lib.FocalHipError(f"tsne: need 1 <= perplexity < n (got perplexity={perplexity} n={n})")


def tsne_default_slices(n, device):
    """Column slices of focal_tsne_grad: knn_default_slices' rule (about two workgroups per CU) over the gradient's 32-row tiles, never
    more than there are 2048-column chunks."""
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    row_tiles = -(-n // _lib.TSNE_ROW_TILE)
    return max(1, min(-(-n // _lib.TSNE_COL_CHUNK), round(2 * cus / row_tiles)))


def _tsne_x(who, x):
    _need_cuda(x)
    if x.dtype != torch.float32 or x.dim() != 2:
        raise _lib.FocalHipError(f"{who}: x is an fp32 matrix [n, D]")
    return x.shape


def tsne_dist(x, want_norms=False):
    """d2 fp32 [n, n] of the rows of x (fp32 [n, D]) under focal_knn_search's distance, diagonal +0 (focal_tsne_dist: two launches).
    want_norms: also x_sq [n], the squared norms the kernel used -- handed to knn_search_vote as t_sq, its nbr_d2 are these bits."""
    n, D = _tsne_x("tsne_dist", x)
    tsne_check_limits(n, D)
    d2 = torch.empty(n, n, dtype=torch.float32, device=x.device)
    x_sq = torch.empty(n, dtype=torch.float32, device=x.device)
    d = _lib.TsneDesc(n, D, 1)
    check(_lib.load().focal_tsne_dist(C.byref(d), _p(x), _p(x_sq), _p(d2), _stream()))
    return (d2, x_sq) if want_norms else d2


def tsne_affinities(x, perplexity, want_conditional=False):
    """The joint probabilities of exact t-SNE for the rows of x (fp32 [n, D]): distances, 64 bisection steps per row on beta, and the
    symmetrisation, in ONE [n, n] buffer (focal_tsne_dist + focal_tsne_perplexity + focal_tsne_symmetrize; no host read).  Returns
    (P fp32 [n, n], bitwise symmetric with a zero diagonal; beta fp32 [n]; p_log_p fp64 [1] = sum P log P), and with want_conditional
    a copy of the conditional matrix p_j|i as a fourth value."""
    n, D = _tsne_x("tsne_affinities", x)
    tsne_check_limits(n, D, perplexity)
    lib = _lib.load()
    d = _lib.TsneDesc(n, D, 1)
    P = torch.empty(n, n, dtype=torch.float32, device=x.device)
    beta = torch.empty(n, dtype=torch.float32, device=x.device)
    check(lib.focal_tsne_dist(C.byref(d), _p(x), _p(beta), _p(P), _stream()))  # (beta holds the norms until the bisection writes it)
    check(lib.focal_tsne_perplexity(C.byref(d), float(perplexity), _p(P), _p(beta), _stream()))
    cond = P.clone() if want_conditional else None
    ws = torch.empty(lib.focal_tsne_symmetrize_workspace(C.byref(d)), dtype=torch.uint8, device=x.device)
    p_log_p = torch.empty(1, dtype=torch.float64, device=x.device)
    check(lib.focal_tsne_symmetrize(C.byref(d), _p(P), _p(p_log_p), _p(ws), ws.numel(), _stream()))
    return (P, beta, p_log_p, cond) if want_conditional else (P, beta, p_log_p)


def tsne_workspace(n, slices, device):
    """The workspace of tsne_grad_step for these sizes (uint8; reusable across calls)."""
    d = _lib.TsneDesc(n, 4, slices)
    return torch.empty(_lib.load().focal_tsne_grad_workspace(C.byref(d)), dtype=torch.uint8, device=device)


def tsne_record(entries, device):
    """A zeroed device record for tsne_grad_step with room for `entries` KL entries: fp64 [2 + 3 * entries] = {iterations, entries
    written, (iteration, KL, gradient norm) ...}."""
    return torch.zeros(2 + 3 * int(entries), dtype=torch.float64, device=device)


def tsne_read_record(record):
    """The record's one host read: (iterations, float64 tensor [entries, 3] of (iteration, KL, gradient norm))."""
    host = record.cpu()
    k = min(int(host[1].item()), (host.numel() - 2) // 3)
    return int(host[0].item()), host[2:2 + 3 * k].view(k, 3)


def tsne_grad_step(y, P, p_log_p, upd, gains, lr, momentum, exaggeration, record=None, want_kl=False, slices=None, workspace=None):
    """One descent iteration of exact t-SNE, IN PLACE on y, upd and gains (each fp32 [n, 2]): the gradient of KL(e P || Q) from one read
    of P (fp32 [n, n]) and sklearn's gains / momentum update (focal_tsne_grad + focal_tsne_step: two launches, no floating-point
    atomics, no host read).  record (tsne_record) counts the call; with want_kl the entry (iteration, KL, |g|_2) is appended to it, KL =
    p_log_p - sum P log q + log Z being the divergence at exaggeration 1 only.  The results are bit-identical for equal arguments;
    they depend on `slices` (None: tsne_default_slices), which fixes the order of the sums.  workspace: tsne_workspace(...), so that
    repeated calls allocate nothing."""
    _need_cuda(y, P, p_log_p, upd, gains, record, workspace)
    n = y.shape[0]
    if any(t.dtype != torch.float32 or tuple(t.shape) != (n, 2) for t in (y, upd, gains)):
        raise _lib.FocalHipError(f"tsne_grad_step: y, upd and gains are fp32 [{n}, 2]")
    if P.dtype != torch.float32 or tuple(P.shape) != (n, n):
        raise _lib.FocalHipError(f"tsne_grad_step: P must be fp32 [{n}, {n}]")
    tsne_check_limits(n, 4)
    slices = tsne_default_slices(n, y.device) if slices is None else int(slices)
    if not 1 <= slices <= 65535:
        raise _lib.FocalHipError(f"tsne_grad_step: need 1 <= slices <= 65535 (got {slices})")
    cap = 0
    if record is not None:
        if record.dtype != torch.float64 or record.dim() != 1 or record.numel() < 2 or (record.numel() - 2) % 3:
            raise _lib.FocalHipError("tsne_grad_step: record must be fp64 [2 + 3 * entries] (tsne_record)")
        cap = (record.numel() - 2) // 3
    if want_kl and (cap < 1 or p_log_p is None or p_log_p.dtype != torch.float64 or p_log_p.numel() != 1):
        raise _lib.FocalHipError("tsne_grad_step: want_kl needs p_log_p fp64 [1] and a record with room for an entry")
    if workspace is None:
        workspace = tsne_workspace(n, slices, y.device)
    d = _lib.TsneDesc(n, 4, slices)
    lib = _lib.load()
    ws_bytes = workspace.numel() * workspace.element_size()
    check(lib.focal_tsne_grad(C.byref(d), _p(y), _p(P), int(bool(want_kl)), _p(workspace), ws_bytes, _stream()))
    check(lib.focal_tsne_step(C.byref(d), _p(workspace), ws_bytes, _p(p_log_p), _p(y), _p(upd), _p(gains), float(lr), float(momentum),
                              float(exaggeration), int(bool(want_kl)), _p(record), cap, _stream()))
    return y


def mean_time(x, B, T, D):
    y = torch.empty(B, D, dtype=torch.float32, device=x.device)
    check(_lib.load().focal_mean_time(B, T, D, _p(x), _p(y), _stream()))
    return y


def dropout(x, rng, stream_id, p):
    y = torch.empty_like(x)
    check(_lib.load().focal_dropout(x.numel(), _p(x), _p(y), _p(rng), stream_id, p, _stream()))
    return y


def mul_(y, a):
    """y *= a (fp32, element-wise; focal_mul)."""
    _need_cuda(y, a)
    check(_lib.load().focal_mul(y.numel(), _p(a), _p(y), _stream()))
    return y


def axpy(a, x, y):
    check(_lib.load().focal_axpy(x.numel(), a, _p(x), _p(y), _stream()))
