"""Gradient clipping by global norm on the device: the norm pass (focal_grad_norm_multi), the clipped AdamW (focal_adamw_clip_multi /
_advance), the statistics record, capture and replay, the optimizer against torch's clip_grad_norm_ + AdamW on a model's own gradients, and
`train.py -clip_grad` end to end.

The record is written by the update, so the tests that look at the norm pass alone put a clipped update of a 4-element dummy parameter with
max_norm = inf behind it: it re-sums the partial row exactly as every update does and leaves the norm, its square and the coefficient
in the record.

Error bound of the norm (tests 2, 7).  The terms are squares, all non-negative, so every rounding of the summation is a relative one: a
term passes through one rounding of its square and at most L roundings of additions, L the longest addition chain, and the sum of
squares is off by at most (L + 1) * 2^-24 relative.  The chain of the kernels as built, from the exported constants:
    per lane, ONE accumulator over its trips of the grid-stride loop, 4 additions per trip (a float4);
        trips = sum over segments of ceil(n4 / (grid * 256)), grid = min(MAX_BLOCKS, ceil(sum n4 / 256)), n4 = n / 4
    6 levels across the 64 lanes of a wave, 3 additions across the 4 waves of the workgroup            (the norm pass)
    CLIP_SCRATCH_WORDS / 256 - 1 = 3 additions per lane over the partial row, 6 across the wave, 3 across the waves   (the update)
    L = 4 * trips + 21
The root halves the relative error and adds one rounding: |norm - norm64| <= ((L + 1) * 2^-25 + 2^-24) * norm64."""
import math
import os
import subprocess
import sys

import pytest
import torch

from conftest import make_args, no_dropout, record_observed

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
DEV = "cuda"
INF = math.inf


@pytest.fixture(scope="module")
def ops():
    from focal_amd import ops as o
    return o


def _lengths():
    from focal_amd import _lib
    big = 4 * 256 * _lib.MAX_BLOCKS + 4  # one lane makes a second trip of the grid-stride loop
    return [(big,), (1028,), (1020,), (4,), (8, 0, 12)]  # the largest first, the smallest behind it on the same scratch


def chain(lens):
    """L of the module docstring for segments of these lengths."""
    from focal_amd import _lib
    n4 = [n // 4 for n in lens]
    grid = min(_lib.MAX_BLOCKS, max(1, -(-sum(n4) // 256)))
    trips = sum(-(-k // (grid * 256)) for k in n4)
    return 4 * trips + 6 + 3 + (_lib.CLIP_SCRATCH_WORDS // 256 - 1) + 6 + 3


def norm_bound(lens):
    return (chain(lens) + 1) * 2.0 ** -25 + 2.0 ** -24


class Dummy:
    """A 4-element parameter whose clipped update (lr = 0) turns the partial row into the record."""

    def __init__(self, ops):
        self.ops = ops
        self.t = [torch.zeros(4, device=DEV) for _ in range(4)]
        self.lr = torch.zeros(1, device=DEV)
        self.state = ops.new_step_state(DEV, count=1)

    def norm(self, segs, st):
        self.ops.grad_norm(segs, st)
        self.ops.adamw_multi([(*self.t, None)], self.lr, self.state, clip=(st, INF))
        return self.ops.read_clip_stats(st)


def _bits(x):
    return torch.tensor(x, dtype=torch.float32).view(torch.int32).item()


def test_norm_of_ones_is_exact_and_small_grids_read_no_stale_partials(ops):
    from focal_amd import _lib
    st, dummy = ops.new_clip_state(DEV), Dummy(ops)
    for lens in _lengths():
        segs = [torch.ones(n, device=DEV) for n in lens]
        s = dummy.norm(segs, st)
        n = sum(lens)
        grid = min(_lib.MAX_BLOCKS, -(-(n // 4) // 256))
        assert s["last_sq"] == float(n) and s["steps"] == 1 and s["skipped"] == 0 and s["clipped"] == 0 and s["last_coef"] == 1.0, (lens, s)
        assert s["last_norm"] == torch.tensor(float(n)).sqrt().item()
        row = st[0].cpu()
        assert row.numel() == _lib.CLIP_SCRATCH_WORDS and row[grid:].abs().sum().item() == 0.0 and row[:grid].min().item() > 0.0, lens
        assert row.double().sum().item() == float(n)


@pytest.mark.parametrize("largest", ["last", "first"])
def test_norm_against_float64(ops, largest):
    """Normal data scaled per element over 1e-4 .. 1e3, the largest element at one end: within the bound of the module docstring."""
    st, dummy = ops.new_clip_state(DEV), Dummy(ops)
    gen = torch.Generator(device=DEV).manual_seed(1234)
    for lens in _lengths():
        n = sum(lens)
        flat = torch.randn(n, device=DEV, generator=gen) * 10.0 ** (torch.rand(n, device=DEV, generator=gen) * 7.0 - 4.0)
        i, j = int(flat.abs().argmax()), (n - 1 if largest == "last" else 0)
        a, b = flat[i].item(), flat[j].item()
        flat[i], flat[j] = b, a
        segs = [t.clone() for t in flat.split(list(lens))]
        s = dummy.norm(segs, st)
        ref = flat.double().norm().item()
        err = abs(s["last_norm"] - ref) / ref
        record_observed(f"clip_grad.norm_rel_err.largest_{largest}.n{n}", err)
        record_observed(f"clip_grad.norm_rel_bound.n{n}", norm_bound(lens))
        assert err <= norm_bound(lens), (lens, err, norm_bound(lens))


def test_norm_is_bit_repeatable(ops):
    st, dummy = ops.new_clip_state(DEV), Dummy(ops)
    gen = torch.Generator(device=DEV).manual_seed(5)
    for lens in _lengths()[:2] + [(4096 + 8, 1028)]:
        segs = [torch.randn(n, device=DEV, generator=gen) for n in lens]
        a = dummy.norm(segs, st)
        row_a = st[0].clone()
        st[0].fill_(7.0)  # (whatever the row held: every word is rewritten)
        b = dummy.norm(segs, st)
        assert torch.equal(row_a.view(torch.int32), st[0].view(torch.int32)), lens
        assert _bits(a["last_norm"]) == _bits(b["last_norm"]) and _bits(a["last_sq"]) == _bits(b["last_sq"])


LENS = (4096 + 8, 1028)


def _problem(shadow, seed=11, count=3):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    r = lambda n: torch.randn(n, device=DEV, generator=gen)
    segs = [(r(n), r(n), 0.1 * r(n), 0.01 * r(n).square(), torch.zeros(n, dtype=torch.bfloat16, device=DEV) if shadow else None) for n in LENS]
    return {"segs": segs, "lr": torch.full((1,), 1e-3, device=DEV), "step": None, "count": count, "seed": None}


def _clone(pr, ops, grads=None):
    segs = [tuple(None if t is None else t.clone() for t in s) for s in pr["segs"]]
    if grads is not None:
        segs = [(s[0], g, s[2], s[3], s[4]) for s, g in zip(segs, grads)]
    return {"segs": segs, "lr": pr["lr"], "step": ops.new_step_state(DEV, count=pr["count"]), "seed": ops.new_rng_state(99, DEV)}


def _update(ops, q, l2, advance, clip=None):
    ops.adamw_multi(q["segs"], q["lr"], q["step"], weight_decay=0.05, l2_decay=l2, advance=advance, seed_state=q["seed"] if advance else None, clip=clip)


def _same(a, b):
    for sa, sb in zip(a["segs"], b["segs"]):
        for i in (0, 2, 3, 4):
            if sa[i] is not None and not torch.equal(sa[i], sb[i]):
                return False
    return torch.equal(a["step"], b["step"]) and torch.equal(a["seed"], b["seed"])


def _norm64(grads):
    return torch.cat([g.double() for g in grads]).norm().item()


@pytest.mark.parametrize("advance", [False, True])
@pytest.mark.parametrize("shadow", [False, True])
@pytest.mark.parametrize("l2", [False, True])
def test_clipped_update_equals_plain_update_on_prescaled_gradients(ops, l2, shadow, advance):
    pr = _problem(shadow)
    grads = [s[1] for s in pr["segs"]]
    max_norm = 0.5 * _norm64(grads)
    st = ops.new_clip_state(DEV)
    a = _clone(pr, ops)
    ops.grad_norm(grads, st)
    _update(ops, a, l2, advance, clip=(st, max_norm))
    s = ops.read_clip_stats(st)
    assert 0.4 < s["last_coef"] < 0.6 and s["clipped"] == 1, s
    coef = torch.tensor(s["last_coef"], dtype=torch.float32, device=DEV)
    b = _clone(pr, ops, grads=[g * coef for g in grads])
    _update(ops, b, l2, advance)
    assert _same(a, b)
    assert int(a["step"][1]) == pr["count"] + (1 if advance else 0) and int(a["step"][2:].abs().sum()) == 0
    if shadow:
        assert all(torch.equal(sg[4], sg[0].bfloat16()) for sg in a["segs"])
    moved = _clone(pr, ops)
    assert not torch.equal(a["segs"][0][0], moved["segs"][0][0])


@pytest.mark.parametrize("advance", [False, True])
@pytest.mark.parametrize("l2", [False, True])
def test_below_the_threshold_the_step_is_the_plain_step(ops, l2, advance):
    pr = _problem(True)
    grads = [s[1] for s in pr["segs"]]
    plain = _clone(pr, ops)
    _update(ops, plain, l2, advance)
    st = ops.new_clip_state(DEV)
    for max_norm in (2.0 * _norm64(grads), INF):
        a = _clone(pr, ops)
        ops.grad_norm(grads, st)
        _update(ops, a, l2, advance, clip=(st, max_norm))
        s = ops.read_clip_stats(st)
        assert s["last_coef"] == 1.0 and s["clipped"] == 0 and s["steps"] == 1
        assert _same(a, plain), max_norm


def test_coefficient(ops):
    """coef = max_norm / (norm + 1e-6) in fp32, against the same expression in float64 on the float64 norm of the gradients: 2^-22."""
    pr = _problem(False)
    grads = [s[1] for s in pr["segs"]]
    n64 = _norm64(grads)
    st = ops.new_clip_state(DEV)
    for frac in (0.5, 0.9, 0.1, 1e-3):
        max_norm = frac * n64
        a = _clone(pr, ops)
        ops.grad_norm(grads, st)
        _update(ops, a, False, False, clip=(st, max_norm))
        s = ops.read_clip_stats(st)
        want = float(torch.tensor(max_norm, dtype=torch.float32)) / (n64 + 1e-6)  # (the bound travels as fp32)
        err = abs(s["last_coef"] - want) / want
        record_observed(f"clip_grad.coef_rel_err.frac{frac:g}", err)
        assert err <= 2.0 ** -22, (frac, err)


def test_record_counts_and_a_nan_gradient_skips_the_step(ops):
    pr = _problem(True, count=0)
    base = [s[1] for s in pr["segs"]]
    n64 = _norm64(base)
    max_norm = 0.5 * n64
    q, st = _clone(pr, ops), ops.new_clip_state(DEV)
    norms = []
    for call, scale in enumerate((1.0, 0.25, 2.0, float("nan"), 3.0)):
        grads = [g * scale for g in base]
        if scale != scale:
            grads = [g.clone() for g in base]
            grads[1][17] = float("nan")
        else:
            norms.append(_norm64(grads))
        q["segs"] = [(s[0], g, s[2], s[3], s[4]) for s, g in zip(q["segs"], grads)]
        before = {"segs": [tuple(None if t is None else t.clone() for t in s) for s in q["segs"]], "step": q["step"].clone(), "seed": q["seed"].clone()}
        ops.grad_norm(grads, st)
        _update(ops, q, False, True, clip=(st, max_norm))
        if scale != scale:
            for sa, sb in zip(q["segs"], before["segs"]):
                assert all(torch.equal(sa[i], sb[i]) for i in (0, 2, 3, 4))
            assert torch.equal(q["step"], before["step"])
            assert int(q["seed"][1]) == int(before["seed"][1]) + 1 and int(q["seed"][0]) != int(before["seed"][0])
        else:
            assert not torch.equal(q["segs"][0][0], before["segs"][0][0])
            assert int(q["step"][1]) == int(before["step"][1]) + 1 and int(q["seed"][1]) == int(before["seed"][1]) + 1
    assert int(q["step"][1]) == 4 and int(q["seed"][1]) == 5 and int(q["step"][2:].abs().sum()) == 0
    assert torch.isfinite(q["segs"][0][0]).all() and torch.isfinite(q["segs"][1][0]).all()
    s = ops.read_clip_stats(st)
    assert (s["steps"], s["clipped"], s["skipped"]) == (5, 3, 1), s
    bnd = norm_bound(LENS)
    assert abs(s["norm_sum"] - sum(norms)) <= (bnd + 4 * 2.0 ** -24) * sum(norms)   # (four fp32 additions of the record on top)
    assert abs(s["norm_max"] - max(norms)) <= bnd * max(norms) and abs(s["last_norm"] - norms[-1]) <= bnd * norms[-1]
    assert abs(s["norm_mean"] - sum(norms) / 4) <= (bnd + 5 * 2.0 ** -24) * sum(norms) / 4
    z = ops.read_clip_stats(st)
    assert (z["steps"], z["clipped"], z["skipped"], z["norm_sum"], z["norm_max"], z["last_norm"]) == (0, 0, 0, 0.0, 0.0, 0.0)


def test_capture_and_replay(ops):
    """The norm pass and the clipped update in ONE graph: three replays with new gradients in the same buffers equal three eager calls."""
    pr = _problem(True, count=0)
    base = [s[1] for s in pr["segs"]]
    gen = torch.Generator(device=DEV).manual_seed(77)
    sets = [base, [0.3 * g for g in base], [torch.randn(g.numel(), device=DEV, generator=gen) for g in base]]
    max_norm = 0.5 * _norm64(base)

    eager, st_e = _clone(pr, ops), ops.new_clip_state(DEV)
    for grads in sets:
        eager["segs"] = [(s[0], g, s[2], s[3], s[4]) for s, g in zip(eager["segs"], grads)]
        ops.grad_norm(grads, st_e)
        _update(ops, eager, False, True, clip=(st_e, max_norm))

    bufs = [torch.zeros_like(g) for g in base]
    rep, st_r = _clone(pr, ops, grads=bufs), ops.new_clip_state(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        ops.grad_norm(bufs, st_r)
        _update(ops, rep, False, True, clip=(st_r, max_norm))
    for grads in sets:
        for b, g in zip(bufs, grads):
            b.copy_(g)
        graph.replay()
    torch.cuda.synchronize()
    rep["segs"] = [(s[0], e[1], s[2], s[3], s[4]) for s, e in zip(rep["segs"], eager["segs"])]
    assert _same(rep, eager)
    assert int(rep["step"][1]) == 3 and int(rep["seed"][1]) == 3
    se, sr = ops.read_clip_stats(st_e), ops.read_clip_stats(st_r)
    assert se == sr and (sr["steps"], sr["clipped"], sr["skipped"]) == (3, 2, 0), (se, sr)


def _deepsense(cfg, ct, clip_grad):
    from models.DeepSense import DeepSense
    from models.FOCALModules import FOCAL
    from models.loss import FOCALLoss
    from oracle.weights import fill_state_dict_, synthetic_freq_input
    from train_utils.optimizer import define_optimizer
    args = make_args(no_dropout(cfg), "DeepSense", torch.device("cuda"), ct)
    args.clip_grad = True
    args.dataset_config["FOCAL"]["pretrain_optimizer"]["clip_grad"] = clip_grad
    net = DeepSense(args)
    fill_state_dict_(net.state_dict())
    net = net.to("cuda")
    focal = FOCAL(args, net)
    to = lambda d: {l: {m: v.cuda() for m, v in mm.items()} for l, mm in d.items()}
    x = to(synthetic_freq_input(cfg, 8, seed=101)), to(synthetic_freq_input(cfg, 8, seed=202))
    return args, net, focal, FOCALLoss(args), define_optimizer(args, focal.parameters()), x


@pytest.mark.parametrize("ct", ["fp32", "bf16"])
def test_clipped_optimizer_equals_torch_clip_and_adamw_on_the_same_gradients(cfg, ct):
    """tests/test_swt_parity_gpu.py::test_adamw_updates_equal_torch_adamw_on_the_same_gradients with clipping on: DeepSense on MOD, B = 8,
    three steps, max_norm = half the first step's norm (read through a first run with max_norm = inf); the reference is clip_grad_norm_ +
    torch.optim.AdamW on a clone of the arena fed the HIP path's own gradients; masters within 1e-6, the shadow their bf16 rounding."""
    args, net, focal, loss_fn, opt, (x1, x2) = _deepsense(cfg, ct, INF)
    net.train()
    opt.zero_grad()
    a, b = focal(x1, x2, proj_head=True)
    loss_fn(a, b).backward()
    opt.step()
    first = opt.clip_stats()
    assert (first["steps"], first["clipped"], first["skipped"]) == (1, 0, 0) and first["last_norm"] > 0.0
    max_norm = 0.5 * first["last_norm"]

    args, net, focal, loss_fn, opt, (x1, x2) = _deepsense(cfg, ct, max_norm)
    net.train()
    assert opt.max_grad_norm == max_norm
    ref_p, ref_opt = None, None
    oc = cfg["FOCAL"]["pretrain_optimizer"]
    for it in range(3):
        opt.zero_grad()
        a, b = focal(x1, x2, proj_head=True)
        loss_fn(a, b).backward()
        torch.cuda.synchronize()
        ar = net.arena()
        if ref_p is None:
            ref_p = torch.nn.Parameter(ar.flat.detach().clone())
            ref_opt = torch.optim.AdamW([ref_p], lr=oc["start_lr"], weight_decay=oc["weight_decay"])
        ref_p.grad = ar.grad.detach().clone()
        opt.step()
        torch.nn.utils.clip_grad_norm_([ref_p], max_norm)
        ref_opt.step()
        torch.cuda.synchronize()
        err = (ar.flat - ref_p.detach()).abs().max().item()
        record_observed(f"clip_grad.deepsense_vs_torch_clip_adamw.{ct}.step{it}.max_abs", err)
        assert err < 1e-6, (it, err)
        if ct == "bf16":
            assert torch.equal(ar.shadow, ar.flat.bfloat16())
    s = opt.clip_stats()
    assert s["steps"] == 3 and s["clipped"] >= 1 and s["skipped"] == 0, s


def test_captured_pretraining_step_replays_with_clipping_on(cfg):
    """CapturedTrainStep (what `train.py -learn_framework=FOCAL -clip_grad` runs): the norm pass and the clipped update are captured with
    the rest of the step; every step, eager or replayed, lands in the record, and the record survives its per-epoch read."""
    from focal_amd.graph_step import CapturedTrainStep
    args, net, focal, loss_fn, opt, (x1, x2) = _deepsense(cfg, "bf16", 5.0)
    net.train()
    step = CapturedTrainStep(focal, loss_fn, opt)
    losses = [step(x1, x2).item() for _ in range(5)]
    assert step.replays >= 2 and step.eager_steps + step.replays == 5, (step.replays, step.eager_steps)
    s = opt.clip_stats()
    assert s["steps"] == 5 and s["skipped"] == 0 and s["norm_max"] >= s["norm_mean"] > 0.0, s
    assert all(l == l for l in losses) and torch.isfinite(net.arena().flat).all()
    assert int(opt._step_state[1]) == 5
    step(x1, x2).item()
    s = opt.clip_stats()
    assert s["steps"] == 1 and int(opt._step_state[1]) == 6, s


def _train_py(*extra):
    src = os.path.join(ROOT, "focal_amd", "src")
    r = subprocess.run([sys.executable, os.path.join(src, "train.py"), "-model=DeepSense", "-dataset=MOD", "-learn_framework=no", *extra,
                        "-epochs=1", "-synthetic_batches=4"], capture_output=True, text=True, timeout=600, cwd=src)
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-3000:]
    return log


def test_train_py_logs_the_gradient_norm_only_with_the_switch():
    import re
    log = _train_py("-clip_grad")
    m = re.search(r"epoch 0: gradient norm mean (\S+), max (\S+); (\d+) of (\d+) steps clipped, (\d+) skipped \(max_norm 5\)", log)
    assert m, log[-3000:]
    assert float(m.group(1)) > 0.0 and float(m.group(2)) >= float(m.group(1)) and int(m.group(4)) == 4 and int(m.group(5)) == 0
    r = re.search(r"epoch 0: (\d+) graph replays", log)
    assert r and int(r.group(1)) >= 1, log[-3000:]
    assert "gradient norm" not in _train_py()
