"""Multi-location DeepSense on the GPU (focal_amd/deepsense_engine.py: DeepSenseMultiLocEncoder; csrc/conv.hip: focal_conv_in_bwd_data,
focal_rows_mean): the two kernels against float64 with bounds derived from the fp32 unit roundoff, the in-conv at the second block's
shapes, the second-level stack against the torch modules, the FOCAL step on HAR3LOC against the reference fixture
(tests/golden/DeepSense_3loc_b8.npz, gen_golden_deepsense_multiloc.py), one pass against two, the captured step, train.py end to end,
and the single-location step's launches against the multiset recorded before the engine was split
(tests/golden/DeepSense_MOD_b8_launches.json).  Every observed error is recorded (conftest.record_observed)."""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import no_dropout, record_observed

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLD = os.path.join(ROOT, "tests", "golden")
DEV = "cuda"
U = 2.0 ** -24  # fp32 unit roundoff


def rnd(*shape, scale=1.0, seed=0, dtype=torch.float32):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV).to(dtype)


def rel_err(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


@pytest.fixture(scope="module")
def ops():
    from focal_amd import ops as o
    return o


def _traced(fn):
    """Kernel names the library launched inside fn()."""
    from focal_amd import _lib
    lib = _lib.load()
    torch.cuda.synchronize()
    _lib.check(lib.focal_trace_begin(8192, _lib.TRACE_DISPATCH))
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        lib.focal_trace_end()
    n = lib.focal_trace_count()
    recs = (_lib.TraceRecord * max(n, 1))()
    _lib.check(lib.focal_trace_read(0, n, recs))
    return out, [recs[i].kernel.decode() for i in range(n)]


# ---------------------------------------------------------------------------------------------- focal_conv_in_bwd_data
def _conv_in_bwd_data_ref(dz, w, tokens, S, k):
    """float64 autograd of F.conv2d(..., padding="same") on a one-channel [tokens, 1, 1, S] input; and the same with |dz|, |w|."""
    out = []
    for a, b in ((dz.double().cpu(), w.double().cpu()), (dz.double().cpu().abs(), w.double().cpu().abs())):
        x = torch.zeros(tokens, 1, 1, S, dtype=torch.float64, requires_grad=True)
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # (torch notes that an even 'same' filter needs a padded copy)
            y = F.conv2d(x, b, padding="same").permute(0, 2, 3, 1).reshape(-1, 64)
        (y * a).sum().backward()
        out.append(x.grad.reshape(tokens, S))
    return out


@pytest.mark.parametrize("zt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("tokens,S,k", [(1, 128, 4), (37, 128, 4), (160, 128, 4), (160, 128, 3), (160, 128, 5), (160, 128, 1), (37, 20, 4),
                                        (37, 3, 4)])
def test_conv_in_bwd_data_against_float64(ops, tokens, S, k, zt):
    """Bound per element: (64 k + 2) u scale sum_{c,t} |dz w| -- 64 k products summed in fp32 in any order (each rounding at most u = 2^-24
    of the running sum of magnitudes), one rounding for `scale` as a float and one for the multiplication by it.  dz in bf16: the
    reference sees the same rounded values.  (37, 3, 4): S < k, both paddings overlap; 37 tokens: the tail tile."""
    dz = rnd(tokens * S, 64, seed=300 + k, dtype=zt)
    w = rnd(64, 1, 1, k, scale=k ** -0.5, seed=310 + k)
    d = ops.conv_in_desc(tokens, 1, 1, S, S, k, 1, (k - 1) // 2, 64)
    ref, mag = _conv_in_bwd_data_ref(dz.float(), w, tokens, S, k)
    for scale in (1.0, 1.0 / 3.0):
        got = ops.conv_in_bwd_data(d, dz, w, scale)
        again = ops.conv_in_bwd_data(d, dz, w, scale)
        torch.cuda.synchronize()
        assert got.shape == (tokens, S) and got.dtype == torch.float32
        assert torch.equal(got, again)  # no atomics: bit-identical from call to call
        err = (got.cpu().double() - scale * ref).abs()
        bound = (64 * k + 2) * U * scale * mag
        worst = (err / bound.clamp_min(1e-300)).max().item()
        record_observed(f"conv_in_bwd_data.t{tokens}.S{S}.k{k}.{str(zt)[6:]}.scale{scale:.2f}.err_over_bound", worst)
        assert bool((err <= bound).all()), worst


def test_conv_in_bwd_data_more_than_four_taps_and_whole_batches(ops):
    """k = 9 takes three passes of four taps (later passes add onto dx); B x I tokens with I > 1 (the token is (b, i))."""
    B, I, S, k = 3, 5, 20, 9
    dz, w = rnd(B * I * S, 64, seed=331), rnd(64, 1, 1, k, scale=1 / 3, seed=332)
    got = ops.conv_in_bwd_data(ops.conv_in_desc(B, 1, I, S, S, k, 1, (k - 1) // 2, 64), dz, w, 1.0)
    ref, mag = _conv_in_bwd_data_ref(dz, w, B * I, S, k)
    over = ((got.cpu().double() - ref).abs() / ((64 * k + 2) * U * mag).clamp_min(1e-300)).max().item()
    record_observed("conv_in_bwd_data.k9.B3.I5.S20.err_over_bound", over)
    assert over <= 1.0, over


def test_conv_in_bwd_data_refuses_other_shapes_before_any_launch(ops):
    from focal_amd._lib import FocalHipError
    S, k = 20, 4
    dz = rnd(10 * S, 64, seed=340)
    for kw in (dict(cin=2), dict(stride=2)):
        cin, stride = kw.get("cin", 1), kw.get("stride", 1)
        d = ops.conv_in_desc(10, cin, 1, S, S, k, stride, 1, 64)
        w = rnd(64, cin, 1, k, seed=341)

        def call():
            with pytest.raises(FocalHipError, match="conv_in_bwd_data"):
                ops.conv_in_bwd_data(d, dz, w, 1.0)
        _, launched = _traced(call)
        assert launched == [], launched


def test_conv_in_fwd_and_bwd_weight_at_the_second_block_shapes(ops):
    """cin = 1, k = 4, S = 128 (the second ConvBlock's in-conv: K = 4 takes the `tiny` weight-gradient kernel): bounds of
    tests/test_kernels_gpu.py::test_conv_in."""
    B, cin, I, C, S, k = 16, 1, 10, 64, 128, 4
    x = rnd(B, cin, I, S, scale=10.0, seed=70)
    w, b = rnd(C, cin, 1, k, scale=(cin * k) ** -0.5, seed=71), rnd(C, seed=72)
    d = ops.conv_in_desc(B, cin, I, S, S, k, 1, (k - 1) // 2, C)
    z = ops.conv_in_fwd(d, x, w, b)
    xr, wr, br = x.double().cpu(), w.double().cpu().requires_grad_(True), b.double().cpu().requires_grad_(True)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ref_tok = F.conv2d(xr, wr, br, padding="same").permute(0, 2, 3, 1).reshape(-1, C)
    e = rel_err(z.cpu(), ref_tok.detach())
    record_observed("conv_in.cin1_k4_S128.fwd_rel", e)
    assert e < 1e-5
    for zt in (torch.float32, torch.bfloat16):
        dz = rnd(B * I * S, C, seed=73, dtype=zt)
        dw, db = torch.zeros_like(w), torch.zeros(C, device=DEV)
        ops.conv_in_bwd_weight(d, x, dz, dw, db)
        wr.grad = br.grad = None
        (ref_tok * dz.double().cpu()).sum().backward(retain_graph=True)
        e_w, e_b = rel_err(dw.cpu(), wr.grad), rel_err(db.cpu(), br.grad)
        record_observed(f"conv_in.cin1_k4_S128.dw_rel.{str(zt)[6:]}", e_w)
        record_observed(f"conv_in.cin1_k4_S128.db_rel.{str(zt)[6:]}", e_b)
        assert e_w < 2e-5 and e_b < 2e-5, (e_w, e_b)


# ---------------------------------------------------------------------------------------------- focal_rows_mean
@pytest.mark.parametrize("L", [2, 3, 8])
@pytest.mark.parametrize("n", [1, 7, 20480])
def test_rows_mean_against_float64(ops, L, n):
    """Bound: (L + 1) u sum_l |x_l| / L -- L - 1 additions and one division, each rounding at most u of the sum of magnitudes."""
    xs = [rnd(n, scale=3.0, seed=400 + 10 * L + l) for l in range(L)]
    y = ops.rows_mean(xs)
    ref = sum(x.double().cpu() for x in xs) / L
    bound = (L + 1) * U * sum(x.double().cpu().abs() for x in xs) / L
    err = (y.cpu().double() - ref).abs()
    record_observed(f"rows_mean.L{L}.n{n}.err_over_bound", (err / bound.clamp_min(1e-300)).max().item())
    assert bool((err <= bound).all())
    # inputs that are not 16-byte aligned take the scalar form: same values
    if n > 1:
        base = [rnd(n + 1, scale=3.0, seed=400 + 10 * L + l) for l in range(L)]
        off = ops.rows_mean([b[1:] for b in base])
        ref_off = sum(b[1:].double().cpu() for b in base) / L
        bound_off = (L + 1) * U * sum(b[1:].double().cpu().abs() for b in base) / L
        over = ((off.cpu().double() - ref_off).abs() / bound_off.clamp_min(1e-300)).max().item()
        record_observed(f"rows_mean.unaligned.L{L}.n{n}.err_over_bound", over)
        assert over <= 1.0, over


def test_rows_mean_is_capturable(ops):
    """The pointers travel by value: nothing is uploaded, so the launch records into a graph and replays on new contents."""
    L, n = 3, 20480
    xs = [rnd(n, seed=450 + l) for l in range(L)]
    y = torch.empty(n, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.rows_mean(xs, out=y)
    torch.cuda.current_stream().wait_stream(side)
    eager = y.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.rows_mean(xs, out=y)
    y.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, eager)
    for x in xs:
        x.mul_(2.0)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, ops.rows_mean(xs))


# ---------------------------------------------------------------------------------------------- the second-level stack alone
class _StackOnly:
    """A backbone holding one second-level ConvBlock only (the stack needs the arena, the buffers, the BatchNorm counters, the rng)."""

    @staticmethod
    def build(ct, S=128, k=4, n_inter=3):
        from focal_amd.backbone import HipBackbone
        from models.ConvModules import ConvBlock
        from models.DeepSense import DeepSense

        class Net(HipBackbone):
            bump_bn_counters, buffer = DeepSense.bump_bn_counters, DeepSense.buffer

            def __init__(self):
                super().__init__()
                self.config = {}
                self._init_hip(argparse.Namespace(compute_dtype=ct, train_mode="contrastive", stage="pretrain"))
                self._hot = lambda name: True
                self.drop_rate, self.sync_bn, self._buffers_by_name = 0.0, False, None
                self.mod_extractors = nn.ModuleDict({"m": ConvBlock(in_channels=1, out_channels=128, in_spectrum_len=S,
                                                                    conv_lens=[[1, k]] * 3, dropout_ratio=0.0, num_inter_layers=n_inter)})
        return Net()


def _stack_reference(net, xs, dy, B, I, S, groups):
    """float64 CPU: mean of the inputs -> nn.Conv2d / BatchNorm2d / GELU layers -> flatten -> nn.Conv1d, as the reference's ConvBlock runs
    them (train mode; each of the `groups` equal parts of the batch is one backbone call with its own batch statistics)."""
    import warnings
    sd = {k[len("mod_extractors.m."):]: v.detach().cpu().double() for k, v in net.state_dict().items()}
    n_inter = len(net.mod_extractors["m"].conv_layers_inter)
    k = net.mod_extractors["m"].conv_lens[1][1]

    def layer(cin, kk):
        return nn.ModuleDict(dict(conv=nn.Conv2d(cin, 64, [1, kk], padding="same"), batch_norm=nn.BatchNorm2d(64)))
    mods = nn.ModuleDict(dict(conv_layer_in=layer(1, net.mod_extractors["m"].conv_lens[0][1]),
                              conv_layers_inter=nn.ModuleList([layer(64, k) for _ in range(n_inter)]),
                              conv_layer_out=nn.Conv1d(64 * S, 128, 1))).double()
    mods.load_state_dict(sd)
    mods.train()
    act = nn.GELU()
    leaves = [x.detach().cpu().double().requires_grad_(True) for x in xs]
    xm = (sum(leaves) / len(leaves)).view(B, 1, I, S)
    outs, zs = [], []

    def keep(name, z):  # the convolution outputs: their gradients dz bound the (analytically zero) conv-bias gradients
        z.retain_grad()
        zs.append((name, z))
        return z
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for part in xm.chunk(groups, dim=0):
            z = keep("conv_layer_in", mods["conv_layer_in"]["conv"](part))
            h = act(mods["conv_layer_in"]["batch_norm"](z))
            for li, ly in enumerate(mods["conv_layers_inter"]):
                h = h + act(ly["batch_norm"](keep(f"conv_layers_inter.{li}", ly["conv"](h))))
            h = h.permute(0, 1, 3, 2)
            b, c, s, i = h.shape
            outs.append(mods["conv_layer_out"](h.reshape(b, c * s, i)).permute(0, 2, 1).reshape(b * i, 128))
    y = torch.cat(outs, dim=0)
    (y * dy.cpu().double()).sum().backward()
    grads = {f"mod_extractors.m.{n}": p.grad for n, p in mods.named_parameters()}
    dz_mag = {}
    for name, z in zs:  # sum over (b, i, s) of |dz| per channel, over all parts
        dz_mag[name] = dz_mag.get(name, 0) + z.grad.abs().sum(dim=(0, 2, 3))
    return y.detach(), [x.grad for x in leaves], grads, dz_mag


@pytest.mark.parametrize("ct", ["fp32", "bf16"])
@pytest.mark.parametrize("groups", [1, 2])
def test_second_level_stack_against_torch_modules(ops, ct, groups):
    """rows_mean of 3 + the ConvBlock with cin = 1, S = 128, k = 4, 3 inter layers at B*I = 160 tokens: output, the gradient reaching each of
    the 3 inputs (the stack's one input gradient, times 1 / 3) and every parameter gradient; fp32 1e-4 / bf16 1e-2 of the reference's
    max, as tests/test_multiloc_gpu.py::test_loc_stage_against_torch_encoder_layer.
    A conv bias in front of a train-mode BatchNorm has an analytically zero gradient (the column sum of dz, which BatchNorm's backward
    centres): what the kernels leave is rounding.  Per channel it is bounded by eps * sum_rows |dz| with eps = n u for the fp32 sums
    over the n rows (the two centring statistics and the column sum itself: the standard n u bound of an n-term sum), plus 2^-8 in the
    bf16 mode, where every dz element is stored rounded to bf16 (2^-9 of itself; the factor 2 covers |dz| taken from the reference)."""
    from focal_amd.deepsense_engine import ConvStack
    from oracle.weights import fill_state_dict_
    B, I, S, L = 16, 10, 128, 3
    net = _StackOnly.build(ct)
    fill_state_dict_(net.state_dict())
    net = net.cuda().train()
    geo = net.mod_extractors["m"].geometry
    assert (geo["C"], geo["S"], geo["k_in"], geo["k"], geo["n_inter"], geo["pad_in"]) == (64, 128, 4, 4, 3, 1)
    xs = [rnd(B * I, S, seed=500 + l) for l in range(L)]
    dy = rnd(B * I, 128, seed=510)
    stack = ConvStack(net, "mod_extractors.m", geo, 0)
    net.arena().zero_grad()
    with torch.no_grad():
        xm = ops.rows_mean(xs)
        y, sv = stack.forward(xm.view(B, 1, I, S), 0, True, None, groups)
        dxm = stack.backward(sv, dy, need_dx=True, dx_scale=1.0 / L)
    torch.cuda.synchronize()
    ref_y, ref_dx, ref_g, dz_mag = _stack_reference(net, xs, dy, B, I, S, groups)
    tol = 1e-4 if ct == "fp32" else 1e-2
    rel = lambda a, b: (a.cpu().double() - b).abs().max().item() / max(b.abs().max().item(), 1e-12)
    e_y = rel(y, ref_y)
    e_dx = max(rel(dxm, g) for g in ref_dx)
    record_observed(f"ds_stack2.g{groups}.{ct}.out_rel", e_y)
    record_observed(f"ds_stack2.g{groups}.{ct}.dx_rel", e_dx)
    assert e_y < tol and e_dx < tol, (e_y, e_dx)
    params = dict(net.named_parameters())
    assert set(ref_g) == set(params) and len(ref_g) == 18
    worst = 0.0
    for n, g in ref_g.items():
        if n.endswith("conv.bias"):
            eps = B * I * S * U + (2.0 ** -8 if ct == "bf16" else 0.0)
            bound = eps * dz_mag[n[len("mod_extractors.m."):-len(".conv.bias")]]
            over = (params[n].grad.cpu().double().abs() / bound).max().item()
            record_observed(f"ds_stack2.g{groups}.{ct}.{n}.zero_grad_over_bound", over)
            assert over <= 1.0, (n, over)
            continue
        worst = max(worst, rel(params[n].grad, g))
    record_observed(f"ds_stack2.g{groups}.{ct}.dparam_rel_worst", worst)
    assert worst < tol, worst
    assert int(net.state_dict()["mod_extractors.m.conv_layers_inter.2.batch_norm.num_batches_tracked"]) == groups


# ---------------------------------------------------------------------------------------------- the step on HAR3LOC
def _cfg3(dropout=False):
    from oracle.config import load_config
    cfg = load_config(os.path.join(ROOT, "focal_amd", "src", "data", "HAR3LOC.yaml"))
    return cfg if dropout else no_dropout(cfg)


def build(ct, dropout=False, cfg=None):
    from models.DeepSense import DeepSense
    from models.FOCALModules import FOCAL
    from models.loss import FOCALLoss
    from oracle.weights import fill_state_dict_
    cfg = cfg or _cfg3(dropout)
    args = argparse.Namespace(model="DeepSense", dataset="HAR3LOC", device=torch.device("cuda"), train_mode="contrastive",
                              learn_framework="FOCAL", stage="pretrain", task="activity_classification", tag=None, dataset_config=cfg,
                              compute_dtype=ct)
    net = DeepSense(args)
    fill_state_dict_(net.state_dict())
    net = net.to("cuda")
    return args, net, FOCAL(args, net), FOCALLoss(args)


def inputs(cfg, B=8):
    from oracle.weights import synthetic_freq_input
    to = lambda d: {l: {m: v.cuda() for m, v in mm.items()} for l, mm in d.items()}
    return to(synthetic_freq_input(cfg, B, seed=311)), to(synthetic_freq_input(cfg, B, seed=312))


def scale_err(a, ref):
    return ((a - ref).abs().max() / ref.abs().max()).item()


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLD, "DeepSense_3loc_b8.npz"))


@pytest.mark.parametrize("ct", ["fp32", "bf16"])
def test_train_step_loss_and_gradients(fx, ct):
    """bf16 embeddings: observed 0.65e-2 (acc) / 0.48e-2 (gyr) of scale on an MI355X -- inside the 1e-2 of the single-location fixtures, so
    that is asserted, not the 2e-2 the project grants SW_Transformer on HAR3LOC.  Observed besides: fp32 embeddings 1.7e-6, gradient norms
    1.9e-6 at worst; bf16 loss terms <= 2.6e-4, gradient norms 1.15e-2 at worst with no name beyond 6e-2."""
    args, net, focal, loss_fn = build(ct)
    net.train()
    x1, x2 = inputs(args.dataset_config)
    f1, f2 = focal(x1, x2, proj_head=True)
    for m in f1:
        e1 = scale_err(f1[m].detach().cpu(), torch.from_numpy(fx[f"train.emb1.{m}"]))
        e2 = scale_err(f2[m].detach().cpu(), torch.from_numpy(fx[f"train.emb2.{m}"]))
        record_observed(f"deepsense_3loc.train.emb.{m}.{ct}.max_err_over_max_ref", max(e1, e2))
        assert max(e1, e2) < (1e-3 if ct == "fp32" else 1e-2), (m, e1, e2)
    net.arena().zero_grad()
    loss = loss_fn(f1, f2)
    loss.backward()
    terms = loss_fn.last_terms.cpu().numpy()
    rel = 1e-3 if ct == "fp32" else 1e-2
    for i, k in enumerate(("shared", "private", "orth", "rank", "total")):
        ref = float(fx[f"train.loss.{k}"])
        record_observed(f"deepsense_3loc.train.loss.{k}.{ct}.abs_err_over_max1", abs(terms[i] - ref) / max(1.0, abs(ref)))
        assert abs(terms[i] - ref) < rel * max(1.0, abs(ref)), (k, terms[i], ref)
    names, norms = [str(n) for n in fx["train.grad_names"]], fx["train.grad_norms"]
    params = dict(net.named_parameters())
    assert {n for n, p in params.items() if p.grad is not None} == set(names)
    assert sum(n.startswith("mod_extractors.") for n in names) == 36
    bad, worst, worst_slice = [], 0.0, 0.0
    for n, ref in zip(names, norms):
        got = params[n].grad.double().norm().item()
        if n.endswith("conv.bias") and ref < 1e-5:
            # a conv bias in front of a train-mode BatchNorm has an analytically zero gradient: both sides are noise
            assert got < 5e-3, (n, got)
            continue
        if n.startswith("mod_extractors."):
            assert got > 0, n
        worst = max(worst, abs(got - ref) / max(ref, 1e-6))
        tol = 2e-3 if ct == "fp32" else 6e-2
        if abs(got - ref) > tol * max(ref, 1e-6) + 1e-6:
            bad.append((n, got, float(ref)))
        if ct == "fp32":
            sl = torch.from_numpy(fx[f"train.gradslice.{n}"])
            flat = params[n].grad.detach().reshape(-1).cpu().double()
            mine = flat[::max(1, flat.numel() // 16)][:16]
            e_sl = (mine - sl).abs().max().item() / max(sl.abs().max().item(), ref / max(flat.numel() ** 0.5, 1), 1e-6)
            worst_slice = max(worst_slice, e_sl)
            assert (mine - sl).abs().max().item() < 2e-3 * max(sl.abs().max().item(), ref / max(flat.numel() ** 0.5, 1), 1e-6) + 1e-6, n
    record_observed(f"deepsense_3loc.train.grad_norm.{ct}.worst_rel", worst)
    record_observed(f"deepsense_3loc.train.grad_norm.{ct}.outliers", len(bad))
    if ct == "fp32":
        record_observed("deepsense_3loc.train.grad_slice.fp32.worst_rel", worst_slice)
    if ct == "fp32":
        assert not bad, bad[:8]
    else:
        assert not [b for b in bad if b[0].startswith("mod_extractors.")], bad[:8]
        assert len(bad) <= max(1, len(names) * 3 // 100), bad[:8]
        assert all(abs(g - r) < 0.25 * max(r, 1e-6) for _, g, r in bad), bad[:8]
    sd = net.state_dict()
    bufs = [k for k in fx.files if k.startswith("train.buf.")]
    assert any(k.startswith("train.buf.mod_extractors.") for k in bufs) and any(k.startswith("train.buf.loc_mod_extractors.") for k in bufs)
    worst_buf = 0.0
    for k in bufs:
        name = k[len("train.buf."):]
        e = scale_err(sd[name].cpu(), torch.from_numpy(fx[k]))
        worst_buf = max(worst_buf, e)
        assert e < (2e-4 if ct == "fp32" else 2e-2), (name, e)
    record_observed(f"deepsense_3loc.train.buffers.{ct}.worst_err_over_max_ref", worst_buf)
    assert int(sd["loc_mod_extractors.ankle.gyr.conv_layers_inter.3.batch_norm.num_batches_tracked"]) == 2
    assert int(sd["mod_extractors.acc.conv_layer_in.batch_norm.num_batches_tracked"]) == 2


@pytest.mark.parametrize("ct", ["fp32", "bf16"])
def test_three_adamw_steps_follow_reference(fx, ct):
    """Bounds of tests/test_deepsense_evenk_gpu.py::test_three_adamw_steps_follow_reference, at the fixture's learning rate adamw.lr = 1e-4
    (the DeepSense section's own optimizer.start_lr).  At the FOCAL section's 1e-3 the REFERENCE's own trajectory on this model is no
    yardstick -- gradient noise of 1e-6 of each tensor's maximum moves its third loss by up to 5e-2, bf16 autocast by 15 % -- while at 1e-4
    the same batch descends as steeply (26.35 -> 13.74 -> 5.60) and the reference stays within 1.1e-4 under that noise and within
    1.5e-2 under bf16 autocast: tests/golden/gen_golden_deepsense_multiloc.py asserts both, to a quarter of the bounds below, before it
    writes the fixture."""
    import copy
    cfg = copy.deepcopy(_cfg3())
    cfg["FOCAL"]["pretrain_optimizer"]["start_lr"] = float(fx["adamw.lr"])
    from train_utils.optimizer import define_optimizer
    args, net, focal, loss_fn = build(ct, cfg=cfg)
    net.train()
    opt = define_optimizer(args, focal.parameters())
    assert all(g["lr"] == float(fx["adamw.lr"]) for g in opt.param_groups)
    x1, x2 = inputs(args.dataset_config)
    traj = []
    for it in range(3):
        opt.zero_grad()
        a, b = focal(x1, x2, proj_head=True)
        loss = loss_fn(a, b)
        loss.backward()
        opt.step()
        traj.append(loss.item())
    ref = fx["adamw.loss_traj"]
    for i, (got, r) in enumerate(zip(traj, ref)):
        record_observed(f"deepsense_3loc.adamw.loss_step{i}.{ct}.rel", abs(got - r) / abs(r))
    if ct == "fp32":
        p = dict(net.named_parameters())[str(fx["adamw.probe_name"])].detach().reshape(-1).cpu().double()
        e_probe = (p[::max(1, p.numel() // 32)][:32] - torch.from_numpy(fx["adamw.probe_after3"])).abs().max().item()
        record_observed("deepsense_3loc.adamw.probe_after3.fp32.max_abs", e_probe)
        for got, r in zip(traj, ref):
            assert abs(got - r) < 2e-3 * abs(r), (traj, ref)
        assert e_probe < 2e-4, e_probe
    else:
        # AdamW's first updates are sign-like: bf16 rounding of near-zero gradients sends the two runs down different (equally valid)
        # trajectories -- step 0 is pinned, the later steps must show the same steep descent (tests/test_deepsense_evenk_gpu.py)
        assert abs(traj[0] - ref[0]) < 1e-2 * abs(ref[0]), (traj, ref)
        assert abs(traj[1] - ref[1]) < 0.15 * abs(ref[1]) and abs(traj[2] - ref[2]) < 0.15 * abs(ref[2]), (traj, ref)


@pytest.mark.parametrize("ct", ["fp32", "bf16"])
def test_eval_embeddings_settled_statistics(fx, ct):
    """Eval mode on the running statistics the reference model settled by itself, loaded into the HIP model."""
    args, net, _, _ = build(ct)
    sd = net.state_dict()
    for k in fx.files:
        if k.startswith("settled.buffer."):
            sd[k[len("settled.buffer."):]].copy_(torch.from_numpy(fx[k]))
    net.eval()
    x1, _ = inputs(args.dataset_config)
    with torch.no_grad():
        emb = net(x1, class_head=False, proj_head=True)
        feat = net(x1, class_head=False, proj_head=False)
    for m in emb:
        ref = torch.from_numpy(fx[f"settled.eval.emb.{m}"])
        e = scale_err(emb[m].cpu(), ref)
        cos = F.cosine_similarity(emb[m].cpu(), ref, dim=-1).min().item()
        ef = scale_err(feat[m].cpu(), torch.from_numpy(fx[f"settled.eval.feat.{m}"]))
        record_observed(f"deepsense_3loc.eval_settled.emb.{m}.{ct}.max_err_over_max_ref", e)
        record_observed(f"deepsense_3loc.eval_settled.emb.{m}.{ct}.min_row_cosine", cos)
        record_observed(f"deepsense_3loc.eval_settled.feat.{m}.{ct}.max_err_over_max_ref", ef)
        assert e < (1e-3 if ct == "fp32" else 1e-2), (m, e)
        assert ef < (1e-3 if ct == "fp32" else 1e-2), (m, ef)
        assert cos > (0.999999 if ct == "fp32" else 0.9999), (m, cos)


@pytest.mark.parametrize("ct", ["fp32", "bf16"])
def test_both_views_in_one_pass_equal_two_passes(ct, monkeypatch):
    """One pass over [view 1; view 2] with per-view statistic groups against two passes side by side (FOCAL_DEEPSENSE_TWO_PASSES=1): every
    stack of both levels keeps its own sinks; bounds of tests/test_deepsense_parity_gpu.py::test_both_views_in_one_pass_equal_two_passes."""
    got = {}
    for mode in ("one", "two"):
        monkeypatch.setenv("FOCAL_DEEPSENSE_TWO_PASSES", "1" if mode == "two" else "0")
        args, net, focal, loss_fn = build(ct)
        x1, x2 = inputs(args.dataset_config)
        net.train()
        assert bool(net.views_share_pass) == (mode == "one")
        f1, f2 = focal(x1, x2, proj_head=True)
        net.arena().zero_grad()
        loss = loss_fn(f1, f2)
        loss.backward()
        torch.cuda.synchronize()
        got[mode] = dict(f1={m: v.detach().clone() for m, v in f1.items()}, f2={m: v.detach().clone() for m, v in f2.items()},
                         terms=loss_fn.last_terms.clone(), grads={n: p.grad.detach().clone() for n, p in net.named_parameters() if p.grad is not None},
                         bufs={k: v.detach().clone() for k, v in net.state_dict().items() if "running_" in k or "num_batches" in k})
    a, b = got["one"], got["two"]
    tol = 2e-5 if ct == "fp32" else 2e-2
    for m in a["f1"]:
        e_m = max(scale_err(a["f1"][m].cpu(), b["f1"][m].cpu()), scale_err(a["f2"][m].cpu(), b["f2"][m].cpu()))
        record_observed(f"deepsense_3loc.one_pass_vs_two.{ct}.emb.{m}", e_m)
        assert e_m < tol, m
    e_terms = (a["terms"] - b["terms"]).abs().max().item() / max(1.0, b["terms"].abs().max().item())
    record_observed(f"deepsense_3loc.one_pass_vs_two.{ct}.terms", e_terms)
    assert e_terms < tol
    assert a["grads"].keys() == b["grads"].keys()
    num = sum((a["grads"][n].double() - b["grads"][n].double()).pow(2).sum().item() for n in a["grads"]) ** 0.5
    den = sum(b["grads"][n].double().pow(2).sum().item() for n in a["grads"]) ** 0.5
    record_observed(f"deepsense_3loc.one_pass_vs_two.{ct}.grad_l2_rel", num / den)
    assert num / den < (1e-4 if ct == "fp32" else 6e-2)
    worst_buf = 0.0
    for k in a["bufs"]:
        if "num_batches" in k:
            assert int(a["bufs"][k]) == int(b["bufs"][k]) == 2, k
        else:
            e_b = scale_err(a["bufs"][k].cpu(), b["bufs"][k].cpu())
            worst_buf = max(worst_buf, e_b)
            assert e_b < (1e-5 if ct == "fp32" else 2e-2), k
    record_observed(f"deepsense_3loc.one_pass_vs_two.{ct}.buffers_worst", worst_buf)


def test_captured_step_matches_eager():
    """Three optimizer steps at learning rate 0 on fixed views, eager and through the captured step (graph_step.CapturedTrainStep), in a
    child process (tests/deepsense_multiloc_capture_worker.py): same loss to 1e-5, same arena gradients to 1e-5 of scale; with dropout
    on, two replays draw different masks and stay finite."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "deepsense_multiloc_capture_worker.py")], capture_output=True, text=True,
                       timeout=600, cwd=ROOT)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["replays"] >= 1
    assert len(out["steps"]) == 3
    for le, lr, e in out["steps"]:
        assert np.isfinite(le) and abs(le - lr) <= 1e-5 * abs(le), (le, lr)
        record_observed("deepsense_3loc.graph_vs_eager.grad_rel", e)
        assert e <= 1e-5, e  # (not bit-identical: the weight-gradient GEMMs accumulate with fp32 atomics in any order)
    assert abs(out["steps"][1][1] - out["steps"][2][1]) <= 1e-6 * abs(out["steps"][1][1])  # p = 0: two replays agree
    d = out["dropout"]
    assert d["replays"] >= 1 and d["finite"]
    assert d["losses"][1] != d["losses"][2] and d["grads_differ"]


def test_train_py_on_har3loc():
    """`train.py -model=DeepSense -dataset=HAR3LOC`: one synthetic epoch (training steps, the KNN estimator and the validation pass in eval
    mode) exits 0 with finite loss terms; the checkpoints it writes are removed."""
    src = os.path.join(ROOT, "focal_amd", "src")
    wdir = os.path.join(ROOT, "weights", "HAR3LOC_DeepSense")
    had = os.path.isdir(wdir)
    try:
        r = subprocess.run([sys.executable, os.path.join(src, "train.py"), "-model=DeepSense", "-dataset=HAR3LOC", "-learn_framework=FOCAL",
                            "-batch_size=16", "-synthetic_batches=2", "-epochs=1"], capture_output=True, text=True, timeout=900, cwd=src)
    finally:
        if not had:
            shutil.rmtree(wdir, ignore_errors=True)
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-3000:]
    assert "Total processing time" in log
    m = re.search(r"terms\[shared,private,orth,rank,total\]=\[([^\]]*)\]", log)
    assert m, log[-2000:]
    terms = [float(v) for v in m.group(1).split(",")]
    assert len(terms) == 5 and all(np.isfinite(terms)), terms
    assert not re.search(r"loss[^\n]*\bnan\b", log, flags=re.I), log[-2000:]


# ---------------------------------------------------------------------------------------------- the single-location path
def test_single_location_launches_unchanged():
    """One eager DeepSense / MOD B = 8 bf16 training step launches the multiset of kernels it launched before the engine was split into
    a conv stack and a GRU part (recorded at the parent commit by tests/golden/gen_deepsense_mod_launches.py)."""
    sys.path.insert(0, GOLD)
    try:
        from gen_deepsense_mod_launches import step_launches
    finally:
        sys.path.remove(GOLD)
    want = json.load(open(os.path.join(GOLD, "DeepSense_MOD_b8_launches.json")))["launches"]  # ("commit": where it was recorded)
    got = step_launches()
    diff = {k: (want.get(k, 0), got.get(k, 0)) for k in set(want) | set(got) if want.get(k, 0) != got.get(k, 0)}
    assert not diff, diff
    assert not any("conv_in_bwd_data" in k or "rows_mean" in k for k in got)
