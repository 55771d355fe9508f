"""SW_Transformer's `APE` and `in_stride` switches on the GPU: the patch-embedding kernels (focal_pad_patch_embed_ape_ln*_fwd) and the
position embedding's gradient kernel (focal_ape_bwd) against float64 restatements, the FOCAL step on MOD with APE on and with
in_stride 2 against the reference fixtures (tests/golden/gen_golden_ape_stride.py), the captured step, and the classifier path."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import make_args, no_dropout, record_observed

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLD = os.path.join(ROOT, "tests", "golden")
APE = "absolute_pos_embed."

# (x shape, stride, patch width, C0) -- window [3, 3] and three stages pad the patch grid to multiples of 12:
#   0  the issue's case 1: 12 x 24 grid with pad rows and pad columns, 576 tokens: 64-token tile boundaries fall inside a sample
#   1  stride 1, patch [1, 4]    2  stride 4 on a single input channel
#   3  the MOD audio geometry at stride 2 (K = 4 * 40 = 160 taps: the contraction runs in two chunks)    4  the same at 128 channels (chunks of 85)
#   5  K = 80 at stride 1: with a position embedding this is the matrix-core instance
CASES = [((2, 2, 10, 40), 2, 1, 64), ((2, 2, 10, 40), 1, 4, 64), ((2, 1, 10, 40), 4, 1, 64),
         ((2, 2, 10, 160), 2, 40, 64), ((2, 2, 10, 160), 2, 40, 128), ((2, 2, 10, 160), 1, 40, 64)]


def _case(i):
    """Inputs of CASES[i] and the float64 restatement (oracle.swt.pad_and_embed in double) of tokens, a1 and stats, with and without ape."""
    from oracle.config import swt_geometry
    from oracle.swt import pad_and_embed
    shape, stride, pw, C0 = CASES[i]
    b, cin, I, S = shape
    cfg = {"num_segments": I, "loc_mod_spectrum_len": {"l": {"m": S}}, "loc_mod_in_freq_channels": {"l": {"m": cin}},
           "SW_Transformer": {"in_stride": {"m": stride}, "patch_size": {"freq": {"m": [1, pw]}}, "window_size": {"m": [3, 3]},
                              "time_freq_block_num": {"m": [2, 2, 2]}, "time_freq_out_channels": C0, "time_freq_head_num": 4}}
    geo = swt_geometry(cfg, "l", "m")
    Hp, Wp = geo["grid"]
    g = torch.Generator().manual_seed(40 + i)
    rn = lambda *s: torch.randn(*s, generator=g)
    x = rn(b, cin, I, S) * 3.0
    P = {"patch_embed.l.m.proj.weight": rn(C0, cin * stride, 1, pw) * 0.3, "patch_embed.l.m.proj.bias": rn(C0) * 0.1,
         "patch_embed.l.m.norm.weight": 1 + 0.2 * rn(C0), "patch_embed.l.m.norm.bias": 0.1 * rn(C0)}
    ape = rn(Hp * Wp, C0) * 0.5
    g2, b2 = 1 + 0.2 * rn(C0), 0.1 * rn(C0)
    emb = pad_and_embed({k: v.double() for k, v in P.items()}, cfg, x.double(), "l", "m")  # [b, Hp*Wp, C0]
    assert emb.shape == (b, Hp * Wp, C0)
    ref = {}
    for with_ape in (False, True):
        t = emb + ape.double() if with_ape else emb
        mean, var = t.mean(-1), t.var(-1, unbiased=False)
        a1 = F.layer_norm(t, (C0,), g2.double(), b2.double(), 1e-5)
        ref[with_ape] = (t.reshape(-1, C0), a1.reshape(-1, C0), torch.stack([mean, (var + 1e-5).rsqrt()], -1).reshape(-1, 2))
    return dict(x=x, P=P, ape=ape, g2=g2, b2=b2, Hp=Hp, Wp=Wp, pw=pw, stride=stride, C0=C0, ref=ref)


@pytest.fixture(scope="module")
def cases():
    return {}


def _get(cases, i):
    if i not in cases:
        cases[i] = _case(i)
    return cases[i]


def _rel(got, ref):
    return ((got.detach().cpu().double() - ref).abs().max() / ref.abs().max()).item()


@pytest.mark.parametrize("with_ape", [False, True])
@pytest.mark.parametrize("i", range(len(CASES)))
def test_embedding_kernel_against_float64(cases, i, with_ape):
    from focal_amd import ops
    c = _get(cases, i)
    dev = lambda t: t.cuda().contiguous()
    w, b, gm, be = (dev(c["P"][f"patch_embed.l.m.{k}"]) for k in ("proj.weight", "proj.bias", "norm.weight", "norm.bias"))
    x, ape = dev(c["x"]), (dev(c["ape"]) if with_ape else None)
    g2, b2 = dev(c["g2"]), dev(c["b2"])
    r_tok, r_a1, r_st = c["ref"][with_ape]
    run = lambda **kw: ops.pad_patch_embed_ape_ln(x, w, b, gm, be, c["Hp"], c["Wp"], c["pw"], stride=c["stride"], ape=ape, **kw)
    tok = run()
    tok32, a32, st32 = run(next_ln=(g2, b2, torch.float32))
    tok16, a16, st16 = run(next_ln=(g2, b2, torch.bfloat16))
    torch.cuda.synchronize()
    errs = dict(plain=_rel(tok, r_tok), ln2_tok=_rel(tok32, r_tok), ln2_a1=_rel(a32, r_a1), ln2_stats=_rel(st32, r_st),
                ln2_bf16_tok=_rel(tok16, r_tok), ln2_bf16_stats=_rel(st16, r_st))
    for k, e in errs.items():
        record_observed(f"ape_stride.embed.case{i}.ape{int(with_ape)}.{k}", e)
    print(i, with_ape, errs)
    assert all(e < 1e-5 for e in errs.values()), errs
    # the bf16 a1 is the fp32 a1 rounded once (half a unit in the last of bf16's 8 significand bits)
    a32c = a32.cpu()
    assert a16.dtype == torch.bfloat16 and bool(((a16.cpu().float() - a32c).abs() <= a32c.abs() * 2.0 ** -8 + 1e-30).all())
    if with_ape:  # the add really happened, and before the second LayerNorm
        plain = ops.pad_patch_embed_ape_ln(x, w, b, gm, be, c["Hp"], c["Wp"], c["pw"], stride=c["stride"])
        assert _rel(tok - plain, (c["ref"][True][0] - c["ref"][False][0])) < 1e-5
        assert _rel(a32, c["ref"][False][1]) > 1e-2


@pytest.mark.parametrize("i", [1, 5])
def test_new_entry_point_without_ape_and_stride_is_the_old_one_bit_for_bit(cases, i):
    from focal_amd import ops
    c = _get(cases, i)
    assert c["stride"] == 1
    dev = lambda t: t.cuda().contiguous()
    w, b, gm, be = (dev(c["P"][f"patch_embed.l.m.{k}"]) for k in ("proj.weight", "proj.bias", "norm.weight", "norm.bias"))
    x, g2, b2 = dev(c["x"]), dev(c["g2"]), dev(c["b2"])
    assert torch.equal(ops.pad_patch_embed_ln(x, w, b, gm, be, c["Hp"], c["Wp"], c["pw"]),
                       ops.pad_patch_embed_ape_ln(x, w, b, gm, be, c["Hp"], c["Wp"], c["pw"]))
    for ct in (torch.float32, torch.bfloat16):
        old = ops.pad_patch_embed_ln(x, w, b, gm, be, c["Hp"], c["Wp"], c["pw"], next_ln=(g2, b2, ct))
        new = ops.pad_patch_embed_ape_ln(x, w, b, gm, be, c["Hp"], c["Wp"], c["pw"], next_ln=(g2, b2, ct))
        assert all(torch.equal(o, n) for o, n in zip(old, new))


def test_embedding_launcher_refuses_misaligned_and_indivisible_input(cases):
    from focal_amd import ops
    from focal_amd._lib import FocalHipError
    c = _get(cases, 0)
    dev = lambda t: t.cuda().contiguous()
    w, b, gm, be = (dev(c["P"][f"patch_embed.l.m.{k}"]) for k in ("proj.weight", "proj.bias", "norm.weight", "norm.bias"))
    x = dev(c["x"])
    off = torch.zeros(c["ape"].numel() + 1, device="cuda")[1:].view(c["ape"].shape)  # 4 bytes past a 16-byte boundary
    with pytest.raises(FocalHipError, match="aligned"):
        ops.pad_patch_embed_ape_ln(x, w, b, gm, be, c["Hp"], c["Wp"], c["pw"], stride=c["stride"], ape=off)
    with pytest.raises(FocalHipError, match="multiple of stride"):
        ops.pad_patch_embed_ape_ln(x, w, b, gm, be, c["Hp"], c["Wp"], c["pw"], stride=3)


@pytest.mark.parametrize("N", [3, 1])
def test_ape_gradient_kernel_accumulates_the_column_sum(N):
    from focal_amd import ops
    L, Cc = 288, 64
    g = torch.randn(N * L, Cc, generator=torch.Generator().manual_seed(N)).cuda()
    dape = torch.full((1, L, Cc), 0.5, device="cuda")
    ops.ape_bwd(g, dape)
    torch.cuda.synchronize()
    ref = 0.5 + g.cpu().double().view(N, L, Cc).sum(0, keepdim=True)
    e = _rel(dape, ref)
    record_observed(f"ape_stride.ape_bwd.N{N}.rel", e)
    assert e < 1e-5, e
    x = g.clone()
    ops.ape_add(x, dape)  # the supervised path's forward add, in place
    assert _rel(x, (g.cpu().double().view(N, L, Cc) + dape.cpu().double()).view(N * L, Cc)) < 1e-6


# ---------------------------------------------------------------------------------------------- the model
SEEDS = {"ape": (707, 808), "stride": (909, 1010)}


def _cfg(cfg, tag):
    c = no_dropout(cfg)
    c["SW_Transformer"]["APE"] = True
    if tag == "stride":
        c["SW_Transformer"]["in_stride"] = {"audio": 2, "seismic": 1}
    return c


def _model(cfg, tag, ct):
    from models.SW_Transformer import SW_Transformer
    from oracle.weights import fill_state_dict_
    c = _cfg(cfg, tag)
    args = make_args(c, "SW_Transformer", torch.device("cuda"), ct)
    net = SW_Transformer(args)
    fill_state_dict_(net.state_dict())
    return c, args, net.cuda().train()


def _inputs(c, tag):
    from oracle.weights import synthetic_freq_input
    dev = lambda d: {l: {m: v.cuda() for m, v in mm.items()} for l, mm in d.items()}
    return dev(synthetic_freq_input(c, 8, seed=SEEDS[tag][0])), dev(synthetic_freq_input(c, 8, seed=SEEDS[tag][1]))


@pytest.mark.parametrize("ct", ["fp32", "bf16"])
@pytest.mark.parametrize("tag", ["ape", "stride"])
def test_focal_step_against_the_reference_fixture(cfg, tag, ct):
    """Structure and bounds of test_multiloc_gpu.py::test_har3loc_step_against_the_reference_fixture; fp32: 1e-3 (2e-3 on gradient
    norms and the trajectory, as there); bf16: the README's 1e-2 of scale on embeddings, 1e-2 max(1, |term|) on loss terms, 6e-2 on
    gradient norms (every position-embedding tensor; of the encoders' tensors at most 3 % outside, as in the other fixtures' tests)."""
    from models.FOCALModules import FOCAL
    from models.loss import FOCALLoss
    from train_utils.optimizer import define_optimizer
    fx = np.load(os.path.join(GOLD, f"SW_Transformer_{tag}_b8.npz"))
    c, args, net = _model(cfg, tag, ct)
    x1, x2 = _inputs(c, tag)
    focal, loss_fn = FOCAL(args, net), FOCALLoss(args)
    tol = 1e-3 if ct == "fp32" else 1e-2
    misses = []

    def check(key, err, bound):
        record_observed(f"ape_stride.{tag}.{ct}.{key}", err)
        print(f"{tag}.{ct}.{key} = {err:.4e} (bound {bound:.1e})")
        if not err < bound:
            misses.append((key, err, bound))

    for mode in ("eval", "train"):
        net.train(mode == "train")
        with torch.no_grad():
            for v, x in (("1", x1), ("2", x2)):
                emb, feat = net(x, class_head=False, proj_head=True), net(x, class_head=False, proj_head=False)
                for m in c["modality_names"]:
                    for name, got in (("emb", emb[m]), ("feat", feat[m])):
                        ref = torch.from_numpy(fx[f"pass.{mode}.{name}{v}.{m}"])
                        check(f"{mode}.{name}{v}.{m}.max_err_over_max_ref", ((got.cpu() - ref).abs().max() / ref.abs().max()).item(), tol)
    net.train()
    net.arena().zero_grad()
    f1, f2 = focal(x1, x2, proj_head=True)
    for m in c["modality_names"]:
        for v, got in (("1", f1[m]), ("2", f2[m])):
            ref = torch.from_numpy(fx[f"train.emb{v}.{m}"])
            check(f"train.emb{v}.{m}.max_err_over_max_ref", ((got.detach().cpu() - ref).abs().max() / ref.abs().max()).item(), tol)
    loss = loss_fn(f1, f2)
    loss.backward()
    torch.cuda.synchronize()
    terms = loss_fn.last_terms.cpu().numpy()
    for i, k in enumerate(("shared", "private", "orth", "rank", "total")):
        ref = float(fx[f"train.loss.{k}"])
        check(f"train.loss.{k}.abs_err_over_max1", abs(terms[i] - ref) / max(1.0, abs(ref)), tol)
    params = dict(net.named_parameters())
    names = [str(n) for n in fx["train.grad_names"]]
    assert {n for n, p in params.items() if p.grad is not None} == set(names)
    assert sum(n.startswith(APE) for n in names) == 2
    worst, bad = 0.0, []
    gtol = 2e-3 if ct == "fp32" else 6e-2
    for n, ref in zip(names, fx["train.grad_norms"]):
        got = params[n].grad.double().norm().item()
        e = abs(got - ref) / max(ref, 1e-6)
        worst = max(worst, e)
        if n.startswith(APE):
            assert got > 0, n
            check(f"train.grad_norm.{n}.rel", e, gtol)
        elif e > gtol:
            bad.append((n, got, float(ref)))
    record_observed(f"ape_stride.{tag}.{ct}.train.grad_norm.worst_rel", worst)
    print(f"{tag}.{ct}.grad_norm worst {worst:.4e}, outside {gtol:.0e}: {bad[:8]}")
    if len(bad) > (0 if ct == "fp32" else max(1, len(names) * 3 // 100)):
        misses.append(("grad_norms", bad[:6], gtol))
    # The position embeddings' gradients element by element: asserted in fp32 only, as in the test this one follows (bf16 is pinned by
    # the norms above; the slices' figures are recorded: 2.2e-2 ... 8.1e-2 of the slice's largest element on the MI355X).
    for k in fx.files:
        if k.startswith("train.gradslice."):
            n = k[len("train.gradslice."):]
            ref = torch.from_numpy(fx[k])
            f = params[n].grad.detach().reshape(-1)
            got = f[::max(1, f.numel() // 16)][:16].cpu().double()
            check(f"train.gradslice.{n}.rel", ((got - ref).abs().max() / ref.abs().max()).item(), 1e-3 if ct == "fp32" else float("inf"))
    assert not misses, misses
    if ct != "fp32":
        return
    # three AdamW steps from the fixture's weights
    c, args, net = _model(cfg, tag, ct)
    focal = FOCAL(args, net)
    opt = define_optimizer(args, focal.parameters())
    traj = []
    for _ in range(3):
        opt.zero_grad()
        a, b = focal(x1, x2, proj_head=True)
        l_ = loss_fn(a, b)
        l_.backward()
        opt.step()
        traj.append(float(loss_fn.last_terms[4]))
    ref = fx["adamw.loss_traj"]
    e = max(abs(t - r) / max(1.0, abs(r)) for t, r in zip(traj, ref))
    record_observed(f"ape_stride.{tag}.adamw.loss_traj.fp32.rel", e)
    assert e < 2e-3, (traj, ref.tolist())
    probe = str(fx["adamw.probe_name"])
    assert probe.startswith(APE)
    w = dict(net.named_parameters())[probe].detach().reshape(-1)
    got = w[::max(1, w.numel() // 32)][:32].cpu().double()
    assert (got - torch.from_numpy(fx["adamw.probe_after3"])).abs().max().item() < 1e-3
    assert (got - torch.from_numpy(fx["adamw.probe_before"])).abs().max().item() > 1e-3  # (three steps of lr 1e-3: it moved)


def _trajectory(cfg, replay, lr, steps=4):
    """`steps` optimizer steps on the APE fixture's views, eager or through the captured step (the first call runs eagerly and ends with
    the capture, the rest replay): the losses, the arena's gradients after every step, the audio table before and after."""
    from focal_amd import graph_step, runtime
    from models.FOCALModules import FOCAL
    from models.loss import FOCALLoss
    from train_utils.optimizer import define_optimizer
    c, args, net = _model(cfg, "ape", "fp32")
    if lr is not None:
        c["FOCAL"]["pretrain_optimizer"]["start_lr"] = lr
    x1, x2 = _inputs(c, "ape")
    focal, loss_fn = FOCAL(args, net), FOCALLoss(args)
    opt = define_optimizer(args, focal.parameters())
    step = graph_step.CapturedTrainStep(focal, loss_fn, opt, warm_steps=1, enabled=replay)
    runtime.rng_state("cuda", seed=1234)
    probe = dict(net.named_parameters())[f"{APE}shake.audio"]
    p0 = probe.detach().clone()
    out = []
    for _ in range(steps):
        loss = step(x1, x2)
        torch.cuda.synchronize()
        out.append((float(loss), net.arena().grad.clone()))
    spans = {n: net.arena().index[n][:2] for n in net.arena().index if n.startswith(APE)}
    return out, step, p0, probe.detach().clone(), spans


def test_captured_step_with_ape_matches_eager(cfg):
    """Three replays of the captured step against eager steps, as test_multiloc_gpu.py::test_har3loc_captured_step_matches_eager compares
    them and at its bound: weights held in place (start_lr = 0, so every step sees the same model and only the summation order of the
    atomics separates the runs), 1e-5 on the loss and on the arena's gradients -- and on the position embeddings' slots by themselves."""
    eager, _, _, _, spans = _trajectory(cfg, False, 0.0)
    replayed, st, _, _, _ = _trajectory(cfg, True, 0.0)
    assert st.replays == 3 and len(spans) == 2
    for (le, ge), (lr, gr) in zip(eager, replayed):
        assert np.isfinite(le) and abs(le - lr) <= 1e-5 * abs(le), (le, lr)
        e = ((ge - gr).abs().max() / ge.abs().max()).item()
        record_observed("ape_stride.graph_vs_eager.grad_rel", e)
        assert e <= 1e-5, e
        for n, (o, k) in spans.items():
            assert ge[o:o + k].abs().max().item() > 0
            assert ((ge[o:o + k] - gr[o:o + k]).abs().max() / ge[o:o + k].abs().max()).item() <= 1e-5, n
    assert abs(replayed[1][0] - replayed[2][0]) <= 1e-6 * abs(replayed[1][0])  # two replays of the same step agree


def test_captured_step_trains_the_position_embedding(cfg):
    """The replayed steps at the config's learning rate: the loss follows the reference's AdamW trajectory (2e-3, the fixture tests'
    bound), and the audio table moves, the way it moves in eager steps.  (Eager against replayed LOSSES are not compared at 1e-5 here:
    AdamW's first steps move every element by ~lr in the direction of its gradient's sign, an element whose gradient is at rounding
    level may flip between two runs, and by the fourth step the loss, fallen from 46 to 4.7, carried 1.7e-5 of that in one of three
    runs on the MI355X -- the frozen-weight test above is the sharp one.)"""
    eager, _, _, pe, _ = _trajectory(cfg, False, None)
    replayed, st, p0, pr, _ = _trajectory(cfg, True, None)
    assert st.replays == 3
    ref = np.load(os.path.join(GOLD, "SW_Transformer_ape_b8.npz"))["adamw.loss_traj"]
    for traj in (eager, replayed):
        assert max(abs(t - r) / max(1.0, abs(r)) for (t, _), r in zip(traj, ref)) < 2e-3, ([t for t, _ in traj], ref.tolist())
    e = max(abs(a - b) / max(1.0, abs(a)) for (a, _), (b, _) in zip(eager, replayed))
    record_observed("ape_stride.graph_vs_eager.adamw_loss_traj_rel", e)
    assert e < 2e-3, e
    moved = (pr - p0).abs().max().item()
    record_observed("ape_stride.captured.probe_moved", moved)
    # (in L2 over the table, as test_train_dp_gpu.py measures updates: one element with a rounding-level gradient may flip by 2 lr)
    assert moved > 1e-3 and (pr - pe).double().norm().item() < 0.1 * (pr - p0).double().norm().item()


def test_data_parallel_buckets_keep_the_position_embedding_out_of_the_first(cfg):
    """The table's gradient is the last thing an encoder's backward pass writes: in a split backward pass (data parallel) it is not
    among the gradients that are final when the first phase ends, so it travels in the second all-reduce bucket."""
    _, _, net = _model(cfg, "ape", "bf16")
    ar = net.arena()
    names = [n for n in ar.index if n.startswith(APE)]
    first = set(net.final_after_first_phase())
    assert len(names) == 2 and not first & set(names)
    assert {n for n in ar.index if n.startswith(("mod_in_layers.", "mod_projectors."))} <= first


@pytest.mark.parametrize("ct", ["fp32", "bf16"])
def test_supervised_classifier_path_with_ape_and_stride(cfg, ct):
    """`backbone(freq_x, class_head=True)` trained from scratch with APE on and audio at stride 2, at test_supervised_gpu.py's bounds.
    The reference is the oracle's classifier (oracle/finetune.py: classifier_logits, which supervised_loss_and_grads differentiates)
    with the position embeddings among the leaves -- supervised_loss_and_grads' own parameter filter is the APE-off one; its logits,
    loss and every gradient it does produce are checked to be the same numbers."""
    from models.loss import CrossEntropyLoss
    from models.SW_Transformer import SW_Transformer
    from oracle.finetune import classifier_logits, supervised_loss_and_grads
    from oracle.weights import fill_state_dict_, synthetic_freq_input
    c = _cfg(cfg, "stride")
    args = make_args(c, "SW_Transformer", torch.device("cuda"), ct)
    args.train_mode, args.learn_framework = "supervised", "no"
    net = SW_Transformer(args)
    fill_state_dict_(net.state_dict())
    state = {k: v.detach().clone() for k, v in net.state_dict().items()}
    net = net.cuda().train()
    xs = synthetic_freq_input(c, 8, seed=1111)
    labels = torch.randint(0, c[args.task]["num_classes"], (8,), generator=torch.Generator().manual_seed(5))
    net.arena().zero_grad()
    logits = net({l: {m: v.cuda() for m, v in mm.items()} for l, mm in xs.items()})
    loss = CrossEntropyLoss()(logits, labels.cuda())
    loss.backward()
    torch.cuda.synchronize()
    r_logits, r_loss, r_grads = supervised_loss_and_grads("SW_Transformer", state, c, xs, labels, train=True)
    P = dict(state)
    keys = [k for k in P if k.startswith((APE, "patch_embed."))]
    for k in keys:
        P[k] = P[k].clone().requires_grad_(True)
    o_logits = classifier_logits("SW_Transformer", P, c, xs, train=True, new_buffers={})
    o_grads = dict(zip(keys, torch.autograd.grad(F.cross_entropy(o_logits, labels), [P[k] for k in keys])))
    assert torch.equal(o_logits.detach(), r_logits)
    for k in keys:
        if k in r_grads:
            assert torch.allclose(o_grads[k], r_grads[k], rtol=1e-6, atol=1e-9), k
    e_logits = ((logits.detach().cpu() - r_logits).abs().max() / r_logits.abs().max()).item()
    e_loss = abs(loss.item() - r_loss.item()) / max(1.0, r_loss.item())
    record_observed(f"ape_stride.supervised.{ct}.logits.max_err_over_max_ref", e_logits)
    print(ct, "logits", e_logits, "loss", e_loss)
    assert e_logits < (1e-3 if ct == "fp32" else 3e-2), e_logits
    assert e_loss < (1e-3 if ct == "fp32" else 2e-2), e_loss
    params = dict(net.named_parameters())
    assert sum(k.startswith(APE) for k in keys) == 2
    worst = 0.0
    for k in keys:
        assert params[k].grad is not None, k
        r = o_grads[k].double().norm().item()
        e = abs(params[k].grad.double().norm().item() - r) / max(r, 1e-8)
        print(ct, k, e)
        worst = max(worst, e)
        assert e < (2e-3 if ct == "fp32" else 6e-2), (k, e)
    record_observed(f"ape_stride.supervised.{ct}.ape_and_patch_embed_grad_norm.worst_rel", worst)


def test_finetune_with_ape_and_stride_moves_nothing_but_the_head(cfg):
    from general_utils.weight_utils import set_learnable_params_finetune
    from models.loss import CrossEntropyLoss
    from models.SW_Transformer import SW_Transformer
    from oracle.finetune import finetune_loss_and_grads
    from oracle.weights import fill_state_dict_, synthetic_freq_input
    from train_utils.optimizer import define_optimizer
    c = _cfg(cfg, "stride")
    args = make_args(c, "SW_Transformer", torch.device("cuda"), "fp32")
    args.stage = "finetune"
    net = SW_Transformer(args)
    fill_state_dict_(net.state_dict())
    state = {k: v.detach().clone() for k, v in net.state_dict().items()}
    net = net.cuda().train()
    learnable = set_learnable_params_finetune(args, net)
    xs = synthetic_freq_input(c, 8, seed=1212)
    labels = torch.randint(0, c[args.task]["num_classes"], (8,), generator=torch.Generator().manual_seed(6))
    net.arena().zero_grad()
    logits = net({l: {m: v.cuda() for m, v in mm.items()} for l, mm in xs.items()}, class_head=True)
    CrossEntropyLoss()(logits, labels.cuda()).backward()
    torch.cuda.synchronize()
    r_logits, _, r_grads = finetune_loss_and_grads("SW_Transformer", state, c, xs, labels, train=True)
    assert ((logits.detach().cpu() - r_logits).abs().max() / r_logits.abs().max()).item() < 1e-3
    params = dict(net.named_parameters())
    for n, g in r_grads.items():
        assert ((params[n].grad.cpu() - g).abs().max() / g.abs().max().clamp_min(1e-8)).item() < 2e-3, n
    assert all(params[n].grad is None for n in params if n.startswith(APE))
    before = {k: v.detach().clone() for k, v in net.state_dict().items()}
    define_optimizer(args, learnable).step()
    torch.cuda.synchronize()
    after = net.state_dict()
    for k in before:
        assert (not torch.equal(before[k], after[k])) == (k in r_grads), k
