"""The supervised / finetune step as a replayed hipGraph with the `fixed` pipeline drawn on the device: focal_mixup_draw against the host
restatement of the header's formulas (tests/mix_restatement.py), focal_mixup_multi against the kernel it restates (focal_mixup_fwd),
the captured classifier step against the reference fixtures and against the eager step, the draws of a replay, the shape policy, and
train.py's two classifier stages."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import mix_restatement as mr
from conftest import make_args, no_dropout, record_observed

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SRC = os.path.join(ROOT, "focal_amd", "src")
MIX = dict(mixup_alpha=1.0, cutmix_alpha=1.0, prob=1.0, switch_prob=0.75)
SLOTS = [(10, 1600), (10, 20)]
STREAM = 0x4D495846


def draws(cfg, B, n, seed, slots=SLOTS):
    """n consecutive advancing draws from one seed word, read back once -> (records, perm [n, B], state words)."""
    from focal_amd import ops
    state = ops.new_rng_state(seed, "cuda")
    rec = torch.zeros(n, ops.MIX_RECORD_BYTES, dtype=torch.uint8, device="cuda")
    perm = torch.full((n, B), -1, dtype=torch.int32, device="cuda")
    for k in range(n):
        ops.mixup_draw(cfg, B, slots, state, STREAM, rec[k], perm[k])
    torch.cuda.synchronize()
    raw = rec.cpu().numpy()
    return [ops._lib.MixRecord.from_buffer_copy(raw[k].tobytes()) for k in range(n)], perm.cpu().numpy(), state.cpu().numpy()


# ---------------------------------------------------------------------------------------------- 1. the draw
@pytest.mark.parametrize("B", [1, 2, 8, 257])
def test_draw_equals_the_host_restatement(B):
    seed = 0x1234567
    recs, perm, state = draws(MIX, B, 64, seed)
    s = seed
    for k, r in enumerate(recs):
        want = mr.draw(s, STREAM, MIX, B, SLOTS)
        assert (r.apply, r.cut) == (want["apply"], want["cut"]), k
        assert np.float32(r.lam).tobytes() == want["lam"].tobytes(), (k, r.lam, want["lam"])
        assert [list(b) for b in r.box] == want["boxes"], (k, [list(b) for b in r.box], want["boxes"])
        assert sorted(perm[k].tolist()) == list(range(B)), k
        assert perm[k].tolist() == want["perm"].tolist(), k
        s = mr.next_seed(s)
    # the state words advanced once per call
    assert int(state[0]) & 0xFFFFFFFF == s and int(state[1]) == 64 and int(state[2]) == 0 and int(state[3]) == 0


def test_draw_identity_when_the_coin_misses_and_without_advance():
    from focal_amd import ops
    recs, perm, _ = draws(dict(MIX, prob=0.0), 8, 4, 99)
    for r in recs:
        assert (r.apply, r.cut, r.lam) == (0, 0, 1.0) and all(list(b) == [0, 0, 0, 0] for b in r.box)
    # advance = 0 reads the words and leaves them: the same draw twice
    state = ops.new_rng_state(31337, "cuda")
    rec, p = torch.zeros(2, ops.MIX_RECORD_BYTES, dtype=torch.uint8, device="cuda"), torch.zeros(2, 8, dtype=torch.int32, device="cuda")
    for k in range(2):
        ops.mixup_draw(MIX, 8, SLOTS, state, STREAM, rec[k], p[k], advance=False)
    assert torch.equal(rec[0], rec[1]) and torch.equal(p[0], p[1]) and state.tolist() == [31337, 0, 0, 0]


def test_draw_statistics():
    """1024 draws from a fixed seed, read back once.  The cut coin and perm[0] are held to 5 binomial standard errors; lambda at
    alpha in {0.4, 2.0} (the Marsaglia-Tsang branch) to 5 standard errors of the sample mean and the sample variance, computed from
    Beta(a, a)'s own moments (mean 1/2, variance 1 / (4 (2a + 1)), kurtosis 3 - 6 / (2a + 3)).  numpy.random.beta passes the same bounds:
    test_classifier_step_cpu.py::test_numpy_beta_passes_the_bounds_the_device_draw_is_held_to."""
    recs, perm, _ = draws(MIX, 8, 1024, 2024)
    cuts = sum(r.cut for r in recs)
    record_observed("mixup_draw.cut_count_of_1024", cuts)
    assert abs(cuts - 768) < 5 * np.sqrt(1024 * 0.75 * 0.25), cuts
    firsts = np.bincount(perm[:, 0], minlength=8)
    assert np.all(np.abs(firsts - 128) < 5 * np.sqrt(1024 * 0.125 * 0.875)), firsts
    for alpha in (0.4, 2.0):
        recs, _, _ = draws(dict(MIX, mixup_alpha=alpha, cutmix_alpha=0.0), 8, 1024, 777)
        lam = np.array([r.lam for r in recs], dtype=np.float64)
        assert all(r.cut == 0 and r.apply == 1 for r in recs) and lam.min() >= 0.0 and lam.max() <= 1.0
        mb, var, vb = mr.beta_moment_bounds(alpha, 1024)
        print(f"alpha {alpha}: mean {lam.mean():.5f} (0.5 +- {mb:.5f}), var {lam.var():.5f} ({var:.5f} +- {vb:.5f})")
        record_observed(f"mixup_draw.alpha{alpha}.mean_lam", lam.mean())
        record_observed(f"mixup_draw.alpha{alpha}.var_lam", lam.var())
        assert abs(lam.mean() - 0.5) < mb and abs(lam.var() - var) < vb, (alpha, lam.mean(), lam.var(), var)
    # only cutmix configured: every applied draw cuts
    recs, _, _ = draws(dict(MIX, mixup_alpha=0.0), 8, 16, 5)
    assert all(r.cut == 1 for r in recs)


def test_draw_host_checks():
    from focal_amd import ops
    from focal_amd._lib import FocalHipError
    state, rec = ops.new_rng_state(1, "cuda"), ops.new_mix_record("cuda")
    perm = torch.zeros(4097, dtype=torch.int32, device="cuda")
    for cfg, B, slots in ((MIX, 0, SLOTS), (MIX, 4097, SLOTS), (MIX, 8, [(10, 20)] * 9), (dict(MIX, mixup_alpha=0.0, cutmix_alpha=0.0), 8, SLOTS),
                          (dict(MIX, prob=1.5), 8, SLOTS), (MIX, 8, [(10, 0)])):
        with pytest.raises(FocalHipError):
            ops.mixup_draw(cfg, B, slots, state, STREAM, rec, perm)
    torch.cuda.synchronize()
    assert state.tolist() == [1, 0, 0, 0] and not rec.any().item()   # refused before anything ran


# ---------------------------------------------------------------------------------------------- 2. the mix pass
def ulp_of_larger(a, o):
    """One fp32 unit in the last place of max(|a|, |o|), per element."""
    v = torch.maximum(a.abs(), o.abs()).clamp_min(2.0 ** -100)
    # 2^(floor(log2 v) - 23), built from the exponent bits: the device's ldexp / pow are approximations, not exact powers of two
    return ((((v.view(torch.int32) >> 23) & 0xFF) - 23) << 23).view(torch.float32)


def _tensors(B, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(B, 1, 10, 1600, generator=g).cuda(), torch.randn(B, 1, 10, 20, generator=g).cuda()]


def test_mix_pass_equals_the_kernel_it_restates():
    """focal_mixup_multi (device record) against focal_mixup_fwd (host arguments) on the same tensors.  The CutMix paste and the
    copy-through are pure selects: bit for bit.  The blend is held to one ulp of max(|a|, |o|): at these sizes mixup_kernel runs its
    remainder loop, which the compiler left unfused (two products, one add), while focal_mixup_multi pins the product + fused
    multiply-add form of mixup_kernel's unrolled loop; observed: exactly 1 ulp at worst, on about a quarter of the elements
    (recorded as mixup_multi.blend.worst_diff_in_ulp_of_max_operand)."""
    from focal_amd import ops
    xs = _tensors(8, 11)
    rec, perm = ops.new_mix_record("cuda"), torch.zeros(8, dtype=torch.int32, device="cuda")
    ops.mixup_draw(dict(MIX, switch_prob=0.0), 8, SLOTS, ops.new_rng_state(4242, "cuda"), STREAM, rec, perm)   # a drawn blend
    drawn = ops.read_mix_record(rec)
    assert drawn.apply == 1 and drawn.cut == 0 and sorted(perm.tolist()) == list(range(8))
    cases = [("drawn", dict(apply=1, cut=0, lam=drawn.lam, boxes=[(0, 0, 0, 0)] * 2)),
             ("blend", dict(apply=1, cut=0, lam=0.3, boxes=[(0, 0, 0, 0)] * 2)),
             ("cut", dict(apply=1, cut=1, lam=0.6, boxes=[(2, 7, 100, 1101), (3, 9, 5, 17)])),
             ("cut_edge", dict(apply=1, cut=1, lam=0.2, boxes=[(0, 4, 1203, 1600), (6, 10, 0, 9)])),   # boxes clipped at an edge
             ("cut_empty", dict(apply=1, cut=1, lam=0.999, boxes=[(5, 5, 800, 800), (0, 0, 0, 0)])),
             ("miss", dict(apply=0, cut=0, lam=1.0, boxes=[(0, 0, 0, 0)] * 2))]
    worst_ulp = 0.0
    for tag, kw in cases:
        ops.write_mix_record(rec, **kw)
        got = ops.mixup_multi([dict(x=x, slot=i) for i, x in enumerate(xs)], rec, perm)
        for i, (x, y) in enumerate(zip(xs, got)):
            if not kw["apply"]:
                assert torch.equal(y, x), tag
                continue
            want = ops.mixup(x, perm, kw["lam"], kw["boxes"][i] if kw["cut"] else None)
            if kw["cut"]:
                assert torch.equal(y, want), (tag, i)   # pure selects
                if tag == "cut_empty":
                    assert torch.equal(y, x)
            else:
                worst_ulp = max(worst_ulp, ((y - want).abs() / ulp_of_larger(x, x[perm.long()])).max().item())
    record_observed("mixup_multi.blend.worst_diff_in_ulp_of_max_operand", worst_ulp)
    print("mixup_multi blend against focal_mixup_fwd: worst difference", worst_ulp, "ulp of max(|a|, |o|)")
    assert worst_ulp <= 1.0, worst_ulp
    # the scalar path: 3 * 5 * 7 values per sample
    x = torch.randn(3, 3, 5, 7, generator=torch.Generator().manual_seed(2)).cuda()
    p3 = torch.tensor([2, 0, 1], dtype=torch.int32, device="cuda")
    for kw in (dict(apply=1, cut=0, lam=0.7, boxes=[(0, 0, 0, 0)]), dict(apply=1, cut=1, lam=0.5, boxes=[(1, 4, 2, 7)]), dict(apply=0)):
        ops.write_mix_record(rec, **kw)
        (y,) = ops.mixup_multi([dict(x=x, slot=0)], rec, p3)
        if not kw["apply"]:
            assert torch.equal(y, x)
        elif kw["cut"]:
            assert torch.equal(y, ops.mixup(x, p3, kw["lam"], kw["boxes"][0]))
        else:
            want = ops.mixup(x, p3, kw["lam"], None)
            assert ((y - want).abs() <= ulp_of_larger(x, x[p3.long()])).all()


def test_mix_pass_clamps_a_hand_written_record():
    """perm entries outside [0, B) and boxes outside the tensor are clamped before they move a read: the result is the clamped
    restatement's, and the kernel reads nothing outside its tensors."""
    from focal_amd import ops
    xs = _tensors(8, 12)
    rec = ops.new_mix_record("cuda")
    perm = torch.tensor([-5, 100, 2, 7, 8, -1, 3, 2 ** 31 - 1], dtype=torch.int32, device="cuda")
    boxes = [(-3, 99, -1, 1000), (4, 2 ** 30, -(2 ** 30), 11)]
    ops.write_mix_record(rec, apply=1, cut=1, lam=0.5, boxes=boxes)
    got = ops.mixup_multi([dict(x=x, slot=i) for i, x in enumerate(xs)], rec, perm)
    for x, y, box in zip(xs, got, boxes):
        assert np.array_equal(y.cpu().numpy(), mr.mix(x.cpu().numpy(), perm.cpu().numpy(), 1, 1, 0.5, box))
    ops.write_mix_record(rec, apply=1, cut=0, lam=0.25, boxes=boxes)
    got = ops.mixup_multi([dict(x=x, slot=i) for i, x in enumerate(xs)], rec, perm)
    clamped = perm.clamp(0, 7)
    for x, y in zip(xs, got):
        want = ops.mixup(x, clamped, 0.25, None)
        assert ((y - want).abs() <= ulp_of_larger(x, x[clamped.long()])).all()


# ---------------------------------------------------------------------------------------------- the models
def build(cfg, model, ct, stage="supervised", **mix):
    from oracle.weights import fill_state_dict_
    c = no_dropout(cfg)
    c["mixup"].update(mix)
    args = make_args(c, model, torch.device("cuda"), ct)
    if stage == "supervised":
        args.train_mode, args.learn_framework = "supervised", "no"
    else:
        args.stage = "finetune"
    if model == "SW_Transformer":
        from models.SW_Transformer import SW_Transformer as Net
    else:
        from models.DeepSense import DeepSense as Net
    net = Net(args)
    fill_state_dict_(net.state_dict())
    return args, net.to("cuda").train()


def make_step(args, net, **kw):
    from focal_amd.graph_step import CapturedClassifierStep
    from general_utils.weight_utils import set_learnable_params_finetune
    from models.loss import CrossEntropyLoss
    from train_utils.optimizer import define_optimizer
    params = set_learnable_params_finetune(args, net) if args.stage == "finetune" else net.parameters()
    opt = define_optimizer(args, params)
    return CapturedClassifierStep(net, CrossEntropyLoss(), opt, **kw), opt


def windows(cfg, B, seed):
    g = torch.Generator().manual_seed(seed)
    return {loc: {mod: torch.randn(B, cfg["loc_mod_in_time_channels"][loc][mod], cfg["num_segments"], cfg["loc_mod_spectrum_len"][loc][mod],
                                   generator=g).cuda() for mod in cfg["modality_names"]} for loc in cfg["location_names"]}


@torch.no_grad()
def restore(net, opt, state0):
    """Parameters, buffers, moments and the step counter back to the seeded start, in place (bench.py --dump-outputs does the same)."""
    torch.cuda.synchronize()
    cur = net.state_dict()
    for k, v in state0.items():
        cur[k].copy_(v)
    for ar in opt._arenas():
        for t in ar.moments():
            t.zero_()
        ar.sync_shadow(force=True)
    if opt._step_state is not None:
        opt._step_state.zero_()
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- 3. the captured body against the fixtures
@pytest.mark.parametrize("model", ["SW_Transformer", "DeepSense"])
@pytest.mark.parametrize("ct", ["fp32", "bf16"])
def test_replayed_step_matches_reference_fixture(cfg, model, ct):
    """The tolerances tests/test_supervised_gpu.py asserts for the eager step, on a REPLAY from the seeded state."""
    from oracle.weights import synthetic_freq_input
    fx = np.load(os.path.join(GOLD, f"supervised_{model}_b8.npz"))
    args, net = build(cfg, model, ct)
    step, opt = make_step(args, net)
    state0 = {k: v.detach().clone() for k, v in net.state_dict().items()}
    x = {l: {m: v.cuda() for m, v in mm.items()} for l, mm in synthetic_freq_input(cfg, 8, seed=505).items()}
    labels = torch.from_numpy(fx["labels"]).cuda()
    names, norms = [str(n) for n in fx["train.grad_names"]], fx["train.grad_norms"]
    params = dict(net.named_parameters())
    eager_loss = step(x, labels).item()
    eager_norms = {n: params[n].grad.double().norm().item() for n in names}
    step(x, labels)
    assert step.replay is not None and (step.replays, step.eager_steps) == (0, 2), "the step was not captured"
    restore(net, opt, state0)
    loss = step(x, labels).item()
    torch.cuda.synchronize()
    assert step.replays == 1
    ref = torch.from_numpy(fx["train.logits"])
    e = ((step.segments.logits.cpu() - ref).abs().max() / ref.abs().max()).item()
    assert e < (1e-3 if ct == "fp32" else 3e-2), e
    assert abs(loss - float(fx["train.loss"])) < (1e-3 if ct == "fp32" else 2e-2) * max(1.0, float(fx["train.loss"]))
    bad, worst, vs_eager = [], 0.0, abs(loss - eager_loss) / max(1.0, abs(eager_loss))
    for n, r in zip(names, norms):
        g = params[n].grad
        got = g.double().norm().item()
        if n.endswith("conv.bias") and r < 1e-5:
            continue  # analytically zero in front of a train-mode BatchNorm
        rel = abs(got - r) / max(r, 1e-8)
        worst = max(worst, rel)
        vs_eager = max(vs_eager, abs(got - eager_norms[n]) / max(eager_norms[n], 1e-8))
        if rel > (2e-3 if ct == "fp32" else 6e-2):
            bad.append((n, got, r))
        if ct == "fp32":
            flat = g.detach().reshape(-1).cpu().double()
            mine = flat[::max(1, flat.numel() // 16)][:16]
            sl = torch.from_numpy(fx[f"train.gradslice.{n}"])
            assert (mine - sl).abs().max().item() < 2e-3 * max(sl.abs().max().item(), r / max(flat.numel() ** 0.5, 1), 1e-7) + 1e-7, n
    record_observed(f"classifier_step.{model}.{ct}.replay.grad_norm.worst_rel_err", worst)
    record_observed(f"classifier_step.{model}.{ct}.replay_vs_eager.worst_rel_diff", vs_eager)
    if ct == "fp32":
        assert not bad, bad[:6]
    else:
        assert len(bad) <= max(1, len(names) * 3 // 100), bad[:6]


# ---------------------------------------------------------------------------------------------- 4. steps replayed against eager
@pytest.mark.parametrize("model", ["SW_Transformer", "DeepSense"])
def test_replayed_steps_follow_the_eager_ones(cfg, model):
    """fp32, dropout off, the mix and phase coins forced to miss: four steps (two warm-up, two replays) against four eager ones from
    the same weights, on the same windows with DIFFERENT labels per step -- a replay that read stale labels would not follow."""
    from data_augmenter.Augmenter import Augmenter
    from focal_amd import runtime
    c = no_dropout(cfg)
    c["phase_shift"]["prob"] = 0.0
    runs = {}
    for graph in (False, True):
        args, net = build(c, model, "fp32", prob=0.0)
        aug = Augmenter(args)
        assert aug.fixed_device_draws_supported()
        runtime.view_state("cuda", seed=4321)
        step, _ = make_step(args, net, enabled=graph)
        losses = []
        for k in range(4):
            x = windows(c, 8, 900)
            labels = ((torch.arange(8) * 3 + k) % c["vehicle_classification"]["num_classes"]).cuda()
            losses.append(step.step_from_inputs(aug, x, labels, "fixed").item())
        torch.cuda.synchronize()
        assert (step.replays, step.eager_steps) == ((2, 2) if graph else (0, 4))
        runs[graph] = (losses, dict(net.named_parameters())["class_layer.0.weight"].detach().double().cpu().clone())
    (le, we), (lg, wg) = runs[False], runs[True]
    rel = max(abs(a - b) / max(1.0, abs(b)) for a, b in zip(lg, le))
    wrel = ((wg - we).norm() / we.norm()).item()
    record_observed(f"classifier_step.{model}.fp32.replayed_vs_eager.loss_rel", rel)
    record_observed(f"classifier_step.{model}.fp32.replayed_vs_eager.probe_weight_rel", wrel)
    assert len(set(round(v, 6) for v in le)) == 4, le   # the labels do change the loss
    assert rel < 1e-3 and wrel < 1e-3, (le, lg, wrel)


# ---------------------------------------------------------------------------------------------- 5. the same draws eager and replayed
def test_a_replay_draws_what_the_eager_pipeline_draws(cfg):
    from data_augmenter.Augmenter import Augmenter
    from focal_amd import ops, runtime
    args = make_args(cfg, "SW_Transformer", torch.device("cuda"))   # SW_Transformer's pipeline: mixup, then phase_shift
    args.train_mode, args.learn_framework = "supervised", "no"
    aug = Augmenter(args)
    x = windows(cfg, 8, 17)
    words = runtime.view_state("cuda", seed=2468)
    st = aug._fixed_state(x)
    assert st["draw_state"] is words

    def snapshot():
        torch.cuda.synchronize()
        return [st["rec"].clone(), st["perm"].clone(), st["plans"].clone()] + [st["out"][k].clone() for k in st["flat"]] + [words.clone()]
    out = aug.forward_fixed_device(x)
    assert all(out[l][m].data_ptr() == st["out"][(l, m)].data_ptr() for l, m in st["flat"])
    eager = snapshot()
    assert words.tolist()[1] == 2   # one advance by the mix draw, one by the phase draw
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            aug.forward_fixed_device(x)
    torch.cuda.synchronize()
    words.copy_(ops.new_rng_state(2468, "cuda"))
    graph.replay()
    replayed = snapshot()
    for a, b in zip(eager, replayed):
        assert torch.equal(a, b)
    graph.replay()
    again = snapshot()
    assert again[-1].tolist()[1] == 4 and not torch.equal(again[1], replayed[1])   # a replay draws anew
    rec = ops.read_mix_record(eager[0])
    want = mr.draw(2468, aug.FIXED_MIX_STREAM, cfg["mixup"], 8, [tuple(x[l][m].shape[2:]) for l, m in st["flat"]])
    assert (rec.apply, rec.cut) == (want["apply"], want["cut"]) and eager[1].tolist() == want["perm"].tolist()
    assert [list(b) for b in rec.box] == want["boxes"] and np.float32(rec.lam).tobytes() == want["lam"].tobytes()
    plans = ops.read_view_plans(eager[2])
    assert all(p.kind in (ops._lib.VIEW_NONE, ops._lib.VIEW_PHASE_SHIFT) for p in plans)
    # the spectra are those of the host-argument kernels on the drawn values
    mixed = [ops.mixup(x[l][m], eager[1], rec.lam, tuple(rec.box[i]) if rec.cut else None) for i, (l, m) in enumerate(st["flat"])]
    for i, (k, p) in enumerate(zip(st["flat"], plans)):
        ref = ops.fft_realpack(mixed[i], phase=float(np.arctan2(p.aug.phase_sin, p.aug.phase_cos)))
        assert (eager[3 + i] - ref).abs().max().item() <= 1e-4 * ref.abs().max().item(), k


# ---------------------------------------------------------------------------------------------- 6. shapes
@pytest.mark.parametrize("stage,model", [("supervised", "DeepSense"), ("finetune", "SW_Transformer")])
def test_odd_batch_runs_eagerly_and_the_next_one_replays(cfg, stage, model):
    from data_augmenter.Augmenter import Augmenter
    args, net = build(cfg, model, "bf16", stage=stage)
    aug = Augmenter(args)
    step, _ = make_step(args, net)
    before = {k: v.detach().clone() for k, v in net.state_dict().items()}
    counts = []
    for k, B in enumerate([16, 16, 16, 16, 8, 16]):
        labels = torch.randint(0, 7, (B,), generator=torch.Generator().manual_seed(k)).cuda()
        loss = step.step_from_inputs(aug, windows(cfg, B, 40 + k), labels, "fixed" if stage == "supervised" else "no")
        assert np.isfinite(loss.item())
        counts.append((step.replays, step.eager_steps))
        if k == 0:   # what ONE eager step advances
            first = {n: int(v) for n, v in net.state_dict().items() if n.endswith("num_batches_tracked")}
    assert counts == [(0, 1), (0, 2), (1, 2), (2, 2), (2, 3), (3, 3)], counts
    after = net.state_dict()
    moved = sorted(k for k in before if before[k].is_floating_point() and not torch.equal(before[k], after[k]))
    if stage == "finetune":   # the frozen encoders stay put under replay, the head moves
        learnable = sorted(n for n, p in net.named_parameters() if p.requires_grad)
        assert moved == learnable, (set(moved) ^ set(learnable))
    else:                     # BatchNorm under replay: every step, eager or replayed, advanced the counters and the running statistics
        # (six steps, three of them replays, moved every counter six times as far as the first eager step did: a counter that only the
        # eager steps advanced would stand at three times)
        per_step = {n: first[n] - int(before[n]) for n in first}
        assert per_step and max(per_step.values()) >= 1, per_step
        wrong = {n: (int(after[n]) - int(before[n]), d) for n, d in per_step.items() if int(after[n]) - int(before[n]) != 6 * d}
        assert not wrong, wrong
        assert any(k.endswith("running_mean") for k in moved)


# ---------------------------------------------------------------------------------------------- 7. train.py
def _train(*flags):
    r = subprocess.run([sys.executable, os.path.join(SRC, "train.py"), "-dataset=MOD", "-batch_size=16", *flags],
                       capture_output=True, text=True, timeout=900, cwd=SRC)
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-3000:]
    return log


def _counts(log):
    found = re.findall(r"(\d+) graph replays, (\d+) eager steps so far", log)
    assert found, log[-2000:]
    return int(found[-1][0]), int(found[-1][1])


def test_train_py_supervised_replays_and_no_graph_does_not():
    base = ["-model=DeepSense", "-learn_framework=no", "-synthetic_batches=4", "-epochs=2"]
    log = _train(*base)
    assert _counts(log) == (6, 2), _counts(log)
    for needle in ("Training loss:", "Val acc:", "fixed pipeline drawn on the device"):
        assert needle in log, (needle, log[-2000:])
    log = _train(*base, "-no_graph")
    assert "0 graph replays" in log and _counts(log) == (0, 8)
    assert "Training loss:" in log and "Val acc:" in log


def test_train_py_host_draws_replays_the_body_behind_the_eager_pipeline():
    log = _train("-model=DeepSense", "-learn_framework=no", "-synthetic_batches=4", "-epochs=1", "-host_draws")
    assert "fixed pipeline drawn on the host" in log and _counts(log) == (2, 2), _counts(log)
    log = _train("-model=DeepSense", "-learn_framework=no", "-synthetic_batches=4", "-epochs=1", "-host_draws", "-no_graph")
    assert "launched eagerly" in log and _counts(log) == (0, 4)
    assert "Training loss:" in log and "Val acc:" in log


def test_train_py_finetune_replays():
    base = ["-model=SW_Transformer", "-learn_framework=FOCAL", "-synthetic_batches=2"]
    _train(*base, "-epochs=1")   # the pretraining checkpoint the stage loads
    log = _train(*base, "-stage=finetune", "-epochs=2")
    replays, eager = _counts(log)
    assert replays >= 1 and replays + eager == 4, (replays, eager)
    assert "Training loss:" in log and "Val acc:" in log
