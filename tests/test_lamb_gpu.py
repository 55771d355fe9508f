"""LAMB on the device (focal_lamb_multi / _advance, ops.lamb_multi, optim.FocalLAMB) against a float64 restatement of its definition.

The reference.  No independent LAMB implementation is installed here (timm, apex and torch_optimizer are absent), so the comparison target
is `Lamb64` below: You et al. 2020, Algorithm 2, with AdamW's conventions, written from the formulas in float64 and sharing no code with the
kernels.  Per tensor T (one row of ParamArena.index inside the optimizer's span), t the step count:
    m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;  r = (m / (1 - b1^t)) / (sqrt(v / (1 - b2^t)) + eps);  u = r + lambda_T w
    phi_T = |w_T| / |u_T| if T is adapted and both norms are positive and finite, else 1;  phi_T = min(phi_T, max_trust);  w -= lr phi_T u
b1, b2, eps, lr and lambda enter as the float64 values of the fp32 numbers the kernels are handed (the hyper-parameters are fp32 inputs,
not results).

The bounds come from the number formats, u32 = 2^-24 the unit roundoff of fp32, and accumulate over the steps (each step adds its term):
    m, v:  2 u32 (|b old| + |(1 - b) new term|)          -- one rounding of each summand and one of the sum; 1 - b is exact in fp32
    w:     u32 (|w'| + K lr phi (|r| + lambda |w|))       -- the rounding of w' and K roundings' worth on the update lr phi u
    phi:   (K + 4) u32 phi per step taken so far          -- the two sums of squares (their depth twice halved by the roots), the roots, the
                                                             quotient and the 8 elementwise roundings of u; w, m and v carry the
                                                             earlier steps' errors into the norms, each step at most as much again;
                                                             exact (bound 0) where phi is the fallback 1 or clearly above the clamp
K = 8 + (elements one lane adds serially) + log2(256 * pieces of the largest tensor), from the kernels' summation as built:
    lamb_moments_kernel: one accumulator per lane over its FOCAL_LAMB_PIECE / 256 = 32 elements of the piece (8 float4), 6 levels across the
        wave, 2 across the four waves (a tree): log2(256) = 8;
    lamb_apply_kernel: lane l adds the partials of pieces first + l, first + l + 64, ...: one term each up to 64 pieces, then 6 levels of
        which ceil(log2(pieces)) see a non-zero term;
    8 for the elementwise roundings of u (1 / bc1, m / bc1, sqrt, its scaling, + eps, the quotient, lambda w + r) and of powf / rsqrtf.
Observed error / bound per quantity goes to record_observed (committed as tests/golden/OBSERVED_lamb.json)."""
import copy
import json
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
U32 = 2.0 ** -24
LR, WD, EPS, B1, B2 = 1e-2, 0.05, 1e-8, 0.9, 0.999


def f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


def piece():
    from focal_amd import _lib
    return _lib.LAMB_PIECE


# ------------------------------------------------------------------------------------------------ the float64 restatement
class Lamb64:
    def __init__(self, index, flat, lr, wd, exclude_1d, max_trust, lo=0, hi=None, b1=B1, b2=B2, eps=EPS):
        hi = flat.numel() if hi is None else hi
        self.rows = [(n, o, k, shp) for n, (o, k, shp) in index.items() if lo <= o < hi and k > 0]
        self.lo, self.hi = lo, hi
        self.w = flat.detach().double().clone()
        self.m, self.v = torch.zeros_like(self.w), torch.zeros_like(self.w)
        self.e_m, self.e_v, self.e_w = torch.zeros_like(self.w), torch.zeros_like(self.w), torch.zeros_like(self.w)
        self.lr, self.wd, self.b1, self.b2, self.eps = f32(lr), f32(wd), f32(b1), f32(b2), f32(eps)
        self.exclude_1d, self.max_trust = exclude_1d, f32(max_trust)
        self.t = 0
        P = piece()
        pieces = max(-(-((k + 7) // 8 * 8) // P) for _, _, k, _ in self.rows)
        self.K = 8 + P // 256 + math.log2(256 * pieces)
        self.phi, self.phi_bound, self.branches = {}, {}, set()

    def step(self, grad, lr=None):
        if lr is not None:
            self.lr = f32(lr)
        g = torch.zeros_like(self.w)
        g[self.lo:self.hi] = grad.detach().double()[self.lo:self.hi]
        self.t += 1
        b1, b2, t = self.b1, self.b2, self.t
        new_m, new_v = (1.0 - b1) * g, (1.0 - b2) * g * g
        self.e_m += 2.0 * U32 * ((b1 * self.m).abs() + new_m.abs())
        self.e_v += 2.0 * U32 * ((b2 * self.v).abs() + new_v.abs())
        inside = torch.zeros_like(self.w, dtype=torch.bool)
        inside[self.lo:self.hi] = True
        self.m = torch.where(inside, b1 * self.m + new_m, self.m)
        self.v = torch.where(inside, b2 * self.v + new_v, self.v)
        r = (self.m / (1.0 - b1 ** t)) / ((self.v / (1.0 - b2 ** t)).sqrt() + self.eps)
        for name, o, k, shp in self.rows:
            sl = slice(o, o + k)
            adapted = not (self.exclude_1d and len(shp) <= 1)
            lam = self.wd if adapted else 0.0
            w = self.w[sl]
            u = r[sl] + lam * w
            nw, nu = w.norm().item(), u.norm().item()
            if adapted and nw > 0.0 and nu > 0.0 and math.isfinite(nw) and math.isfinite(nu):
                phi = nw / nu
                branch = "below_one" if phi < 1.0 else "above_one"
            else:
                phi = 1.0
                branch = "not_adapted" if not adapted else ("w_zero" if nw == 0.0 else "u_zero")
            rel = self.t * (self.K + 4) * U32
            near_clamp = False
            if phi > self.max_trust:
                near_clamp = phi <= self.max_trust * (1.0 + rel)  # (fp32 may land just below the clamp)
                phi, branch = self.max_trust, "clamped"
            self.branches.add(branch)
            new_w = w - self.lr * phi * u
            self.e_w[sl] += U32 * (new_w.abs() + self.K * self.lr * phi * (r[sl].abs() + lam * w.abs()))
            self.w[sl] = new_w
            self.phi[name] = phi
            exact = branch in ("not_adapted", "w_zero", "u_zero") or (branch == "clamped" and not near_clamp)
            self.phi_bound[name] = 0.0 if exact else rel * phi


def worst(got, ref, bound):
    """max |got - ref| / bound over the elements; where the bound is zero (pad elements, untouched words) the values must agree exactly."""
    err = (got.detach().double() - ref).abs()
    zero = bound == 0
    if bool((err[zero] != 0).any()):
        return INF
    ratio = err[~zero] / bound[~zero]
    return float(ratio.max()) if ratio.numel() else 0.0


def check_against(ref, ar, phi, tag, step):
    m, v = ar.moments()
    for what, got, want, bound in (("m", m, ref.m, ref.e_m), ("v", v, ref.v, ref.e_v), ("w", ar.flat, ref.w, ref.e_w)):
        q = worst(got, want, bound)
        record_observed(f"lamb.{tag}.step{step}.{what}.err_over_bound", q)
        assert q <= 1.0, (tag, step, what, q)
    q = 0.0
    for name, want in ref.phi.items():
        err, bound = abs(phi[name] - want), ref.phi_bound[name]
        assert err <= bound, (tag, step, name, phi[name], want, bound)
        if bound > 0.0:
            q = max(q, err / bound)
    record_observed(f"lamb.{tag}.step{step}.phi.err_over_bound", q)


# ------------------------------------------------------------------------------------------------ the throw-away module
def toy_shapes():
    P = piece()
    return [("b1", (1,)), ("b3", (3,)), ("b8", (8,)), ("b255", (255,)), ("w75", (7, 5)), ("w_below", (2, (P - 8) // 2)), ("w_at", (2, P // 2)),
            ("w_above", (2, (P + 8) // 2)), ("w_four", (2, (3 * P + 8) // 2)), ("w_zero", (4, 6)), ("w_still", (4, 6)), ("w_large", (8, 8))]


class Toy(torch.nn.Module):
    """Twelve tensors, about 6 P elements: padded 1-D tails, a piece boundary at -1, 0 and +1 vector group, four pieces in one tensor, a zero
    weight, a weight whose gradient is zero, a small weight (phi < 1) and a large one (phi above 2)."""

    def __init__(self, seed=0, shapes=None):
        super().__init__()
        gen = torch.Generator().manual_seed(seed)
        for name, shp in (toy_shapes() if shapes is None else shapes):
            w = torch.randn(*shp, generator=gen)
            scale = {"w_zero": 0.0, "w75": 0.1, "w_large": 50.0}.get(name, 1.0)
            setattr(self, name, torch.nn.Parameter(w * scale))


def toy_arena(ct=torch.float32, seed=0, shapes=None):
    from focal_amd.arena import ParamArena
    net = Toy(seed, shapes).to(DEV)
    return net, ParamArena(net, lambda n: True, ct)


def toy_grads(ar, step, seed=0):
    """Seeded N(0, 0.1) gradients of one step over the real elements (pads stay zero); w_still's gradient is zero."""
    gen = torch.Generator().manual_seed(1000 * seed + step)
    g = torch.zeros(ar.size)
    for name, (o, k, _) in ar.index.items():
        if name != "w_still":
            g[o:o + k] = 0.1 * torch.randn(k, generator=gen)
    return g.to(DEV)


def make_opt(params, **kw):
    from focal_amd.optim import FocalLAMB
    kw.setdefault("lr", LR)
    kw.setdefault("weight_decay", WD)
    return FocalLAMB(list(params), betas=(B1, B2), eps=EPS, **kw)


def state_bits(ar, opt=None):
    m, v = ar.moments()
    out = [ar.flat.view(torch.int32).clone(), m.view(torch.int32).clone(), v.view(torch.int32).clone()]
    if ar.shadow is not None:
        out.append(ar.shadow.view(torch.int16).clone())
    if opt is not None:
        out += [t["record"].view(torch.int32).clone() for _, t in opt._tables.values()] + [opt._step_state.clone()]
    return out


def same_bits(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ 1. five steps against float64
@pytest.mark.parametrize("exclude_1d,max_trust,wd", [(True, INF, WD), (True, 2.0, WD), (False, INF, WD), (False, 2.0, WD), (True, INF, 0.0)])
def test_five_steps_against_float64(exclude_1d, max_trust, wd):
    net, ar = toy_arena()
    opt = make_opt(net.parameters(), weight_decay=wd, exclude_1d=exclude_1d, max_trust=max_trust)
    ref = Lamb64(ar.index, ar.flat, LR, wd, exclude_1d, max_trust)
    assert ref.K == 8 + 32 + 10  # 32 elements per lane, log2(256 * 4 pieces)
    tag = f"toy.exclude_{int(exclude_1d)}.trust_{max_trust:g}.wd_{wd:g}"
    for step in range(5):
        g = toy_grads(ar, step)
        ar.grad.copy_(g)
        opt.step()
        ref.step(g)
        torch.cuda.synchronize()
        assert torch.equal(ar.grad, g)  # the gradient is still the gradient
        stats = opt.trust_stats()
        check_against(ref, ar, stats["phi"], tag, step)
        if step == 0:
            assert (stats["phi"]["w_zero"] == 1.0) and (wd != 0.0 or stats["phi"]["w_still"] == 1.0)
    assert int(opt._step_state[1]) == 5 and int(opt._step_state[2:].abs().sum()) == 0
    # the float64 run went through every branch this parametrisation can reach
    want = {"below_one", "above_one", "w_zero"} | ({"not_adapted"} if exclude_1d else set()) | ({"clamped"} if max_trust == 2.0 else set()) | (
        {"u_zero"} if wd == 0.0 else set())
    assert want <= ref.branches, (want, ref.branches)
    if wd == 0.0:  # |u| = 0: the weight keeps its bits
        o, k, _ = ar.index["w_still"]
        assert torch.equal(ar.flat[o:o + k], Toy().w_still.reshape(-1).to(DEV))
    # the pad elements are zero in every buffer
    pad = torch.ones(ar.size, dtype=torch.bool, device=DEV)
    for o, k, _ in ar.index.values():
        pad[o:o + k] = False
    assert all(float(t[pad].abs().sum()) == 0.0 for t in (ar.flat, *ar.moments()))


# ------------------------------------------------------------------------------------------------ 2. shadow, repeatability
def test_shadow_is_the_rounded_master_and_two_runs_give_the_same_bits():
    runs = []
    for _ in range(2):
        net, ar = toy_arena(torch.bfloat16)
        opt = make_opt(net.parameters())
        for step in range(3):
            ar.grad.copy_(toy_grads(ar, step))
            opt.step()
            torch.cuda.synchronize()
            assert torch.equal(ar.shadow.view(torch.int16), ar.flat.bfloat16().view(torch.int16)), step  # round to nearest even
        runs.append(state_bits(ar, opt))
    assert same_bits(*runs)
    net, fresh = toy_arena(torch.bfloat16)
    assert not torch.equal(runs[0][0], fresh.flat.view(torch.int32))


# ------------------------------------------------------------------------------------------------ 3. span
def test_span_leaves_every_word_outside_it_alone():
    net, ar = toy_arena(torch.bfloat16)
    names = list(ar.index)
    mine = [ar.params[n] for n in names[-3:]]
    opt = make_opt(mine)
    lo, hi = opt._span(ar)
    assert lo == ar.index[names[-3]][0] and hi == ar.size and lo > 6 * piece() - 64
    m, v = ar.moments()
    poison, poison16 = 0x7FC0DEAD, 0x7FDE
    for t in (ar.flat, ar.grad, m, v):
        t.view(torch.int32)[:lo] = poison
    ar.shadow.view(torch.int16)[:lo] = poison16
    ref = Lamb64(ar.index, ar.flat, LR, WD, True, INF, lo, hi)
    for step in range(2):
        g = toy_grads(ar, step)
        ar.grad[lo:].copy_(g[lo:])
        opt.step()
        ref.step(ar.grad)
    torch.cuda.synchronize()
    for t in (ar.flat, ar.grad, m, v):
        assert bool((t.view(torch.int32)[:lo] == poison).all())
    assert bool((ar.shadow.view(torch.int16)[:lo] == poison16).all())
    stats = opt.trust_stats()
    assert sorted(stats["phi"]) == sorted(names[-3:])
    for what, got, want, bound in (("m", m, ref.m, ref.e_m), ("v", v, ref.v, ref.e_v), ("w", ar.flat, ref.w, ref.e_w)):
        assert worst(got[lo:], want[lo:], bound[lo:]) <= 1.0, what
    assert all(abs(stats["phi"][n] - ref.phi[n]) <= ref.phi_bound[n] for n in ref.phi)


# ------------------------------------------------------------------------------------------------ 4. advance
def _segment(ar):
    m, v = ar.moments()
    return (ar.flat, ar.grad, m, v, ar.shadow)


@pytest.mark.parametrize("clip", [False, True])
def test_advance_leaves_the_words_adamw_leaves(clip):
    from focal_amd import ops
    words = []
    for which in ("lamb", "adamw"):
        net, ar = toy_arena()
        ar.grad.copy_(toy_grads(ar, 0))
        step, seed = ops.new_step_state(DEV, count=3), ops.new_rng_state(99, DEV)
        lr = torch.full((1,), LR, device=DEV)
        st = None
        if clip:
            st = ops.new_clip_state(DEV)
            ops.grad_norm([ar.grad], st)
        kw = dict(advance=True, seed_state=seed, clip=(st, 1.0) if clip else None)
        if which == "lamb":
            tb = ops.lamb_table_upload(ops.lamb_table(ar.index.values(), 0, ar.size), DEV)
            ops.lamb_multi([_segment(ar)], [tb], lr, step, B1, B2, EPS, WD, **kw)
        else:
            ops.adamw_multi([_segment(ar)], lr, step, B1, B2, EPS, WD, **kw)
        torch.cuda.synchronize()
        words.append((step.clone(), seed.clone()))
    assert torch.equal(words[0][0], words[1][0]) and torch.equal(words[0][1], words[1][1])
    assert int(words[0][0][1]) == 4 and int(words[0][0][2:].abs().sum()) == 0 and int(words[0][1][1]) == 1


# ------------------------------------------------------------------------------------------------ 5. clipping
@pytest.mark.parametrize("ct", [torch.float32, torch.bfloat16])
def test_clipped_step_equals_the_plain_step_on_prescaled_gradients(ct):
    from focal_amd import ops
    net, a = toy_arena(ct)
    g = toy_grads(a, 0)
    norm64 = g.double().norm().item()
    a.grad.copy_(g)
    opt_a = make_opt(net.parameters(), max_grad_norm=0.5 * norm64)
    opt_a.step()
    s = opt_a.clip_stats()
    assert 0.4 < s["last_coef"] < 0.6 and (s["steps"], s["clipped"], s["skipped"]) == (1, 1, 0), s
    assert torch.equal(a.grad, g)
    net_b, b = toy_arena(ct)
    b.grad.copy_(g * torch.tensor(s["last_coef"], dtype=torch.float32, device=DEV))
    opt_b = make_opt(net_b.parameters())
    opt_b.step()
    torch.cuda.synchronize()
    assert same_bits(state_bits(a, opt_a), state_bits(b, opt_b))
    fresh = toy_arena(ct)[1]
    assert not torch.equal(a.flat, fresh.flat)


def test_a_non_finite_gradient_skips_the_step():
    net, ar = toy_arena(torch.bfloat16)
    opt = make_opt(net.parameters(), max_grad_norm=1.0)
    ar.grad.copy_(toy_grads(ar, 0))
    opt.step()
    torch.cuda.synchronize()
    before = state_bits(ar, opt)
    assert opt.clip_stats()["skipped"] == 0
    g = toy_grads(ar, 1)
    g[ar.index["w_four"][0] + 2 * piece() + 17] = INF
    ar.grad.copy_(g)
    opt.step()
    torch.cuda.synchronize()
    assert same_bits(state_bits(ar, opt), before)  # w, m, v, the shadow, the trust record and the step count
    s = opt.clip_stats()
    assert (s["steps"], s["clipped"], s["skipped"]) == (1, 0, 1) and int(opt._step_state[1]) == 1, s
    ar.grad.copy_(toy_grads(ar, 2))
    opt.step()
    torch.cuda.synchronize()
    assert int(opt._step_state[1]) == 2 and bool(torch.isfinite(ar.flat).all()) and not torch.equal(state_bits(ar)[0], before[0])


# ------------------------------------------------------------------------------------------------ 6. capture
def test_three_replays_equal_three_eager_steps():
    """One eager step (it builds and uploads the piece table, which a capture must not), then three more: eagerly on one arena, as three
    replays of one captured step() on the other, the gradients rewritten in place; the learning rate is halved before the last."""
    from focal_amd import runtime
    net_e, eager = toy_arena(torch.bfloat16)
    net_r, rep = toy_arena(torch.bfloat16)
    opt_e, opt_r = make_opt(net_e.parameters()), make_opt(net_r.parameters())
    grads = [toy_grads(eager, s) for s in range(4)]
    for ar, opt in ((eager, opt_e), (rep, opt_r)):
        ar.grad.copy_(grads[0])
        opt.step()
    for s in (1, 2, 3):
        if s == 3:
            opt_e.param_groups[0]["lr"] = 0.5 * LR
        eager.grad.copy_(grads[s])
        opt_e.step()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        # (step() joins every side stream the backbones ever made in this process, as it does inside a captured training step, where they
        # were forked from the capturing stream: fork them here too, so that the join stays inside the capture)
        for st in runtime._SIDE.values():
            st.wait_stream(side)
        opt_r.step()
    assert int(opt_r._step_state[1]) == 1  # a capture runs nothing
    after_two = None
    for s in (1, 2, 3):
        if s == 3:
            after_two = rep.flat.clone()
            opt_r.param_groups[0]["lr"] = 0.5 * LR
            opt_r.sync_lr()
        rep.grad.copy_(grads[s])
        graph.replay()
    torch.cuda.synchronize()
    assert same_bits(state_bits(rep, opt_r), state_bits(eager, opt_e))
    assert int(opt_r._step_state[1]) == 4
    # the halved rate took effect: the last step with the old rate lands somewhere else
    net_x, other = toy_arena(torch.bfloat16)
    opt_x = make_opt(net_x.parameters())
    for s in range(4):
        other.grad.copy_(grads[s])
        opt_x.step()
    torch.cuda.synchronize()
    assert not torch.equal(other.flat, rep.flat) and not torch.equal(after_two, rep.flat)


# ------------------------------------------------------------------------------------------------ 7. two arenas
def test_two_arenas_in_one_optimizer():
    P = piece()
    net_a, a = toy_arena(torch.bfloat16)
    net_b, b = toy_arena(torch.float32, seed=5, shapes=[("v75", (7, 5)), ("c3", (3,)), ("w_two", (2, (P + 16) // 2))])
    opt = make_opt(list(net_a.parameters()) + list(net_b.parameters()))
    refs = [Lamb64(ar.index, ar.flat, LR, WD, True, INF) for ar in (a, b)]
    for step in range(2):
        for ar, ref in zip((a, b), refs):
            g = toy_grads(ar, step, seed=ar.size)
            ar.grad.copy_(g)
            ref.step(g)
        opt.step()
    torch.cuda.synchronize()
    assert len(opt._tables) == 2 and int(opt._step_state[1]) == 2
    stats = opt.trust_stats()
    for tag, ar, ref in (("a", a, refs[0]), ("b", b, refs[1])):
        m, v = ar.moments()
        for what, got, want, bound in (("m", m, ref.m, ref.e_m), ("v", v, ref.v, ref.e_v), ("w", ar.flat, ref.w, ref.e_w)):
            assert worst(got, want, bound) <= 1.0, (tag, what)
        assert all(abs(stats["phi"][n] - ref.phi[n]) <= ref.phi_bound[n] for n in ref.phi), tag
    assert len(stats["phi"]) == len(a.index) + len(b.index)
    assert torch.equal(a.shadow.view(torch.int16), a.flat.bfloat16().view(torch.int16)) and b.shadow is None


# ------------------------------------------------------------------------------------------------ 8. model level
def _model(cfg, model, ct, **keys):
    from models.FOCALModules import FOCAL
    from models.loss import FOCALLoss
    from oracle.weights import fill_state_dict_, synthetic_freq_input
    from train_utils.optimizer import define_optimizer
    c = copy.deepcopy(no_dropout(cfg))
    c["FOCAL"]["pretrain_optimizer"]["name"] = "LAMB"
    c["FOCAL"]["pretrain_optimizer"].update(keys)
    args = make_args(c, model, torch.device("cuda"), ct)
    if model == "DeepSense":
        from models.DeepSense import DeepSense as Net
    else:
        from models.SW_Transformer import SW_Transformer as Net
    net = Net(args)
    fill_state_dict_(net.state_dict())
    net = net.to("cuda")
    focal = FOCAL(args, net)
    to = lambda d: {l: {m: v.cuda() for m, v in mm.items()} for l, mm in d.items()}
    x = to(synthetic_freq_input(cfg, 8, seed=101)), to(synthetic_freq_input(cfg, 8, seed=202))
    return args, net, focal, FOCALLoss(args), define_optimizer(args, focal.parameters()), x


@pytest.mark.parametrize("model,ct", [("DeepSense", "fp32"), ("DeepSense", "bf16"), ("SW_Transformer", "fp32")])
def test_model_steps_equal_the_restatement_on_the_same_gradients(cfg, model, ct):
    """tests/test_clip_grad_gpu.py::test_clipped_optimizer_equals_torch_clip_and_adamw_on_the_same_gradients with LAMB: MOD, B = 8, three FOCAL
    steps through define_optimizer (`name: LAMB`); after each step the masters agree with Lamb64 on a clone of the arena fed the HIP path's
    own gradients, within the bounds of the module docstring."""
    from focal_amd.optim import FocalLAMB
    args, net, focal, loss_fn, opt, (x1, x2) = _model(cfg, model, ct)
    assert type(opt) is FocalLAMB and opt.exclude_1d and opt.max_trust == INF
    net.train()
    oc = cfg["FOCAL"]["pretrain_optimizer"]
    ref = None
    for it in range(3):
        opt.zero_grad()
        a, b = focal(x1, x2, proj_head=True)
        loss = loss_fn(a, b)
        loss.backward()
        torch.cuda.synchronize()
        ar = net.arena()
        if ref is None:
            wd = oc["weight_decay"][model] if isinstance(oc["weight_decay"], dict) else oc["weight_decay"]
            ref = Lamb64(ar.index, ar.flat, oc["start_lr"], wd, True, INF)
        g = ar.grad.detach().clone()
        opt.step()
        ref.step(g)
        torch.cuda.synchronize()
        assert math.isfinite(loss.item())
        stats = opt.trust_stats()
        check_against(ref, ar, stats["phi"], f"{model}.{ct}", it)
        assert stats["min_name"] in ar.index and stats["max_name"] in ar.index and stats["min"] <= stats["median"] <= stats["max"]
        assert stats["tensors"] == sum(len(shp) > 1 for _, k, shp in ar.index.values() if k > 0)
        if ct == "bf16":
            assert torch.equal(ar.shadow, ar.flat.bfloat16())
    assert len(ar.index) > (200 if model == "SW_Transformer" else 50) and int(opt._step_state[1]) == 3


# ------------------------------------------------------------------------------------------------ 9. resume
def test_resume_continues_bit_for_bit():
    net_a, a = toy_arena(torch.bfloat16)
    opt_a = make_opt(net_a.parameters())
    for s in range(4):
        a.grad.copy_(toy_grads(a, s))
        opt_a.step()
    net_b, b = toy_arena(torch.bfloat16)
    opt_b = make_opt(net_b.parameters())
    for s in range(2):
        b.grad.copy_(toy_grads(b, s))
        opt_b.step()
    state, weights = opt_b.train_state(), {k: v.detach().cpu().clone() for k, v in net_b.state_dict().items()}
    assert state["step"] == 2
    net_c = Toy(seed=3)
    net_c.load_state_dict(weights)
    from focal_amd.arena import ParamArena
    net_c = net_c.to(DEV)
    c = ParamArena(net_c, lambda n: True, torch.bfloat16)
    opt_c = make_opt(net_c.parameters())
    opt_c.load_train_state(state)
    for s in (2, 3):
        c.grad.copy_(toy_grads(c, s))
        opt_c.step()
    torch.cuda.synchronize()
    assert same_bits(state_bits(c), state_bits(a)) and int(opt_c._step_state[1]) == 4
    assert torch.equal(opt_c._step_state[1], opt_a._step_state[1])


# ------------------------------------------------------------------------------------------------ 10. the captured training step
def test_captured_training_step_matches_eager():
    """graph_step's pretraining step with FocalLAMB (DeepSense, MOD, B = 8), as tests/test_deepsense_evenk_gpu.py::
    test_captured_step_matches_eager states it for AdamW: three steps at learning rate 0 on fixed views in a child process
    (tests/lamb_capture_worker.py), eager and captured -- same loss to 1e-5, same arena gradients to 1e-5 of scale, two replays agree."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "lamb_capture_worker.py")], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["optimizer"] == "FocalLAMB" and out["replays"] >= 1 and len(out["steps"]) == 3 and out["step_count"] == [3, 3]
    for le, lr, e in out["steps"]:
        assert math.isfinite(le) and abs(le - lr) <= 1e-5 * abs(le), (le, lr)
        record_observed("lamb.graph_vs_eager.grad_rel", e)
        assert e <= 1e-5, e  # (not bit-identical: the weight-gradient GEMMs accumulate with fp32 atomics in any order)
    assert abs(out["steps"][1][1] - out["steps"][2][1]) <= 1e-6 * abs(out["steps"][1][1])
    assert out["trust"]["tensors"] > 0 and out["trust"]["min"] > 0.0 and out["weights_moved"] is False
