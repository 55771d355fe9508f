"""The GRU kernels (gru.hip) and the small helpers of gru.hip / head.hip against plain float64 references of the same operation.

Whole-sequence kernels: reference A is oracle/gru.py with the kernels' one deliberate approximation (W_hh in bf16, the operand of
every recurrent product rounded to bf16), evaluated in float64.  The tolerance of each case comes from references alone: d is the
relative L2 distance between A and the same recurrence WITHOUT the operand rounding (B); a tensor must agree with A to
max(0.5 d, 2e-6) as a whole and to max(1.5 d, 2e-6) for every single sample.  0.5 d (2.4e-4 at T = 10) is half of what omitting the
rounding costs and about 4 times what an fp32 evaluation of A differs from float64 on the CPU (at most 5.7e-5; that spread comes from
bf16 roundings that flip between fp32 and float64); one sample reached 3.0e-4 from such flips, against 1.5 d = 7e-4.  2e-6 is the
floor for T = 1, where no recurrent product happens and d = 0.  tests/test_gru_reference_cpu.py pins the reference to torch.nn.GRU
and shows the rule on the CPU.  Every observed error goes to conftest.record_observed (gru.seq.<case>.<tensor>.rel_l2, next to it the
tensor's d as .d_ref and the worst single sample as .worst_sample_rel_l2).

The backward kernel is fed reference A's hs / save (cast to fp32), so a forward error can neither mask nor cause a backward one, and
its d toggles the rounding of the dgh operand alone.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from oracle.gru import gru_seq_backward_reference, gru_seq_reference

pytestmark = pytest.mark.gpu

DEV = "cuda"


def rel_l2(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def rel_err(a, b):
    return rel_l2(a, b)


def worst_sample(a, b, bdim):
    """Largest relative L2 error over everything that belongs to one sample (dimension `bdim`)."""
    a = a.detach().cpu().double().movedim(bdim, 0).flatten(1)
    b = b.detach().cpu().double().movedim(bdim, 0).flatten(1)
    return ((a - b).norm(dim=1) / b.norm(dim=1).clamp_min(1e-30)).max().item()


def cpu_rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


@pytest.fixture(scope="module")
def ops():
    from focal_amd import ops as o
    return o


# ------------------------------------------------------------------------------------------ whole-sequence kernels
# (B, H, T, directions): the smallest shapes that reach each branch of gru_twins and the launchers.
#   "both": forward and reverse in one launch; "first": n_dir = 1; "first_swapped": n_dir = 1 with the REVERSE direction's tensors as
#   the only direction -- blockIdx.y, not the tensor, decides the direction, so the reference runs them forward.
SEQ_CASES = [
    (5, 256, 10, "both"),             # twin form (two lanes per sample, 8 samples a workgroup); B below one workgroup; clamped spare lanes
    (43, 256, 10, "both"),            # twin form; ragged last workgroup
    (64, 256, 10, "first"),           # ceil(64/8) * 1 = 8 <= 128: twin form, one direction
    (64, 256, 10, "first_swapped"),
    (520, 256, 10, "both"),           # ceil(520/8) * 2 = 130 > 128: 16-sample form at its smallest B; ragged (520 = 32 * 16 + 8)
    (1032, 256, 10, "first"),         # ceil(1032/8) = 129 > 128: 16-sample form through the one-direction condition
    (19, 128, 10, "both"),            # H = 128; ragged
    (16, 128, 3, "both"),             # H = 128; T != 10
    (3, 256, 1, "both"),              # T = 1: first and last step coincide; the prefetch clamps
    (3, 128, 1, "both"),
]
FORMS = ["layer0", "last"]  # the two upstream forms of deepsense_engine.backward


def case_id(case):
    return "b%d_h%d_t%d_%s" % case


def _dirs(mode):
    """[(index of the direction's data set, reverse)] for the launch."""
    return {"both": [(0, False), (1, True)], "first": [(0, False)], "first_swapped": [(1, False)]}[mode]


@functools.lru_cache(maxsize=None)
def _inputs(case):
    B, H, T, _ = case
    return dict(gi=[cpu_rnd(B * T, 3 * H, seed=300 + d) for d in range(2)],
                whh=[cpu_rnd(3 * H, H, scale=H ** -0.5, seed=310 + d) for d in range(2)],
                bhh=[cpu_rnd(3 * H, scale=0.1, seed=320 + d) for d in range(2)],
                dout=cpu_rnd(B * T, 2 * H, seed=330), dfeat=cpu_rnd(B, 2 * H, seed=331))


@functools.lru_cache(maxsize=None)
def _fwd_ref(case):
    """Reference A of every direction of the launch (float64) and d = rel L2 (B, A) per tensor.  Computed once per case."""
    B, H, T, mode = case
    inp = _inputs(case)
    A, outB, d = [], [], {}
    for k, (di, reverse) in enumerate(_dirs(mode)):
        a = gru_seq_reference(inp["gi"][di], inp["whh"][di], inp["bhh"][di], T, reverse, torch.float64, True)
        b = gru_seq_reference(inp["gi"][di], inp["whh"][di], inp["bhh"][di], T, reverse, torch.float64, False)
        A.append(a)
        outB.append(b[0])
        d[f"hs.d{k}"] = rel_l2(b[1][1:], a[1][1:])
        d[f"save.d{k}"] = rel_l2(b[2], a[2])
    out = torch.cat([a[0] for a in A], 2)
    d["out"] = rel_l2(torch.cat(outB, 2), out)
    return dict(A=A, out=out, d=d)


@functools.lru_cache(maxsize=None)
def _bwd_ref(case, form):
    """Backward reference A from reference A's forward state as the kernel gets it (cast to fp32), and d per tensor."""
    B, H, T, mode = case
    inp, fw = _inputs(case), _fwd_ref(case)
    res = []
    for k, (di, reverse) in enumerate(_dirs(mode)):
        if form == "layer0":
            up, scale = inp["dout"].view(B, T, 2 * H)[:, :, k * H:(k + 1) * H], 1.0
        else:
            up, scale = inp["dfeat"][:, None, k * H:(k + 1) * H].expand(B, T, H), 1.0 / T
        hs32, save32 = fw["A"][k][1].float(), fw["A"][k][2].float()
        a = gru_seq_backward_reference(up, scale, inp["whh"][di], hs32, save32, T, reverse, torch.float64, True)
        b = gru_seq_backward_reference(up, scale, inp["whh"][di], hs32, save32, T, reverse, torch.float64, False)
        res.append(dict(dgi=a[0], dgh=a[1], d_dgi=rel_l2(b[0], a[0]), d_dgh=rel_l2(b[1], a[1])))
    return res


class Judge:
    """Records every figure of a case first, asserts afterwards: a failing tensor does not hide the others' numbers."""

    def __init__(self, cid):
        self.cid, self.fails = cid, []

    def check(self, name, got, ref, d, bdim):
        from conftest import record_observed
        got = got.detach().cpu()
        e = rel_l2(got, ref) if not torch.isnan(got).any() else float("inf")
        ps = worst_sample(got, ref, bdim) if e != float("inf") else float("inf")
        bound, bound_ps = max(0.5 * d, 2e-6), max(1.5 * d, 2e-6)
        key = f"gru.seq.{self.cid}.{name}"
        record_observed(key + ".rel_l2", e)
        record_observed(key + ".worst_sample_rel_l2", ps)
        record_observed(key + ".d_ref", d)
        print(f"{key}: rel_l2 {e:.3e} (bound {bound:.3e})  worst sample {ps:.3e} (bound {bound_ps:.3e})  d {d:.3e}")
        if not e < bound:
            self.fails.append(f"{key}: rel L2 {e:.3e} >= {bound:.3e}")
        if not ps < bound_ps:
            self.fails.append(f"{key}: worst sample {ps:.3e} >= {bound_ps:.3e}")

    def done(self):
        assert not self.fails, "\n".join(self.fails)


def _run_fwd(ops, case, frag=False):
    B, H, T, mode = case
    inp = _inputs(case)
    sel = [di for di, _ in _dirs(mode)]
    gi = [inp["gi"][di].to(DEV) for di in sel]
    bhh = [inp["bhh"][di].to(DEV) for di in sel]
    if frag:
        whh = [torch.empty(3 * H * H, dtype=torch.bfloat16, device=DEV) for _ in sel]
        ops.pack_multi([(inp["whh"][di].to(DEV), w, 3 * H, H, 1, ops.PACK_FRAG) for di, w in zip(sel, whh)], torch.bfloat16)
    else:
        whh = [inp["whh"][di].to(DEV).bfloat16() for di in sel]
    out = nan(B, T, 2 * H)
    hs = [nan(T + 1, B, H) for _ in sel]
    save = [nan(T, 4, B, H) for _ in sel]
    ops.gru_seq_fwd(ops.GRUDesc(B, T, H, 1 if frag else 0), gi, whh, bhh, hs, save, out)
    torch.cuda.synchronize()
    return out, hs, save


def _run_bwd(ops, case, form, frag=False):
    B, H, T, mode = case
    inp, fw = _inputs(case), _fwd_ref(case)
    sel = [di for di, _ in _dirs(mode)]
    hs = [a[1].float().to(DEV) for a in fw["A"]]
    save = [a[2].float().to(DEV) for a in fw["A"]]
    if frag:
        whh_t = [torch.empty(3 * H * H, dtype=torch.bfloat16, device=DEV) for _ in sel]
        ops.pack_multi([(inp["whh"][di].to(DEV), w, 3 * H, H, 1, ops.PACK_FRAG_T) for di, w in zip(sel, whh_t)], torch.bfloat16)
    else:
        whh_t = [ops.permute_pack(inp["whh"][di].to(DEV), 1, 3 * H, H, torch.bfloat16) for di in sel]
    if form == "layer0":
        dout, ld_b, ld_t, scale = inp["dout"].to(DEV), T * 2 * H, 2 * H, 1.0
    else:
        dout, ld_b, ld_t, scale = inp["dfeat"].to(DEV), 2 * H, 0, 1.0 / T
    dgi = [nan(B * T, 3 * H) for _ in sel]
    dgh = [nan(T, B, 3 * H) for _ in sel]
    ops.gru_seq_bwd(ops.GRUDesc(B, T, H, 1 if frag else 0), dout, ld_b, ld_t, scale, whh_t, hs, save, dgi, dgh)
    torch.cuda.synchronize()
    return dgi, dgh


@pytest.mark.parametrize("case", SEQ_CASES, ids=case_id)
def test_gru_seq_fwd_against_float64_reference(ops, case):
    B, H, T, mode = case
    ref = _fwd_ref(case)
    out, hs, save = _run_fwd(ops, case)
    nd = len(ref["A"])
    j = Judge(case_id(case))
    j.check("out", out[:, :, :nd * H], ref["out"], ref["d"]["out"], 0)
    for k in range(nd):
        j.check(f"hs.d{k}", hs[k][1:], ref["A"][k][1][1:], ref["d"][f"hs.d{k}"], 1)
        j.check(f"save.d{k}", save[k], ref["A"][k][2], ref["d"][f"save.d{k}"], 2)
        assert torch.isnan(hs[k][0]).all()  # h_0 is the caller's (zeros in the engine): the kernel starts from 0 without reading or writing it
    if nd == 1:  # one direction: blockIdx.y = 0 writes columns [0, H) and nothing else
        assert torch.isnan(out[:, :, H:]).all()
    j.done()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", SEQ_CASES, ids=case_id)
def test_gru_seq_bwd_against_float64_reference(ops, case, form):
    B, H, T, mode = case
    ref = _bwd_ref(case, form)
    dgi, dgh = _run_bwd(ops, case, form)
    j = Judge(case_id(case))
    for k, r in enumerate(ref):
        j.check(f"dgi.d{k}.{form}", dgi[k].view(B, T, 3 * H), r["dgi"], r["d_dgi"], 0)
        j.check(f"dgh.d{k}.{form}", dgh[k], r["dgh"], r["d_dgh"], 1)
    j.done()


@pytest.mark.parametrize("case", [(43, 256, 10, "both"), (19, 128, 10, "both")], ids=case_id)
def test_gru_seq_fragment_order_operands_are_bit_identical(ops, case):
    """W_hh / W_hh^T handed over in MFMA-fragment order (GRUDesc whh_frag = 1): the same fragments in the same registers."""
    out, hs, save = _run_fwd(ops, case)
    out_f, hs_f, save_f = _run_fwd(ops, case, frag=True)
    assert not torch.isnan(out).any() and torch.equal(out_f, out)
    for k in range(2):
        assert torch.equal(hs_f[k][1:], hs[k][1:]) and torch.equal(save_f[k], save[k])
    for form in FORMS:
        dgi, dgh = _run_bwd(ops, case, form)
        dgi_f, dgh_f = _run_bwd(ops, case, form, frag=True)
        for k in range(2):
            assert not torch.isnan(dgi[k]).any() and not torch.isnan(dgh[k]).any()
            assert torch.equal(dgi_f[k], dgi[k]) and torch.equal(dgh_f[k], dgh[k])


def test_gru_seq_refuses_unsupported_hidden_size(ops):
    """H = 64: the library's unsupported error (FOCAL_EUNSUPPORTED = -2) as the exception ops.check raises, before any launch."""
    from focal_amd._lib import FocalHipError
    B, T, H = 4, 3, 64
    gd = ops.GRUDesc(B, T, H)
    z = lambda *s: torch.zeros(*s, device=DEV)
    w = torch.zeros(3 * H, H, dtype=torch.bfloat16, device=DEV)
    out, hs, save = nan(B, T, 2 * H), nan(T + 1, B, H), nan(T, 4, B, H)
    with pytest.raises(FocalHipError, match=r"error -2: gru_seq_fwd: hidden size 64"):
        ops.gru_seq_fwd(gd, [z(B * T, 3 * H)], [w], [z(3 * H)], [hs], [save], out)
    dgi, dgh = nan(B * T, 3 * H), nan(T, B, 3 * H)
    with pytest.raises(FocalHipError, match=r"error -2: gru_seq_bwd: hidden size 64"):
        ops.gru_seq_bwd(gd, z(B * T, 2 * H), T * 2 * H, 2 * H, 1.0, [w.view(H, 3 * H)], [z(T + 1, B, H)], [z(T, 4, B, H)], [dgi], [dgh])
    torch.cuda.synchronize()
    for t in (out, hs, save, dgi, dgh):
        assert torch.isnan(t).all()


# ------------------------------------------------------------------------------------------ per-step gate kernels
def _gate_fwd_ref(gi, gh, h_prev, t):
    H = gh.shape[1] // 3
    g, gh = gi.double()[:, t], gh.double()
    r = torch.sigmoid(g[:, :H] + gh[:, :H])
    z = torch.sigmoid(g[:, H:2 * H] + gh[:, H:2 * H])
    ghn = gh[:, 2 * H:]
    n = torch.tanh(g[:, 2 * H:] + r * ghn)
    h = (1 - z) * n + (z * h_prev.double() if h_prev is not None else 0)
    return h, torch.stack([r, z, n, ghn])


def _gate_bwd_ref(up, scale, dh_rec, dhz_in, save, h_prev):
    r, z, n, ghn = save.double()
    dh = scale * up.double()
    if dh_rec is not None:
        dh = dh + dh_rec.double() + dhz_in.double()
    hp = h_prev.double() if h_prev is not None else 0
    dn = dh * (1 - z) * (1 - n * n)
    dz = dh * (hp - n) * z * (1 - z)
    dr = dn * ghn * r * (1 - r)
    return torch.cat([dr, dz, dn], 1), torch.cat([dr, dz, dn * r], 1), dh * z


def _fp32_close(got, ref):
    """(relative L2, max element error / max |ref|) of an fp32 element-wise kernel against float64."""
    got, ref = got.detach().cpu().double(), ref.double()
    assert not torch.isnan(got).any()
    return rel_l2(got, ref), ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


@pytest.mark.parametrize("B,H", [(7, 256), (300, 128), (33, 96)])
def test_gru_gate_kernels_against_float64(ops, B, H):
    """focal_gru_gate_fwd / _bwd: element-wise fp32 (libm tanhf, IEEE divide), no matrix product when gh is given.  Every output against
    the float64 formula on the same fp32 inputs; rows of out / dgi at other times keep their NaN pre-fill."""
    from conftest import record_observed
    T = 4
    gd = ops.GRUDesc(B, T, H)
    gi, gh, hp = cpu_rnd(B, T, 3 * H, seed=400), cpu_rnd(B, 3 * H, seed=401), cpu_rnd(B, H, scale=0.5, seed=402)
    gi_d, gh_d, hp_d = gi.to(DEV), gh.to(DEV), hp.to(DEV)
    worst = dict(fwd=[0.0, 0.0], bwd=[0.0, 0.0])

    def note(kind, got, ref):
        e, m = _fp32_close(got, ref)
        worst[kind] = [max(worst[kind][0], e), max(worst[kind][1], m)]

    for t in (0, T - 1):
        for dir_off in (0, H):
            for h_prev in (None, hp):
                h_new, out, save = nan(B, H), nan(B, T, 2 * H), nan(4, B, H)
                ops.gru_gate_fwd(gd, t, dir_off, gi_d.view(B * T, 3 * H), gh_d, None if h_prev is None else hp_d, h_new, out, save)
                h_ref, save_ref = _gate_fwd_ref(gi, gh, h_prev, t)
                written = torch.zeros(B, T, 2 * H, dtype=torch.bool)
                written[:, t, dir_off:dir_off + H] = True
                assert torch.equal(torch.isnan(out).cpu(), ~written)
                note("fwd", h_new, h_ref)
                note("fwd", out[:, t, dir_off:dir_off + H], h_ref)
                for k in range(4):
                    note("fwd", save[k], save_ref[k])
    save = _gate_fwd_ref(gi, gh, hp, 1)[1].float()  # a consistent set of saved gate values
    save_d = save.to(DEV)
    dout, dfeat = cpu_rnd(B, T, 2 * H, seed=403), cpu_rnd(B, 2 * H, seed=404)
    rec, dhz_in = cpu_rnd(B, H, seed=405), cpu_rnd(B, H, seed=406)
    forms = [(dout.to(DEV), T * 2 * H, 2 * H, lambda t, o: dout[:, t, o:o + H]), (dfeat.to(DEV), 2 * H, 0, lambda t, o: dfeat[:, o:o + H])]
    for t in (0, T - 1):
        for dir_off in (0, H):
            for h_prev in (None, hp):
                for carry in (False, True):
                    for up_d, ld_b, ld_t, pick in forms:
                        for scale in (1.0, 1.0 / T):
                            dgi, dgh, dhz = nan(B, T, 3 * H), nan(B, 3 * H), nan(B, H)
                            ops.gru_gate_bwd(gd, t, dir_off, up_d, ld_b, ld_t, scale, rec.to(DEV) if carry else None,
                                             dhz_in.to(DEV) if carry else None, save_d, None if h_prev is None else hp_d, dgi.view(B * T, 3 * H),
                                             dgh, dhz)
                            r_dgi, r_dgh, r_dhz = _gate_bwd_ref(pick(t, dir_off), scale, rec if carry else None, dhz_in if carry else None,
                                                                save, h_prev)
                            written = torch.zeros(B, T, 3 * H, dtype=torch.bool)
                            written[:, t] = True
                            assert torch.equal(torch.isnan(dgi).cpu(), ~written)
                            note("bwd", dgi[:, t], r_dgi)
                            note("bwd", dgh, r_dgh)
                            note("bwd", dhz, r_dhz)
    for kind in ("fwd", "bwd"):
        record_observed(f"gru.gate.b{B}_h{H}.{kind}.rel_l2", worst[kind][0])
        record_observed(f"gru.gate.b{B}_h{H}.{kind}.max_err_over_max_ref", worst[kind][1])
        print(f"gru.gate.b{B}_h{H}.{kind}: rel_l2 {worst[kind][0]:.3e}  max err / max |ref| {worst[kind][1]:.3e}")
    for kind in ("fwd", "bwd"):
        assert worst[kind][0] < 2e-6 and worst[kind][1] < 1e-5, (kind, worst[kind])


def test_gru_fp32_per_step_path_against_torch_gru_float64(ops):
    """The engine's fp32 mode: per step one fp32 GEMM (focal_linear_fwd, fp32 operands) and the gate kernel, backward the gate kernel and
    focal_linear_bwd_data -- both directions, against torch.nn.GRU in float64 with the unrounded weights.  nn.GRU's input projection
    is set to the identity, so its input is gi and the input's gradient is dgi; dgh (per step, which nn.GRU does not expose) comes
    from oracle/gru.py without any rounding, whose forward is checked against nn.GRU here as well."""
    from conftest import record_observed
    B, H, T = 12, 256, 4
    f32c = ops.code(torch.float32)
    gd = ops.GRUDesc(B, T, H)
    d_hh = ops.linear_desc(f32c, B, 3 * H, H, f32c, f32c)
    gi = [cpu_rnd(B * T, 3 * H, seed=500 + d) for d in range(2)]
    whh = [cpu_rnd(3 * H, H, scale=H ** -0.5, seed=510 + d) for d in range(2)]
    bhh = [cpu_rnd(3 * H, scale=0.1, seed=520 + d) for d in range(2)]
    dout = cpu_rnd(B * T, 2 * H, seed=530)
    gru = torch.nn.GRU(3 * H, H, batch_first=True, bidirectional=True).double()
    with torch.no_grad():
        for d, suf in enumerate(("", "_reverse")):
            getattr(gru, f"weight_ih_l0{suf}").copy_(torch.eye(3 * H, dtype=torch.float64))
            getattr(gru, f"bias_ih_l0{suf}").zero_()
            getattr(gru, f"weight_hh_l0{suf}").copy_(whh[d].double())
            getattr(gru, f"bias_hh_l0{suf}").copy_(bhh[d].double())
    out = nan(B, T, 2 * H)
    dout_d = dout.to(DEV)
    figures = {}
    for di in range(2):
        gi_d, w_d, b_d = gi[di].to(DEV), whh[di].to(DEV), bhh[di].to(DEV)
        hs = torch.zeros(T + 1, B, H, device=DEV)
        save = nan(T, 4, B, H)
        gh = nan(B, 3 * H)
        for s in range(T):
            t = s if di == 0 else T - 1 - s
            ops.linear_fwd(d_hh, hs[s], w_d, b_d, None, gh)
            ops.gru_gate_fwd(gd, t, di * H, gi_d, gh, hs[s], hs[s + 1], out, save[s])
        dgi, dgh = nan(B * T, 3 * H), nan(T, B, 3 * H)
        dhz, dh_rec = nan(2, B, H), nan(B, H)
        have = False
        for s in range(T - 1, -1, -1):
            t = s if di == 0 else T - 1 - s
            ops.gru_gate_bwd(gd, t, di * H, dout_d, T * 2 * H, 2 * H, 1.0, dh_rec if have else None, dhz[(s + 1) & 1] if have else None,
                             save[s], hs[s], dgi, dgh[s], dhz[s & 1])
            if s > 0:
                ops.linear_bwd_data(d_hh, dgh[s], w_d, None, dh_rec)
                have = True
        x = gi[di].double().view(B, T, 3 * H).clone().requires_grad_(True)
        y = gru(x)[0][:, :, di * H:(di + 1) * H]
        up = dout.double().view(B, T, 2 * H)[:, :, di * H:(di + 1) * H]
        (y * up).sum().backward()
        o_ref, hs_ref, save_ref = gru_seq_reference(gi[di], whh[di], bhh[di], T, di == 1, torch.float64, False, round_weight=False)
        assert rel_l2(o_ref, y.detach()) < 1e-12
        dgi_ref, dgh_ref = gru_seq_backward_reference(up, 1.0, whh[di], hs_ref, save_ref, T, di == 1, torch.float64, False, round_weight=False)
        assert rel_l2(dgi_ref, x.grad.view(B, T, 3 * H)) < 1e-12
        figures[f"out.d{di}"] = rel_l2(out[:, :, di * H:(di + 1) * H], y.detach())
        figures[f"dgi.d{di}"] = rel_l2(dgi.view(B, T, 3 * H), x.grad)
        figures[f"dgh.d{di}"] = rel_l2(dgh, dgh_ref)
    for k, v in figures.items():
        record_observed(f"gru.fp32_steps.b{B}_h{H}_t{T}.{k}.rel_l2", v)
        print(f"gru.fp32_steps.b{B}_h{H}_t{T}.{k}: rel_l2 {v:.3e}")
    assert not torch.isnan(out).any()
    assert all(v < 1e-5 for v in figures.values()), figures


# ------------------------------------------------------------------------------------------ helpers of gru.hip
GRID_CAP = 256 * 2048  # elements one pass of the element-wise helpers' grid covers: one more and the grid-stride loop runs


@pytest.mark.parametrize("B,T,D", [(5, 10, 512), (300, 3, 100), (1, 1, 7)])
def test_mean_time(ops, B, T, D):
    x = cpu_rnd(B, T, D, seed=600)
    y = ops.mean_time(x.to(DEV), B, T, D)
    assert rel_err(y, x.double().mean(1)) < 1e-6


@pytest.mark.parametrize("n", [1, 255, GRID_CAP + 3])
def test_axpy_and_mul(ops, n):
    x, y0, a = cpu_rnd(n, seed=610).to(DEV), cpu_rnd(n, seed=611).to(DEV), -0.37
    y = y0.clone()
    ops.axpy(a, x, y)
    assert rel_err(y, y0 + a * x) < 1e-7  # (the kernel's multiply-add is fused)
    assert rel_err(y, y0.double() + float(torch.tensor(a, dtype=torch.float32)) * x.double()) < 1e-7
    m = y0.clone()
    assert ops.mul_(m, x) is m
    assert torch.equal(m, y0 * x)


def test_dropout_helper(ops):
    n, p = GRID_CAP + 3, 0.3
    x = cpu_rnd(n, seed=620)
    x = (x + torch.sign(x) * 0.1).to(DEV)  # no zeros: a dropped element is told from a kept one
    assert (x != 0).all()
    rng = ops.new_rng_state(11, DEV)
    y = ops.dropout(x, rng, 5, p)
    kept = y != 0
    ratio = (y[kept].double() / x[kept].double())
    assert (ratio - 1 / (1 - p)).abs().max().item() < 1e-6 / (1 - p)  # values are only 0 or x / (1 - p)
    rate = kept.double().mean().item()
    assert abs(rate - (1 - p)) < 0.005, rate  # sigma = sqrt(0.21 / n) = 6.3e-4: about 8 sigma
    assert torch.equal(ops.dropout(x, rng, 5, p), y)          # same (rng, stream_id): same mask
    assert not torch.equal(ops.dropout(x, rng, 6, p) != 0, kept)  # another stream_id: another mask
    assert torch.equal(ops.dropout(x, rng, 5, 0.0), x)        # p = 0 is the identity


# ------------------------------------------------------------------------------------------ helpers of head.hip
@pytest.mark.parametrize("B,C,shift", [(8, 7, False), (300, 7, True), (257, 3, False)])
def test_cross_entropy(ops, B, C, shift):
    """B > 256: a thread takes a second row.  shift: one row's logits moved by +80 and another's by -80, so the maximum has to be
    subtracted before exp (the per-row loss then carries half an ulp of 80, 4e-6, which the mean over 300 rows keeps below the bound)."""
    logits = cpu_rnd(B, C, seed=700 + B)
    if shift:
        logits[3] += 80.0
        logits[B - 2] -= 80.0
    labels = torch.randint(0, C, (B,), generator=torch.Generator().manual_seed(710 + B))
    loss, dlogits = ops.cross_entropy(logits.to(DEV), labels.to(DEV))
    x = logits.double().requires_grad_(True)
    ref = F.cross_entropy(x, labels)
    ref.backward()
    assert abs(loss.item() - ref.item()) / abs(ref.item()) < 1e-6
    assert (dlogits.cpu().double() - x.grad).abs().max().item() < 1e-7


@pytest.mark.parametrize("need_dx", [True, False])
@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("B,N,K", [(8, 7, 256), (33, 7, 100), (1, 1, 1)])
def test_small_linear(ops, B, N, K, with_bias, need_dx):
    x, w, b = cpu_rnd(B, K, seed=800), cpu_rnd(N, K, scale=K ** -0.5, seed=801), cpu_rnd(N, seed=802)
    dy = cpu_rnd(B, N, seed=803)
    dw0, db0 = cpu_rnd(N, K, seed=804), cpu_rnd(N, seed=805)  # what the gradients hold before: the kernel accumulates
    x_d, w_d, b_d = x.to(DEV), w.to(DEV), b.to(DEV) if with_bias else None
    y = ops.small_linear_fwd(x_d, w_d, b_d)
    assert rel_err(y, x.double() @ w.double().t() + (b.double() if with_bias else 0)) < 1e-6
    dw, db = dw0.clone().to(DEV), db0.clone().to(DEV) if with_bias else None
    dx = ops.small_linear_bwd(dy.to(DEV), x_d, w_d, dw, db, need_dx=need_dx)
    assert rel_err(dw, dw0.double() + dy.double().t() @ x.double()) < 1e-6
    if with_bias:
        assert rel_err(db, db0.double() + dy.double().sum(0)) < 1e-6
    if need_dx:
        assert rel_err(dx, dy.double() @ w.double()) < 1e-6
    else:
        assert dx is None
