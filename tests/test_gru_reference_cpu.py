"""oracle/gru.py is the reference tests/test_gru_gpu.py judges the GRU kernels by: here it is itself pinned to torch.nn.GRU
(float64, forward and autograd), and the tolerance rule of the GPU test is shown to separate what it must separate."""
import pytest
import torch

from oracle.gru import bf16_round, gru_seq_backward_reference, gru_seq_reference


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def _inputs(B, H, T, seed):
    g = torch.Generator().manual_seed(seed)
    gi = [torch.randn(B, T, 3 * H, generator=g, dtype=torch.float64) for _ in range(2)]
    whh = [bf16_round(torch.randn(3 * H, H, generator=g, dtype=torch.float64) * H ** -0.5) for _ in range(2)]
    bhh = [torch.randn(3 * H, generator=g, dtype=torch.float64) * 0.1 for _ in range(2)]
    return g, gi, whh, bhh


def _torch_gru(H, whh, bhh):
    """nn.GRU whose input projection is the identity: its input IS gi, and the input's gradient IS dgi."""
    gru = torch.nn.GRU(3 * H, H, batch_first=True, bidirectional=True).double()
    with torch.no_grad():
        for d, suf in enumerate(("", "_reverse")):
            getattr(gru, f"weight_ih_l0{suf}").copy_(torch.eye(3 * H, dtype=torch.float64))
            getattr(gru, f"bias_ih_l0{suf}").zero_()
            getattr(gru, f"weight_hh_l0{suf}").copy_(whh[d])
            getattr(gru, f"bias_hh_l0{suf}").copy_(bhh[d])
    return gru


@pytest.mark.parametrize("B,H,T", [(6, 128, 4), (7, 128, 5)])
@pytest.mark.parametrize("form", ["full", "mean"])
def test_reference_equals_torch_gru_forward_and_autograd(B, H, T, form):
    g, gi, whh, bhh = _inputs(B, H, T, 1234 + B)
    gru = _torch_gru(H, whh, bhh)
    # a bidirectional nn.GRU feeds both directions the same input: one run per direction's gi, the other half ignored
    if form == "full":
        up, scale = torch.randn(B, T, 2 * H, generator=g, dtype=torch.float64), 1.0
    else:
        dfeat, scale = torch.randn(B, 2 * H, generator=g, dtype=torch.float64), 1.0 / T
    for d, reverse in enumerate((False, True)):
        x = gi[d].clone().requires_grad_(True)
        gru.zero_grad()
        y = gru(x)[0][:, :, d * H:(d + 1) * H]
        out, hs, save = gru_seq_reference(gi[d], whh[d], bhh[d], T, reverse, torch.float64, round_operand=False)
        assert rel_l2(out, y.detach()) < 1e-12
        # the layout: hs[s + 1] is the state after step s, i.e. the output at that step's time
        for s in range(T):
            assert torch.equal(hs[s + 1], out[:, T - 1 - s if reverse else s])
        assert torch.equal(hs[0], torch.zeros(B, H, dtype=torch.float64))
        if form == "full":
            dout = up[:, :, d * H:(d + 1) * H]
            (y * dout).sum().backward()
        else:
            dout = dfeat[:, None, d * H:(d + 1) * H].expand(B, T, H)
            (y.mean(1) * dfeat[:, d * H:(d + 1) * H]).sum().backward()
        dgi, dgh = gru_seq_backward_reference(dout, scale, whh[d], hs, save, T, reverse, torch.float64, round_operand=False)
        suf = "_reverse" if reverse else ""
        assert rel_l2(dgi, x.grad) < 1e-12
        # dgh is the gradient of W_hh h + b_hh per step: through nn.GRU it shows as the gradients of W_hh and b_hh
        assert rel_l2(dgh.sum((0, 1)), getattr(gru, f"bias_hh_l0{suf}").grad) < 1e-12
        assert rel_l2(torch.einsum("sbg,sbh->gh", dgh, hs[:T]), getattr(gru, f"weight_hh_l0{suf}").grad) < 1e-12
        # ... and element by element through autograd over the same recurrence with W_hh h + b_hh + e_s, e_s = 0 a leaf
        eps = [torch.zeros(B, 3 * H, dtype=torch.float64, requires_grad=True) for _ in range(T)]
        h, ys = torch.zeros(B, H, dtype=torch.float64), [None] * T
        for s in range(T):
            t = T - 1 - s if reverse else s
            gh = h @ whh[d].t() + bhh[d] + eps[s]
            r = torch.sigmoid(gi[d][:, t, :H] + gh[:, :H])
            z = torch.sigmoid(gi[d][:, t, H:2 * H] + gh[:, H:2 * H])
            n = torch.tanh(gi[d][:, t, 2 * H:] + r * gh[:, 2 * H:])
            h = (1 - z) * n + z * h
            ys[t] = h
            for k, v in enumerate((r, z, n, gh[:, 2 * H:])):
                assert rel_l2(save[s, k], v.detach()) < 1e-12
        y2 = torch.stack(ys, 1)
        assert rel_l2(y2.detach(), y.detach()) < 1e-12
        (y2 * dout * scale).sum().backward()
        assert rel_l2(dgh, torch.stack([e.grad for e in eps])) < 1e-12


def test_operand_rounding_is_what_the_flags_say():
    """round_operand only changes the operand of the recurrent products; W_hh is rounded to bf16 unless round_weight is off."""
    B, H, T = 3, 128, 3
    g = torch.Generator().manual_seed(5)
    gi = torch.randn(B, T, 3 * H, generator=g)
    w = torch.randn(3 * H, H, generator=g) * H ** -0.5
    b = torch.randn(3 * H, generator=g) * 0.1
    a = gru_seq_reference(gi, w, b, T, False)
    assert all(torch.equal(x, y) for x, y in zip(a, gru_seq_reference(gi, bf16_round(w), b, T, False)))
    assert not torch.equal(a[0], gru_seq_reference(gi, w, b, T, False, round_weight=False)[0])
    nb = gru_seq_reference(gi, w, b, T, False, round_operand=False)
    # the first product has h = 0 and the second step's r, z, n only see the product: out differs from the second step on
    assert torch.equal(a[0][:, 0], nb[0][:, 0]) and not torch.equal(a[0][:, 1], nb[0][:, 1])
    # step by step by hand
    h = torch.zeros(B, H, dtype=torch.float64)
    wd, gd, bd = bf16_round(w).double(), gi.double(), b.double()
    for s in range(T):
        gh = bf16_round(h) @ wd.t() + bd
        r, z = torch.sigmoid(gd[:, s, :H] + gh[:, :H]), torch.sigmoid(gd[:, s, H:2 * H] + gh[:, H:2 * H])
        h = (1 - z) * torch.tanh(gd[:, s, 2 * H:] + r * gh[:, 2 * H:]) + z * h
        assert torch.equal(a[1][s + 1], h)
    dout = torch.randn(B, T, H, generator=g)
    ra = gru_seq_backward_reference(dout, 1.0, w, a[1], a[2], T, False)
    rb = gru_seq_backward_reference(dout, 1.0, w, a[1], a[2], T, False, round_operand=False)
    assert torch.equal(ra[1][T - 1], rb[1][T - 1]) and not torch.equal(ra[1][T - 2], rb[1][T - 2])


@pytest.mark.parametrize("B,H,T", [(43, 256, 10), (19, 128, 10)])
def test_tolerance_rule_separates_fp32_arithmetic_from_a_missing_operand_rounding(B, H, T):
    """The GPU test bounds a kernel by max(0.5 d, 2e-6), d = rel L2 between the float64 references without (B) and with (A)
    the operand rounding.  An fp32 evaluation of A -- what a correct kernel computes, up to its own summation order -- must pass
    that bound (observed: at most 0.12 d, from bf16 roundings of the operand that flip between fp32 and float64); reference B (a
    kernel that skipped the rounding) must not."""
    g = torch.Generator().manual_seed(300)
    gi = torch.randn(B, T, 3 * H, generator=g)
    w = torch.randn(3 * H, H, generator=g) * H ** -0.5
    b = torch.randn(3 * H, generator=g) * 0.1
    dout = torch.randn(B, T, H, generator=g)
    for reverse in (False, True):
        A = gru_seq_reference(gi, w, b, T, reverse)
        Bn = gru_seq_reference(gi, w, b, T, reverse, round_operand=False)
        E = gru_seq_reference(gi, w, b, T, reverse, dtype=torch.float32)
        for k, name in enumerate(("out", "hs", "save")):
            d = rel_l2(Bn[k], A[k])
            bound = max(0.5 * d, 2e-6)
            assert rel_l2(E[k], A[k]) < bound, (name, rel_l2(E[k], A[k]), d)
            assert not rel_l2(Bn[k], A[k]) < bound
        hs32, save32 = A[1].float(), A[2].float()
        bA = gru_seq_backward_reference(dout, 1.0, w, hs32, save32, T, reverse)
        bB = gru_seq_backward_reference(dout, 1.0, w, hs32, save32, T, reverse, round_operand=False)
        bE = gru_seq_backward_reference(dout, 1.0, w, hs32, save32, T, reverse, dtype=torch.float32)
        for k, name in enumerate(("dgi", "dgh")):
            d = rel_l2(bB[k], bA[k])
            bound = max(0.5 * d, 2e-6)
            assert rel_l2(bE[k], bA[k]) < bound, (name, rel_l2(bE[k], bA[k]), d)
            assert not rel_l2(bB[k], bA[k]) < bound
