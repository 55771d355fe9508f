"""[1, k] 'same' convolutions with an EVEN k through the C ABI, against the definition in float64.

torch pads an even 'same' filter asymmetrically: k - 1 zeros in all, (k - 1) // 2 on the left, the rest on the right.  The library follows
it: the forward convolution, its BatchNorm-statistics form and the weight gradient read token s + t - (k - 1) // 2 at tap t, the data gradient
runs the flipped taps with k // 2 on the left.  Covered here: the sliding-window GEMM (every k, fp32 and bf16), the row-ring kernel at k = 4
(64 -> 64 channels, bf16, whole 64-row tiles), the in-convolution with k = 4, and the asymmetry itself on a one-hot row.
Bounds: those tests/test_kernels_gpu.py applies to the same functions at odd k (an even k changes the tap count, not the arithmetic)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"


def rel_err(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def rnd(*shape, scale=1.0, seed=0, dtype=torch.float32):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV).to(dtype)


@pytest.fixture(scope="module")
def ops():
    from focal_amd import ops as o
    return o


def same_conv64(x_tok, w, b, n_int, S, k):
    """The definition: tokens [n_int * S, C_in] (float64) -> ([n_int * S, C_out], the NCHW leaf the gradient lands on)."""
    C = x_tok.shape[1]
    lw = (k - 1) // 2
    xi = x_tok.view(n_int, S, C).permute(0, 2, 1).unsqueeze(2).contiguous().requires_grad_(True)  # [n_int, C, 1, S]
    y = F.conv2d(F.pad(xi, (lw, k - 1 - lw)), w, b)
    return y.squeeze(2).permute(0, 2, 1).reshape(n_int * S, -1), xi


def tokens_of(nchw):
    return nchw.squeeze(2).permute(0, 2, 1).reshape(-1, nchw.shape[1])


# ---------------------------------------------------------------------------------------------- sliding-window GEMM
@pytest.mark.parametrize("ct", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,I,S,k", [(3, 10, 20, 2), (3, 10, 20, 4), (3, 10, 20, 6), (64, 1, 3, 4)])
def test_even_k_sliding_window_gemm(ops, ct, B, I, S, k):
    """600 rows are no whole 64-row tiles and S = 3 < k = 4 (every output loses taps on both sides): the GEMM path in both precisions."""
    C = 64
    rows = B * I * S
    x = rnd(rows, C, seed=74, dtype=ct)
    w, b = rnd(C, C, 1, k, scale=(C * k) ** -0.5, seed=75), rnd(C, seed=76)
    d = ops.conv_desc(ops.code(ct), rows, S, C, C, k)
    w_fwd, w_bwd = ops.permute_pack(w, C, C, k, ct), ops.conv_pack_bwd(d, w, ct)
    z = ops.conv_fwd(d, x, w_fwd, b)
    wq = w if ct == torch.float32 else w.bfloat16().float()
    wr = wq.double().requires_grad_(True)
    ref, xi = same_conv64(x.double(), wr, b.double(), B * I, S, k)
    e_fwd = rel_err(z, ref)
    dz = rnd(rows, C, seed=77, dtype=ct)
    ref.backward(dz.double())
    g_in = rnd(rows, C, seed=78)
    g = g_in.clone()
    ops.conv_bwd_data(d, dz, w_bwd, g, g)
    e_dx = rel_err(g - g_in, tokens_of(xi.grad))
    dwp, db = torch.zeros(C, k * C, device=DEV), torch.zeros(C, device=DEV)
    ops.conv_bwd_weight(d, dz, x, dwp, db)
    dw = torch.zeros_like(w)
    ops.permute_unpack_add(dwp, dw, C, C, k)
    e_dw, e_db = rel_err(dw, wr.grad), rel_err(db, dz.double().sum(0))
    print(f"even-k GEMM {ct} k={k} S={S}: fwd {e_fwd:.3e} dx {e_dx:.3e} dw {e_dw:.3e} db {e_db:.3e}")
    assert e_fwd < (1e-5 if ct == torch.float32 else 5e-3)
    assert e_dx < (1e-5 if ct == torch.float32 else 6e-3)
    assert e_dw < (2e-5 if ct == torch.float32 else 2e-4)
    assert e_db < 1e-4


# ---------------------------------------------------------------------------------------------- row-ring kernel, k = 4
@pytest.mark.parametrize("B,I,S,groups", [(4, 4, 4, 1), (16, 10, 20, 1), (32, 10, 20, 2), (2, 4, 128, 1)])
def test_even_k_row_ring_kernel(ops, B, I, S, groups, monkeypatch):
    """conv_ring_kernel<4, .> against the definition in float64 on the same bf16 operands, against the sliding-window GEMM (FOCAL_CONV_RING=0),
    and its BatchNorm statistics against the tensor it wrote: one tile with S == k, 50 tiles, two statistics groups, and S = 128 (the
    geometry of DeepSense's second ConvBlock: 64 channels over loc_mod_out_channels = 128 positions)."""
    C, k, ct = 64, 4, torch.bfloat16
    rows = B * I * S
    assert rows % (64 * groups) == 0
    x = rnd(rows, C, seed=374, dtype=ct)
    w, b = rnd(C, C, 1, k, scale=(C * k) ** -0.5, seed=375), rnd(C, seed=376)
    d = ops.conv_desc(ops.code(ct), rows, S, C, C, k)
    w_fwd, w_bwd = ops.permute_pack(w, C, C, k, ct), ops.conv_pack_bwd(d, w, ct)
    dz, g_in = rnd(rows, C, seed=377, dtype=ct), rnd(rows, C, seed=378)
    d_bn = ops.bn_desc(ops.code(ct), rows, C, I * S, 0.0, None, 0, momentum=1.0, groups=groups)

    from focal_amd import _lib
    lib = _lib.load()

    def run():
        g = g_in.clone()
        torch.cuda.synchronize()
        _lib.check(lib.focal_trace_begin(64, _lib.TRACE_DISPATCH))
        try:
            z = ops.conv_fwd(d, x, w_fwd, b)
            rm, rv = torch.zeros(groups, C, device=DEV), torch.zeros(groups, C, device=DEV)
            z2, mr = ops.conv_fwd_bn(d, x, w_fwd, b, d_bn, rm, rv)
            ops.conv_bwd_data(d, dz, w_bwd, g, g)
            torch.cuda.synchronize()
        finally:
            lib.focal_trace_end()
        n = lib.focal_trace_count()
        recs = (_lib.TraceRecord * max(n, 1))()
        _lib.check(lib.focal_trace_read(0, n, recs))
        return z, z2, mr, rm, rv, g, [recs[i].kernel.decode() for i in range(n)]

    monkeypatch.setenv("FOCAL_CONV_RING", "0")
    z0, z20, mr0, rm0, rv0, g0, names0 = run()
    assert not any("conv_ring_kernel" in n for n in names0), names0
    monkeypatch.delenv("FOCAL_CONV_RING")
    z, z2, mr, rm, rv, g, names = run()
    assert sum("conv_ring_kernelILi4E" in n for n in names) == 3, names   # (mangled symbols: conv_ring_kernel<4, epilogue>)
    ref, xi = same_conv64(x.double(), w.bfloat16().double(), b.double(), B * I, S, k)
    ref.backward(dz.double())
    e_fwd, e_dx = rel_err(z, ref), rel_err(g - g_in, tokens_of(xi.grad))
    e_z_gemm, e_g_gemm = rel_err(z, z0), rel_err(g, g0)
    print(f"even-k ring B={B} I={I} S={S} G={groups}: fwd {e_fwd:.3e} dx {e_dx:.3e} vs GEMM fwd {e_z_gemm:.3e} dx {e_g_gemm:.3e}")
    assert e_fwd < 2e-6 and torch.equal(z2, z)
    assert e_z_gemm < 2e-6 and e_g_gemm < 2e-6
    assert e_dx < 2e-5
    rg = rows // groups
    for h in range(groups):
        zh = z[h * rg:(h + 1) * rg].double()
        mean, var = zh.mean(0), zh.var(0, unbiased=False)
        assert rel_err(mr[h * 2 * C:h * 2 * C + C], mean) < 1e-4 and rel_err(mr[h * 2 * C + C:(h + 1) * 2 * C], (var + d_bn.eps).rsqrt()) < 1e-4
        assert rel_err(rm[h], mean) < 1e-4 and rel_err(rv[h], var * rg / (rg - 1)) < 1e-4
    assert rel_err(mr, mr0) < 1e-5 and rel_err(rm, rm0) < 1e-5 and rel_err(rv, rv0) < 1e-5
    # the sums-only form + the BatchNorm launch that finishes the statistics == the one-launch form followed by focal_bn_act_fwd
    assert ops.conv_fwd_bn_sums_supported(d, d_bn, x, w_fwd)
    gam, bet, res = 1 + 0.1 * rnd(C, seed=379), 0.1 * rnd(C, seed=380), rnd(rows, C, seed=381)
    y0, ya0 = ops.bn_act_fwd(d_bn, z2, mr, gam, bet, res, ct)
    zs, sums = ops.conv_fwd_bn_sums(d, x, w_fwd, b, d_bn)
    rm1, rv1 = torch.zeros(groups, C, device=DEV), torch.zeros(groups, C, device=DEV)
    y1, ya1, mr1 = ops.bn_act_fwd_sums(d_bn, zs, sums, rm1, rv1, gam, bet, res, ct)
    assert torch.equal(zs, z2) and rel_err(mr1, mr) < 1e-6 and rel_err(rm1, rm) < 1e-6 and rel_err(rv1, rv) < 1e-6
    # (the slot sums of two launches differ in their last bits -- atomics in another order --, so a few bf16 copies round the other way)
    assert rel_err(y1, y0) < 1e-5 and (ya1 != ya0).float().mean().item() < 1e-3 and rel_err(ya1.float(), ya0.float()) < 1e-2
    monkeypatch.setenv("FOCAL_CONV_BN_SUMS", "0")
    assert not ops.conv_fwd_bn_sums_supported(d, d_bn, x, w_fwd)


# ---------------------------------------------------------------------------------------------- the asymmetry itself
@pytest.mark.parametrize("ct,k", [(torch.float32, 2), (torch.float32, 4), (torch.bfloat16, 4), (torch.bfloat16, 6)])
@pytest.mark.parametrize("s_hot", [0, 13, 31])
def test_even_k_taps_land_where_torch_puts_them(ops, ct, k, s_hot):
    """A one-hot input row and a filter of distinct taps (tap t = t + 1, exact in bf16): output position s of the hot interval carries tap
    s_hot - s + (k - 1) // 2 and nothing else does -- a symmetric or right-heavy padding puts every tap one position off.  The data gradient
    of a one-hot dz carries tap s - s_hot + (k - 1) // 2.  Two intervals of 32 tokens = one 64-row tile: bf16 with k = 4 is the row-ring
    kernel, the others the sliding-window GEMM; the hot row at an interval's first and last token shows that nothing leaks across."""
    C, S, c0, n_int, hot_int = 64, 32, 5, 2, 1
    rows, pf = n_int * S, (k - 1) // 2
    x = torch.zeros(rows, C, device=DEV, dtype=ct)
    x[hot_int * S + s_hot, c0] = 1.0
    w = torch.zeros(C, C, 1, k, device=DEV)
    w[:, c0, 0, :] = torch.arange(1, k + 1, device=DEV, dtype=torch.float32)
    d = ops.conv_desc(ops.code(ct), rows, S, C, C, k)
    z = ops.conv_fwd(d, x, ops.permute_pack(w, C, C, k, ct), torch.zeros(C, device=DEV))
    want = torch.zeros(rows, device=DEV)
    for s in range(S):
        t = s_hot - s + pf
        if 0 <= t < k:
            want[hot_int * S + s] = t + 1
    assert torch.equal(z, want[:, None].expand(rows, C)), (z[:, 0].view(n_int, S), want.view(n_int, S))
    # data gradient: dx[s][c0] = sum over output channels n of w[n][c0][t] dz[s - t + pf][n]; dz one-hot in row s_hot, channel 0
    dz = torch.zeros(rows, C, device=DEV, dtype=ct)
    dz[hot_int * S + s_hot, 0] = 1.0
    g = torch.zeros(rows, C, device=DEV)
    ops.conv_bwd_data(d, dz, ops.conv_pack_bwd(d, w, ct), g, g)
    want_dx = torch.zeros(rows, C, device=DEV)
    for s in range(S):
        t = s - s_hot + pf
        if 0 <= t < k:
            want_dx[hot_int * S + s, c0] = t + 1
    assert torch.equal(g, want_dx), (g[:, c0].view(n_int, S), want_dx[:, c0].view(n_int, S))


# ---------------------------------------------------------------------------------------------- in-convolution
@pytest.mark.parametrize("dz_ct", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("S_in,k,stride,pad_left,cin", [(20, 4, 1, 1, 2), (128, 4, 1, 1, 1)])
def test_conv_in_even_k(ops, S_in, k, stride, pad_left, cin, dz_ct):
    """The in-convolution with an even 'same' filter: pad_left = (k - 1) // 2, the other k - 1 - pad_left zeros on the right (cin * k = 8 / 4:
    the forward FMA kernel and the K <= 16 weight-gradient kernel with fp32 and with bf16 output gradients -- 64 output channels are the
    only width the in-convolution accepts, so these are the kernels every K <= 16 call reaches)."""
    B, I, C = 3, 10, 64
    S_out = S_in
    x = rnd(B, cin, I, S_in, scale=10.0, seed=70)
    w, b = rnd(C, cin, 1, k, scale=(cin * k) ** -0.5, seed=71), rnd(C, seed=72)
    d = ops.conv_in_desc(B, cin, I, S_in, S_out, k, stride, pad_left, C)
    z = ops.conv_in_fwd(d, x, w, b)
    wr, br = w.double().requires_grad_(True), b.double().requires_grad_(True)
    out = F.conv2d(F.pad(x.double(), (pad_left, k - 1 - pad_left)), wr, br, stride=(1, stride)).permute(0, 2, 3, 1).reshape(-1, C)
    e_fwd = rel_err(z, out)
    dz = rnd(B * I * S_out, C, seed=73, dtype=dz_ct)   # (bf16: the reference takes the same rounded values)
    dw, db = torch.zeros_like(w), torch.zeros(C, device=DEV)
    ops.conv_in_bwd_weight(d, x, dz, dw, db)
    (out * dz.double()).sum().backward()
    e_dw, e_db = rel_err(dw, wr.grad), rel_err(db, br.grad)
    print(f"conv_in k={k} cin={cin} S={S_in} dz {dz_ct}: fwd {e_fwd:.3e} dw {e_dw:.3e} db {e_db:.3e}")
    assert e_fwd < 1e-5
    assert e_dw < 2e-5 and e_db < 2e-5
