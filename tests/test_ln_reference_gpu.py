"""The LayerNorm kernels of focal_amd/csrc/norm.hip (forward, backward, both with PatchMerging's 2x2 gather, the masked copy, mask_cast)
against float64 at every width and grid regime they accept (tests/ln_reference.py: CASES).  Every row of y, mean, rstd and dx and every
column of dgamma and dbeta must satisfy

    err <= max(4 * E_plain, 8 * 2^-23)

in the metric of its quantity, E_plain being what a plain fp32 restatement makes on the same row or column.  Each call runs inside a launch
trace and must have launched the instantiation, grid and block the case was written for; y, stats, dx_masked and (accumulate = 0) dx are
handed in full of NaN, so an element no lane wrote fails.  The masked copy and mask_cast must equal dtype(dx * mask) exactly, the mask
drawn through the residual epilogue of an identity GEMM.  Recorded per case: layernorm.<case>.<quantity>, the worst figure in units of
2^-23 (the bound is 8 wherever the yardstick is under 2)."""
import ctypes as C

import pytest
import torch

import ln_reference as lr
from conftest import record_observed

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    from focal_amd import ops as o
    return o


def traced(fn, capacity=16):
    """fn() inside a dispatch trace -> [((kernel, dtype, NV), grid, block)] of the library launches it made, in order."""
    from focal_amd import _lib
    lib = _lib.load()
    torch.cuda.synchronize()
    _lib.check(lib.focal_trace_begin(capacity, _lib.TRACE_DISPATCH))
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        lib.focal_trace_end()
    cnt = lib.focal_trace_count()
    recs = (_lib.TraceRecord * max(cnt, 1))()
    _lib.check(lib.focal_trace_read(0, cnt, recs))
    out = []
    for r in recs[:cnt]:
        assert tuple(r.grid)[1:] == (1, 1) and tuple(r.block)[1:] == (1, 1), r.kernel
        out.append((lr.kernel_ident(r.kernel.decode()), int(r.grid[0]), int(r.block[0])))
    return out


def refused(fn, text):
    """fn() must raise FocalHipError from the argument check (FOCAL_EINVAL, the named message), with no launch recorded."""
    from focal_amd import _lib
    lib = _lib.load()
    torch.cuda.synchronize()
    _lib.check(lib.focal_trace_begin(4, _lib.TRACE_DISPATCH))
    try:
        with pytest.raises(_lib.FocalHipError) as e:
            fn()
    finally:
        lib.focal_trace_end()
    assert lib.focal_trace_count() == 0
    assert "error -1:" in str(e.value) and text in str(e.value), str(e.value)


def abi_fwd(ops, d, x, gamma, beta, y, stats):
    from focal_amd import _lib
    _lib.check(_lib.load().focal_layernorm_fwd(C.byref(d), ops._p(x), ops._p(gamma), ops._p(beta), ops._p(y), ops._p(stats), ops._stream()))


def abi_bwd(ops, d, dy, x, stats, gamma, dx, accumulate, dgamma, dbeta, dx_masked, mask):
    from focal_amd import _lib
    _lib.check(_lib.load().focal_layernorm_bwd(C.byref(d), ops._p(dy), ops._p(x), ops._p(stats), ops._p(gamma), ops._p(dx), int(accumulate), ops._p(dgamma),
                                               ops._p(dbeta), ops._p(dx_masked), C.byref(mask) if mask is not None else None, ops._stream()))


def abi_mask_cast(ops, code, rows, Cc, g, mask, out):
    from focal_amd import _lib
    _lib.check(_lib.load().focal_mask_cast(code, rows, Cc, ops._p(g), C.byref(mask) if mask is not None else None, ops._p(out), ops._stream()))


def _ct(bf16):
    return torch.bfloat16 if bf16 else torch.float32


# ---------------------------------------------------------------------------------------------- forward and backward against float64
def run_ln_case(ops, case):
    Cc, rows, dt, ct = case.C, case.rows, "bf16" if case.bf16 else "f32", _ct(case.bf16)
    x, gamma, beta, dy, old = lr.make_inputs(rows, Cc, case.seed, case.bf16, case.tiny)
    R = lr.reference(x, gamma, beta, dy)
    gather = None
    if case.gather:
        B, H, W = case.gather
        gather = (B, H, W, Cc // 4)
        to_dev = lambda t: lr.scatter_tokens(t, B, H, W).contiguous().to(DEV)      # the token tensor [B, H, W, Cin]
        to_cat = lambda t: lr.gather_cat(t.cpu())
    else:
        to_dev, to_cat = (lambda t: t.to(DEV)), (lambda t: t.cpu())
    xd, gd, bd, dyd = to_dev(x), gamma.to(DEV), beta.to(DEV), dy.to(DEV).to(ct)
    figures, failures = {}, []

    def hold(q, e, lim, tag=""):
        fig = lr.worst(e) / lr.EPS
        prev = figures.get(q, 0.0)
        figures[q] = prev if fig <= prev else fig                                    # (a NaN sticks)
        n = lr.over(e, lim)
        print(f"{case.id} {q}{tag}: worst {fig:.2f} eps; over the bound: {n} of {e.numel()}")
        if n:
            failures.append((q + tag, fig, n))

    # forward
    want = lr.expected_launch("fwd", dt, rows, Cc)
    assert want[1:] == (case.fwd, 256)
    y = torch.full((rows, Cc), NAN, dtype=ct, device=DEV)
    stats = torch.full((rows, 2), NAN, device=DEV)
    d = ops.ln_desc(ops.code(ct), rows, Cc, gather=gather)
    launched = traced(lambda: abi_fwd(ops, d, xd, gd, bd, y, stats))
    assert launched == [want], (case.id, launched, want)
    lim = lr.bounds(R)
    hold("y", lr.err_y(y, R, lim["y"] if case.bf16 else None), lim["y"])
    hold("mean", lr.err_mean(stats[:, 0], R), lim["mean"])
    hold("rstd", lr.err_rstd(stats[:, 1], R), lim["rstd"])
    # backward, from the kernel's own stats as the product runs it: into a NaN-filled dx, then accumulating onto `old`
    want = lr.expected_launch("bwd", dt, rows, Cc)
    assert want[1] == case.bwd
    d = ops.ln_desc(ops.code(ct), rows, Cc, gather=gather)
    for acc in (0, 1):
        o = old if acc else None
        dx = to_dev(old) if acc else torch.full_like(xd, NAN)
        dg, db = torch.full((Cc,), lr.PREFILL[0], device=DEV), torch.full((Cc,), lr.PREFILL[1], device=DEV)
        launched = traced(lambda: ops.layernorm_bwd(dyd, xd.view(-1, xd.shape[-1]), stats, gd, dx, acc, dg, db, gather=gather, desc=d))
        assert launched == [want], (case.id, acc, launched, want)
        lim = lr.bounds(R, o, lr.PREFILL)
        assert dx.shape == xd.shape
        hold("dx", lr.err_dx(to_cat(dx), R, o), lim["dx"], f" accumulate={acc}")
        hold("dgamma", lr.err_dgamma(dg, R, lr.PREFILL[0]), lim["dgamma"], f" accumulate={acc}")
        hold("dbeta", lr.err_dbeta(db, R, lr.PREFILL[1]), lim["dbeta"], f" accumulate={acc}")
    for q, fig in figures.items():
        record_observed(f"layernorm.{case.id}.{q}", fig)
    assert not failures, (case.id, failures)


# ---------------------------------------------------------------------------------------------- the masked copy and mask_cast
def forward_mask(ops, dd, M, N):
    """The multipliers the forward residual epilogue draws for an [M, N] token tensor: y = 0 + mask * (1 @ I)."""
    from focal_amd._lib import EPI_RESIDUAL
    y, _ = ops.linear(torch.ones(M, N, device=DEV), torch.eye(N, device=DEV), None, compute=torch.float32, y_dtype=torch.float32,
                      resid=torch.zeros(M, N, device=DEV), epilogue=EPI_RESIDUAL, out_drop=dd)
    return y


def run_mask_case(ops, case):
    (B, H, W), Cin, ct, dt = lr.MASK_BHW, lr.MASK_CIN, _ct(case.bf16), "bf16" if case.bf16 else "f32"
    M = B * H * W
    state = ops.new_rng_state(9, DEV)
    dd = ops.drop_desc(state, 21, case.p[0], 25, case.p[1], case.rps)
    mask = forward_mask(ops, dd, M, Cin)
    assert bool((mask != 1).any()) and int((mask == 0).sum()) < mask.numel() // 2 and bool(torch.isfinite(mask).all())
    if case.layout == "plain":
        rows, Cc, gather, acc = M, Cin, None, 1
    else:
        rows, Cc, gather, acc = M // 4, 4 * Cin, (B, H, W, Cin), 0
    cat, gamma, beta, dy, old = lr.make_inputs(rows, Cc, 500 + Cc)
    tokens = (lr.scatter_tokens(cat, B, H, W).reshape(M, Cin) if gather else cat).contiguous().to(DEV)
    g = lr.make_inputs(M, Cin, 77)[4].to(DEV)                                        # a gradient on the token tensor
    gd, dyd = gamma.to(DEV), dy.to(DEV).to(ct)
    y, stats = ops.layernorm_fwd(tokens, gd, beta.to(DEV), torch.float32, gather=gather)
    want = lr.expected_launch("bwd", dt, rows, Cc)
    outs = {}
    for name, m in (("masked", dd), ("copy", None)):
        dx = g.clone() if acc else torch.full((M, Cin), NAN, device=DEV)
        dxm = torch.full((M, Cin), NAN, dtype=ct, device=DEV)
        dg, db = torch.zeros(Cc, device=DEV), torch.zeros(Cc, device=DEV)
        launched = traced(lambda: ops.layernorm_bwd(dyd, tokens, stats, gd, dx, acc, dg, db, gather=gather, dx_masked=dxm, mask=m))
        assert launched == [want], (case.id, name, launched, want)
        assert torch.isfinite(dx).all()
        outs[name] = (dx, dxm)
    dx, dxm = outs["masked"]
    wrong = int((dxm != (dx * mask).to(ct)).sum())           # the same fp32 product and the same cast: exact (a NaN counts as wrong)
    dx2, copy = outs["copy"]
    assert torch.equal(dx2, dx) and torch.equal(copy, dx.to(ct))                     # mask = None with a buffer: the plain dtype copy
    wrong_cast = 0
    if case.layout == "plain":
        out = torch.full((M, Cin), NAN, dtype=ct, device=DEV)
        launched = traced(lambda: abi_mask_cast(ops, ops.code(ct), M, Cin, g, dd, out))
        assert launched == [lr.expected_launch("mask_cast", dt, M, Cin)], (case.id, launched)
        wrong_cast = int((out != (g * mask).to(ct)).sum())
        assert torch.equal(ops.mask_cast(g, dd, ct), out) and torch.equal(ops.mask_cast(g, None, ct), g.to(ct))
        record_observed(f"layernorm.{case.id}.mask_cast_mismatches", wrong_cast)
    record_observed(f"layernorm.{case.id}.dx_masked_mismatches", wrong)
    print(f"{case.id}: dx_masked != dtype(dx * mask) at {wrong} of {dxm.numel()} elements; mask_cast at {wrong_cast}")
    assert wrong == 0 and wrong_cast == 0, (case.id, wrong, wrong_cast)


@pytest.mark.parametrize("case", lr.CASES, ids=lr.CASE_IDS)
def test_kernel_meets_the_fp32_bound(ops, case):
    (run_ln_case if case.kind == "ln" else run_mask_case)(ops, case)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_mask_cast_beyond_its_grid_cap(ops, bf16):
    """9217 x 256: 589 888 float4 on 2048 x 256 lanes, a ragged second trip round the grid."""
    rows, Cc = lr.MASK_CAST_BIG
    ct, dt = _ct(bf16), "bf16" if bf16 else "f32"
    dd = ops.drop_desc(ops.new_rng_state(11, DEV), 3, 0.2, 5, 0.1, 100)
    mask = forward_mask(ops, dd, rows, Cc)
    g = torch.randn(rows, Cc, generator=torch.Generator().manual_seed(12)).to(DEV)
    out = torch.full((rows, Cc), NAN, dtype=ct, device=DEV)
    want = lr.expected_launch("mask_cast", dt, rows, Cc)
    assert want[1] == lr.MASK_MAX_GRID and lr.passes("mask_cast", rows, Cc) == (2, True)
    launched = traced(lambda: abi_mask_cast(ops, ops.code(ct), rows, Cc, g, dd, out))
    assert launched == [want], (launched, want)
    wrong = int((out != (g * mask).to(ct)).sum())
    record_observed(f"layernorm.mask-cast-9217x256-{dt}.mask_cast_mismatches", wrong)
    assert wrong == 0


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals_launch_nothing(ops):
    f32 = ops.code(torch.float32)
    t = lambda *s: torch.full(s, NAN, device=DEV)
    x, gam, y, st = torch.ones(4, 2048, device=DEV), torch.ones(2048, device=DEV), t(4, 2048), t(4, 2)
    untouched = lambda: bool(torch.isnan(y).all() and torch.isnan(st).all())
    # widths outside {16, ..., 1024}
    for Cc in (8, 48, 2048):
        d = ops.ln_desc(f32, 4, Cc)
        refused(lambda: abi_fwd(ops, d, x, gam, gam, y, st), f"C={Cc} must be a power of two in [16, 1024]")
        refused(lambda: abi_bwd(ops, d, x, x, st, gam, y, 0, gam, gam, None, None), f"C={Cc} must be a power of two in [16, 1024]")
    # a dtype code that is neither fp32 nor bf16
    assert 7 not in (f32, ops.code(torch.bfloat16))
    refused(lambda: abi_fwd(ops, ops.ln_desc(7, 4, 64), x, gam, gam, y, st), "layernorm: bad dtype")
    refused(lambda: abi_bwd(ops, ops.ln_desc(7, 4, 64), x, x, st, gam, y, 0, gam, gam, None, None), "layernorm: bad dtype")
    refused(lambda: abi_mask_cast(ops, 7, 4, 64, x, None, y), "mask_cast: bad dtype")
    # a gather that does not add up: Cin * 4 != C, odd H, odd W, rows != B (H/2) (W/2)
    for rows, Cc, gather in ((6, 64, (1, 4, 6, 32)), (6, 64, (1, 5, 6, 16)), (6, 64, (1, 4, 7, 16)), (5, 64, (1, 4, 6, 16)), (12, 64, (1, 4, 6, 16))):
        d = ops.ln_desc(f32, rows, Cc, gather=gather)
        refused(lambda: abi_fwd(ops, d, x, gam, gam, y, st), "inconsistent gather geometry")
        refused(lambda: abi_bwd(ops, d, x, x, st, gam, y, 0, gam, gam, None, None), "inconsistent gather geometry")
    # a mask without a buffer for the masked copy (ops.layernorm_bwd only forwards a mask together with one: the C ABI directly)
    dd = ops.drop_desc(ops.new_rng_state(1, DEV), 1, 0.2, 2, 0.1, 2)
    refused(lambda: abi_bwd(ops, ops.ln_desc(f32, 4, 64), x, x, st, gam, y, 0, gam, gam, None, dd), "mask without dx_masked")
    # the mask's 32-bit row arithmetic: token rows x rows_per_sample must stay below 2^32 (checked before any memory is touched)
    big = ops.drop_desc(ops.new_rng_state(1, DEV), 1, 0.2, 2, 0.1, 65536)
    refused(lambda: abi_bwd(ops, ops.ln_desc(f32, 65536, 64), x, x, st, gam, y, 0, gam, gam, y, big), "exceed the mask's 32-bit row arithmetic")
    refused(lambda: abi_mask_cast(ops, f32, 65536, 64, x, big, y), "exceed the mask's 32-bit row arithmetic")
    # gathered: the TOKEN rows count (B H W = 2^22 tokens x 1024 = 2^32), four times the LayerNorm's own rows
    k = ops.drop_desc(ops.new_rng_state(1, DEV), 1, 0.2, 2, 0.1, 1024)
    refused(lambda: abi_bwd(ops, ops.ln_desc(f32, 1 << 20, 64, gather=(1024, 64, 64, 16)), x, x, st, gam, y, 0, gam, gam, y, k),
            "exceed the mask's 32-bit row arithmetic")
    assert untouched() and bool((x == 1).all()) and bool((gam == 1).all())
