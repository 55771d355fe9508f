"""What the LayerNorm kernels of focal_amd/csrc/norm.hip are measured against: the float64 expectation (from x, gamma, beta, dy alone), the
error metrics (each normalised by the conditioning of its quantity) and their bound, a plain fp32 restatement as the yardstick of what fp32
can do on the same inputs, an fp32 restatement of the kernels' own summation order (the bound must be attainable by a correct fp32
implementation), the dispatch of the three launchers restated, and the table of cases -- every width, both dtypes, both layouts, at every
grid regime.  A plain helper module: no fixtures, no GPU."""
import re
from collections import namedtuple

import torch

EPS = 2.0 ** -23
# err <= max(MARGIN * E_plain, FLOOR): the project's figures (tests/fft_reference.py).  Here the floor is what decides nearly everywhere: the
# yardstick's sums are pairwise and land within 1 to 2 eps in these metrics.
MARGIN, FLOOR = 4.0, 8 * EPS
LN_EPS = 1e-5
BF16_HALF_ULP = 2.0 ** -8          # round-to-nearest of a bf16 (8 significant bits, 7 of them stored): at most 2^-8 of the value rounded
WIDTHS = (16, 32, 64, 128, 256, 512, 1024)
FWD_MAX_GRID, BWD_MAX_GRID, MASK_MAX_GRID = 2048, 256, 2048
F64, F32 = torch.float64, torch.float32


def bound(E_plain):
    """E_plain: a figure, or a tensor of them (one per row or per column: each is held to its own)."""
    return E_plain.mul(MARGIN).clamp(min=FLOOR) if isinstance(E_plain, torch.Tensor) else max(MARGIN * E_plain, FLOOR)


# ---------------------------------------------------------------------------------------------- the 2x2 gather
def gather_cat(x4):
    """[B, H, W, Cin] -> [B * H/2 * W/2, 4 Cin], cat order x00, x10, x01, x11 (norm.hip: RowMap; the first index is the row parity)."""
    B, H, W, Cin = x4.shape
    return torch.cat([x4[:, 0::2, 0::2], x4[:, 1::2, 0::2], x4[:, 0::2, 1::2], x4[:, 1::2, 1::2]], -1).reshape(-1, 4 * Cin)


def scatter_tokens(cat, B, H, W, swap=False):
    """The inverse: [rows, 4 Cin] -> [B, H, W, Cin].  swap=True exchanges x10 and x01 (what the CPU test shows the bound rejects)."""
    Cin = cat.shape[1] // 4
    c = cat.reshape(B, H // 2, W // 2, 4, Cin)
    x4 = torch.empty(B, H, W, Cin, dtype=cat.dtype)
    s10, s01 = (2, 1) if swap else (1, 2)
    x4[:, 0::2, 0::2], x4[:, 1::2, 0::2], x4[:, 0::2, 1::2], x4[:, 1::2, 1::2] = c[:, :, :, 0], c[:, :, :, s10], c[:, :, :, s01], c[:, :, :, 3]
    return x4


# ---------------------------------------------------------------------------------------------- float64 expectation
Ref = namedtuple("Ref", "x gamma beta dy mean rstd xhat y dx dgamma dbeta S G xmax")


def reference(x, gamma, beta, dy):
    """x [rows, C], gamma, beta [C], dy [rows, C] (any float dtype, CPU; the values the kernel is handed) -> float64 Ref.
    S_r = max(rstd_r max_c |x_rc|, max_c |xhat_rc|): how far the row's normalised values can be moved by one rounding of x, mean or xhat.
    G_r = max_c |dy_rc gamma_c|."""
    x, gamma, beta, dy = (t.detach().cpu().to(F64) for t in (x, gamma, beta, dy))
    mean = x.mean(1)
    d = x - mean[:, None]
    var = (d * d).mean(1)
    rstd = 1.0 / torch.sqrt(var + LN_EPS)
    xhat = d * rstd[:, None]
    y = xhat * gamma + beta
    g = dy * gamma
    dx = rstd[:, None] * (g - g.mean(1, keepdim=True) - xhat * (g * xhat).mean(1, keepdim=True))
    xmax = x.abs().amax(1)
    S = torch.maximum(rstd * xmax, xhat.abs().amax(1))
    return Ref(x, gamma, beta, dy, mean, rstd, xhat, y, dx, (dy * xhat).sum(0), dy.sum(0), S, g.abs().amax(1), xmax)


# ---------------------------------------------------------------------------------------------- the metrics
def _ratio(num, den):
    """num / den where 0 / 0 is 0 (nothing to get wrong) and a NaN numerator stays NaN (an unwritten element passes no bound)."""
    out = num / den
    return torch.where((den == 0) & (num == 0), torch.zeros_like(out), out)


def _64(t):
    return t.detach().cpu().to(F64)


def err_y(got, R, lim=None):
    """Per row: max_c |dy_rc| / (|gamma_c| S_r + |beta_c|).  lim (the bound of the fp32 metric, a figure or one per row) names a bf16 result:
    the allowance per element is then a + 2^-8 (|y64| + a) with a = lim * denominator -- one round-to-nearest of a value within a of y64 --
    and the figure returned is what is left of the error after that rounding term, in the same units, so that `<= lim` is the test in both
    dtypes.  (2^-8, not 2^-9: bf16 keeps 8 significant bits, so a value just above a power of two rounds by up to 2^-8 of itself; with 2^-9
    the correctly rounded float64 y itself fails on one element in four -- test_ln_reference_cpu.py holds both ends.)"""
    den = R.gamma.abs() * R.S[:, None] + R.beta.abs()
    d = (_64(got) - R.y).abs()
    if lim is not None:
        a = (lim[:, None] if isinstance(lim, torch.Tensor) else lim) * den
        d = (d - BF16_HALF_ULP * (R.y.abs() + a)).clamp(min=0.0)
    return _ratio(d, den).amax(1)


def err_mean(got, R):
    return _ratio((_64(got) - R.mean).abs(), R.xmax)


def err_rstd(got, R):
    return _ratio((_64(got) - R.rstd).abs(), R.rstd)


def err_dx(got, R, old=None):
    """Per row: max_c |ddx_rc| / (rstd_r G_r max(S_r, 1) + |old_rc|); old = what was accumulated into (None: nothing).
    The direct term (the 1): in dx = rstd (g - m1 - xhat m2) the roundings of g = dy gamma, of m1 = mean_c(g) and of their difference are each
    eps/2 of G_r whatever x is, so |ddx| reaches about 2 eps rstd G on every row.  rstd G S covers that only while S >= 1, which max |xhat|
    grants every row whose variance is well above the LayerNorm's 1e-5; on a row of 1e-4 N(0, 1) (rstd = 316, S = 0.06 to 0.1) both this
    module's plain fp32 restatement and its kernel-order one measure 10 to 27 eps against rstd G S alone, and 1 to 2 eps with the term."""
    want, den = R.dx, (R.rstd * R.G * R.S.clamp(min=1.0))[:, None]
    if old is not None:
        want, den = want + _64(old), den + _64(old).abs()
    return _ratio((_64(got) - want).abs(), den.expand_as(want)).amax(1)


def err_dgamma(got, R, prefill=0.0):
    return _ratio((_64(got) - (R.dgamma + prefill)).abs(), (R.dy.abs() * R.S[:, None]).sum(0) + abs(prefill))


def err_dbeta(got, R, prefill=0.0):
    return _ratio((_64(got) - (R.dbeta + prefill)).abs(), R.dy.abs().sum(0) + abs(prefill))


QUANTITIES = ("y", "mean", "rstd", "dx", "dgamma", "dbeta")


def all_errors(out, R, old=None, prefill=(0.0, 0.0), bf16_lim=None):
    """{quantity: error tensor} of a result dict with the keys of `plain_fp32` (those present)."""
    fns = dict(y=lambda t: err_y(t, R, bf16_lim), mean=lambda t: err_mean(t, R), rstd=lambda t: err_rstd(t, R), dx=lambda t: err_dx(t, R, old),
               dgamma=lambda t: err_dgamma(t, R, prefill[0]), dbeta=lambda t: err_dbeta(t, R, prefill[1]))
    return {q: fns[q](out[q]) for q in QUANTITIES if q in out}


def worst(e):
    """The largest entry; NaN if any is NaN."""
    return float("nan") if bool(torch.isnan(e).any()) else float(e.max())


# ---------------------------------------------------------------------------------------------- the yardstick
def plain_fp32(x, gamma, beta, dy, old=None, prefill=(0.0, 0.0), variant=None):
    """The operation in plain fp32: two-pass statistics with torch's CPU sums, the backward given these fp32 mean / rstd.  Shares nothing with
    the code under test.  variant: one of the altered restatements that the bound must reject (tests/test_ln_reference_cpu.py)."""
    x, gamma, beta, dy = (t.detach().cpu().to(F32) for t in (x, gamma, beta, dy))
    C = x.shape[1]
    eps = torch.tensor(LN_EPS, dtype=F32)
    mean = x.sum(1) / C
    d = x - mean[:, None]
    var = (d * d).sum(1) / C
    if variant == "one_pass":
        var = (x * x).sum(1) / C - mean * mean
    if variant == "unbiased":
        var = (d * d).sum(1) / (C - 1)
    rstd = 1.0 / torch.sqrt(var + eps)
    if variant == "eps_outside":
        rstd = 1.0 / (torch.sqrt(var.clamp(min=0.0)) + eps)
    xhat = d * rstd[:, None]
    y = xhat * gamma + beta
    g = dy * gamma
    m1 = g.sum(1, keepdim=True) / C
    if variant == "no_mean_g":
        m1 = torch.zeros_like(m1)
    dx = rstd[:, None] * (g - m1 - xhat * ((g * xhat).sum(1, keepdim=True) / C))
    if old is not None:
        dx = dx + old.detach().cpu().to(F32)
    out = dict(y=y, mean=mean, rstd=rstd, dx=dx, dgamma=(dy * xhat).sum(0) + prefill[0], dbeta=dy.sum(0) + prefill[1])
    assert all(t.dtype == F32 for t in out.values())
    return out


def e_plain(R, old=None, prefill=(0.0, 0.0)):
    """{quantity: the yardstick's error in that quantity's metric, per row (y, mean, rstd, dx) or per column (dgamma, dbeta)} on the inputs
    of R.  Kept per row: the yardstick's own bad rows (torch's blocked sum of a constant row is not exact, and its rstd there is off by
    hundreds of eps; the kernels' butterfly of equal values is exact) must not loosen the bound of the others."""
    return all_errors(plain_fp32(R.x, R.gamma, R.beta, R.dy, old, prefill), R, old, prefill)


def bounds(R, old=None, prefill=(0.0, 0.0)):
    """{quantity: bound per row / per column}."""
    return {q: bound(e) for q, e in e_plain(R, old, prefill).items()}


def over(e, lim):
    """How many entries miss their bound (a NaN misses)."""
    return int((~(e <= lim)).sum())


# ---------------------------------------------------------------------------------------------- the dispatch
def geometry(C):
    """(lanes per row, rows per wave, float4 per lane) of ln_geometry."""
    lpr = min(C // 4, 64)
    return lpr, 64 // lpr, C // (4 * lpr)


def accepted(C):
    return 16 <= C <= 1024 and C & (C - 1) == 0


def bwd_block(C):
    return 256 if C >= 1024 else 1024


def expected_launch(op, dtype, rows, C):
    """((kernel, dtype, NV), grid, block) of one call, the three launchers restated.  op: "fwd", "bwd", "mask_cast"; dtype: "f32" / "bf16"
    (the output type forward, dy's type backward)."""
    if op == "mask_cast":
        return ("mask_cast", dtype, None), min(-(-(rows * C // 4) // 256), MASK_MAX_GRID), 256
    lpr, rpw, nv = geometry(C)
    if op == "fwd":
        return ("ln_fwd", dtype, nv), min(-(-rows // (4 * rpw)), FWD_MAX_GRID), 256
    block = bwd_block(C)
    return ("ln_bwd", dtype, nv), min(-(-rows // (rpw * (block // 64) * 2)), BWD_MAX_GRID), block


def passes(op, rows, C):
    """(trips of the busiest workgroup round its row loop, whether the last trip is ragged: some lane or workgroup without a row)."""
    _, grid, block = expected_launch(op, "f32", rows, C)
    work, per = (rows * C // 4, grid * 256) if op == "mask_cast" else (rows, grid * (block // 64) * geometry(C)[1])
    return -(-work // per), work % per != 0


_TY = {"f": "f32", "float": "f32", "DF16b": "bf16", "__bf16": "bf16"}
_KERNEL_NAMES = [   # mangled (what the launch trace records), then demangled (its fallback)
    (re.compile(r"ln_(fwd|bwd)_kernelI(f|DF16b)Li(\d+)E"), lambda m: (f"ln_{m[1]}", _TY[m[2]], int(m[3]))),
    (re.compile(r"ln_(fwd|bwd)_kernel<(float|__bf16), ?(\d+)>"), lambda m: (f"ln_{m[1]}", _TY[m[2]], int(m[3]))),
    (re.compile(r"mask_cast_kernelI(f|DF16b)E"), lambda m: ("mask_cast", _TY[m[1]], None)),
    (re.compile(r"mask_cast_kernel<(float|__bf16)>"), lambda m: ("mask_cast", _TY[m[1]], None)),
]


def kernel_ident(name):
    """A trace record's kernel name -> (kernel, dtype, NV) or None for a kernel that is not one of norm.hip's three."""
    for pat, fn in _KERNEL_NAMES:
        m = pat.search(name)
        if m:
            return fn(m)
    return None


# ---------------------------------------------------------------------------------------------- the kernels' order in fp32
def _tree(s, ascending):
    """The butterfly over the last axis: every lane ends with the same value, so it is a pairwise tree.  ascending: xor 1, 2, 4, ... (the DPP
    row sum and the whole-row shuffles behind it, and the backward's cross-row fold); else xor n/2, ..., 1 (rows of 4 and 8 lanes)."""
    while s.shape[-1] > 1:
        h = s.shape[-1] // 2
        s = s[..., 0::2] + s[..., 1::2] if ascending else s[..., :h] + s[..., h:]
    return s[..., 0]


def _lane_sum(t, lpr, nv):
    """t [rows, C] -> [rows]: ((a + b) + c) + d per float4, the lane's float4s in turn, then the butterfly over the row's lanes."""
    t = t.reshape(t.shape[0], nv, lpr, 4)
    q = ((t[..., 0] + t[..., 1]) + t[..., 2]) + t[..., 3]
    s = q[:, 0]
    for k in range(1, nv):
        s = s + q[:, k]
    return _tree(s, lpr >= 16)


def kernel_order_fp32(x, gamma, beta, dy, old=None, prefill=(0.0, 0.0), bwd_grid=None, wrong_lpr=False, drop_last_pass=False):
    """ln_fwd_kernel / ln_bwd_kernel in torch fp32 on the CPU, add for add: four adds per lane and float4, a butterfly over the row's lanes,
    lane-private column partials over the grid-stride rows, the fold over the rows of a wave, the waves of a workgroup in turn, the
    workgroups in index order onto the prefilled sums (the GPU's atomics arrive in any order).  What it does not restate: rsqrtf's own
    rounding and the compiler's FMA contraction.
    wrong_lpr: the row reductions run over twice the lanes, taking in the neighbouring row.  drop_last_pass: the column sums leave out the
    rows of the last, ragged trip round the grid."""
    x, gamma, beta, dy = (t.detach().cpu().to(F32) for t in (x, gamma, beta, dy))
    rows, C = x.shape
    lpr, rpw, nv = geometry(C)
    eps = torch.tensor(LN_EPS, dtype=F32)

    def row_sum(t):
        if not wrong_lpr:
            return _lane_sum(t, lpr, nv)
        assert nv == 1 and rows % 2 == 0
        s = _lane_sum(t.reshape(rows // 2, 2 * C), 2 * lpr, 1)       # lanes of two rows in one butterfly
        return s.repeat_interleave(2)

    mean = row_sum(x) / C
    d = x - mean[:, None]
    rstd = 1.0 / torch.sqrt(row_sum(d * d) / C + eps)
    xhat = d * rstd[:, None]
    y = xhat * gamma + beta
    g = dy * gamma
    m1, m2 = row_sum(g) / C, row_sum(g * xhat) / C
    dx = rstd[:, None] * ((g - m1[:, None]) - xhat * m2[:, None])
    if old is not None:
        dx = dx + old.detach().cpu().to(F32)
    # column sums
    grid = bwd_grid or expected_launch("bwd", "f32", rows, C)[1]
    wpb = bwd_block(C) // 64
    per = grid * wpb * rpw
    trips = -(-rows // per)
    cols = []
    for p, fill in ((dy * xhat, prefill[0]), (dy, prefill[1])):
        pad = torch.zeros(trips * per, C, dtype=F32)
        pad[:rows] = p
        pad = pad.reshape(trips, grid * wpb, rpw, C)
        if drop_last_pass:
            pad = pad[:rows // per]
        lane = torch.zeros(grid * wpb, rpw, C, dtype=F32)
        for t in range(pad.shape[0]):
            lane = lane + pad[t]
        wave = _tree(lane.transpose(1, 2), True).reshape(grid, wpb, C)
        acc = torch.full((C,), fill, dtype=F32)
        blk = torch.zeros(grid, C, dtype=F32)
        for w in range(wpb):
            blk = blk + wave[:, w]
        for b in range(grid):
            acc = acc + blk[b]
        cols.append(acc)
    return dict(y=y, mean=mean, rstd=rstd, dx=dx, dgamma=cols[0], dbeta=cols[1])


# ---------------------------------------------------------------------------------------------- the mask's row / rows_per_sample
def magic(rps):
    return 0xFFFFFFFF // rps + 1


def magic_div(row, rps):
    """__umulhi(row, magic): what store_masked4_row takes for row / rps (row: int or an int64 tensor below 2^32)."""
    m = magic(rps)
    if isinstance(row, torch.Tensor):          # 64-bit product of two 32-bit values does not fit int64: split the row
        hi, lo = row >> 16, row & 0xFFFF
        return (hi * m + ((lo * m) >> 16)) >> 16
    return (row * m) >> 32


# ---------------------------------------------------------------------------------------------- inputs
KINDS = ("normal", "offset", "ramp", "constant")


def row_kinds(rows, tiny):
    """Kind index per row: r % 4 over KINDS; with tiny, every row with r % 8 == 4 is a 1e-4 N(0, 1) row instead (index 4)."""
    r = torch.arange(rows)
    k = r % 4
    return torch.where(r % 8 == 4, torch.full_like(k, 4), k) if tiny else k


def make_inputs(rows, C, seed, bf16=False, tiny=False):
    """(x [rows, C], gamma, beta, dy, old) fp32 on the CPU.  All rows of one call mix the kinds, so one launch covers them all and a leak
    between the rows that share a wave shows: 2 N + 0.5; N + 100; a ramp with mean 10 (r % 97) and std 1 + r % 5; constant rows, the
    value 50 N per row; (tiny) 1e-4 N.  gamma = 1 + 0.1 N, beta = 0.1 N, dy = N (rounded to bf16 first in the bf16 cases), old = N."""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    n = torch.randn(rows, C, generator=gen)
    r = torch.arange(rows)
    ramp = (torch.arange(C, dtype=F64) - (C - 1) / 2) / ((C * C - 1) / 12.0) ** 0.5               # mean 0, biased variance 1
    ramp = (10.0 * (r % 97))[:, None] + (1.0 + r % 5)[:, None] * ramp[None]
    const = (50.0 * torch.randn(rows, generator=gen))[:, None].expand(rows, C)
    kind = row_kinds(rows, tiny)[:, None]
    x = torch.where(kind == 0, 2 * n + 0.5, torch.where(kind == 1, n + 100.0, torch.where(kind == 2, ramp.to(F32), torch.where(kind == 3, const, 1e-4 * n))))
    gamma = 1 + 0.1 * torch.randn(C, generator=gen)
    beta = 0.1 * torch.randn(C, generator=gen)
    dy = torch.randn(rows, C, generator=gen)
    if bf16:
        dy = dy.bfloat16().float()
    old = torch.randn(rows, C, generator=gen)
    return x.contiguous(), gamma, beta, dy, old


# ---------------------------------------------------------------------------------------------- the table
# kind "ln": forward, backward into a NaN-filled dx, backward accumulating onto `old`.  gather: (B, H, W) or None.  fwd / bwd: the grids the
# case is FOR, written out; regime: what the busiest forward and backward workgroups do -- "one" (a single trip), "cap" (the grid is at its
# cap), "ragged" (a later trip that leaves lanes or workgroups without a row).  test_ln_reference_cpu.py holds them against expected_launch,
# the GPU test holds expected_launch against the launch trace.
Case = namedtuple("Case", "id kind C bf16 rows gather tiny fwd bwd seed")
PREFILL = (0.5, -0.5)


def case_rows(C):
    """{name: rows} of the plain cases at this width: one row; one more than a wave holds; R_mid; R_big = a full forward grid at its cap plus
    R_mid rows -- a ragged second forward trip and a ragged third (C = 1024: ninth) backward trip."""
    rpw = geometry(C)[1]
    mid = 37 * rpw + 1
    return {"one": 1, "wave+1": rpw + 1 if rpw > 1 else 3, "mid": mid, "big": FWD_MAX_GRID * 4 * rpw + mid}


_PLAIN_GRIDS = {"one": (1, 1, 1), "wave+1": (1, 1, 1), "mid": (10, 2, 5), "big": (2048, 256, 256)}     # fwd, bwd below 1024, bwd at 1024
_GATHER_45 = {16: (1, 1), 32: (2, 1), 64: (3, 1), 128: (6, 1), 256: (12, 2), 512: (12, 2), 1024: (12, 6)}


def _dt(bf16):
    return "bf16" if bf16 else "f32"


def _ln_cases():
    out = []
    for C in WIDTHS:
        for bf16 in (False, True):
            for name, rows in case_rows(C).items():
                fwd, b1, b2 = _PLAIN_GRIDS[name]
                out.append(Case(f"c{C}-{_dt(bf16)}-{name}", "ln", C, bf16, rows, None, name == "mid", fwd, b2 if C >= 1024 else b1, 100 * C + len(out)))
    for C in WIDTHS:
        for bf16 in (False, True):
            out.append(Case(f"gather-c{C}-{_dt(bf16)}-1x2x2", "ln", C, bf16, 1, (1, 2, 2), False, 1, 1, 100 * C + len(out)))
            out.append(Case(f"gather-c{C}-{_dt(bf16)}-3x6x10", "ln", C, bf16, 45, (3, 6, 10), False, *_GATHER_45[C], 100 * C + len(out)))
    for bf16 in (False, True):   # beyond the caps: 32 802 rows at 64 channels (both), 2106 rows at 1024 (the backward's only)
        out.append(Case(f"gather-c64-{_dt(bf16)}-7x132x142", "ln", 64, bf16, 32802, (7, 132, 142), False, 2048, 256, 6400 + len(out)))
        out.append(Case(f"gather-c1024-{_dt(bf16)}-3x52x54", "ln", 1024, bf16, 2106, (3, 52, 54), False, 527, 256, 102400 + len(out)))
    return out


# kind "mask": the masked copy of layernorm_bwd and mask_cast on the [288, 64] token tensor of B, H, W = 4, 6, 12.
# layout "plain": C = 64, 288 rows; "gather": C = 256 (Cin = 64), 72 rows.  p = (p_elem, p_path); rps = rows_per_sample (100 does not divide 288).
MaskCase = namedtuple("MaskCase", "id kind layout bf16 p rps")
MASK_BHW, MASK_CIN = (4, 6, 12), 64
MASK_PS = ((0.2, 0.0), (0.0, 0.1), (0.2, 0.1))
MASK_RPS = (1, 72, 100)
MASK_CAST_BIG = (9217, 256)          # 589 888 float4 on 2048 x 256 lanes: a ragged second trip


def _mask_cases():
    return [MaskCase(f"mask-{layout}-{_dt(bf16)}-e{p[0]}-p{p[1]}-rps{rps}", "mask", layout, bf16, p, rps)
            for layout in ("plain", "gather") for bf16 in (False, True) for p in MASK_PS for rps in MASK_RPS]


LN_CASES = _ln_cases()
MASK_CASES = _mask_cases()
CASES = LN_CASES + MASK_CASES
CASE_IDS = [c.id for c in CASES]


def regime(op, rows, C):
    trips, ragged = passes(op, rows, C)
    cap = expected_launch(op, "f32", rows, C)[1] == {"fwd": FWD_MAX_GRID, "bwd": BWD_MAX_GRID, "mask_cast": MASK_MAX_GRID}[op]
    return "one" if trips == 1 else ("ragged" if ragged else "cap") + f"-{trips}" if cap else "several"
