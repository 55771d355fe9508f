"""The yardstick of the LayerNorm kernel tests, checked without a GPU: the bound of tests/ln_reference.py is attainable by an fp32
restatement of the kernels' own summation order at every width, input kind and quantity; it rejects each of seven subtly wrong
restatements; the mask's magic division is exact where the launchers' guard allows it and not beyond; and the restated dispatch gives the
grids the table says each case is for, with every grid regime reached."""
import pytest
import torch

import ln_reference as lr


def _measure(C, name, bf16=False, seed=None):
    rows = lr.case_rows(C)[name]
    x, g, b, dy, old = lr.make_inputs(rows, C, seed or 31 * C, bf16, tiny=(name == "mid"))
    R = lr.reference(x, g, b, dy)
    return rows, (x, g, b, dy, old), R, lr.bounds(R, old, lr.PREFILL)


def _misses(out, R, lim, old, which=None):
    """{quantity: entries over their bound}"""
    errs = lr.all_errors(out, R, old, lr.PREFILL)
    return {q: lr.over(e, lim[q]) for q, e in errs.items() if which is None or q in which}


ATTAIN = [(C, name) for C in lr.WIDTHS for name in ("one", "wave+1", "mid")] + [(16, "big"), (64, "big"), (1024, "big")]


@pytest.mark.parametrize("C,name", ATTAIN, ids=[f"c{C}-{n}" for C, n in ATTAIN])
def test_kernel_order_fp32_meets_the_bound(C, name):
    """The kernels' order of additions in fp32 against float64: every row and column of every quantity within max(4 E_plain, 8 * 2^-23),
    on every input kind (the mid cases hold the tiny rows), fp32 and bf16 dy, accumulating onto `old` and not."""
    for bf16 in (False, True):
        rows, (x, g, b, dy, old), R, lim = _measure(C, name, bf16)
        out = lr.kernel_order_fp32(x, g, b, dy, old, lr.PREFILL)
        errs = lr.all_errors(out, R, old, lr.PREFILL)
        print(f"C {C} {name} ({rows} rows) {'bf16' if bf16 else 'f32'}: " + " ".join(f"{q} {lr.worst(e) / lr.EPS:.2f}" for q, e in errs.items()) + " eps")
        assert not any(_misses(out, R, lim, old).values()), _misses(out, R, lim, old)
        fresh = lr.kernel_order_fp32(x, g, b, dy, None, lr.PREFILL)
        assert lr.over(lr.err_dx(fresh["dx"], R), lr.bound(lr.err_dx(lr.plain_fp32(x, g, b, dy)["dx"], R))) == 0


def test_e_plain_of_an_ordinary_row_is_below_the_floor():
    """On the normal, offset and ramp rows the yardstick stays under 2 eps in the row metrics, so the 8-eps floor is the bound there; the
    rows where it does not are its own constant rows (a blocked sum of equal values is not exact)."""
    for C in lr.WIDTHS:
        rows, (x, g, b, dy, old), R, _ = _measure(C, "mid")
        E = lr.e_plain(R, old, lr.PREFILL)
        kinds = lr.row_kinds(rows, True)
        for q in ("y", "mean", "rstd", "dx"):
            assert float(E[q][kinds < 3].max()) < 4 * lr.EPS, (C, q)


@pytest.mark.parametrize("C", lr.WIDTHS)
def test_altered_statistics_fail_the_bound(C):
    rows, (x, g, b, dy, old), R, lim = _measure(C, "mid")
    kinds = lr.row_kinds(rows, True)
    # one-pass variance: E[x^2] - mean^2 cancels on the offset (kind 1) and ramp (kind 2) rows
    out = lr.plain_fp32(x, g, b, dy, old, lr.PREFILL, variant="one_pass")
    bad = ~(lr.err_rstd(out["rstd"], R) <= lim["rstd"])
    assert bad[kinds == 1].any() and bad[kinds == 2].any()
    assert (~(lr.err_y(out["y"], R) <= lim["y"]))[(kinds == 1) | (kinds == 2)].any()
    # unbiased variance: rstd off by 1 / 2C (5e-4 at 1024) on every row that has a variance
    out = lr.plain_fp32(x, g, b, dy, old, lr.PREFILL, variant="unbiased")
    bad = ~(lr.err_rstd(out["rstd"], R) <= lim["rstd"])
    assert bad[kinds < 3].all(), C
    assert (~(lr.err_y(out["y"], R) <= lim["y"]))[kinds < 3].any() and (~(lr.err_dx(out["dx"], R, old) <= lim["dx"]))[kinds < 3].any()
    # eps outside the square root: shows where the variance is not far above it -- the constant (kind 3) and tiny (kind 4) rows
    out = lr.plain_fp32(x, g, b, dy, old, lr.PREFILL, variant="eps_outside")
    bad = ~(lr.err_rstd(out["rstd"], R) <= lim["rstd"])
    assert bad[kinds == 3].all() and bad[kinds == 4].all()
    assert (~(lr.err_y(out["y"], R) <= lim["y"]))[kinds == 4].all() and (~(lr.err_dx(out["dx"], R, old) <= lim["dx"]))[kinds >= 3].all()
    # dx without the mean_c(g) term
    out = lr.plain_fp32(x, g, b, dy, old, lr.PREFILL, variant="no_mean_g")
    bad = ~(lr.err_dx(out["dx"], R, old) <= lim["dx"])           # (a constant row's allowance carries its S of 1e3 to 1e5: most still miss)
    assert bad[kinds != 3].all() and bad.double().mean() > 0.8
    assert not any(_misses(out, R, lim, old, which=("y", "mean", "rstd", "dgamma", "dbeta")).values())


@pytest.mark.parametrize("C", [16, 32])
def test_a_reduction_over_the_neighbouring_rows_lanes_fails_the_bound(C):
    """The wrong lanes-per-row: rows of 4 and 8 lanes reduced over 8 and 16, so two rows of different kinds share their sums."""
    rows = 37 * lr.geometry(C)[1] + 2
    x, g, b, dy, old = lr.make_inputs(rows, C, 5 * C)
    R = lr.reference(x, g, b, dy)
    lim = lr.bounds(R, old, lr.PREFILL)
    good = lr.kernel_order_fp32(x, g, b, dy, old, lr.PREFILL)
    assert not any(_misses(good, R, lim, old).values())
    out = lr.kernel_order_fp32(x, g, b, dy, old, lr.PREFILL, wrong_lpr=True)
    m = _misses(out, R, lim, old)
    assert min(m["mean"], m["rstd"], m["y"], m["dx"]) >= 0.95 * rows and m["dgamma"] > 0, m


@pytest.mark.parametrize("C", [16, 256])
def test_a_gather_with_x10_and_x01_swapped_fails_the_bound(C):
    B, H, W = 3, 6, 10
    rows = B * (H // 2) * (W // 2)
    cat, g, b, dy, old = lr.make_inputs(rows, C, 9 * C)
    x4 = lr.scatter_tokens(cat, B, H, W)
    assert torch.equal(lr.gather_cat(x4), cat) and x4.shape == (B, H, W, C // 4)
    # the order is x00, x10, x01, x11: segment 1 of merged row (b, y2, x2) is token (2 y2 + 1, 2 x2)
    assert torch.equal(x4[1, 3, 4], cat[(1 * 3 + 1) * 5 + 2, C // 4:C // 2]) and torch.equal(x4[1, 2, 5], cat[(1 * 3 + 1) * 5 + 2, C // 2:3 * C // 4])
    R = lr.reference(cat, g, b, dy)
    lim = lr.bounds(R, old, lr.PREFILL)
    swapped = lr.gather_cat(lr.scatter_tokens(cat, B, H, W, swap=True))            # what a kernel with the two segments exchanged reads
    out = lr.plain_fp32(swapped, g, b, dy, old, lr.PREFILL)
    m = _misses(out, R, lim, old)
    kinds = lr.row_kinds(rows, False)
    assert not (lr.err_y(out["y"], R) <= lim["y"])[kinds < 3].any(), m              # every row that is not constant
    assert m["dgamma"] > 0 and m["dx"] > 0 and m["mean"] == 0                       # (the mean does not see the order)
    # and the scatter of dx: a dx laid out with the segments exchanged, read back in the right order
    dx4 = lr.scatter_tokens(lr.plain_fp32(cat, g, b, dy)["dx"], B, H, W, swap=True)
    assert lr.over(lr.err_dx(lr.gather_cat(dx4), R), lr.bound(lr.err_dx(lr.plain_fp32(cat, g, b, dy)["dx"], R))) > 0


@pytest.mark.parametrize("C", [16, 64, 1024])
def test_column_sums_that_drop_the_last_ragged_pass_fail_the_bound(C):
    rows, (x, g, b, dy, old), R, lim = _measure(C, "big")
    trips, ragged = lr.passes("bwd", rows, C)
    assert trips >= 3 and ragged
    out = lr.kernel_order_fp32(x, g, b, dy, old, lr.PREFILL, drop_last_pass=True)
    m = _misses(out, R, lim, old)
    assert m["dbeta"] >= 0.99 * C and m["dx"] == 0, m
    # dgamma's allowance, sum_r |dy| S_r, is carried by the offset, ramp and constant rows (S of 1e2 to 1e5: their xhat really is that
    # ill-conditioned), so a few hundred missing rows do not show in it at this row count; dbeta, summed by the same code, shows them.
    # Without those rows (normal rows only) dgamma shows them too:
    xn = lr.make_inputs(rows, C, 31 * C)[0][0::4].repeat_interleave(4, 0)[:rows]
    Rn = lr.reference(xn, g, b, dy)
    outn = lr.kernel_order_fp32(xn, g, b, dy, old, lr.PREFILL, drop_last_pass=True)
    assert lr.over(lr.err_dgamma(outn["dgamma"], Rn, lr.PREFILL[0]), lr.bounds(Rn, old, lr.PREFILL)["dgamma"]) >= 0.99 * C


RPS = (2, 3, 72, 100, 576, 4608, 65535)


@pytest.mark.parametrize("rps", RPS)
def test_magic_division_is_exact_up_to_the_guard_and_not_beyond(rps):
    """store_masked4_row takes row / rps as __umulhi(row, 0xFFFFFFFF / rps + 1).  With magic = (2^32 + e) / rps, 0 <= e < rps, the product's
    high word is floor(row / rps + row e / (rps 2^32)): right for every row with row * e < 2^32, which row * rps < 2^32 -- the launchers'
    guard -- implies.  Beyond the guard the first wrong row is the first one congruent to rps - 1 with row * e >= 2^32 (none when rps is a
    power of two: e = 0)."""
    m = lr.magic(rps)
    e = m * rps - 2 ** 32
    assert 0 <= e < rps
    rmax = (2 ** 32 - 1) // rps                                         # the largest row the guard lets through
    assert rmax * rps < 2 ** 32 <= (rmax + 1) * rps
    n = 200_000
    top = torch.arange(max(rmax - n, 0), rmax + 1, dtype=torch.int64)
    g = torch.Generator().manual_seed(rps)
    rnd = torch.randint(0, rmax + 1, (n,), generator=g, dtype=torch.int64)
    ends = (torch.randint(0, rmax // rps + 1, (n,), generator=g, dtype=torch.int64) * rps + rps - 1).clamp(max=rmax)   # the last row of a sample
    for rows in (torch.arange(0, min(n, rmax + 1), dtype=torch.int64), top, rnd, ends, ends - (rps - 1)):
        assert torch.equal(lr.magic_div(rows, rps), rows // rps)
    assert lr.magic_div(rmax, rps) == rmax // rps == (rmax * m) >> 32
    assert int(lr.magic_div(torch.tensor([rmax], dtype=torch.int64), rps)[0]) == rmax // rps     # (the split product agrees with Python's)
    if e == 0:
        assert rps == 2                                                 # exact for every 32-bit row
        return
    q = -(-(-(-(2 ** 32) // e) - (rps - 1)) // rps)                     # first row = q rps + rps - 1 with row * e >= 2^32
    first = q * rps + rps - 1
    assert first * e >= 2 ** 32 > (first - rps) * e and first > rmax and first < 2 ** 32
    assert lr.magic_div(first, rps) == first // rps + 1                 # wrong: the sample index is one too many
    below = torch.arange(rmax + 1, min(first, rmax + 1 + n), dtype=torch.int64)
    assert torch.equal(lr.magic_div(below, rps), below // rps)          # (the guard is sufficient, not tight)


def test_expected_launch_reproduces_the_table_and_reaches_every_regime():
    seen = {"fwd": set(), "bwd": set()}
    for c in lr.LN_CASES:
        dt = "bf16" if c.bf16 else "f32"
        lpr, rpw, nv = lr.geometry(c.C)
        assert lr.accepted(c.C) and lpr * rpw == 64 and 4 * lpr * nv == c.C and nv in (1, 2, 4)
        if c.gather:
            B, H, W = c.gather
            assert c.rows == B * (H // 2) * (W // 2) and H % 2 == 0 and W % 2 == 0 and (c.C // 4) % 4 == 0
        assert lr.expected_launch("fwd", dt, c.rows, c.C) == (("ln_fwd", dt, nv), c.fwd, 256), c.id
        assert lr.expected_launch("bwd", dt, c.rows, c.C) == (("ln_bwd", dt, nv), c.bwd, 256 if c.C == 1024 else 1024), c.id
        assert c.rows * c.C <= 8.5e6, c.id                               # the largest tensor of the table: 8.4 M elements
        for op in seen:
            seen[op].add((c.C, c.bf16, bool(c.gather), lr.regime(op, c.rows, c.C).split("-")[0]))
    for C in lr.WIDTHS:
        for bf16 in (False, True):
            # plain: a single trip, and a ragged later trip round a capped grid, forward and backward, at every width and dtype
            for op in seen:
                assert (C, bf16, False, "one") in seen[op] and (C, bf16, False, "ragged") in seen[op], (op, C, bf16)
            assert (C, bf16, True, "one") in seen["fwd"] and (C, bf16, True, "one") in seen["bwd"]
    for bf16 in (False, True):
        assert (64, bf16, True, "ragged") in seen["fwd"] and (64, bf16, True, "ragged") in seen["bwd"] and (1024, bf16, True, "ragged") in seen["bwd"]
    # the trips themselves
    for C in lr.WIDTHS:
        big = lr.case_rows(C)["big"]
        assert lr.passes("fwd", big, C) == (2, True)
        assert lr.passes("bwd", big, C) == ((9, True) if C == 1024 else (3, True))
        assert lr.passes("fwd", lr.case_rows(C)["mid"], C) == (1, True) and lr.passes("fwd", 1, C) == (1, True)
    assert lr.passes("bwd", 32802, 64) == (3, True) and lr.passes("fwd", 32802, 64) == (2, True) and lr.passes("bwd", 2106, 1024) == (3, True)
    # a grid exactly at its cap with one full trip, and one row more: the cap is where the second trip starts
    assert lr.expected_launch("fwd", "f32", 2048 * 16, 64)[1] == 2048 and lr.passes("fwd", 2048 * 16, 64) == (1, False)
    assert lr.passes("fwd", 2048 * 16 + 1, 64) == (2, True)
    assert lr.expected_launch("bwd", "f32", 256 * 8, 1024)[1:] == (256, 256) and lr.expected_launch("bwd", "bf16", 256 * 32, 512)[1:] == (256, 1024)
    # mask_cast: the 288 x 64 token tensor in one trip, 9217 x 256 in a ragged second
    assert lr.expected_launch("mask_cast", "bf16", 288, 64) == (("mask_cast", "bf16", None), 18, 256) and lr.passes("mask_cast", 288, 64) == (1, False)
    assert lr.expected_launch("mask_cast", "f32", *lr.MASK_CAST_BIG)[1] == 2048 and lr.passes("mask_cast", *lr.MASK_CAST_BIG) == (2, True)
    assert len({c.id for c in lr.CASES}) == len(lr.CASES)
    assert len(lr.MASK_CASES) == 2 * 2 * 3 * 3
    for C in (8, 48, 2048, 12, 0):
        assert not lr.accepted(C)


def test_kernel_ident_reads_both_spellings():
    assert lr.kernel_ident("_Z13ln_fwd_kernelIfLi1EEvPKfS1_S1_PT_Pfiiif6RowMap") == ("ln_fwd", "f32", 1)
    assert lr.kernel_ident("_Z13ln_bwd_kernelIDF16bLi4EEvPKT_PKfS4_S4_Pfi") == ("ln_bwd", "bf16", 4)
    assert lr.kernel_ident("void ln_bwd_kernel<float, 2>(float const*, float const*)") == ("ln_bwd", "f32", 2)
    assert lr.kernel_ident("void ln_fwd_kernel<__bf16, 4>(float const*)") == ("ln_fwd", "bf16", 4)
    assert lr.kernel_ident("_Z16mask_cast_kernelIDF16bEvPKfPT_l15focal_drop_desci") == ("mask_cast", "bf16", None)
    assert lr.kernel_ident("void mask_cast_kernel<float>(float const*, float*, long, focal_drop_desc, int)") == ("mask_cast", "f32", None)
    assert lr.kernel_ident("_Z12adamw_kernelPf") is None


def test_metrics_flag_one_element_and_an_unwritten_one():
    rows, (x, g, b, dy, old), R, lim = _measure(64, "mid")
    out = lr.plain_fp32(x, g, b, dy, old, lr.PREFILL)
    assert not any(_misses(out, R, lim, old).values())
    y = out["y"].clone()
    y[17, 5] += 1e-3 * float(R.gamma[5].abs() * R.S[17] + R.beta[5].abs())
    e = lr.err_y(y, R)
    assert lr.over(e, lim["y"]) == 1 and abs(float(e[17]) - 1e-3) < 1e-5
    y = out["y"].clone()
    y[3, 0] = float("nan")
    assert lr.over(lr.err_y(y, R), lim["y"]) == 1 and lr.worst(lr.err_y(y, R)) != lr.worst(lr.err_y(y, R))
    # bf16: the rounding of a right value passes, the next bf16 value does not
    yb = out["y"].bfloat16()
    assert lr.over(lr.err_y(yb, R, lim["y"]), lim["y"]) == 0
    exact = R.y.float().bfloat16()                          # the float64 y itself, rounded: inside the allowance, and beyond 2^-9 of |y|
    assert lr.over(lr.err_y(exact, R, lim["y"]), lim["y"]) == 0
    off = (exact.double() - R.y).abs() / R.y.abs()
    assert 2.0 ** -9 < float(off.max()) <= 2.0 ** -8 and float((off > 2.0 ** -9).double().mean()) > 0.1
    up = yb.clone()
    up[20, 7] = (yb[20, 7].float() * (1 + 2.0 ** -7)).bfloat16()
    assert up[20, 7] != yb[20, 7] and lr.over(lr.err_y(up, R, lim["y"]), lim["y"]) == 1
    # the column metric sees one dropped row
    dg = out["dgamma"] - (dy[9] * ((x[9] - out["mean"][9]) * out["rstd"][9]))
    assert lr.over(lr.err_dgamma(dg, R, lr.PREFILL[0]), lim["dgamma"]) > 0
