"""What the DFT kernels of focal_amd/csrc/fft.hip are measured against: the float64 expectation (the restatement of test_augment_ex_cpu.py),
a plain fp32 matrix DFT as the yardstick of what fp32 can do on the same rows, the error metric and its bound, an fp32 restatement of the
four-step algorithm (the bound must be attainable by a correct fp32 implementation), the dispatch of fft_launch_t / fft_multi restated,
and the table of cases -- every kernel form at every length and grid regime it accepts.  A plain helper module: no fixtures, no GPU."""
import functools
import math
import re
from collections import namedtuple

import numpy as np
import torch

from test_augment_ex_cpu import restate, restate_time, restated_noise

EPS = 2.0 ** -23
# row_error <= max(MARGIN * E_plain, FLOOR).  MARGIN: the four-step form has at most four rounding stages (two summations, the inner
# twiddle product, the output rotation), each no worse than the yardstick's single summation.  FLOOR: on an impulse row the yardstick is
# exact apart from one table rounding, while a four-step bin is a product of up to three rounded table entries and a rotation.
MARGIN, FLOOR = 4.0, 8 * EPS
PLAIN_ROWS = 64          # E_plain is taken on the first min(rows, 64) augmented rows


# ---------------------------------------------------------------------------------------------- float64 expectation
def _restate_kw(x, aug):
    """The keywords of ops.fft_realpack -> those of `restate` (jitter=(std, key) / noise_salt= become the noise tensor added)."""
    kw = {k: aug[k] for k in ("scale", "flip", "perm", "phase", "chan", "time_mask", "freq_mask") if aug.get(k) is not None}
    if aug.get("jitter") is not None:
        std, key = aug["jitter"]
        kw["noise"] = restated_noise(key, aug.get("noise_salt") or 0, tuple(x.shape)) * std
    return kw


def packed_fp64(x, **aug):
    """float64 [B, 2C, I, n]: what the transform of x [B, C, I, n] with these keywords is."""
    return restate(x.cpu(), **_restate_kw(x, aug))


def augmented_fp64(x, **aug):
    """float64 [B, C, I, n]: the time-domain rows the transform is taken of (x_aug of `row_error`)."""
    kw = _restate_kw(x, aug)
    kw.pop("phase", None)
    kw.pop("freq_mask", None)
    return restate_time(x.cpu(), **kw)


# ---------------------------------------------------------------------------------------------- the yardstick
@functools.lru_cache(maxsize=2)
def _plain_table(n):
    j = np.arange(n, dtype=np.int64)
    ang = 2.0 * np.pi * ((j[:, None] * j[None, :]) % n).astype(np.float64) / n
    return np.concatenate([np.cos(ang), -np.sin(ang)], axis=1).astype(np.float32)    # [n, 2n]: rounded ONCE


def plain_fp32_dft(rows):
    """[R, n] -> (Re, Im) fp32 [R, n]: one rows @ W product in numpy float32.  Shares nothing with the code under test."""
    rows = np.ascontiguousarray(np.asarray(rows, dtype=np.float32))
    n = rows.shape[1]
    y = rows @ _plain_table(n)
    assert y.dtype == np.float32
    return y[:, :n], y[:, n:]


# ---------------------------------------------------------------------------------------------- the metric
def _np64(a):
    return (a.detach().cpu().double().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, dtype=np.float64))


def _rows_error(re, im, ref_re, ref_im, xrows):
    """[R, n] each -> [R]: max_k max(|dRe|, |dIm|) / ||x_row||_2.  A row whose x is all zero must be exactly 0 (error 0, else inf).  A NaN
    anywhere in a row makes its error NaN, which no bound accepts."""
    d = np.maximum(np.abs(re - ref_re), np.abs(im - ref_im)).max(axis=1)
    norm = np.sqrt((xrows * xrows).sum(axis=1))
    zero = norm == 0.0
    exact0 = (re == 0.0).all(axis=1) & (im == 0.0).all(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = d / norm
    e[zero] = np.where(exact0[zero], 0.0, np.inf)
    return e


def _unpack(p):
    """packed [B, 2C, I, n] -> (Re, Im) as [B*C*I, n]"""
    p = _np64(p)
    B, C2, I, n = p.shape
    q = p.reshape(B, C2 // 2, 2, I, n)
    return q[:, :, 0].reshape(-1, n), q[:, :, 1].reshape(-1, n)


def row_error(got, ref64, x_aug64):
    """Per output row (b, c, i) of a packed [B, 2C, I, n] result: max_k max(|dRe|, |dIm|) / ||x_aug_row||_2 -> float64 [B*C*I].
    Invariant to the row's scale, and to a DC offset in the sense that the offset's own bin does not set the scale of the others."""
    re, im = _unpack(got)
    rr, ri = _unpack(ref64)
    xr = _np64(x_aug64)
    return _rows_error(re, im, rr, ri, xr.reshape(-1, xr.shape[-1]))


def e_plain(x_aug64):
    """The largest row error of the yardstick on the first min(rows, 64) augmented rows (their fp32 roundings: what a kernel is handed)."""
    xr = _np64(x_aug64)
    xr = xr.reshape(-1, xr.shape[-1])[:PLAIN_ROWS]
    f = np.fft.fft(xr, axis=-1)
    re, im = plain_fp32_dft(xr.astype(np.float32))
    return float(_rows_error(re.astype(np.float64), im.astype(np.float64), f.real, f.imag, xr).max())


def bound(E_plain):
    return max(MARGIN * E_plain, FLOOR)


# ---------------------------------------------------------------------------------------------- the algorithm in fp32
def four_step_fp32(rows, n1, n2, table=None):
    """The header comment of fft.hip in numpy float32:
         X[k1 + n1*k2] = sum_{m2} W_{n2}^{m2 k2} * ( W_n^{m2 k1} * sum_{m1} x[n2*m1 + m2] W_{n1}^{m1 k1} )
    with every factor read from ONE n-point table {cos, -sin}(2 pi j / n) computed in float64 and rounded to fp32, as the kernels' is.
    [R, n] -> (Re, Im) fp32 [R, n].  table=(cos, -sin): another table (the CPU test shows a carelessly made one fails the bound)."""
    rows = np.asarray(rows, dtype=np.float32)
    R, n = rows.shape
    assert n1 * n2 == n
    ang = 2.0 * np.pi * np.arange(n, dtype=np.float64) / n
    twc, tws = table or (np.cos(ang).astype(np.float32), (-np.sin(ang)).astype(np.float32))
    i1, i2 = np.arange(n1), np.arange(n2)
    t1 = ((i1[:, None] * i1[None, :]) % n1) * n2            # W_n1[m1][k1]
    t2 = ((i2[:, None] * i2[None, :]) % n2) * n1            # W_n2[m2][k2]
    tt = (i2[:, None] * i1[None, :]) % n                    # W_n[m2][k1]
    x = rows.reshape(R, n1, n2)                             # [r, m1, m2]
    re = np.einsum("rab,ak->rbk", x, twc[t1])               # [r, m2, k1]
    im = np.einsum("rab,ak->rbk", x, tws[t1])
    c, s = twc[tt][None], tws[tt][None]
    yr, yi = re * c - im * s, re * s + im * c
    c2, s2 = twc[t2], tws[t2]
    xr = np.einsum("rbk,bq->rkq", yr, c2) - np.einsum("rbk,bq->rkq", yi, s2)   # [r, k1, k2]
    xi = np.einsum("rbk,bq->rkq", yr, s2) + np.einsum("rbk,bq->rkq", yi, c2)
    assert xr.dtype == np.float32 and xi.dtype == np.float32
    # k = k1 + n1*k2
    return xr.transpose(0, 2, 1).reshape(R, n), xi.transpose(0, 2, 1).reshape(R, n)


# ---------------------------------------------------------------------------------------------- the dispatch
MFMA_SIDES = (8, 16, 24, 32, 40, 48)
MFMA_MAX_GRID, GENERIC_MAX_GRID, SMALL_MAX_GRID = 1024, 4096, 1024
SMALL_MAX_N, MULTI_FLUSH = 64, 8
LDS_BYTES = 64 * 1024


def factor(n):
    """The default factorisation (restated: test_fft_reference_cpu.py holds it against ops._factor)."""
    if n <= SMALL_MAX_N:
        return n, 1
    best = max(a for a in range(1, math.isqrt(n) + 1) if n % a == 0)
    return n // best, best


def accepted(n):
    """fft_launch_t's rule: five rows of n floats in 64 KB of LDS."""
    return 5 * n * 4 <= LDS_BYTES


def expected_launch(n, n1, n2, rows, via_multi):
    """(kernel family, grid size) of one transform: fft_launch_t and fft_multi restated.  Families: "small" (fft_small_multi_kernel; the
    grid is this problem's share of the shared launch), "mfma<N>" (fft_realpack_mfma_kernel<N, N>), "generic" (fft_realpack_kernel)."""
    if via_multi and n <= SMALL_MAX_N and n2 == 1 and n1 == n:
        rpb = 256 // n
        return "small", min(-(-rows // rpb), SMALL_MAX_GRID)
    if n1 == n2 and n1 in MFMA_SIDES and rows % 2 == 0:
        return f"mfma{n1}", min(rows // 2, MFMA_MAX_GRID)
    return "generic", min(rows, GENERIC_MAX_GRID)


_KERNEL_NAMES = [   # mangled (what the launch trace records), then demangled (its fallback)
    (re.compile(r"fft_realpack_mfma_kernelILi(\d+)ELi(\d+)ELb([01])E"), lambda m: (f"mfma{m[1]}", m[3] == "1") if m[1] == m[2] else None),
    (re.compile(r"fft_realpack_mfma_kernel<(\d+), ?(\d+), ?(true|false)>"), lambda m: (f"mfma{m[1]}", m[3] == "true") if m[1] == m[2] else None),
    (re.compile(r"fft_realpack_kernelILb([01])E"), lambda m: ("generic", m[1] == "1")),
    (re.compile(r"fft_realpack_kernel<(true|false)>"), lambda m: ("generic", m[1] == "true")),
    (re.compile(r"fft_small_multi_kernelILb([01])E"), lambda m: ("small", m[1] == "1")),
    (re.compile(r"fft_small_multi_kernel<(true|false)>"), lambda m: ("small", m[1] == "true")),
]


def kernel_family(name):
    """A trace record's kernel name -> (family, extended build?) or None for a kernel that is not one of fft.hip's three."""
    for pat, fn in _KERNEL_NAMES:
        m = pat.search(name)
        if m:
            return fn(m)
    return None


# ---------------------------------------------------------------------------------------------- inputs and augmentations
INPUTS = ("normal", "offset", "impulse")
OFFSET = 50.0


def make_input(kind, shape, seed):
    """(a) unit normals, (b) unit normals + 50 (a sensor bias: every non-DC bin becomes a cancellation), (c) impulse rows: row r is 1.0 at
    (7r + 3) mod n.  fp32 [B, C, I, n] on the CPU."""
    B, C, I, n = shape
    if kind == "impulse":
        x = torch.zeros(B * C * I, n)
        r = torch.arange(B * C * I)
        x[r, (7 * r + 3) % n] = 1.0
        return x.reshape(shape)
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(*shape, generator=g)
    return x + OFFSET if kind == "offset" else x


def some_perm(I):
    """A permutation of range(I) that is neither the identity nor a reversal (test_augment_ex_gpu.cases_for's)."""
    return [(3 * i + 1) % I for i in range(I)] if I % 3 else [(i + 1) % I for i in range(I)]


def aug_kwargs(name, shape):
    """The augmentations of the table by name -> keywords of ops.fft_realpack."""
    I = shape[2]
    if name == "identity":
        return {}
    if name == "composed":
        return dict(scale=-1.25, flip=True, perm=some_perm(I), phase=0.7)
    if name == "perm":
        return dict(perm=some_perm(I))
    raise KeyError(name)


# ---------------------------------------------------------------------------------------------- the table
# path: "single" = ops.fft_realpack; "abi" = focal_fft_realpack_fwd / focal_augment_fft_fwd with the descriptor's (n1, n2) named;
# "multi" = ops.fft_realpack_multi; "ex" = the composed case of test_augment_ex_gpu.cases_for (the EX build, through the multi call).
# form / grid / passes are written out: what the case is FOR.  test_fft_reference_cpu.py holds them against expected_launch, the GPU test
# holds expected_launch against the launch trace.  passes = the most trips one workgroup makes round its row loop.
Case = namedtuple("Case", "id path shape n1n2 augs form grid passes")
BOTH = ("identity", "composed")


def _case(id, path, shape, form, grid, passes=1, n1n2=None, augs=BOTH):
    return Case(id, path, shape, tuple(n1n2 or factor(shape[-1])), tuple(augs), form, grid, passes)


CASES = (
    # MFMA, one pass: 60 rows, 30 pairs
    [_case(f"mfma-{n}", "single", (3, 2, 10, n), f"mfma{math.isqrt(n)}", 30) for n in (256, 576, 1024, 1600, 2304)]
    + [_case("mfma-64-abi-8x8", "abi", (3, 2, 10, 64), "mfma8", 30, n1n2=(8, 8))]
    # MFMA, several passes: 2049 pairs (workgroup 0 makes three), 1025 pairs (exactly one workgroup makes a second)
    + [_case("mfma-256-three-passes", "single", (683, 1, 6, 256), "mfma16", 1024, 3),
       _case("mfma-1600-one-second-pass", "single", (205, 1, 10, 1600), "mfma40", 1024, 2)]
    # an odd row count at an MFMA length
    + [_case("odd-rows-1600", "single", (1, 1, 3, 1600), "generic", 3), _case("odd-rows-576", "single", (1, 3, 3, 576), "generic", 9)]
    # generic, one pass (97 is prime: n2 = 1; 3276 = 63 x 52 is the largest length accepted)
    + [_case(f"generic-{n}", "single", (3, 2, 10, n), "generic", 60) for n in (65, 96, 97, 360, 3276)]
    + [_case("generic-20-abi-4x5", "abi", (3, 2, 10, 20), "generic", 60, n1n2=(4, 5)),
       _case("generic-20-abi-1x20", "abi", (3, 2, 10, 20), "generic", 60, n1n2=(1, 20)),
       _case("generic-1600-abi-50x32", "abi", (3, 2, 10, 1600), "generic", 60, n1n2=(50, 32))]
    # generic, several passes (8200 rows); the permutation table's limit (32 intervals)
    + [_case("generic-96-three-passes", "single", (82, 10, 10, 96), "generic", 4096, 3),
       _case("generic-96-perm-32-intervals", "single", (1, 2, 32, 96), "generic", 64, augs=("perm", "composed"))]
    # short rows in the shared launch: 150 rows, 256 // n rows per workgroup, the last workgroup partial (n = 33: 25 lanes idle)
    + [_case(f"small-{n}", "multi", (5, 3, 10, n), "small", g) for n, g in ((1, 1), (2, 2), (3, 2), (7, 5), (20, 13), (33, 22), (63, 38), (64, 38))]
    # short rows, several passes: 2050 and 1050 workgroups' worth on 1024
    + [_case("small-20-three-passes", "multi", (246, 10, 10, 20), "small", 1024, 3),
       _case("small-64-two-passes", "multi", (42, 10, 10, 64), "small", 1024, 2)]
    # the EX build at the lengths it has never run
    + [_case(f"ex-{n}", "ex", (2, 3, 10, n), f"mfma{math.isqrt(n)}", 30, augs=("composed",)) for n in (576, 2304)]
)
CASE_IDS = [c.id for c in CASES]


def case_passes(c):
    """The trips of the busiest workgroup, from the shape and expected_launch."""
    rows, n = c.shape[0] * c.shape[1] * c.shape[2], c.shape[-1]
    fam, grid = expected_launch(n, *c.n1n2, rows, c.path in ("multi", "ex"))
    work = rows // 2 if fam.startswith("mfma") else -(-rows // (256 // n)) if fam == "small" else rows
    return -(-work // grid)


# one multi call: nine short problems, one 576 and one 2304 -- the flush at eight, and the long rows launched in between
MIXED_SHAPES = [(2, 1, 10, 20), (2, 3, 10, 7), (1, 2, 10, 64), (2, 3, 10, 576), (3, 1, 10, 33), (2, 2, 5, 20), (1, 1, 10, 1), (2, 3, 10, 63),
                (4, 1, 10, 20), (2, 3, 10, 2304), (3, 3, 10, 3)]


def expected_mixed_launches(shapes):
    """[(family, grid)] of one multi call over these shapes (default factorisations): short problems gather until eight are held or the call
    ends, long ones are launched where they stand."""
    out, held = [], 0
    count = 0
    for (B, C, I, n) in shapes:
        fam, grid = expected_launch(n, *factor(n), B * C * I, True)
        if fam == "small":
            held += grid
            count += 1
            if count == MULTI_FLUSH:
                out.append(("small", held))
                held = count = 0
        else:
            out.append((fam, grid))
    if count:
        out.append(("small", held))
    return out
