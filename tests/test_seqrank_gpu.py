"""The fused block-pool kernel (focal_seq_rank, ops.seq_rank), the scores built on it (train_utils/temporal.py: sequence_ranking,
neighbour_ranks) and eval_temporal.py end to end.

Exact inputs: every row is an integer centre of its sequence (in [-1, 1] on the first max(1, D / 32) columns, 0 elsewhere, so that the
sequences overlap) plus integer noise in [-1, 1], stored as fp32; the margin is 2.
Every d2 is an exact integer in fp32 and so is every partial sum, either side of the two comparisons and the scaled hinge sum (asserted:
all below 2^24), so with fn = sqdist the outputs equal the int64 brute force in any order of the additions, for every `slices`;
hinge_sum is that integer over L^2 (L^2 - L): one fp32 division.

Real inputs: r = default_rng(seed); per sequence a centre N(0, I) plus sigma_a N(0, I), sigma_a ~ U(0.2, 1.5); fn = dist.  Rounding
bound, u = 2^-24, as tests/test_pairsum_gpu.py derives it: any correct fp32 d2 lies within delta_i = 2 D u (|z_i|^2 + max |z|^2) of the
float64 value, a term sqrt(max(d2, 0)) within e_ij = min(delta_i / sqrt(d2_64), sqrt(delta_i)) + 2 u sqrt(d2_64), so
    |P - P64|(a, b)  <= BP = sum of e_ij over the block + L^2 u P64           (the L^2 fp32 additions)
    |I - I64|(a)     <= BI = sum of e_ij over i != j     + (L^2 - L) u I64
    |inter - inter64|(a) <= sum_b BP(a, b) + (S - 1) u inter64
and, x(a, b) = I / (L^2 - L) - P / L^2 + margin being carried as (I L^2 + margin L^2 (L^2 - L)) - P (L^2 - L) (a product, a sum, a
product, a difference: one rounding each) and divided once after the sum,
    eps(a, b) = BI / (L^2 - L) + BP / L^2 + u (2 I64 / (L^2 - L) + |margin| + P64 / L^2 + |x64|)
    |hinge - hinge64|(a) <= sum_b eps(a, b) + (S - 1) u hinge64 + u hinge64   (the additions, the division)
all times 1 + 1e-5 for the terms of second order in u.  eps(a, b) without its last term bounds the two sides of a comparison against
each other, so each integer count lies between the float64 count of the gaps below -eps and the one of the gaps below +eps.
Condition on the inputs, asserted from the float64 values alone: the pairs whose gap lies inside +-eps are at most 1 % of the ordered
pairs, and the violated share is neither 0 nor 1.  Observed largest error / bound per shape: tests/golden/OBSERVED_temporal.json."""
import copy
import ctypes
import functools
import importlib.util
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import record_observed

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SRC = os.path.join(ROOT, "focal_amd", "src")
DEV = "cuda"
U = 2.0 ** -24
EXACT = [(8, 2, 4), (32, 16, 4), (148, 4, 12), (520, 8, 128), (256, 4, 256), (144, 2, 8), (272, 16, 36)]
REAL = [(148, 4, 12), (148, 4, 128), (520, 8, 256)]
INT_MARGIN = 2
FLOATS = ("intra_sum", "inter_sum", "hinge_sum")
NAMES = ("intra_d2", "intra_sum", "before", "viol", "hinge_sum", "inter_sum")


@pytest.fixture(scope="module")
def ops():
    from focal_amd import ops as o
    return o


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def run(z, L, margin, fn, slices=None):
    from focal_amd import ops as o
    t = dev(z)
    out = o.seq_rank(t, (t * t).sum(1), L, margin, fn=fn, slices=slices)
    n, S = z.shape[0], z.shape[0] // L
    assert tuple(out["intra_d2"].shape) == (n, L) and all(tuple(out[k].shape) == (S,) for k in NAMES[1:])
    assert out["before"].dtype == torch.int32 and out["viol"].dtype == torch.int32 and out["hinge_sum"].dtype == torch.float32
    return {k: v.cpu().numpy() for k, v in out.items()}


# ------------------------------------------------------------------------------------------ 1: exact, integer inputs
@functools.lru_cache(maxsize=None)
def exact_inputs(n, L, D):
    r = np.random.default_rng(1000 * n + 10 * L + D)
    centre = r.integers(-1, 2, (n // L, 1, D))
    centre[:, :, max(1, D // 32):] = 0
    return (centre + r.integers(-1, 2, (n // L, L, D))).reshape(n, D).astype(np.float32)


@functools.lru_cache(maxsize=None)
def int_reference(n, L, D, margin=INT_MARGIN):
    """The int64 brute force: d2, intra_sum, inter_sum, before, viol, the hinge sum times L^2 (L^2 - L), and the largest number any
    fp32 step of a correct kernel holds."""
    Z = exact_inputs(n, L, D).astype(np.int64)
    S, L2, L2L = n // L, L * L, L * L - L
    sq = (Z * Z).sum(1)
    d2 = sq[:, None] + sq[None, :] - 2 * (Z @ Z.T)
    P = d2.reshape(S, L, S, L).sum((1, 3))
    intra = np.diagonal(P).copy()  # (d2(i, i) = 0)
    off = ~np.eye(S, dtype=bool)
    thr_b, thr_v = intra * L2, intra * L2 + margin * L2 * L2L
    before = ((P * L2L < thr_b[:, None]) & off).sum(1)
    viol = ((P * L2L < thr_v[:, None]) & off).sum(1)
    hinge = (np.maximum(thr_v[:, None] - P * L2L, 0) * off).sum(1)
    inter = (P * off).sum(1)
    largest = max(int((P * L2L).max()), int(thr_v.max()), int(hinge.max()), int(inter.max()), int(sq.max()) * 4)
    return d2, intra, inter, before, viol, hinge, largest


@pytest.mark.parametrize("shape", EXACT, ids=["x".join(map(str, s)) for s in EXACT])
def test_exact_integer_inputs(shape):
    n, L, D = shape
    d2, intra, inter, before, viol, hinge, largest = int_reference(*shape)
    S, L2, L2L = n // L, L * L, L * L - L
    pairs = S * (S - 1)
    print(f"exact {shape}: largest fp32 integer {largest}, before {before.sum()} / {pairs}, viol {viol.sum()} / {pairs}")
    assert largest < 2 ** 24
    assert S < 8 or 0 < before.sum() < viol.sum() < pairs  # the counts are not trivial
    own = d2.reshape(S, L, S, L)[np.arange(S), :, np.arange(S), :].reshape(n, L)
    for slices in (1, 2, 5):
        got = run(exact_inputs(*shape), L, float(INT_MARGIN), "sqdist", slices=slices)
        assert np.array_equal(got["intra_d2"], own.astype(np.float32)), slices
        assert np.array_equal(got["intra_sum"].astype(np.int64), intra) and np.array_equal(got["inter_sum"].astype(np.int64), inter), slices
        assert np.array_equal(got["before"], before) and np.array_equal(got["viol"], viol), slices
        # one fp32 division of an exact integer
        assert np.array_equal(got["hinge_sum"], hinge.astype(np.float32) / np.float32(L2 * L2L)), slices


@pytest.mark.parametrize("shape", EXACT[:5], ids=["x".join(map(str, s)) for s in EXACT[:5]])
def test_torch_form_equals_fused_on_integers(shape):
    from train_utils.temporal import sequence_ranking
    n, L, D = shape
    z = dev(exact_inputs(*shape))
    fused = sequence_ranking(z, L, float(INT_MARGIN), fn="sqdist")
    for chunk in (8192, 8 * L):
        plain = sequence_ranking(z, L, float(INT_MARGIN), fused=False, fn="sqdist", chunk=chunk)
        for k in NAMES:
            assert plain[k].dtype == fused[k].dtype and torch.equal(plain[k], fused[k]), (k, chunk)


# ------------------------------------------------------------------------------------------ 2: the search's bits
def test_same_bits_as_the_rank_kernel(ops):
    for n, L, D in ((148, 4, 12), (520, 8, 256), (144, 2, 8), (272, 16, 36)):
        z = dev(real_inputs(n, L, D))
        z_sq = (z * z).sum(1)
        got = ops.seq_rank(z, z_sq, L, 1.0, fn="dist", slices=3)["intra_d2"]
        rows = torch.arange(n, device=DEV)
        for c in range(L):
            pos = (rows - rows % L + c).to(torch.int32)
            _, _, pos_d2 = ops.rank_positive(z, z, z_sq, pos, want_d2=True)
            assert got[:, c].cpu().numpy().tobytes() == pos_d2.cpu().numpy().tobytes(), (n, L, D, c)


# ------------------------------------------------------------------------------------------ 3: real inputs, float64 reference
@functools.lru_cache(maxsize=None)
def real_inputs(n, L, D, seed=0):
    r = np.random.default_rng(7919 * seed + 1000 * n + 10 * L + D)
    S = n // L
    centre = r.standard_normal((S, 1, D))
    sigma = r.uniform(0.2, 1.5, (S, 1, 1))
    return (centre + sigma * r.standard_normal((S, L, D))).reshape(n, D).astype(np.float32)


def float64_reference(Z, L, margin):
    """The float64 values and their bounds (module docstring): dict of intra_sum, inter_sum, hinge_sum, each (value, bound), the gaps
    g_b = P / L^2 - I / (L^2 - L) and g_v = g_b - margin with eps [S, S], and the off-diagonal mask."""
    n, D = Z.shape
    S, L2, L2L = n // L, L * L, L * L - L
    Z64 = Z.astype(np.float64)
    sq = (Z64 * Z64).sum(1)
    # (the differences themselves, 32 rows at a time: two copies of a row are at exactly 0, which the product form misses by ~1e-14)
    d2 = np.concatenate([((Z64[lo:lo + 32, None, :] - Z64[None, :, :]) ** 2).sum(-1) for lo in range(0, n, 32)])
    delta = 2.0 * D * U * (sq + sq.max())
    v = np.sqrt(d2)
    e = np.minimum(delta[:, None] / np.maximum(v, 1e-300), np.sqrt(delta)[:, None]) + 2.0 * U * v
    slack = 1.0 + 1e-5
    P = v.reshape(S, L, S, L).sum((1, 3))
    BP = (e.reshape(S, L, S, L).sum((1, 3)) + L2 * U * P) * slack
    own = ~np.eye(n, dtype=bool)
    I = np.diagonal((v * own).reshape(S, L, S, L).sum((1, 3))).copy()
    BI = (np.diagonal((e * own).reshape(S, L, S, L).sum((1, 3))) + L2L * U * I) * slack
    off = ~np.eye(S, dtype=bool)
    inter = (P * off).sum(1)
    Binter = ((BP * off).sum(1) + (S - 1) * U * inter) * slack
    x = I[:, None] / L2L - P / L2 + margin
    cmp_eps = (BI[:, None] / L2L + BP / L2 + U * (2 * I[:, None] / L2L + abs(margin) + P / L2)) * slack
    eps = cmp_eps + U * np.abs(x) * slack
    hinge = (np.maximum(x, 0) * off).sum(1)
    Bhinge = ((eps * off).sum(1) + S * U * hinge) * slack
    return {"intra_sum": (I, BI), "inter_sum": (inter, Binter), "hinge_sum": (hinge, Bhinge), "gap_before": P / L2 - I[:, None] / L2L,
            "gap_viol": -x, "cmp_eps": cmp_eps, "off": off}


@functools.lru_cache(maxsize=None)
def real_reference(n, L, D, margin):
    return float64_reference(real_inputs(n, L, D), L, margin)


def check_against_float64(got, ref, what):
    """Every float within its bound, every count inside the float64 interval; returns the largest error / bound."""
    worst = 0.0
    for k in FLOATS:
        want, bound = ref[k]
        assert np.isfinite(got[k]).all() and (np.abs(got[k] - want) <= bound).all(), (what, k, np.abs(got[k] - want).max(), bound.max())
        worst = max(worst, float((np.abs(got[k] - want) / np.maximum(bound, 1e-300)).max()))
    for k, gap in (("before", ref["gap_before"]), ("viol", ref["gap_viol"])):
        lo = ((gap < -ref["cmp_eps"]) & ref["off"]).sum(1)
        hi = ((gap < ref["cmp_eps"]) & ref["off"]).sum(1)
        assert (lo <= got[k]).all() and (got[k] <= hi).all(), (what, k)
    return worst


@pytest.mark.parametrize("margin", [0.0, 1.0])
@pytest.mark.parametrize("shape", REAL, ids=["x".join(map(str, s)) for s in REAL])
def test_real_inputs_against_float64(shape, margin):
    n, L, D = shape
    ref = real_reference(n, L, D, margin)
    S = n // L
    pairs = S * (S - 1)
    close = sum(int(((np.abs(ref[g]) <= ref["cmp_eps"]) & ref["off"]).sum()) for g in ("gap_before", "gap_viol"))
    violated = ((ref["gap_viol"] < 0) & ref["off"]).sum() / pairs
    rel = max(float((ref[k][1] / ref[k][0]).max()) for k in ("intra_sum", "inter_sum"))
    print(f"real {shape} margin {margin}: pairs inside +-eps {close} of {2 * pairs}, violated share {violated:.4f}, largest bound / value {rel:.3e}")
    assert close <= 0.01 * pairs and 0.0 < violated < 1.0
    got = run(real_inputs(n, L, D), L, margin, "dist")
    ratio = check_against_float64(got, ref, (shape, margin))
    print(f"real {shape} margin {margin}: largest error / bound = {ratio:.4f}")
    record_observed(f"temporal/seq_rank_error_over_bound/{'x'.join(map(str, shape))}/margin{margin:g}", ratio)


def test_duplicated_rows_stay_finite_and_within_the_bound():
    """The padded last subsequence repeats its final sample: d2 of the copies is 0 up to rounding, possibly below 0 before the clamp."""
    n, L, D = 148, 4, 128
    Z = real_inputs(n, L, D).copy()
    Z[-2:] = Z[-3]          # the last sequence: one sample and three copies of the next
    Z[5] = Z[4]; Z[6] = Z[4]; Z[7] = Z[4]  # a sequence that is one sample four times
    Z[64:68] = Z[4:8]       # ... and a second sequence equal to it, in the next tile
    for margin in (0.0, 1.0):
        ref = float64_reference(Z, L, margin)
        got = run(Z, L, margin, "dist", slices=2)
        check_against_float64(got, ref, ("duplicates", margin))
        assert ref["intra_sum"][0][1] == 0.0 and ref["gap_before"][1, 16] == 0.0 and 0.0 <= got["intra_sum"][1] <= ref["intra_sum"][1][1]


# ------------------------------------------------------------------------------------------ 4: repeatability, slices
def test_repeatable_and_slices():
    n, L, D = REAL[2]
    Z = real_inputs(n, L, D)
    ref = real_reference(n, L, D, 1.0)
    outs = {}
    for s in (1, 2, 7, 64, None):
        outs[s] = run(Z, L, 1.0, "dist", slices=s)
        again = run(Z, L, 1.0, "dist", slices=s)
        for k in NAMES:
            assert outs[s][k].tobytes() == again[k].tobytes(), (s, k)
        check_against_float64(outs[s], ref, s)
    assert -(-n // 64) < 64  # with 64 slices most of them are empty
    for s in (2, 7, 64, None):
        for k in ("intra_d2", "intra_sum", "before", "viol"):
            assert outs[s][k].tobytes() == outs[1][k].tobytes(), (s, k)
        for k in ("inter_sum", "hinge_sum"):
            assert (np.abs(outs[s][k] - outs[1][k]) <= ref[k][1]).all(), (s, k)


# ------------------------------------------------------------------------------------------ 5: capture
@pytest.mark.parametrize("slices", [3, 1], ids=["3-slices", "one-slice-direct"])
def test_capture_and_replay(ops, slices):
    n, L, D = REAL[1]
    others = [dev(real_inputs(n, L, D, seed=k)) for k in (1, 2)]
    call = lambda x: ops.seq_rank(x, (x * x).sum(1), L, 1.0, fn="dist", slices=slices)
    eager = [{k: v.clone() for k, v in call(x).items()} for x in others]
    static_z = dev(real_inputs(n, L, D)).clone()
    call(static_z)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call(static_z)
    for x, want in zip(others, eager):
        static_z.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        for k in NAMES:
            assert torch.equal(out[k], want[k]), k
    assert not torch.equal(eager[0]["hinge_sum"], eager[1]["hinge_sum"])


# ------------------------------------------------------------------------------------------ 6: limits, NaN
def call_entry(d, z, z_sq, outs, ws, ws_bytes=None):
    from focal_amd import _lib
    lib = _lib.load()
    ptr = lambda x: None if x is None else x.data_ptr()
    nbytes = (0 if ws is None else ws.numel()) if ws_bytes is None else ws_bytes
    return lib.focal_seq_rank(ctypes.byref(d), ptr(z), ptr(z_sq), *[ptr(o) for o in outs], ptr(ws), ctypes.c_size_t(nbytes),
                              torch.cuda.current_stream().cuda_stream)


GOOD = dict(n=48, D=36, L=4, slices=2, fn=1, margin=1.0)
FIELDS = ("n", "D", "L", "slices", "fn", "margin")
LIMITS = [("D=34", dict(D=34), "D % 4 == 0"), ("D=0", dict(D=0), "D >= 4"), ("L=3", dict(L=3), "L in {2, 4, 8, 16}"),
          ("L=32", dict(L=32, n=64), "L in {2, 4, 8, 16}"), ("L=1", dict(L=1), "L in {2, 4, 8, 16}"), ("n=46", dict(n=46), "n % L == 0"),
          ("n=0", dict(n=0), "n % L == 0"), ("S=1", dict(n=4), "S = n / L >= 2"), ("slices=0", dict(slices=0), "1 <= slices <= 65535"),
          ("slices=65536", dict(slices=65536), "1 <= slices <= 65535"), ("grid", dict(n=2 ** 31 - 4, slices=65535), "exceeds the launch grid"),
          ("fn=2", dict(fn=2), "fn in 0 .. 1"), ("fn=-1", dict(fn=-1), "fn in 0 .. 1"), ("margin=nan", dict(margin=float("nan")), "finite margin"),
          ("margin=inf", dict(margin=float("inf")), "finite margin"), ("misaligned z", dict(), "16-byte aligned"),
          ("short ws", dict(), "workspace of"), ("null output", dict(), "null tensor")]


@pytest.mark.parametrize("name,change,match", LIMITS, ids=[n.replace(" ", "-") for n, _, _ in LIMITS])
def test_limits_refused_before_any_launch(ops, name, change, match):
    from focal_amd import _lib
    v = dict(GOOD, **change)
    n, D = GOOD["n"], v["D"] if v["D"] > 0 else 36
    offset = 1 if name == "misaligned z" else 0
    z = torch.zeros(n * D + 4, device=DEV)[offset:offset + n * D].view(n, D)
    z_sq = torch.zeros(n, device=DEV)
    outs = [torch.full((n, 16), -7.0, device=DEV), torch.full((n,), -7.0, device=DEV), torch.full((n,), -7, dtype=torch.int32, device=DEV),
            torch.full((n,), -7, dtype=torch.int32, device=DEV), torch.full((n,), -7.0, device=DEV), torch.full((n,), -7.0, device=DEV)]
    good = _lib.SeqRankDesc(*[GOOD[k] for k in FIELDS])
    need = _lib.load().focal_seq_rank_workspace(ctypes.byref(good))
    assert need == 2 * 1 * 2 * 64 * 4
    ws = torch.full((need,), 0xF9, dtype=torch.uint8, device=DEV)
    d = _lib.SeqRankDesc(*[v[k] for k in FIELDS])
    passed = [None if name == "null output" and i == 4 else o for i, o in enumerate(outs)]
    with pytest.raises(_lib.FocalHipError, match=re.escape(match)):
        _lib.check(call_entry(d, z, z_sq, passed, ws, ws_bytes=need - 1 if name == "short ws" else None))
    if name not in ("short ws", "null output", "grid", "n=0", "n=46", "S=1", "D=0", "L=32"):  # (the wrapper reads the sizes off the tensors)
        with pytest.raises(_lib.FocalHipError, match=re.escape(match)):
            ops.seq_rank(z, z_sq, v["L"], v["margin"], fn=v["fn"], slices=v["slices"])
    torch.cuda.synchronize()
    assert all((o == -7).all() for o in outs) and (ws == 0xF9).all()


def test_wrapper_refuses_other_tensors(ops):
    from focal_amd._lib import FocalHipError
    z, z_sq = torch.zeros(48, 36, device=DEV), torch.zeros(48, device=DEV)
    with pytest.raises(FocalHipError, match="fp32"):
        ops.seq_rank(z.double(), z_sq, 4, 1.0)
    with pytest.raises(FocalHipError, match="a matrix"):
        ops.seq_rank(z[0], z_sq, 4, 1.0)
    with pytest.raises(FocalHipError, match="norms"):
        ops.seq_rank(z, z_sq[:5], 4, 1.0)
    with pytest.raises(FocalHipError, match="contiguous"):
        ops.seq_rank(torch.zeros(48, 72, device=DEV)[:, ::2], z_sq, 4, 1.0)
    with pytest.raises(FocalHipError, match=re.escape("n % L == 0")):
        ops.seq_rank(z[:46], z_sq[:46], 4, 1.0)
    with pytest.raises(FocalHipError, match=re.escape("S = n / L >= 2")):
        ops.seq_rank(z[:8], z_sq[:8], 8, 1.0)
    with pytest.raises(FocalHipError, match=re.escape("fn in 0 .. 1")):
        ops.seq_rank(z, z_sq, 4, 1.0, fn="gauss")


@pytest.mark.parametrize("slices", [1, 3])
def test_nan_rule(slices):
    """A NaN pooled value is never counted and makes that sequence's two float sums NaN: one NaN row poisons P(a, b) for its own sequence b
    and every a, so every sequence's sums are NaN, no count includes b, and the counts among the others are those without b."""
    n, L, D = 148, 4, 12
    Z = real_inputs(n, L, D).copy()
    bad = 70  # sequence 17, in the second gallery tile
    Z[bad, 3] = np.nan
    got = run(Z, L, 1.0, "dist", slices=slices)
    b = bad // L
    assert np.isnan(got["hinge_sum"]).all() and np.isnan(got["inter_sum"]).all()
    assert np.isnan(got["intra_sum"][b]) and np.isfinite(np.delete(got["intra_sum"], b)).all()
    assert got["before"][b] == 0 and got["viol"][b] == 0
    assert np.isnan(got["intra_d2"][b * L:(b + 1) * L]).any() and np.isfinite(np.delete(got["intra_d2"], np.arange(b * L, (b + 1) * L), 0)).all()
    clean = run(np.delete(Z, np.arange(b * L, (b + 1) * L), 0), L, 1.0, "dist", slices=slices)
    assert np.array_equal(np.delete(got["before"], b), clean["before"]) and np.array_equal(np.delete(got["viol"], b), clean["viol"])
    assert clean["viol"].sum() > 0 and np.isfinite(clean["hinge_sum"]).all()


# ------------------------------------------------------------------------------------------ 7: neighbour ranks
@pytest.mark.parametrize("shape", [(148, 4, 12), (144, 2, 8), (272, 16, 36)], ids=["148x4x12", "144x2x8", "272x16x36"])
def test_neighbour_ranks_against_brute_force(shape):
    """Integer rows from a small range: many exact ties, among siblings and with the window itself (duplicated rows: d2 = 0 = d2(i, i))."""
    from train_utils.temporal import neighbour_ranks, sequence_ranking
    n, L, D = shape
    Z = exact_inputs(n, L, D).copy()
    Z[9] = Z[8]      # a window whose nearest sibling is its own copy, at the larger index: the window itself orders first
    Z[17] = Z[16]    # ... and at the smaller index: the sibling orders first
    Z[40] = Z[3]     # a copy in another sequence
    z = dev(Z)
    rank = sequence_ranking(z, L, 1.0, fn="sqdist")
    ranks, tied, pos = neighbour_ranks(z, L, rank["intra_d2"])
    Zi = Z.astype(np.int64)
    sq = (Zi * Zi).sum(1)
    d2 = sq[:, None] + sq[None, :] - 2 * (Zi @ Zi.T)
    idx = np.arange(n)
    want_pos, want_rank, want_tied = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    for i in range(n):
        sib = [j for j in range(i - i % L, i - i % L + L) if j != i]
        p = min(sib, key=lambda j: (d2[i, j], j))
        others = idx != i
        want_pos[i] = p
        want_rank[i] = 1 + (others & ((d2[i] < d2[i, p]) | ((d2[i] == d2[i, p]) & (idx < p)))).sum()
        want_tied[i] = (others & (idx != p) & (d2[i] == d2[i, p])).sum()
    assert np.array_equal(pos.numpy(), want_pos) and np.array_equal(ranks.numpy(), want_rank) and np.array_equal(tied.numpy(), want_tied)
    assert pos[8] == 9 and pos[9] == 8 and ranks[8] == 1 and want_tied.max() > 0 and 1 <= ranks.min() and ranks.max() <= n - 1


# ------------------------------------------------------------------------------------------ 8: eval_temporal.py
def temporal_entry():
    spec = importlib.util.spec_from_file_location("focal_eval_temporal_entry", os.path.join(SRC, "eval_temporal.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def temporal_parsed(monkeypatch, argv):
    from params.temporal_params import parse_temporal_params
    monkeypatch.setattr(sys, "argv", ["eval_temporal.py"] + argv)
    return parse_temporal_params()


def write_seeded_backbone(args):
    """Name-seeded weights under the name the pretraining loop would use (its checkpoints are the backbone's whole state dict)."""
    from oracle.weights import fill_state_dict_
    from train_utils.model_selection import init_backbone_model
    net = init_backbone_model(copy.copy(args))
    torch.save(fill_state_dict_({k: v.detach().cpu().clone() for k, v in net.state_dict().items()}), args.backbone_weight)


NUM = r"(-?[\d.]+(?:e[-+]?\d+)?|nan|-?inf)"
TEMPORAL = re.compile(rf"Temporal \[(\S+)\] \(split=(\w+), sequences=(\d+), seq_len=(\d+), D=(\d+)\): ranking loss {NUM} \(margin {NUM}\), "
                      rf"margin satisfied {NUM}, ordered {NUM}, mean intra {NUM}, mean inter {NUM}, ratio {NUM}")
NEIGHBOURS = re.compile(rf"Temporal neighbours \[(\S+)\] \(n=(\d+)\): (.*), MRR {NUM}, median rank {NUM}")


def report_lines(text):
    return [line for line in text.splitlines() if line.startswith(("Temporal", "chance"))]


def test_eval_temporal_end_to_end_deepsense(monkeypatch, tmp_path, capsys):
    """DeepSense on MOD in fp32 (its forward repeats exactly): the synthetic test split is one batch of 32 windows, 8 subsequences of 4."""
    from train_utils.retrieval import retrieval_metrics
    from train_utils.temporal import temporal_metrics
    argv = ["-model=DeepSense", "-dataset=MOD", "-learn_framework=FOCAL", f"-model_weight={tmp_path}", "-batch_size=32", "-compute_dtype=fp32",
            "-synthetic_batches=2"]
    args = temporal_parsed(monkeypatch, argv)
    assert args.backbone_weight == os.path.join(str(tmp_path), "MOD_DeepSense_pretrain_best.pt")
    assert args.temporal_ks == [1, 5, 10] and args.temporal_split == "test" and args.temporal_margin is None and args.stage == "pretrain"
    write_seeded_backbone(args)
    capsys.readouterr()
    out, kept = temporal_entry().evaluate_temporal(args, keep=True)
    text = capsys.readouterr().out
    mods = list(args.dataset_config["modality_names"])
    L = args.dataset_config["seq_len"]
    margin = float(args.dataset_config["FOCAL"]["inter_rank_margin"])
    n = out["n"]
    assert n == 32 == out["N"] and L == 4 == out["seq_len"] and out["margin"] == margin
    printed = {m.group(1): m for m in TEMPORAL.finditer(text)}
    neighbours = {m.group(1): m for m in NEIGHBOURS.finditer(text)}
    assert set(printed) == set(neighbours) == set(mods) | {"features"} == set(out["temporal"]) == set(kept["scored"])
    for name, m in printed.items():
        z = kept["scored"][name]
        assert z.dtype == torch.float32 and z.shape[0] == n
        if name != "features":
            assert z.shape[1] == args.dataset_config["FOCAL"]["emb_dim"]
        assert (m.group(2), int(m.group(3)), int(m.group(4)), int(m.group(5))) == ("test", n // L, L, z.shape[1])
        assert float(m.group(7)) == margin
        ref = float64_reference(z.cpu().numpy(), L, margin)
        got = {k: v.cpu().numpy() for k, v in kept["ranking"][name].items()}
        check_against_float64(got, ref, name)
        t = out["temporal"][name]
        assert t == dict(temporal_metrics(kept["ranking"][name], L), D=z.shape[1])
        pairs = (n // L) * (n // L - 1)
        assert abs(t["ranking_loss"] - ref["hinge_sum"][0].sum() / pairs) <= ref["hinge_sum"][1].sum() / pairs
        shown = [float(m.group(k)) for k in (6, 8, 9, 10, 11, 12)]
        want = [t[k] for k in ("ranking_loss", "margin_satisfied", "ordered", "mean_intra", "mean_inter", "ratio")]
        assert all(abs(a - b) <= 5.1e-6 for a, b in zip(shown, want)), (shown, want)
        ranks, tied = kept["ranks"][name], kept["tied"][name]
        assert ranks.numel() == n and int(ranks.min()) >= 1 and int(ranks.max()) <= n - 1
        assert out["neighbours"][name] == retrieval_metrics(ranks, tied, args.temporal_ks)
        nb = neighbours[name]
        recall = {int(k): float(v) for k, v in re.findall(r"R@(\d+) ([\d.]+)", nb.group(3))}
        assert int(nb.group(2)) == n and all(abs(recall[k] - out["neighbours"][name]["recall"][k]) <= 5.1e-6 for k in args.temporal_ks)
    assert out["chance"] == {k: min(k, n - 1) / (n - 1) for k in args.temporal_ks} and f"R@1 = 1 / {n - 1}" in text
    r = subprocess.run([sys.executable, os.path.join(SRC, "eval_temporal.py")] + argv, capture_output=True, text=True, timeout=300, cwd=SRC)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert report_lines(r.stdout) == report_lines(text) and len(report_lines(text)) == 2 * (len(mods) + 1) + 1


def test_eval_temporal_multi_location_swin_and_subset(monkeypatch, tmp_path, capsys):
    """SW_Transformer on HAR3LOC in bf16, cut to 3 whole subsequences of the 4: it builds, runs and prints finite numbers."""
    argv = ["-model=SW_Transformer", "-dataset=HAR3LOC", "-learn_framework=FOCAL", f"-model_weight={tmp_path}", "-batch_size=16",
            "-temporal_max_rows=14", "-temporal_margin=0.5", "-temporal_k=1,2"]
    args = temporal_parsed(monkeypatch, argv)
    assert len(args.dataset_config["location_names"]) > 1
    write_seeded_backbone(args)
    capsys.readouterr()
    out, kept = temporal_entry().evaluate_temporal(args, keep=True)
    text = capsys.readouterr().out
    L = args.dataset_config["seq_len"]
    assert (out["N"], out["n"], out["margin"]) == (16, 14 // L * L, 0.5) and f"{out['n']} of 16 rows" in text
    assert len(TEMPORAL.findall(text)) == len(NEIGHBOURS.findall(text)) == len(args.dataset_config["modality_names"]) + 1
    for name, t in out["temporal"].items():
        assert t["sequences"] == out["n"] // L and all(math.isfinite(t[k]) for k in ("ranking_loss", "mean_intra", "mean_inter", "ratio"))
        assert 0.0 <= t["margin_satisfied"] <= t["ordered"] <= 1.0 and t["ranking_loss"] >= 0.0
        m = out["neighbours"][name]
        assert m["n"] == out["n"] and 0.0 <= m["recall"][1] <= m["recall"][2] <= 1.0
