"""The fused pair-sum kernel (focal_pair_sums, ops.pair_sums), the scores built on it (train_utils/geometry.py: silhouette, uniformity)
and eval_geometry.py end to end.

Exact inputs: T and Q are integers in [-3, 3] stored as fp32, group ids uniform in [-1, G).  Every d2 is an exact integer in fp32 and so
is every partial sum of a group (asserted: every group sum is below 2^24), so with fn = sqdist S equals the integer brute force in any
order of the additions, for every `slices`.

Real inputs: r = default_rng(seed); mu = 0.3 r.standard_normal((G, D)); g = r.integers(0, G, nt) with the first G ids set to 0 .. G - 1
when nt >= G; T = mu[g] + N(0, 1); Q likewise from fresh draws; for gauss (scale = 2) the rows are made unit length in float64 and stored
as fp32.  Rounding bound, u = 2^-24: any correct fp32 d2 lies within delta_i = 2 D u (|q_i|^2 + max |t|^2) of the float64 value (half of
bound(q) of tests/test_rank_gpu.py), so a correct kernel satisfies
    |S - S64|[i, g] <= sum_j e_ij + m_g u S64[i, g]        (m_g the group's row count: the fp32 additions)
    dist:  e_ij = min(delta_i / sqrt(d2_64), sqrt(delta_i)) + 2 u sqrt(d2_64)
    gauss: e_ij = v64 (expm1(scale delta_i) + 4 u).
Condition on the inputs, asserted: the bound is at most 1e-3 of S64 wherever S64 > 0 -- smaller than what one lost pair changes.
Propagation: a row's silhouette is 1 - a / b (or b / a - 1) with a and b each within eps = that row's largest relative bound, so it lies
within 4 eps of the float64 value; log of a sum within relative eps lies within -log1p(-eps).
Observed largest error / bound per shape: tests/golden/OBSERVED_geometry.json.

End to end, the effective rank is compared with RankMe from numpy's SVD of the centred float64 rows within 5e-3 relative: the tool takes
the squared singular values as eigenvalues of the D x D scatter matrix, where a null direction's eigenvalue is wrong by up to about
D 2^-53 of the largest, its sigma by the root of that (3e-7 at D = 1024), its entropy term by about 15 times that, times at most 1024
null directions."""
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
SHAPES = [(70, 333, 36, 5, 1), (257, 1500, 64, 7, 2), (130, 4099, 128, 64, 3), (65, 300, 1024, 3, 4), (64, 128, 4, 2, 5),
          (200, 700, 256, 6, 6), (1, 333, 36, 1, 1), (70, 1, 36, 1, 1)]
IDS = ["x".join(map(str, s[:4])) for s in SHAPES]
SCALE = 2.0


@pytest.fixture(scope="module")
def ops():
    from focal_amd import ops as o
    return o


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


@functools.lru_cache(maxsize=None)
def exact_inputs(nq, nt, D, G, seed):
    r = np.random.default_rng(seed)
    T = r.integers(-3, 4, (nt, D)).astype(np.float32)
    Q = r.integers(-3, 4, (nq, D)).astype(np.float32)
    g = r.integers(-1, G, nt).astype(np.int32)
    return T, Q, g


@functools.lru_cache(maxsize=None)
def real_inputs(nq, nt, D, G, seed, unit=False):
    r = np.random.default_rng(seed)
    mu = 0.3 * r.standard_normal((G, D))
    g = r.integers(0, G, nt)
    if nt >= G:
        g[:G] = np.arange(G)
    T = mu[g] + r.standard_normal((nt, D))
    Q = mu[r.integers(0, G, nq)] + r.standard_normal((nq, D))
    if unit:
        T, Q = T / np.linalg.norm(T, axis=1, keepdims=True), Q / np.linalg.norm(Q, axis=1, keepdims=True)
    return T.astype(np.float32), Q.astype(np.float32), g.astype(np.int32)


def float64_sums(Q, T, g, G, fn, scale=SCALE, self_offset=None):
    """(S64, bound) [nq, G] of the module docstring; rows of g outside [0, G) and the self pairs are left out of both."""
    Q64, T64 = Q.astype(np.float64), T.astype(np.float64)
    qsq, tsq = (Q64 * Q64).sum(1), (T64 * T64).sum(1)
    d2 = np.maximum(qsq[:, None] + tsq[None, :] - 2.0 * (Q64 @ T64.T), 0.0)
    keep = np.ones(d2.shape, dtype=bool)
    if self_offset is not None:
        rows = np.arange(Q.shape[0])
        ok = self_offset + rows < T.shape[0]
        keep[rows[ok], self_offset + rows[ok]] = False
    delta = 2.0 * Q.shape[1] * U * (qsq + tsq.max())
    if fn == "dist":
        v = np.sqrt(d2)
        e = np.minimum(delta[:, None] / np.maximum(v, 1e-300), np.sqrt(delta)[:, None]) + 2.0 * U * v
    elif fn == "gauss":
        v = np.exp(-scale * d2)
        e = v * (np.expm1(scale * delta)[:, None] + 4.0 * U)
    else:
        v, e = d2, np.broadcast_to(delta[:, None], d2.shape) + U * d2
    v, e = v * keep, e * keep
    S = np.zeros((Q.shape[0], G))
    B = np.zeros((Q.shape[0], G))
    for k in range(G):
        cols = g == k
        S[:, k] = v[:, cols].sum(1)
        B[:, k] = e[:, cols].sum(1) + cols.sum() * U * S[:, k]
    return S, B


@functools.lru_cache(maxsize=None)
def real_reference(shape, fn):
    nq, nt, D, G, seed = shape
    T, Q, g = real_inputs(*shape, unit=fn == "gauss")
    return float64_sums(Q, T, g, G, fn)


def run(ops, Q, T, g, G, fn, **kw):
    t = dev(T)
    S = ops.pair_sums(dev(Q), t, (t * t).sum(1), None if g is None else dev(g), G=G, fn=fn, **kw)
    assert S.dtype == torch.float32 and tuple(S.shape) == (Q.shape[0], G)
    return S.cpu().numpy()


# ------------------------------------------------------------------------------------------ 1: exact, integer inputs
def int_sums(Q, T, g, G, self_offset=None):
    Qi, Ti = Q.astype(np.int64), T.astype(np.int64)
    d2 = (Qi * Qi).sum(1)[:, None] + (Ti * Ti).sum(1)[None, :] - 2 * (Qi @ Ti.T)
    if self_offset is not None:
        rows = np.arange(Q.shape[0])
        d2[rows, self_offset + rows] = 0
    return np.stack([d2[:, g == k].sum(1) for k in range(G)], axis=1), d2


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_exact_integer_inputs(ops, shape):
    nq, nt, D, G, seed = shape
    T, Q, g = exact_inputs(*shape)
    want, _ = int_sums(Q, T, g, G)
    print(f"exact {shape}: largest group sum {want.max()}, empty groups {[k for k in range(G) if not (g == k).any()]}, ignored rows {(g < 0).sum()}")
    assert want.max() < 2 ** 24
    for slices in (1, 2, 5):
        got = run(ops, Q, T, g, G, "sqdist", slices=slices)
        assert np.array_equal(got.astype(np.int64), want) and np.array_equal(got, want.astype(np.float32)), slices
        # no ids: every row in group 0, summed in a register
        everyone, _ = int_sums(Q, T, np.zeros(nt, np.int32), 1)
        assert everyone.max() < 2 ** 24
        assert np.array_equal(run(ops, Q, T, None, 1, "sqdist", slices=slices), everyone.astype(np.float32)), slices
    # the queries ARE gallery rows off .. off + n - 1: each one's own row is left out
    off = 3 if nt >= nq + 3 else 0
    n = min(nq, nt - off)
    Qs = T[off:off + n]
    want, d2 = int_sums(Qs, T, g, G, self_offset=off)
    assert want.max() < 2 ** 24
    for slices in (1, 2, 5):
        got = run(ops, Qs, T, g, G, "sqdist", self_offset=off, slices=slices)
        assert np.array_equal(got, want.astype(np.float32)), slices


# ------------------------------------------------------------------------------------------ 2: real inputs, float64 reference
@functools.lru_cache(maxsize=None)
def real_run(shape, fn, slices=None):
    from focal_amd import ops as o
    nq, nt, D, G, seed = shape
    T, Q, g = real_inputs(*shape, unit=fn == "gauss")
    return run(o, Q, T, g, G, fn, scale=SCALE, slices=slices)


@pytest.mark.parametrize("fn", ["dist", "gauss"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_real_inputs_against_float64(ops, shape, fn):
    nq, nt, D, G, seed = shape
    S64, B = real_reference(shape, fn)
    got = real_run(shape, fn)
    pos = S64 > 0
    rel = (B[pos] / S64[pos]).max()
    ratio = (np.abs(got - S64)[pos] / B[pos]).max()
    print(f"real {fn} {shape}: largest bound / S64 = {rel:.3e}, largest error / bound = {ratio:.4f}")
    record_observed(f"geometry/pair_sums_error_over_bound/{fn}/{'x'.join(map(str, shape[:4]))}", ratio)
    assert pos.any() and rel <= 1e-3
    assert (np.abs(got - S64) <= B).all()
    if G == 1:  # one group through the general path (ids given) and through the register path (no ids): both within the bound
        T, Q, g = real_inputs(*shape, unit=fn == "gauss")
        assert (np.abs(run(ops, Q, T, None, 1, fn, scale=SCALE) - S64) <= B).all()


# ------------------------------------------------------------------------------------------ 3: the search's bits
def test_same_bits_as_the_search(ops):
    shape = SHAPES[1]
    nq, nt = shape[:2]
    T, Q, _ = real_inputs(*shape)
    q, t = dev(Q), dev(T)
    t_sq = (t * t).sum(1)
    for p in (0, 777, nt - 1):
        pos = torch.full((nq,), p, dtype=torch.int32, device=DEV)
        _, _, pos_d2 = ops.rank_positive(q, t, t_sq, pos, want_d2=True)
        for group in (None, torch.zeros(1, dtype=torch.int32, device=DEV)):
            S = ops.pair_sums(q, t[p:p + 1].contiguous(), t_sq[p:p + 1].contiguous(), group, G=1, fn="sqdist")
            assert S[:, 0].cpu().numpy().tobytes() == pos_d2.clamp_min(0).cpu().numpy().tobytes(), p
    assert float(pos_d2.min()) > 0


# ------------------------------------------------------------------------------------------ 4: repeatability
@pytest.mark.parametrize("fn", ["dist", "gauss"])
def test_repeatable_and_slices_within_the_bound(ops, fn):
    shape = SHAPES[2]
    nq, nt, D, G, seed = shape
    T, Q, g = real_inputs(*shape, unit=fn == "gauss")
    S64, B = real_reference(shape, fn)
    outs = {}
    for s in (1, 2, 7, 64):
        outs[s] = run(ops, Q, T, g, G, fn, scale=SCALE, slices=s)
        again = run(ops, Q, T, g, G, fn, scale=SCALE, slices=s)
        assert outs[s].tobytes() == again.tobytes(), s
        assert (np.abs(outs[s] - S64) <= B).all(), s
    assert -(-nt // 64) * 63 + 64 > nt  # with 64 slices the last one is nearly empty
    default = real_run(shape, fn)
    assert default.tobytes() == run(ops, Q, T, g, G, fn, scale=SCALE).tobytes()
    for s in (2, 7, 64):
        assert (np.abs(outs[s] - outs[1]) <= B).all(), s
    assert (np.abs(default - outs[1]) <= B).all()


# ------------------------------------------------------------------------------------------ 5: edge cases
def test_ignored_ids_and_empty_groups(ops):
    shape = SHAPES[0]
    nq, nt, D, G, seed = shape
    T, Q, g = real_inputs(*shape)
    at = np.array([0, 5, 64, 65, 200, 332])
    minus, beyond = g.copy(), g.copy()
    minus[at] = -1
    beyond[at] = [G, G + 5, 2 ** 31 - 1, 64, -2 ** 31, -7]
    a, b = run(ops, Q, T, minus, G, "dist", slices=3), run(ops, Q, T, beyond, G, "dist", slices=3)
    assert a.tobytes() == b.tobytes()
    S64, B = float64_sums(Q, T, minus, G, "dist")
    assert (np.abs(a - S64) <= B).all()
    gone = g.copy()
    gone[g == 2] = -1
    for fn in ("sqdist", "dist", "gauss"):
        for slices in (1, 4):
            S = run(ops, Q, T, gone, G, fn, scale=0.01, slices=slices)
            assert (S[:, 2] == 0).all() and S[:, 2].tobytes() == np.zeros(nq, np.float32).tobytes()
            assert (S[:, [0, 1, 3, 4]] > 0).all()


def test_self_is_left_out_by_index_not_by_distance(ops):
    shape = SHAPES[1]
    nq, nt, D, G, seed = shape
    T, Q, g = exact_inputs(*shape)
    off = 11
    # (1) integer rows that are NOT the gallery's: self_offset still drops candidate off + i, and nothing else
    incl = run(ops, Q, T, g, G, "sqdist", self_offset=-1, slices=2)
    assert np.array_equal(incl, run(ops, Q, T, g, G, "sqdist", slices=2))  # the default leaves nothing out
    excl = run(ops, Q, T, g, G, "sqdist", self_offset=off, slices=2)
    all_sums, d2 = int_sums(Q, T, g, G)
    want = all_sums.copy()
    for i in range(nq):
        if g[off + i] >= 0:
            want[i, g[off + i]] -= d2[i, off + i]
    assert (d2[np.arange(nq), off + np.arange(nq)] > 0).all() and np.array_equal(incl, all_sums.astype(np.float32))
    assert np.array_equal(excl, want.astype(np.float32))
    # (2) unit rows, the queries are gallery rows off .. off + nq - 1, and row 1400 + i duplicates query i for i < 50: with the self pair
    # left out the duplicate still adds its exp(-scale * 0) = 1, within the bound of that one term and of the additions around it
    T, _, g = real_inputs(*shape, unit=True)
    T = T.copy()
    T[1400:1450] = T[off:off + 50]
    Qs = T[off:off + nq]
    with_dup = run(ops, Qs, T, g, G, "gauss", scale=SCALE, self_offset=off, slices=2)
    S64, B = float64_sums(Qs, T, g, G, "gauss", self_offset=off)
    assert (np.abs(with_dup - S64) <= B).all()
    hidden = g.copy()
    hidden[1400:1450] = -1
    without = run(ops, Qs, T, hidden, G, "gauss", scale=SCALE, self_offset=off, slices=2)
    S64h, Bh = float64_sums(Qs, T, hidden, G, "gauss", self_offset=off)
    rows = np.arange(50)
    term = (with_dup - without)[rows, g[1400:1450]]
    slack = (B + Bh)[rows, g[1400:1450]]
    # (hiding rows 1400 .. 1449 takes out query i's duplicate, a term of 1, and the other hidden rows of that group, `rest`)
    d2 = ((Qs[:50, None, :].astype(np.float64) - T[None, 1400:1450, :].astype(np.float64)) ** 2).sum(-1)
    same = (g[1400:1450][None, :] == g[1400:1450][:, None]) & ~np.eye(50, dtype=bool)
    rest = (np.exp(-SCALE * d2) * same).sum(1)
    print(f"duplicate's term: {(term - rest).min():.7f} .. {(term - rest).max():.7f}, slack {slack.max():.2e}")
    assert (np.abs(term - rest - 1.0) <= slack).all() and (slack < 1e-3).all()
    # ... and with nothing left out the self pair adds one more
    incl = run(ops, Qs, T, g, G, "gauss", scale=SCALE, slices=2)
    S64i, Bi = float64_sums(Qs, T, g, G, "gauss")
    assert (np.abs(incl - S64i) <= Bi).all()
    own = g[off:off + nq]
    assert (np.abs((incl - with_dup)[np.arange(nq), own] - 1.0) <= (B + Bi)[np.arange(nq), own]).all()


# ------------------------------------------------------------------------------------------ 6: limits
def call_entry(d, q, t, t_sq, group, S, ws, ws_bytes=None):
    from focal_amd import _lib
    lib = _lib.load()
    ptr = lambda x: None if x is None else x.data_ptr()
    nbytes = (0 if ws is None else ws.numel()) if ws_bytes is None else ws_bytes
    return lib.focal_pair_sums(ctypes.byref(d), ptr(q), ptr(t), ptr(t_sq), ptr(group), ptr(S), ptr(ws), ctypes.c_size_t(nbytes),
                               torch.cuda.current_stream().cuda_stream)


GOOD = dict(nq=20, nt=50, D=36, G=3, slices=2, fn=1, self_offset=-1, scale=1.0)
LIMITS = [("D=34", dict(D=34), "D % 4 == 0"), ("D=0", dict(D=0), "D >= 4"), ("G=0", dict(G=0), "1 <= G <= 64"),
          ("G=65", dict(G=65), "1 <= G <= 64"), ("slices=0", dict(slices=0), "1 <= slices <= 65535"),
          ("slices=65536", dict(slices=65536), "1 <= slices <= 65535"), ("fn=3", dict(fn=3), "fn in 0 .. 2"),
          ("fn=-1", dict(fn=-1), "fn in 0 .. 2"), ("scale=-1", dict(scale=-1.0), "finite scale >= 0"),
          ("scale=nan", dict(scale=float("nan")), "finite scale >= 0"), ("scale=inf", dict(scale=float("inf")), "finite scale >= 0"),
          ("self_offset=-2", dict(self_offset=-2), "self_offset >= -1"), ("nq=0", dict(nq=0), "nq >= 1"), ("nt=0", dict(nt=0), "nt >= 1"),
          ("grid", dict(nq=2 ** 31 - 1, slices=65535), "exceeds the launch grid"), ("misaligned q", dict(), "16-byte aligned"),
          ("short ws", dict(), "workspace of"), ("no group", dict(), "need the group ids")]


@pytest.mark.parametrize("name,change,match", LIMITS, ids=[n.replace(" ", "-") for n, _, _ in LIMITS])
def test_limits_refused_before_any_launch(ops, name, change, match):
    from focal_amd import _lib
    v = dict(GOOD, **change)
    nq, nt, D = GOOD["nq"], GOOD["nt"], v["D"] if v["D"] > 0 else 36
    offset = 1 if name == "misaligned q" else 0
    q = torch.zeros(nq * D + 4, device=DEV)[offset:offset + nq * D].view(nq, D)
    t = torch.zeros(nt, D, device=DEV)
    t_sq = torch.zeros(nt, device=DEV)
    group = None if name == "no group" else torch.zeros(nt, dtype=torch.int32, device=DEV)
    S = torch.full((nq, 64), -7.0, device=DEV)
    good = _lib.PairSumDesc(*[GOOD[k] for k in ("nq", "nt", "D", "G", "slices", "fn", "self_offset", "scale")])
    need = _lib.load().focal_pair_sums_workspace(ctypes.byref(good))
    assert need == 1 * 2 * 128 * 3 * 4
    ws = torch.full((need,), 0xF9, dtype=torch.uint8, device=DEV)
    d = _lib.PairSumDesc(*[v[k] for k in ("nq", "nt", "D", "G", "slices", "fn", "self_offset", "scale")])
    with pytest.raises(_lib.FocalHipError, match=re.escape(match)):
        _lib.check(call_entry(d, q, t, t_sq, group, S, ws, ws_bytes=need - 1 if name == "short ws" else None))
    if name not in ("short ws", "grid", "nq=0", "nt=0", "D=0"):  # (the wrapper sizes the workspace and reads the sizes off the tensors)
        with pytest.raises(_lib.FocalHipError, match=re.escape(match)):
            ops.pair_sums(q, t, t_sq, group, G=v["G"], fn=v["fn"], scale=v["scale"], self_offset=v["self_offset"], slices=v["slices"])
    torch.cuda.synchronize()
    assert (S == -7).all() and (ws == 0xF9).all()


def test_wrapper_refuses_other_tensors(ops):
    from focal_amd._lib import FocalHipError
    q, t = torch.zeros(8, 36, device=DEV), torch.zeros(12, 36, device=DEV)
    t_sq, group = torch.zeros(12, device=DEV), torch.zeros(12, dtype=torch.int32, device=DEV)
    with pytest.raises(FocalHipError, match="fp32"):
        ops.pair_sums(q.double(), t, t_sq, group, G=2)
    with pytest.raises(FocalHipError, match="fp32"):
        ops.pair_sums(q, t, t_sq.double(), group, G=2)
    with pytest.raises(FocalHipError, match="matrices"):
        ops.pair_sums(q[0], t, t_sq, group, G=2)
    with pytest.raises(FocalHipError, match="int32"):
        ops.pair_sums(q, t, t_sq, group.long(), G=2)
    with pytest.raises(FocalHipError, match="group ids for 12 rows"):
        ops.pair_sums(q, t, t_sq, group[:5], G=2)
    with pytest.raises(FocalHipError, match="norms"):
        ops.pair_sums(q, t, t_sq[:5], group, G=2)
    with pytest.raises(FocalHipError, match="against t"):
        ops.pair_sums(q, torch.zeros(12, 40, device=DEV), t_sq, group, G=2)
    with pytest.raises(FocalHipError, match="contiguous"):
        ops.pair_sums(torch.zeros(8, 72, device=DEV)[:, ::2], t, t_sq, group, G=2)
    with pytest.raises(FocalHipError, match="need the group ids"):
        ops.pair_sums(q, t, t_sq, None, G=2)
    with pytest.raises(FocalHipError, match=re.escape("fn in 0 .. 2")):
        ops.pair_sums(q, t, t_sq, group, G=2, fn="cosine")


# ------------------------------------------------------------------------------------------ 7: capture
@pytest.mark.parametrize("G,slices", [(7, 3), (1, 1)], ids=["groups-3-slices", "one-group-direct"])
def test_capture_and_replay(ops, G, slices):
    shape = SHAPES[1]
    T, Q, g = real_inputs(*shape)
    t = dev(T)
    group = dev(g) if G > 1 else None
    t_sq = (t * t).sum(1)
    r = np.random.default_rng(77)
    others = [dev(r.standard_normal(Q.shape).astype(np.float32)) for _ in range(2)]
    call = lambda x: ops.pair_sums(x, t, t_sq, group, G=G, fn="dist", slices=slices)
    eager = [call(x).clone() for x in others]
    static_q = dev(Q).clone()
    call(static_q)  # warm-up outside the capture: the workspace exists from here on
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats()["allocation.all.allocated"]
    held = call(static_q)
    assert torch.cuda.memory_stats()["allocation.all.allocated"] - before == 1  # the output, nothing else
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call(static_q)
    for x, want in zip(others, eager):
        static_q.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want)
    del held


# ------------------------------------------------------------------------------------------ 8 - 10: the scores
@functools.lru_cache(maxsize=None)
def gallery_reference(i):
    """For q = t = shape i's gallery: the float64 distance sums with their bound (self left out), sklearn's silhouettes, and eps per row."""
    from sklearn.metrics import silhouette_samples
    nq, nt, D, G, seed = SHAPES[i]
    T, _, g = real_inputs(*SHAPES[i])
    S64, B = float64_sums(T, T, g, G, "dist", self_offset=0)
    assert (S64 > 0).all()
    eps = (B / S64).max(1)
    return T, g, silhouette_samples(T.astype(np.float64), g), eps


@pytest.mark.parametrize("i", range(6), ids=IDS[:6])
def test_silhouette_against_sklearn(i):
    from train_utils.geometry import silhouette
    G = SHAPES[i][3]
    T, g, want, eps = gallery_reference(i)
    s, mean, per_class = silhouette(dev(T), dev(g).long(), G)
    assert s.dtype == torch.float64 and tuple(s.shape) == (T.shape[0],) and tuple(per_class.shape) == (G,)
    s = s.cpu().numpy()
    ratio = (np.abs(s - want) / (4 * eps)).max()
    print(f"silhouette {SHAPES[i]}: mean {mean:.6f} (sklearn {want.mean():.6f}), largest eps {eps.max():.2e}, largest error / (4 eps) = {ratio:.4f}")
    record_observed(f"geometry/silhouette_error_over_4eps/{IDS[i]}", ratio)
    assert eps.max() <= 1e-3
    assert (np.abs(s - want) <= 4 * eps).all()
    assert abs(mean - want.mean()) <= 4 * eps.mean() + 1e-15
    pc = per_class.cpu().numpy()
    for k in range(G):
        assert abs(pc[k] - want[g == k].mean()) <= 4 * eps[g == k].mean() + 1e-15


def uniformity_reference(z_unit, t):
    """float64 log mean exp(-t d2) over i != j of the given (already unit, fp32) rows, and eps: the relative bound of the total."""
    S64, B = float64_sums(z_unit, z_unit, np.zeros(z_unit.shape[0], np.int32), 1, "gauss", scale=t, self_offset=0)
    n = z_unit.shape[0]
    return math.log(S64.sum() / (n * (n - 1.0))), B.sum() / S64.sum()


@pytest.mark.parametrize("i", range(6), ids=IDS[:6])
def test_uniformity_against_float64(i):
    from train_utils.geometry import uniformity
    from train_utils.retrieval import unit_rows
    T, _, _, _ = gallery_reference(i)
    z = dev(T)
    for t in (2.0, 0.5):
        got = uniformity(z, t=t)
        want, eps = uniformity_reference(unit_rows(z).cpu().numpy(), t)
        print(f"uniformity {SHAPES[i]} t={t}: {got:.7f} (float64 {want:.7f}), eps {eps:.2e}, error / bound = {abs(got - want) / -math.log1p(-eps):.4f}")
        if t == 2.0:
            record_observed(f"geometry/uniformity_error_over_bound/{IDS[i]}", abs(got - want) / -math.log1p(-eps))
            assert eps <= 1e-3
            assert abs(got - want) <= -math.log1p(-eps)
        else:
            # (a scale that is no power of two: the product scale * d2 rounds once more, u of an argument of at most 4 t)
            assert abs(got - want) <= -math.log1p(-(eps + 4 * t * U))


@pytest.mark.parametrize("i", range(3), ids=IDS[:3])
def test_torch_forms(i):
    from train_utils.geometry import silhouette, uniformity
    from train_utils.retrieval import unit_rows
    G = SHAPES[i][3]
    T, g, want, eps = gallery_reference(i)
    z = dev(T)
    s, mean, _ = silhouette(z, dev(g).long(), G, fused=False, chunk=1000)  # (more than one chunk at 1500 and 4099)
    assert s.dtype == torch.float64
    assert (np.abs(s.cpu().numpy() - want) <= 4 * eps).all()
    got = uniformity(z, fused=False, chunk=1000)
    ref, ueps = uniformity_reference(unit_rows(z).cpu().numpy(), 2.0)
    assert abs(got - ref) <= -math.log1p(-ueps)
    assert abs(got - uniformity(z)) <= 2 * -math.log1p(-ueps)


# ------------------------------------------------------------------------------------------ 11: eval_geometry.py
def geometry_entry():
    spec = importlib.util.spec_from_file_location("focal_eval_geometry_entry", os.path.join(SRC, "eval_geometry.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def geometry_parsed(monkeypatch, argv):
    from params.geometry_params import parse_geometry_params
    monkeypatch.setattr(sys, "argv", ["eval_geometry.py"] + argv)
    return parse_geometry_params()


def write_seeded_backbone(args):
    """Name-seeded weights under the name the pretraining loop would use (its checkpoints are the backbone's whole state dict)."""
    from oracle.weights import fill_state_dict_
    from train_utils.model_selection import init_backbone_model
    net = init_backbone_model(copy.copy(args))
    torch.save(fill_state_dict_({k: v.detach().cpu().clone() for k, v in net.state_dict().items()}), args.backbone_weight)


NUM = r"(-?[\d.]+|nan|-?inf)"
FEATURES = re.compile(rf"Geometry \[features\] \(split=(\w+), n=(\d+), D=(\d+)\): silhouette\s+{NUM}, uniformity \(t=2\)\s+{NUM}, "
                      rf"effective rank {NUM} of (\d+)")
EMBEDDING = re.compile(rf"Geometry \[(\S+) (shared|private)\] \(n=(\d+), D=(\d+)\): uniformity \(t=2\)\s+{NUM}, effective rank {NUM} of (\d+)")
ALIGNMENT = re.compile(rf"Alignment \[(shared|private)\] (\S+) <-> (\S+): {NUM}")


def rankme(X):
    X = X.astype(np.float64)
    sv = np.linalg.svd(X - X.mean(0), compute_uv=False)
    if sv.sum() == 0:
        return 1.0
    p = sv / sv.sum()
    p = p[p > 0]
    return float(np.exp(-(p * np.log(p)).sum()))


def report_lines(text):
    return [line for line in text.splitlines() if line.startswith(("Geometry", "Silhouette", "Alignment"))]


def test_eval_geometry_end_to_end_deepsense(monkeypatch, tmp_path, capsys):
    """DeepSense on MOD in fp32 (its forward repeats exactly): the synthetic test split is one batch of 32 windows."""
    from sklearn.metrics import silhouette_samples
    from train_utils.retrieval import unit_rows
    argv = ["-model=DeepSense", "-dataset=MOD", "-learn_framework=FOCAL", f"-model_weight={tmp_path}", "-batch_size=32", "-compute_dtype=fp32",
            "-synthetic_batches=2"]
    args = geometry_parsed(monkeypatch, argv)
    assert args.backbone_weight == os.path.join(str(tmp_path), "MOD_DeepSense_pretrain_best.pt")
    assert args.geometry_split == "test" and args.geometry_t == 2.0
    write_seeded_backbone(args)
    capsys.readouterr()
    out, kept = geometry_entry().evaluate_geometry(args, keep=True)
    text = capsys.readouterr().out
    feats, labels = kept["features"], kept["labels"].cpu().numpy()
    n, D = feats.shape
    n_cls = args.dataset_config[args.task]["num_classes"]
    assert n == 32 == out["n"] and feats.dtype == torch.float32 and kept["sums"]["silhouette"].shape == (n, n_cls)
    m = FEATURES.search(text)
    assert m, text
    assert (m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(7))) == ("test", n, D, min(n - 1, D))
    X = feats.cpu().numpy()
    # the silhouette: per row within 4 eps of sklearn's on the float64 copies of the very features
    present = np.unique(labels)
    print(f"end to end: n={n}, D={D}, classes present {present.tolist()}")
    if len(present) >= 2:
        S64, B = float64_sums(X, X, labels.astype(np.int32), n_cls, "dist", self_offset=0)
        own_or_other = S64 > 0
        eps = np.where(own_or_other, B / np.where(own_or_other, S64, 1.0), 0.0).max(1)
        want = silhouette_samples(X.astype(np.float64), labels)
        got = kept["silhouettes"].cpu().numpy()
        assert (np.abs(got - want) <= 4 * eps + 1e-15).all()
        assert abs(out["features"]["silhouette"] - got.mean()) <= 1e-15 and abs(float(m.group(4)) - got.mean()) <= 5.1e-6
        assert "Silhouette by class: " in text
    else:
        assert math.isnan(out["features"]["silhouette"]) and "Silhouette is undefined" in text
    # uniformity of the features and of every embedding half: float64 on the unit rows that were scored
    mods = args.dataset_config["modality_names"]
    width = kept["projections"][mods[0]].shape[1]
    h = width // 2
    assert width == args.dataset_config["FOCAL"]["emb_dim"]
    want, eps = uniformity_reference(unit_rows(feats).cpu().numpy(), 2.0)
    assert abs(out["features"]["uniformity"] - want) <= -math.log1p(-eps) and abs(float(m.group(5)) - out["features"]["uniformity"]) <= 5.1e-6
    assert out["features"]["effective_rank"] == pytest.approx(rankme(X), rel=5e-3)
    assert abs(float(m.group(6)) - out["features"]["effective_rank"]) <= 5.1e-4
    printed = {(e.group(1), e.group(2)): e for e in EMBEDDING.finditer(text)}
    assert set(printed) == {(mod, half) for mod in mods for half in ("shared", "private")} == set(out["embeddings"])
    for (mod, half), e in printed.items():
        z = kept["projections"][mod][:, (slice(0, h) if half == "shared" else slice(h, 2 * h))]
        want, eps = uniformity_reference(unit_rows(z).cpu().numpy(), 2.0)
        got = out["embeddings"][(mod, half)]
        assert (int(e.group(3)), int(e.group(4)), int(e.group(7))) == (n, h, min(n - 1, h)) and got["D"] == h
        assert abs(got["uniformity"] - want) <= -math.log1p(-eps) and abs(float(e.group(5)) - got["uniformity"]) <= 5.1e-6
        assert got["effective_rank"] == pytest.approx(rankme(z.cpu().numpy()), rel=5e-3)
        assert abs(float(e.group(6)) - got["effective_rank"]) <= 5.1e-4
        assert tuple(kept["sums"]["uniformity"][(mod, half)].shape) == (n, 1)
    # alignment: one line per unordered pair, both halves
    un = lambda x: x.astype(np.float64) / np.maximum(np.linalg.norm(x.astype(np.float64), axis=1, keepdims=True), 1e-12)
    aligned = {(a.group(1), a.group(2), a.group(3)): float(a.group(4)) for a in ALIGNMENT.finditer(text)}
    pairs = [(a, b) for k, a in enumerate(mods) for b in mods[k + 1:]]
    assert set(aligned) == {(half, a, b) for half in ("shared", "private") for a, b in pairs}
    for (half, a, b), shown in aligned.items():
        cols = slice(0, h) if half == "shared" else slice(h, 2 * h)
        want = ((un(kept["projections"][a][:, cols].cpu().numpy()) - un(kept["projections"][b][:, cols].cpu().numpy())) ** 2).sum(1).mean()
        # (unit rows in fp32: each row moves by at most 2 u of its length, a squared distance of at most 4 by at most 16 u)
        assert abs(out["alignment"][half][(a, b)] - want) <= 16 * U and abs(shown - out["alignment"][half][(a, b)]) <= 5.1e-6
    r = subprocess.run([sys.executable, os.path.join(SRC, "eval_geometry.py")] + argv, capture_output=True, text=True, timeout=300, cwd=SRC)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert report_lines(r.stdout) == report_lines(text) and len(report_lines(text)) >= 2 + 2 * len(mods) + len(pairs)


def test_eval_geometry_multi_location_swin(monkeypatch, tmp_path, capsys):
    """SW_Transformer on HAR3LOC in bf16: it builds, runs and prints finite numbers for the features and the four embedding halves."""
    argv = ["-model=SW_Transformer", "-dataset=HAR3LOC", "-learn_framework=FOCAL", f"-model_weight={tmp_path}", "-batch_size=16"]
    args = geometry_parsed(monkeypatch, argv)
    assert args.backbone_weight == os.path.join(str(tmp_path), "HAR3LOC_SW_Transformer_pretrain_best.pt")
    assert len(args.dataset_config["location_names"]) > 1
    write_seeded_backbone(args)
    capsys.readouterr()
    out, kept = geometry_entry().evaluate_geometry(args, keep=True)
    text = capsys.readouterr().out
    n = kept["labels"].shape[0]
    assert n == 16 == out["n"]
    assert math.isfinite(out["features"]["uniformity"]) and out["features"]["uniformity"] <= 0.0
    assert 1.0 <= out["features"]["effective_rank"] <= n - 1 + 1e-6
    sil = out["features"]["silhouette"]
    assert math.isnan(sil) and "Silhouette is undefined" in text or -1.0 <= sil <= 1.0
    assert len(out["embeddings"]) == 4 and len(EMBEDDING.findall(text)) == 4 and len(ALIGNMENT.findall(text)) == 2
    for v in out["embeddings"].values():
        assert math.isfinite(v["uniformity"]) and v["uniformity"] <= 0.0 and 1.0 <= v["effective_rank"] <= min(n - 1, v["D"]) + 1e-6
    for half in ("shared", "private"):
        for v in out["alignment"][half].values():
            assert 0.0 <= v <= 4.0 + 1e-6
