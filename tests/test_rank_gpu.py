"""The fused rank kernel (focal_rank_positive, ops.rank_positive, train_utils/retrieval.py: cross_modal_ranks) against brute force on the
host, and eval_retrieval.py end to end.

Exact inputs: T and Q are integers in [-3, 3] stored as fp32, pos uniform in [0, nt).  Every product and sum is exact in fp32 (the largest
d2 is 2 * 9 * 1024 + 2 * 9 * 1024 < 2^24), so before, tied and pos_d2 equal the integer brute force for every query; ties are frequent and
pin the (d2, index) order.

Real inputs: r = default_rng(seed); T = r.standard_normal((nt, D)); pos = r.integers(0, nt, nq); N = r.standard_normal((nq, D));
Q = T[pos] + 3 N, all float32.  Rounding bound (the derivation of tests/test_knn_fused_gpu.py), u = 2^-24: any correct fp32 d2 lies within
bound(q) / 2 = 2 D u (|q|^2 + max |t|^2) of the float64 value, so two candidates are ordered for certain when they differ by more than
bound(q), and a correct kernel satisfies
    1 + #{j != p : d2_64(j) < d2_64(p) - bound}  <=  before + 1  <=  1 + #{j != p : d2_64(j) <= d2_64(p) + bound}.
A query is *decided* when the two ends coincide; at most 10 % of a shape's queries may be undecided (a condition on the inputs, which the
reference alone meets: 0, 3.9, 3.1, 0, 0, 0, 0, 0 % for the eight shapes)."""
import copy
import ctypes
import functools
import importlib.util
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SRC = os.path.join(ROOT, "focal_amd", "src")
DEV = "cuda"
U = 2.0 ** -24
SHAPES = [(70, 333, 36, 1), (257, 1500, 64, 2), (130, 4099, 128, 3), (65, 300, 1024, 4), (64, 128, 4, 5), (200, 700, 256, 6),
          (1, 333, 36, 1), (70, 1, 36, 1)]
IDS = ["x".join(map(str, s[:3])) for s in SHAPES]


@pytest.fixture(scope="module")
def ops():
    from focal_amd import ops as o
    return o


@functools.lru_cache(maxsize=None)
def exact_inputs(nq, nt, D, seed):
    r = np.random.default_rng(seed)
    T = r.integers(-3, 4, (nt, D)).astype(np.float32)
    Q = r.integers(-3, 4, (nq, D)).astype(np.float32)
    pos = r.integers(0, nt, nq).astype(np.int32)
    return T, Q, pos


@functools.lru_cache(maxsize=None)
def real_inputs(nq, nt, D, seed):
    r = np.random.default_rng(seed)
    T = r.standard_normal((nt, D)).astype(np.float32)
    pos = r.integers(0, nt, nq)
    N = r.standard_normal((nq, D)).astype(np.float32)
    Q = (T[pos] + np.float32(3.0) * N).astype(np.float32)
    return T, Q, pos.astype(np.int32)


def interval(Q, T, pos):
    """float64 brute force: d2 of the positives, bound(q), and the two ends of the interval `before` must lie in."""
    Q64, T64 = Q.astype(np.float64), T.astype(np.float64)
    qsq, tsq = (Q64 * Q64).sum(1), (T64 * T64).sum(1)
    d2 = qsq[:, None] + tsq[None, :] - 2.0 * (Q64 @ T64.T)
    rows = np.arange(Q.shape[0])
    dp = d2[rows, pos]
    bound = 4.0 * Q.shape[1] * U * (qsq + tsq.max())
    other = np.ones_like(d2, dtype=bool)
    other[rows, pos] = False
    lo = ((d2 < (dp - bound)[:, None]) & other).sum(1)
    hi = ((d2 <= (dp + bound)[:, None]) & other).sum(1)
    return dp, bound, lo, hi


@functools.lru_cache(maxsize=None)
def real_reference(shape):
    T, Q, pos = real_inputs(*shape)
    return interval(Q, T, pos)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def run(ops, Q, T, pos, **kw):
    t = dev(T)
    out = ops.rank_positive(dev(Q), t, (t * t).sum(1), dev(pos), want_d2=True, **kw)
    assert out[0].dtype == torch.int32 and out[1].dtype == torch.int32 and out[2].dtype == torch.float32
    return [o.cpu().numpy() for o in out]


@functools.lru_cache(maxsize=None)
def real_run(shape):
    from focal_amd import ops as o
    T, Q, pos = real_inputs(*shape)
    return run(o, Q, T, pos)


# ------------------------------------------------------------------------------------------ 1: exact, integer inputs
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_exact_integer_inputs(ops, shape):
    T, Q, pos = exact_inputs(*shape)
    before, tied, pos_d2 = run(ops, Q, T, pos)
    Qi, Ti = Q.astype(np.int64), T.astype(np.int64)
    d2 = (Qi * Qi).sum(1)[:, None] + (Ti * Ti).sum(1)[None, :] - 2 * (Qi @ Ti.T)
    rows, cols = np.arange(shape[0]), np.arange(shape[1])
    dp = d2[rows, pos]
    same = d2 == dp[:, None]
    want_before = ((d2 < dp[:, None]) | (same & (cols[None, :] < pos[:, None]))).sum(1)
    want_tied = same.sum(1) - 1
    print(f"exact {shape}: ranks {want_before.min() + 1} .. {want_before.max() + 1}, mean tied {want_tied.mean():.2f}, max d2 {d2.max()}")
    assert d2.max() < 2 ** 24
    assert np.array_equal(before, want_before)
    assert np.array_equal(tied, want_tied)
    assert np.array_equal(pos_d2, dp.astype(np.float32))


# ------------------------------------------------------------------------------------------ 2: real inputs, float64 reference
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_real_inputs_against_float64(shape):
    T, Q, pos = real_inputs(*shape)
    dp, bound, lo, hi = real_reference(shape)
    before, tied, pos_d2 = real_run(shape)
    undecided = float((lo != hi).mean())
    err = np.abs(pos_d2.astype(np.float64) - dp)
    print(f"real {shape}: undecided {undecided:.4f}, ranks {before.min() + 1} .. {before.max() + 1}, "
          f"max d2 error / (bound / 2) = {(err / (bound / 2)).max():.4f}")
    assert undecided <= 0.10
    assert (lo <= before).all() and (before <= hi).all()
    assert (err <= bound / 2).all()
    assert (tied >= 0).all() and (tied <= hi - lo).all()  # a tie with the positive lies inside the band


# ------------------------------------------------------------------------------------------ 3: the search's bits
def test_same_bits_as_the_search(ops):
    shape = SHAPES[1]
    T, Q, pos = real_inputs(*shape)
    before, _, pos_d2 = real_run(shape)
    t = dev(T)
    _, nbr_idx, nbr_d2 = ops.knn_search_vote(dev(Q), t, (t * t).sum(1), torch.zeros(shape[1], dtype=torch.int64, device=DEV), 16, 1,
                                             want_neighbours=True)
    nbr_idx, nbr_d2 = nbr_idx.cpu().numpy(), nbr_d2.cpu().numpy()
    hit = nbr_idx == pos[:, None]
    found = hit.any(1)
    col = hit.argmax(1)
    print(f"positives among the 16 nearest: {found.mean():.4f} of the queries")
    assert found.mean() >= 0.25  # (about 0.6 on these inputs; the test says nothing when there are none)
    assert np.array_equal(before[found], col[found])
    assert pos_d2[found].tobytes() == nbr_d2[found, col[found]].tobytes()
    assert (before[~found] >= 16).all()


# ------------------------------------------------------------------------------------------ 4: duplicates
def test_duplicate_rows_tie_exactly(ops):
    shape = SHAPES[0]
    T, Q, _ = real_inputs(*shape)
    T = T.copy()
    T[200:300] = T[0:100]
    j = np.arange(shape[0], dtype=np.int32)  # 0 .. 69: originals whose copies are rows 200 .. 269
    b_orig, t_orig, d_orig = run(ops, Q, T, j)
    b_copy, t_copy, d_copy = run(ops, Q, T, j + 200)
    b_none, t_none, _ = run(ops, Q, T, j + 100)  # rows without a copy
    assert (t_orig >= 1).all() and (t_copy >= 1).all()
    assert np.array_equal(t_orig, t_copy) and d_orig.tobytes() == d_copy.tobytes()
    assert np.array_equal(b_copy, b_orig + 1)  # the original orders before its copy by index, and nothing else lies between them
    # (independent normal rows: an exact fp32 tie between two different rows does not occur on these inputs)
    assert (t_none == 0).all() and (t_orig == 1).all()
    dp, bound, lo, hi = interval(Q, T, j + 100)
    assert (lo <= b_none).all() and (b_none <= hi).all()


# ------------------------------------------------------------------------------------------ 5: slice invariance
def test_slice_invariance(ops):
    shape = SHAPES[2]
    T, Q, pos = real_inputs(*shape)
    outs = {s: run(ops, Q, T, pos, slices=s) for s in (1, 2, 7, 64)}
    assert -(-shape[1] // 64) * 63 + 64 > shape[1]  # with 64 slices the last one is nearly empty
    for s in (2, 7, 64):
        for a, b in zip(outs[1], outs[s]):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), s
    for a, b in zip(outs[1], real_run(shape)):  # and the default
        assert a.tobytes() == b.tobytes()
    Te, Qe, pe = exact_inputs(*shape)  # with ties in every slice
    exact = {s: run(ops, Qe, Te, pe, slices=s) for s in (1, 7, 64)}
    for s in (7, 64):
        for a, b in zip(exact[1], exact[s]):
            assert a.tobytes() == b.tobytes(), s


def call_entry(d, q, t, t_sq, pos, before, tied, pos_d2, ws, ws_bytes=None):
    from focal_amd import _lib
    lib = _lib.load()
    ptr = lambda x: None if x is None else x.data_ptr()
    nbytes = (0 if ws is None else ws.numel()) if ws_bytes is None else ws_bytes
    return lib.focal_rank_positive(ctypes.byref(d), ptr(q), ptr(t), ptr(t_sq), ptr(pos), ptr(before), ptr(tied), ptr(pos_d2), ptr(ws),
                                   ctypes.c_size_t(nbytes), torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------------------------------ 6: out-of-range positives
def test_out_of_range_positives(ops):
    from focal_amd import _lib
    shape = SHAPES[0]
    nq, nt, D, _ = shape
    T, Q, pos = real_inputs(*shape)
    want = real_run(shape)
    bad = pos.astype(np.int64).copy()
    at = [3, 40, 69]
    bad[at] = [-1, nt, 2 ** 31 - 1]
    bad = bad.astype(np.int32)
    q, t = dev(Q), dev(T)
    t_sq = (t * t).sum(1)
    d = _lib.RankDesc(nq, nt, D, 3)
    need = _lib.load().focal_rank_workspace(ctypes.byref(d))
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    before = torch.full((nq,), -7, dtype=torch.int32, device=DEV)
    tied = torch.full((nq,), -7, dtype=torch.int32, device=DEV)
    pos_d2 = torch.full((nq,), -7.0, device=DEV)
    _lib.check(call_entry(d, q, t, t_sq, dev(bad), before, tied, pos_d2, ws))
    before, tied, pos_d2 = before.cpu().numpy(), tied.cpu().numpy(), pos_d2.cpu().numpy()
    keep = np.ones(nq, dtype=bool)
    keep[at] = False
    assert (before[at] == -1).all() and (tied[at] == -1).all() and np.isnan(pos_d2[at]).all()
    assert np.array_equal(before[keep], want[0][keep]) and np.array_equal(tied[keep], want[1][keep])
    assert pos_d2[keep].tobytes() == want[2][keep].tobytes()
    # the optional outputs left out: `before` alone is the same
    alone = torch.full((nq,), -7, dtype=torch.int32, device=DEV)
    _lib.check(call_entry(d, q, t, t_sq, dev(bad), alone, None, None, ws))
    assert np.array_equal(alone.cpu().numpy(), before)
    # and through the wrapper
    got = ops.rank_positive(q, t, t_sq, dev(bad), want_d2=True)
    assert np.array_equal(got[0].cpu().numpy(), before) and np.array_equal(got[1].cpu().numpy(), tied)


# ------------------------------------------------------------------------------------------ 7: limits
@pytest.mark.parametrize("name,D,slices,offset,short,match", [("D=34", 34, 2, 0, False, "D % 4 == 0"), ("slices=0", 36, 0, 0, False, "1 <= slices <= 65535"),
                                                              ("slices=65536", 36, 65536, 0, False, "1 <= slices <= 65535"),
                                                              ("misaligned q", 36, 2, 1, False, "16-byte aligned"),
                                                              ("short ws", 36, 2, 0, True, "workspace of")],
                         ids=["D=34", "slices=0", "slices=65536", "misaligned-q", "short-ws"])
def test_limits_refused_before_any_launch(ops, name, D, slices, offset, short, match):
    from focal_amd import _lib
    nq, nt = 20, 50
    q = torch.zeros(nq * D + 4, device=DEV)[offset:offset + nq * D].view(nq, D)
    t = torch.zeros(nt, D, device=DEV)
    t_sq, pos = torch.zeros(nt, device=DEV), torch.zeros(nq, dtype=torch.int32, device=DEV)
    before = torch.full((nq,), -7, dtype=torch.int32, device=DEV)
    tied = torch.full((nq,), -7, dtype=torch.int32, device=DEV)
    pos_d2 = torch.full((nq,), -7.0, device=DEV)
    ws = torch.full((nq * 8,), 0xF9, dtype=torch.uint8, device=DEV)
    d = _lib.RankDesc(nq, nt, D, slices)
    good = _lib.RankDesc(nq, nt, 36, 2)
    assert _lib.load().focal_rank_workspace(ctypes.byref(good)) == nq * 8
    with pytest.raises(_lib.FocalHipError, match=re.escape(match)):
        _lib.check(call_entry(d, q, t, t_sq, pos, before, tied, pos_d2, ws, ws_bytes=nq * 8 - 1 if short else None))
    if not short:  # (the wrapper sizes the workspace itself) the same text through the tensor-level wrapper
        with pytest.raises(_lib.FocalHipError, match=re.escape(match)):
            ops.rank_positive(q, t, t_sq, pos, slices=slices)
    torch.cuda.synchronize()
    for buf in (before, tied, pos_d2):
        assert (buf == -7).all()
    assert (ws == 0xF9).all()


def test_wrapper_refuses_other_tensors(ops):
    from focal_amd._lib import FocalHipError
    q, t = torch.zeros(8, 36, device=DEV), torch.zeros(12, 36, device=DEV)
    t_sq, pos = torch.zeros(12, device=DEV), torch.zeros(8, dtype=torch.int32, device=DEV)
    with pytest.raises(FocalHipError, match="fp32"):
        ops.rank_positive(q.double(), t, t_sq, pos)
    with pytest.raises(FocalHipError, match="int32"):
        ops.rank_positive(q, t, t_sq, pos.long())
    with pytest.raises(FocalHipError, match="norms"):
        ops.rank_positive(q, t, t_sq[:5], pos)
    with pytest.raises(FocalHipError, match="contiguous"):
        ops.rank_positive(torch.zeros(8, 72, device=DEV)[:, ::2], t, t_sq, pos)


# ------------------------------------------------------------------------------------------ 8: capture
def test_capture_and_replay(ops):
    shape = SHAPES[1]
    T, Q, pos = real_inputs(*shape)
    t, p = dev(T), dev(pos)
    t_sq = (t * t).sum(1)
    r = np.random.default_rng(77)
    others = [dev(r.standard_normal(Q.shape).astype(np.float32)) for _ in range(2)]
    eager = [[o.clone() for o in ops.rank_positive(x, t, t_sq, p, want_d2=True)] for x in others]
    static_q = dev(Q).clone()
    ops.rank_positive(static_q, t, t_sq, p, want_d2=True)  # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.rank_positive(static_q, t, t_sq, p, want_d2=True)
    for x, want in zip(others, eager):
        static_q.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(out, want):
            assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------ 9: fused against torch
@functools.lru_cache(maxsize=None)
def paired_inputs(n, D, seed):
    """Two [n, D] matrices whose rows i belong together: b = T, a = T + 3 N with the draws of the real inputs at nq = nt = n."""
    r = np.random.default_rng(seed)
    T = r.standard_normal((n, D)).astype(np.float32)
    r.integers(0, n, n)
    N = r.standard_normal((n, D)).astype(np.float32)
    return (T + np.float32(3.0) * N).astype(np.float32), T


@pytest.mark.parametrize("shape", SHAPES[:3], ids=IDS[:3])
def test_fused_against_torch(shape):
    """Both forms on the same unit rows (n = the shape's gallery rows, 333 and 4099 being no multiple of 4: the torch form's product pads):
    equal wherever float64 on those rows decides the rank."""
    from train_utils.retrieval import cross_modal_ranks
    _, n, D, seed = shape
    a, b = paired_inputs(n, D, seed)
    ranks, tied, q, t = cross_modal_ranks(dev(a), dev(b), fused=True)
    ranks_t, tied_t, q_t, t_t = cross_modal_ranks(dev(a), dev(b), fused=False, chunk=1000)  # (more than one chunk at 1500 and 4099)
    assert ranks.dtype == torch.int64 and tied.dtype == torch.int64 and ranks_t.dtype == torch.int64
    assert torch.equal(q, q_t) and torch.equal(t, t_t)
    qn = q.cpu().numpy()
    assert np.allclose((qn.astype(np.float64) ** 2).sum(1), 1.0, atol=1e-6)
    _, _, lo, hi = interval(qn, t.cpu().numpy(), np.arange(n))
    decided = lo == hi
    print(f"fused against torch {shape}: undecided {1 - decided.mean():.4f}, ranks {int(ranks.min())} .. {int(ranks.max())}")
    assert 1 - decided.mean() <= 0.10
    ranks, ranks_t = ranks.cpu().numpy(), ranks_t.cpu().numpy()
    assert np.array_equal(ranks[decided], lo[decided] + 1) and np.array_equal(ranks_t[decided], lo[decided] + 1)
    assert (lo + 1 <= ranks).all() and (ranks <= hi + 1).all()


# ------------------------------------------------------------------------------------------ 10: eval_retrieval.py
def retrieval_entry():
    spec = importlib.util.spec_from_file_location("focal_eval_retrieval_entry", os.path.join(SRC, "eval_retrieval.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def retrieval_parsed(monkeypatch, argv):
    from params.retrieval_params import parse_retrieval_params
    monkeypatch.setattr(sys, "argv", ["eval_retrieval.py"] + argv)
    return parse_retrieval_params()


def write_seeded_backbone(args):
    """Name-seeded weights under the name the pretraining loop would use (its checkpoints are the backbone's whole state dict)."""
    from oracle.weights import fill_state_dict_
    from train_utils.model_selection import init_backbone_model
    net = init_backbone_model(copy.copy(args))
    torch.save(fill_state_dict_({k: v.detach().cpu().clone() for k, v in net.state_dict().items()}), args.backbone_weight)


LINE = re.compile(r"Retrieval \[(\w+)\] (\S+) -> (\S+) \(n=(\d+)\): (.*), MRR ([\d.]+), median rank ([\d.]+), mean tied ([\d.]+)")


def parse_report(text):
    out = {}
    for m in LINE.finditer(text):
        recall = {int(k): float(v) for k, v in re.findall(r"R@(\d+) ([\d.]+)", m.group(5))}
        out[(m.group(1), m.group(2), m.group(3))] = (int(m.group(4)), recall, float(m.group(6)), float(m.group(7)), float(m.group(8)))
    return out, re.findall(r"^(?:chance|Orthogonality).*$", text, re.M)


def test_eval_retrieval_end_to_end_deepsense(monkeypatch, tmp_path, capsys):
    """DeepSense on MOD in fp32 (its forward repeats exactly): the synthetic test split is one batch of 32 windows, so n = 32 per modality."""
    from train_utils.retrieval import retrieval_metrics
    argv = ["-model=DeepSense", "-dataset=MOD", "-learn_framework=FOCAL", f"-model_weight={tmp_path}", "-batch_size=32", "-compute_dtype=fp32",
            "-synthetic_batches=2"]
    args = retrieval_parsed(monkeypatch, argv)
    assert args.backbone_weight == os.path.join(str(tmp_path), "MOD_DeepSense_pretrain_best.pt")
    assert args.retrieval_ks == [1, 5, 10] and args.retrieval_split == "test"
    write_seeded_backbone(args)
    capsys.readouterr()
    out, kept = retrieval_entry().evaluate_retrieval(args, keep=True)
    text = capsys.readouterr().out
    printed, other = parse_report(text)
    mods = args.dataset_config["modality_names"]
    proj = {m: kept["projections"][m] for m in mods}
    n = proj[mods[0]].shape[0]
    assert kept["labels"].shape[0] == n and all(p.dtype == torch.float32 and p.shape[0] == n for p in proj.values())
    width = proj[mods[0]].shape[1]
    assert width == args.dataset_config["FOCAL"]["emb_dim"] and n == 32
    h = width // 2
    cut = {"shared": slice(0, h), "private": slice(h, 2 * h), "full": slice(0, width)}
    pairs = [(a, b) for a in mods for b in mods if a != b]
    assert set(printed) == {(s, a, b) for s in cut for a, b in pairs}
    norm = lambda x: (x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-12))
    for space, cols in cut.items():
        for a, b in pairs:
            ranks, tied = kept["ranks"][space][(a, b)].cpu(), kept["tied"][space][(a, b)].cpu()
            qa = norm(proj[a][:, cols].cpu().numpy().astype(np.float64)).astype(np.float32)
            tb = norm(proj[b][:, cols].cpu().numpy().astype(np.float64)).astype(np.float32)
            # the interval of the float64 distances of the unit rows; normalising in float64 and rounding moves a row by at most u of
            # its length, d2 by at most 4 u: inside the 4 D u (1 + 1) band for every D >= 4
            _, _, lo, hi = interval(qa, tb, np.arange(n))
            assert (lo + 1 <= ranks.numpy()).all() and (ranks.numpy() <= hi + 1).all(), (space, a, b)
            want = retrieval_metrics(ranks, tied, args.retrieval_ks)
            got = out["retrieval"][space][(a, b)]
            # counts, rank sums and the median are integers or halves, exact in float64 in any order; the reciprocals' sum is not: the
            # device adds its n positive terms in another order than the host, each order within (n - 1) 2^-53 of the exact sum
            assert {k: v for k, v in got.items() if k != "mrr"} == {k: v for k, v in want.items() if k != "mrr"}
            assert abs(got["mrr"] - want["mrr"]) <= 2 * n * 2.0 ** -53 * want["mrr"]
            pn, precall, pmrr, pmed, ptied = printed[(space, a, b)]
            assert pn == n == got["n"]
            assert all(abs(precall[k] - got["recall"][k]) <= 5.1e-6 for k in args.retrieval_ks)
            assert abs(pmrr - got["mrr"]) <= 5.1e-6 and abs(pmed - got["median_rank"]) <= 0.051 and abs(ptied - got["mean_tied"]) <= 5.1e-4
    assert any(line.startswith("chance") for line in other) and sum(line.startswith("Orthogonality") for line in other) >= len(mods)
    r = subprocess.run([sys.executable, os.path.join(SRC, "eval_retrieval.py")] + argv, capture_output=True, text=True, timeout=300, cwd=SRC)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert parse_report(r.stdout) == (printed, other)


def test_eval_retrieval_multi_location_swin(monkeypatch, tmp_path):
    """SW_Transformer on HAR3LOC in bf16: it builds, runs, reports 2 ordered pairs x 3 spaces and accounts for every row."""
    argv = ["-model=SW_Transformer", "-dataset=HAR3LOC", "-learn_framework=FOCAL", f"-model_weight={tmp_path}", "-batch_size=16"]
    args = retrieval_parsed(monkeypatch, argv)
    assert args.backbone_weight == os.path.join(str(tmp_path), "HAR3LOC_SW_Transformer_pretrain_best.pt")
    assert len(args.dataset_config["location_names"]) > 1
    write_seeded_backbone(args)
    out, kept = retrieval_entry().evaluate_retrieval(args, keep=True)
    mods = args.dataset_config["modality_names"]
    assert len(mods) == 2
    n = kept["labels"].shape[0]
    assert n == 16
    for space in ("shared", "private", "full"):
        assert len(out["retrieval"][space]) == 2
        for pair, m in out["retrieval"][space].items():
            ranks = kept["ranks"][space][pair]
            assert m["n"] == n == ranks.numel() and int(ranks.min()) >= 1 and int(ranks.max()) <= n
            assert 0.0 <= m["recall"][1] <= m["recall"][5] <= m["recall"][10] <= 1.0
