"""The seven tile kernels of the evaluation tools after the fold of their tile loop into knn_dist.hpp's PairTile: byte equality with what
the parent commit wrote (tests/golden/pair_tile_parent.json, recorded there by tests/golden/gen_pair_tile_parent.py) at an unchanged ABI.

Shapes: the smallest that reach every branch of the shared code -- a ragged last query tile (130, 257, 70, 1, 208, 1472 rows), a ragged
last gallery tile (333, 1500, 65, 77 rows), D % 32 != 0 with one k block (4), two (36) and four (100), and more than one slice, one of
which ends mid-tile (333 / 3 = 111, 1500 / 3 = 500 rows).  `slices` is always passed: the defaults depend on the device."""
import hashlib
import json
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pair_tile_parent.json")


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


def normal(seed, *shape):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def norms(a):
    """|row|^2 on the host, exactly rounded: the same fp32 on every machine."""
    return np.array([math.fsum(float(v) * float(v) for v in row) for row in a], dtype=np.float32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def pair_tile_digests(ops):
    """SHA-256 of the raw bytes the seven exports write, through Python signatures that are the same before and after the fold."""
    d = {}
    for nq, nt, D, k, slices in [(130, 333, 36, 5, 1), (70, 1500, 100, 16, 3), (1, 65, 4, 1, 2)]:
        rng = np.random.default_rng(nq + nt)
        q, t = normal(1000 + nq, nq, D), normal(2000 + nt, nt, D)
        conf = torch.zeros(7 * 7 + 1, dtype=torch.int32, device=DEV)
        preds, idx, d2 = ops.knn_search_vote(dev(q), dev(t), dev(norms(t)), dev(rng.integers(0, 7, nt)), k, 7,
                                             q_labels=dev(rng.integers(0, 7, nq)), conf=conf, want_neighbours=True, slices=slices)
        d[f"knn.{nq}x{nt}x{D}.k{k}.s{slices}"] = sha(preds, idx, d2, conf)
    for nq, nt, D, slices in [(130, 333, 36, 1), (257, 1500, 64, 3)]:
        q, t = normal(3000 + nq, nq, D), normal(4000 + nt, nt, D)
        pos = np.random.default_rng(nq).integers(0, nt, nq).astype(np.int32)
        pos[3], pos[7], pos[-1] = -1, nt, nt + 5
        d[f"rank.{nq}x{nt}x{D}.s{slices}"] = sha(*ops.rank_positive(dev(q), dev(t), dev(norms(t)), dev(pos), slices=slices, want_d2=True))
    for nq, nt, D in [(130, 333, 36), (257, 1500, 100)]:
        q, t = normal(5000 + nq, nq, D), normal(6000 + nt, nt, D)
        tq, tt, t_sq = dev(q), dev(t), dev(norms(t))
        rng = np.random.default_rng(nt)
        g7, g40 = dev(rng.integers(-1, 7, nt).astype(np.int32)), dev(rng.integers(0, 40, nt).astype(np.int32))
        own = tt[:nq].clone()  # q[i] is t[i]
        for slices in (1, 3):
            tag = f"pairsum.{nq}x{nt}x{D}.s{slices}"
            d[f"{tag}.gauss"] = sha(ops.pair_sums(tq, tt, t_sq, fn="gauss", scale=0.02, slices=slices))
            d[f"{tag}.G7.dist.self"] = sha(ops.pair_sums(own, tt, t_sq, group=g7, G=7, fn="dist", self_offset=0, slices=slices))
            d[f"{tag}.G40.sqdist"] = sha(ops.pair_sums(tq, tt, t_sq, group=g40, G=40, fn="sqdist", slices=slices))
    for n, D in [(208, 36), (1472, 100)]:
        z = normal(7000 + n, n, D)
        tz, z_sq = dev(z), dev(norms(z))
        for L in (2, 4, 8, 16):
            for slices in (1, 3):
                for fn in ("sqdist", "dist"):
                    out = ops.seq_rank(tz, z_sq, L, 0.5, fn=fn, slices=slices)
                    d[f"seqrank.{n}x{D}.L{L}.s{slices}.{fn}"] = sha(*[out[key] for key in ("intra_d2", "intra_sum", "before", "viol", "hinge_sum", "inter_sum")])
    for n, D in [(130, 36), (257, 100)]:  # 11 x 7 = 77 gallery rows: a restart / problem straddles the tile boundary
        x, c = normal(8000 + n, n, D), normal(9000 + n, 77, D)
        labels, min_d2 = ops.kmeans_assign(dev(x), dev(c), dev(norms(c)), 7, want_min_d2=True)
        d[f"kmeans.{n}x{D}"] = sha(labels, min_d2)
        y = np.random.default_rng(n).integers(0, 7, n).astype(np.int32)
        d[f"probe.{n}x{D}"] = sha(*ops.probe_forward(dev(x), dev(c), dev(normal(9500 + n, 77)), 7, y=dev(y), want_ce=True, want_g=True, want_preds=True))
    for n, D in [(130, 36), (200, 100)]:
        d[f"tsne.{n}x{D}"] = sha(*ops.tsne_dist(dev(normal(10000 + n, n, D)), want_norms=True))
    return d


def test_the_fold_writes_the_parents_bytes():
    """Every output of the seven exports against the digests recorded at the parent commit.  None of these kernels has a floating-point
    atomic and the integer atomics are order-free, so equality is the expectation, not a tolerance."""
    from focal_amd import _lib, ops
    want = json.load(open(FIXTURE))
    assert len(want["commit"]) == 40
    assert _lib.load().focal_abi_version() == want["abi"]
    got = pair_tile_digests(ops)
    assert set(got) == set(want["sha256"]) and len(got) == 3 + 2 + 12 + 32 + 4 + 2
    diff = sorted(k for k in got if got[k] != want["sha256"][k])
    assert not diff, diff
