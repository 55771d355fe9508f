"""Host half of eval_temporal.py: its flags, what it refuses before anything is built, temporal_metrics on hand-made counts, the torch form
of sequence_ranking against the loss's own definition (oracle.loss.temporal_ranking), the subset cut, the nearest siblings, and the
export's declarations."""
import argparse
import ctypes
import importlib.util
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SRC = os.path.join(ROOT, "focal_amd", "src")
TWO_MODS = {"modality_names": ["seismic", "audio"], "seq_len": 4, "FOCAL": {"emb_dim": 256, "inter_rank_margin": 1.0},
            "activity_classification": {"num_classes": 8}}


def entry():
    spec = importlib.util.spec_from_file_location("focal_eval_temporal_entry", os.path.join(SRC, "eval_temporal.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _run(tmp_path, **kw):
    base = dict(dataset="HAR3LOC", model="SW_Transformer", task="activity_classification", learn_framework="FOCAL", stage="pretrain",
                label_ratio=1.0, model_weight=None, weight_folder=str(tmp_path / "weights" / "HAR3LOC_SW_Transformer"),
                temporal_split="test", temporal_margin=None, temporal_k="1,5,10", temporal_max_rows=65536, temporal_seed=0,
                dataset_config=TWO_MODS, backbone_weight=str(tmp_path / "x.pt"), sequence_sampler=True)
    base.update(kw)
    return argparse.Namespace(**base)


@pytest.fixture
def nothing_is_built(monkeypatch):
    """A loader, a model or a device selected during a refusal fails the test."""
    import input_utils.multi_modal_dataloader as loaders
    import params.params_util as util
    import params.temporal_params as tparams
    import train_utils.model_selection as selection

    def forbidden(*a, **k):
        raise AssertionError("built before the refusal")
    monkeypatch.setattr(loaders, "create_dataloader", forbidden)
    monkeypatch.setattr(selection, "init_backbone_model", forbidden)
    monkeypatch.setattr(util, "select_device", forbidden)
    monkeypatch.setattr(tparams, "set_auto_params", forbidden)
    monkeypatch.setattr(torch.cuda, "set_device", forbidden)
    monkeypatch.delenv("WORLD_SIZE", raising=False)


# ------------------------------------------------------------------------------------------ flags
def test_flags_default_and_parse(monkeypatch):
    from params.base_params import parse_base_args
    from params.temporal_params import refuse_temporal_settings
    monkeypatch.setattr(sys, "argv", ["eval_temporal.py", "-learn_framework=FOCAL"])
    a = parse_base_args("eval_temporal")
    assert a.option == "eval_temporal" and a.temporal_split == "test" and a.temporal_margin is None and a.temporal_k == "1,5,10"
    assert a.temporal_max_rows == 65536 and a.temporal_seed == 0
    assert refuse_temporal_settings(a) == [1, 5, 10]
    monkeypatch.setattr(sys, "argv", ["eval_temporal.py", "-learn_framework=FOCAL", "-temporal_split=val", "-temporal_margin=0.25",
                                      "-temporal_k=2,3", "-temporal_max_rows=1000", "-temporal_seed=7"])
    a = parse_base_args("eval_temporal")
    assert (a.temporal_split, a.temporal_margin, a.temporal_max_rows, a.temporal_seed) == ("val", 0.25, 1000, 7)
    assert refuse_temporal_settings(a) == [2, 3]


# ------------------------------------------------------------------------------------------ refusals
def test_other_frameworks_are_refused(monkeypatch, tmp_path, nothing_is_built):
    from params.temporal_params import parse_temporal_params
    monkeypatch.setattr(sys, "argv", ["eval_temporal.py", "-model=DeepSense", "-dataset=MOD", "-learn_framework=no"])
    with pytest.raises(ValueError, match=r"eval_temporal\.py.*test\.py -model=DeepSense -dataset=MOD -learn_framework=no"):
        parse_temporal_params()
    with pytest.raises(ValueError, match=r"eval_temporal\.py.*test\.py"):
        entry().evaluate_temporal(_run(tmp_path, learn_framework="no"))


def test_data_parallel_is_refused(monkeypatch, tmp_path, nothing_is_built):
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="one process"):
        entry().evaluate_temporal(_run(tmp_path))
    with pytest.raises(SystemExit, match="one process"):
        entry().main_eval_temporal()


def test_missing_checkpoint_is_refused(tmp_path, nothing_is_built):
    from params.knn_params import resolve_backbone_weight
    args = _run(tmp_path)
    args.backbone_weight = resolve_backbone_weight(args)
    with pytest.raises(FileNotFoundError, match=r"train\.py -model=SW_Transformer -dataset=HAR3LOC -learn_framework=FOCAL"):
        entry().evaluate_temporal(args)
    assert not hasattr(args, "classifier")


@pytest.mark.parametrize("name,flags", [("MOD_DeepSense_vehicle_classification_1.0_finetune_best.pt", "-learn_framework=FOCAL -stage=finetune"),
                                        ("MOD_DeepSense_vehicle_classification_best.pt", "-learn_framework=no")])
def test_classifier_checkpoint_is_refused(tmp_path, nothing_is_built, name, flags):
    path = tmp_path / name
    torch.save({"class_layer.0.weight": torch.zeros(2, 2)}, path)
    cfg = dict(TWO_MODS, vehicle_classification={"num_classes": 7})
    args = _run(tmp_path, model="DeepSense", dataset="MOD", task="vehicle_classification", model_weight=str(path), backbone_weight=str(path),
                dataset_config=cfg)
    with pytest.raises(ValueError, match=re.escape(f"test.py -model=DeepSense -dataset=MOD {flags}") + r".*eval_temporal\.py"):
        entry().evaluate_temporal(args)
    assert not hasattr(args, "classifier")


@pytest.mark.parametrize("flag,match", [("-temporal_split=all", "-temporal_split=test"), ("-temporal_margin=inf", "finite -temporal_margin"),
                                        ("-temporal_margin=nan", "FOCAL.inter_rank_margin"), ("-temporal_k=1,,5", "-temporal_k=1,5,10"),
                                        ("-temporal_k=0,5", "-temporal_k=1,5,10"), ("-temporal_k=1,2,3,4,5,6,7,8,9", "at most 8 values"),
                                        ("-temporal_k=one", "-temporal_k=1,5,10"), ("-temporal_max_rows=7", "-temporal_max_rows=65536"),
                                        ("-temporal_max_rows=-4", "2 * seq_len = 8")])
def test_settings_are_refused(monkeypatch, tmp_path, nothing_is_built, flag, match):
    """Every message names what to set instead."""
    from params.temporal_params import parse_temporal_params
    monkeypatch.setattr(sys, "argv", ["eval_temporal.py", "-model=DeepSense", "-dataset=MOD", "-learn_framework=FOCAL", flag])
    with pytest.raises(ValueError, match=r"eval_temporal\.py.*" + re.escape(match)):
        parse_temporal_params()
    name, value = flag[1:].split("=", 1)
    kind = {"temporal_split": str, "temporal_margin": float, "temporal_k": str, "temporal_max_rows": int}[name]
    with pytest.raises(ValueError, match=re.escape(match)):
        entry().evaluate_temporal(_run(tmp_path, **{name: kind(value)}))


def test_dataset_shape_is_refused(monkeypatch, tmp_path, nothing_is_built):
    import yaml
    from input_utils.yaml_utils import load_yaml
    from params.temporal_params import parse_temporal_params, refuse_dataset_shape
    cfg = load_yaml(os.path.join(SRC, "data", "MOD.yaml"))
    assert cfg["seq_len"] == 4 and cfg["FOCAL"]["emb_dim"] == 256
    long = dict(cfg, seq_len=5)
    longer = dict(cfg, seq_len=32)
    odd = dict(cfg, FOCAL=dict(cfg["FOCAL"], emb_dim=38))
    for name, bad, match in (("long.yaml", long, r"seq_len=5.*\{2, 4, 8, 16\}.*dataset's YAML"),
                             ("longer.yaml", longer, r"seq_len=32.*\{2, 4, 8, 16\}"),
                             ("odd.yaml", odd, r"emb_dim=38.*multiple of 4")):
        path = tmp_path / name
        path.write_text(yaml.safe_dump(bad))
        monkeypatch.setattr(sys, "argv", ["eval_temporal.py", "-model=DeepSense", "-dataset=MOD", "-learn_framework=FOCAL", f"-config={path}"])
        with pytest.raises(ValueError, match=match):
            parse_temporal_params()
        with pytest.raises(ValueError, match=match):
            entry().evaluate_temporal(_run(tmp_path, model="DeepSense", dataset="MOD", task="vehicle_classification", dataset_config=bad))
    for L in (2, 4, 8, 16):
        refuse_dataset_shape(_run(tmp_path, temporal_max_rows=2 * L), dict(cfg, seq_len=L))
        with pytest.raises(ValueError, match=rf"2 \* seq_len = {2 * L}"):
            refuse_dataset_shape(_run(tmp_path, temporal_max_rows=2 * L - 1), dict(cfg, seq_len=L))


# ------------------------------------------------------------------------------------------ metrics
def test_temporal_metrics_on_hand_made_counts():
    from train_utils.temporal import temporal_metrics
    L, S = 4, 3
    rank = {"hinge_sum": torch.tensor([0.5, 0.0, 2.5]), "viol": torch.tensor([1, 0, 2], dtype=torch.int32),
            "before": torch.tensor([0, 0, 1], dtype=torch.int32), "intra_sum": torch.tensor([12.0, 24.0, 36.0]),
            "inter_sum": torch.tensor([64.0, 32.0, 96.0])}
    m = temporal_metrics(rank, L)
    assert m["sequences"] == 3
    assert m["ranking_loss"] == 3.0 / 6 and m["margin_satisfied"] == 1 - 3 / 6 and m["ordered"] == 1 - 1 / 6
    assert m["mean_intra"] == 72.0 / (3 * 12) and m["mean_inter"] == 192.0 / (6 * 16) and m["ratio"] == 1.0
    rank["inter_sum"] = torch.zeros(3)
    assert math.isnan(temporal_metrics(rank, L)["ratio"])
    rank["hinge_sum"] = torch.tensor([0.5, float("nan"), 1.0])
    assert math.isnan(temporal_metrics(rank, L)["ranking_loss"])
    with pytest.raises(ValueError, match="S >= 2"):
        temporal_metrics({k: v[:1] for k, v in rank.items()}, L)


# ------------------------------------------------------------------------------------------ the definition is the loss's
@pytest.mark.parametrize("margin", [0.0, 1.0])
@pytest.mark.parametrize("b,L,D", [(8, 4, 16), (5, 2, 8), (3, 8, 12), (4, 16, 8)])
def test_torch_form_is_the_loss_term(b, L, D, margin):
    from oracle.loss import temporal_ranking
    from train_utils.temporal import sequence_ranking, temporal_metrics
    g = torch.Generator().manual_seed(100 * b + L)
    # (centres closer than the widest sequence is wide: some hinges are active at margin 0 too)
    centre = 0.5 * torch.randn(b, 1, D, generator=g, dtype=torch.float64)
    e = centre + torch.linspace(0.2, 1.5, b, dtype=torch.float64)[:, None, None] * torch.randn(b, L, D, generator=g, dtype=torch.float64)
    want = float(temporal_ranking(e, margin))
    for chunk in (8192, 2 * L):  # one chunk, and chunks of two sequences
        rank = sequence_ranking(e.reshape(b * L, D), L, margin, fused=False, chunk=chunk)
        assert rank["hinge_sum"].dtype == torch.float64 and rank["before"].dtype == torch.int32
        m = temporal_metrics(rank, L)
        assert abs(m["ranking_loss"] - want) <= 1e-12, (m["ranking_loss"], want)
    assert want > 0
    # the counts against the block means themselves
    x = e.reshape(b * L, D)
    d = (x[:, None, :] - x[None, :, :]).norm(dim=-1).view(b, L, b, L)
    mean = d.sum((1, 3)) / (L * L)
    intra = torch.stack([d[a, :, a, :].sum() / (L * L - L) for a in range(b)])
    off = ~torch.eye(b, dtype=torch.bool)
    gap = mean - intra[:, None]
    clear = (gap.abs() > 1e-9) & ((gap - margin).abs() > 1e-9)
    assert clear[off].all()
    assert rank["before"].tolist() == ((gap < 0) & off).sum(1).tolist()
    assert rank["viol"].tolist() == ((gap < margin) & off).sum(1).tolist()
    assert torch.allclose(rank["intra_sum"], intra * (L * L - L), rtol=0, atol=1e-12)
    assert torch.allclose(rank["inter_sum"], (d.sum((1, 3)) * off).sum(1), rtol=0, atol=1e-10)
    own = torch.stack([d[a, :, a, :] for a in range(b)]).reshape(b * L, L)
    assert torch.allclose(rank["intra_d2"], own * own, rtol=0, atol=1e-10)


def test_torch_form_nan_rule_and_refusals():
    from train_utils.temporal import sequence_ranking
    g = torch.Generator().manual_seed(5)
    z = torch.randn(24, 8, generator=g, dtype=torch.float64)
    z[9, 3] = float("nan")  # sequence 2 of L = 4
    rank = sequence_ranking(z, 4, 1.0, fused=False)
    assert torch.isnan(rank["hinge_sum"]).all() and torch.isnan(rank["inter_sum"]).all()  # P(a, 2) is NaN for every a
    assert rank["before"][2] == 0 and rank["viol"][2] == 0 and torch.isnan(rank["intra_sum"][2])
    clean = sequence_ranking(torch.cat([z[:8], z[12:]]), 4, 1.0, fused=False)
    keep = [0, 1, 3, 4, 5]
    assert rank["before"][keep].tolist() == clean["before"].tolist() and rank["viol"][keep].tolist() == clean["viol"].tolist()
    for n, L in ((24, 3), (24, 32), (22, 4), (4, 4)):
        with pytest.raises(ValueError, match="seq_len in"):
            sequence_ranking(torch.zeros(n, 8), L, 1.0, fused=False)
    with pytest.raises(ValueError, match="sqdist, dist"):
        sequence_ranking(torch.zeros(8, 8), 4, 1.0, fused=False, fn="gauss")


# ------------------------------------------------------------------------------------------ the subset cut, the siblings
def test_subset_keeps_whole_sequences():
    e = entry()
    rows = e.subset_sequences(40, 4, 65536, 0)
    assert rows.tolist() == list(range(40))
    for L, N, cap in ((4, 400, 50), (8, 800, 64), (2, 10, 4), (16, 1600, 47)):
        rows = e.subset_sequences(N, L, cap, 3)
        assert rows.dtype == torch.int64 and rows.numel() == cap // L * L
        first = rows.view(-1, L)[:, 0]
        assert (first % L == 0).all() and (rows.view(-1, L) == first[:, None] + torch.arange(L)[None, :]).all()
        assert (first[1:] > first[:-1]).all() and int(rows.max()) < N
        assert torch.equal(rows, e.subset_sequences(N, L, cap, 3)) and not torch.equal(rows, e.subset_sequences(N, L, cap, 4))
    with pytest.raises(ValueError, match="whole subsequences"):
        e.subset_sequences(41, 4, 16, 0)


def test_every_loader_kind_yields_whole_subsequences():
    """What eval_temporal.py relies on: rows k L .. k L + L - 1 of the concatenated batches are one subsequence -- the file-backed
    sampler, the packed loader's batches (both from partition_subsequences, the last chunk padded by its final sample) and the
    synthetic loader's batch size."""
    import types
    from input_utils.multi_modal_dataloader import BatchSeqSampler, SyntheticSequenceLoader
    from input_utils.multi_modal_dataset import partition_subsequences
    from input_utils.packed_shards import PackedSequenceLoader
    L = 4
    files = [f"runA_{i}.pt" for i in (3, 0, 1, 2, 4, 5)] + [f"runB_{i}.pt" for i in range(9)] + ["runC_0.pt"]
    subseqs, table = partition_subsequences(files, L)
    assert len(subseqs) == 2 + 3 + 1 and table["runA_4"] == [4, 5, 5, 5] and table["runC_0"] == [15, 15, 15, 15]
    whole = set(map(tuple, table.values()))
    args = argparse.Namespace(dataset_config={"seq_len": L})
    dataset = types.SimpleNamespace(subseqs=subseqs, subseq_to_sample_idx=table)
    packed = object.__new__(PackedSequenceLoader)
    packed.subseqs, packed.subseq_to_sample_idx, packed.subseq_batch = subseqs, table, 2
    packed.shuffle, packed.world, packed.rank, packed.seed, packed.epoch = False, 1, 0, 0, 0
    for batches in (list(BatchSeqSampler(args, 8, dataset, shard=False)), list(packed.batches())):
        rows = [i for b in batches for i in b]
        assert all(len(b) % L == 0 for b in batches) and len(rows) == L * len(subseqs)
        assert {tuple(rows[k:k + L]) for k in range(0, len(rows), L)} == whole
    with pytest.raises(ValueError, match="whole subsequences"):
        SyntheticSequenceLoader(argparse.Namespace(dataset_config={"seq_len": L}, device="cpu"), 30)
    SyntheticSequenceLoader(argparse.Namespace(dataset_config={"seq_len": L}, device="cpu"), 32)


def test_nearest_siblings_ties_and_nan():
    from train_utils.temporal import nearest_siblings
    nan = float("nan")
    d = torch.tensor([[0.0, 3.0, 2.0, 2.0],    # row 0 (self column 0): columns 2 and 3 tie -> 2
                      [1.0, 0.0, nan, 1.0],    # row 1: columns 0 and 3 tie -> 0; NaN orders last
                      [nan, nan, 0.0, nan],    # row 2: all NaN -> the first other column
                      [-1.0, 5.0, 0.0, -9.0],  # row 3 (self column 3, however small its value): column 0
                      [7.0, 0.0, 0.0, 0.0],    # row 4 (self column 0): columns 1 .. 3 tie at 0 -> 1
                      [0.0, 9.0, -0.0, 0.0],   # row 5 (self column 1): -0 == +0 -> 0
                      [4.0, 4.0, 4.0, 4.0],    # row 6 (self column 2) -> 0
                      [nan, 2.0, nan, 0.0]])   # row 7 (self column 3) -> 1
    assert nearest_siblings(d, 4).tolist() == [2, 0, 0, 0, 5, 4, 4, 5]
    with pytest.raises(ValueError, match="intra_d2"):
        nearest_siblings(torch.zeros(6, 4), 4)


# ------------------------------------------------------------------------------------------ declarations
def test_exports_are_declared_at_abi_14():
    from focal_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "focal_hip.h")).read()
    assert re.search(r"#define FOCAL_ABI_VERSION 14\b", hdr) and _lib.ABI_VERSION == 14
    assert re.search(r"typedef struct \{ int n, D, L, slices, fn; float margin; \} focal_seqrank_desc;", hdr)
    assert re.search(r"size_t focal_seq_rank_workspace\(const focal_seqrank_desc\* d\);", hdr)
    assert re.search(r"int focal_seq_rank\(const focal_seqrank_desc\* d, const float\* z, const float\* z_sq, float\* intra_d2, float\* intra_sum, "
                     r"int\* before, int\* viol,\s*float\* hinge_sum, float\* inter_sum, void\* ws, size_t ws_bytes, void\* stream\);", hdr)
    assert len(_lib.PROTOTYPES["focal_seq_rank_workspace"][1]) == 1 and len(_lib.PROTOTYPES["focal_seq_rank"][1]) == 12
    assert [n for n, _ in _lib.SeqRankDesc._fields_] == ["n", "D", "L", "slices", "fn", "margin"]
    assert ctypes.sizeof(_lib.SeqRankDesc) == 24 and _lib.SeqRankDesc.margin.offset == 20
    assert _lib.SEQRANK_FNS == {"sqdist": _lib.PAIR_FNS["sqdist"], "dist": _lib.PAIR_FNS["dist"]} and _lib.SEQRANK_LENGTHS == (2, 4, 8, 16)


def test_library_exports_what_the_header_declares():
    from focal_amd import _lib
    path = os.path.join(ROOT, "focal_amd", "libfocal_hip.so")
    if not os.path.isfile(path):
        pytest.fail("libfocal_hip.so is not built: __graft_entry__.build() builds it")
    lib = ctypes.CDLL(path)
    for name in ("focal_seq_rank", "focal_seq_rank_workspace"):
        assert hasattr(lib, name), name
    lib.focal_seq_rank_workspace.restype = ctypes.c_size_t
    lib.focal_seq_rank_workspace.argtypes = [ctypes.POINTER(_lib.SeqRankDesc)]
    ws = lambda *v: lib.focal_seq_rank_workspace(ctypes.byref(_lib.SeqRankDesc(*v)))
    assert ws(148, 12, 4, 1, 1, 1.0) == 16
    assert ws(148, 12, 4, 5, 1, 1.0) == 2 * 2 * 5 * 64 * 4
    for bad in ((148, 12, 3, 1, 1, 1.0), (150, 12, 4, 1, 1, 1.0), (4, 12, 4, 1, 1, 1.0), (148, 10, 4, 1, 1, 1.0), (148, 12, 4, 0, 1, 1.0),
                (148, 12, 4, 1, 2, 1.0), (148, 12, 4, 1, 1, float("inf"))):
        assert ws(*bad) == 0, bad


def test_seqrank_source_is_built():
    mk = open(os.path.join(ROOT, "focal_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*=\s*(.*)$", mk, re.M).group(1).split()
    assert "seqrank.hip" in srcs and os.path.isfile(os.path.join(ROOT, "focal_amd", "csrc", "seqrank.hip"))
