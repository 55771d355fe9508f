"""Host half of eval_geometry.py: its flags, what it refuses before anything is built, the silhouette from hand-made sum tables against
sklearn, the effective rank against numpy's SVD, the alignment against numpy, and the export's declarations."""
import argparse
import importlib.util
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SRC = os.path.join(ROOT, "focal_amd", "src")
TWO_MODS = {"modality_names": ["seismic", "audio"], "FOCAL": {"emb_dim": 256}, "activity_classification": {"num_classes": 8}}


def entry():
    spec = importlib.util.spec_from_file_location("focal_eval_geometry_entry", os.path.join(SRC, "eval_geometry.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _run(tmp_path, **kw):
    base = dict(dataset="HAR3LOC", model="SW_Transformer", task="activity_classification", learn_framework="FOCAL", stage="pretrain",
                label_ratio=1.0, model_weight=None, weight_folder=str(tmp_path / "weights" / "HAR3LOC_SW_Transformer"),
                geometry_split="test", geometry_t=2.0, geometry_max_rows=65536, geometry_seed=0, dataset_config=TWO_MODS,
                backbone_weight=str(tmp_path / "x.pt"))
    base.update(kw)
    return argparse.Namespace(**base)


@pytest.fixture
def nothing_is_built(monkeypatch):
    """A loader, a model or a device selected during a refusal fails the test."""
    import input_utils.multi_modal_dataloader as loaders
    import params.geometry_params as gparams
    import params.params_util as util
    import train_utils.model_selection as selection

    def forbidden(*a, **k):
        raise AssertionError("built before the refusal")
    monkeypatch.setattr(loaders, "create_dataloader", forbidden)
    monkeypatch.setattr(selection, "init_backbone_model", forbidden)
    monkeypatch.setattr(util, "select_device", forbidden)
    monkeypatch.setattr(gparams, "set_auto_params", forbidden)
    monkeypatch.setattr(torch.cuda, "set_device", forbidden)
    monkeypatch.delenv("WORLD_SIZE", raising=False)


# ------------------------------------------------------------------------------------------ flags
def test_flags_default_and_parse(monkeypatch):
    from params.base_params import parse_base_args
    from params.geometry_params import refuse_geometry_settings
    monkeypatch.setattr(sys, "argv", ["eval_geometry.py", "-learn_framework=FOCAL"])
    a = parse_base_args("eval_geometry")
    assert a.option == "eval_geometry" and a.geometry_split == "test" and a.geometry_t == 2.0
    assert a.geometry_max_rows == 65536 and a.geometry_seed == 0
    refuse_geometry_settings(a)
    monkeypatch.setattr(sys, "argv", ["eval_geometry.py", "-learn_framework=FOCAL", "-geometry_split=train", "-geometry_t=0.5",
                                      "-geometry_max_rows=1000", "-geometry_seed=7"])
    a = parse_base_args("eval_geometry")
    assert (a.geometry_split, a.geometry_t, a.geometry_max_rows, a.geometry_seed) == ("train", 0.5, 1000, 7)
    refuse_geometry_settings(a)


# ------------------------------------------------------------------------------------------ refusals
def test_other_frameworks_are_refused(monkeypatch, tmp_path, nothing_is_built):
    from params.geometry_params import parse_geometry_params
    monkeypatch.setattr(sys, "argv", ["eval_geometry.py", "-model=DeepSense", "-dataset=MOD", "-learn_framework=no"])
    with pytest.raises(ValueError, match=r"eval_geometry\.py.*test\.py -model=DeepSense -dataset=MOD -learn_framework=no"):
        parse_geometry_params()
    with pytest.raises(ValueError, match=r"eval_geometry\.py.*test\.py"):
        entry().evaluate_geometry(_run(tmp_path, learn_framework="no"))


def test_data_parallel_is_refused(monkeypatch, tmp_path, nothing_is_built):
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="one process"):
        entry().evaluate_geometry(_run(tmp_path))
    with pytest.raises(SystemExit, match="one process"):
        entry().main_eval_geometry()


def test_missing_checkpoint_is_refused(tmp_path, nothing_is_built):
    from params.knn_params import resolve_backbone_weight
    args = _run(tmp_path)
    args.backbone_weight = resolve_backbone_weight(args)
    with pytest.raises(FileNotFoundError, match=r"train\.py -model=SW_Transformer -dataset=HAR3LOC -learn_framework=FOCAL"):
        entry().evaluate_geometry(args)
    assert not hasattr(args, "classifier")


@pytest.mark.parametrize("name,flags", [("MOD_DeepSense_vehicle_classification_1.0_finetune_best.pt", "-learn_framework=FOCAL -stage=finetune"),
                                        ("MOD_DeepSense_vehicle_classification_best.pt", "-learn_framework=no")])
def test_classifier_checkpoint_is_refused(tmp_path, nothing_is_built, name, flags):
    path = tmp_path / name
    torch.save({"class_layer.0.weight": torch.zeros(2, 2)}, path)
    cfg = dict(TWO_MODS, vehicle_classification={"num_classes": 7})
    args = _run(tmp_path, model="DeepSense", dataset="MOD", task="vehicle_classification", model_weight=str(path), backbone_weight=str(path),
                dataset_config=cfg)
    with pytest.raises(ValueError, match=re.escape(f"test.py -model=DeepSense -dataset=MOD {flags}") + r".*eval_geometry\.py"):
        entry().evaluate_geometry(args)
    assert not hasattr(args, "classifier")


@pytest.mark.parametrize("flag,match", [("-geometry_split=all", "-geometry_split=test"), ("-geometry_t=0", "-geometry_t=2"),
                                        ("-geometry_t=-1.5", "-geometry_t=2"), ("-geometry_t=inf", "-geometry_t=2"),
                                        ("-geometry_t=nan", "-geometry_t=2"), ("-geometry_max_rows=1", "-geometry_max_rows=65536"),
                                        ("-geometry_max_rows=-4", "-geometry_max_rows=65536")])
def test_settings_are_refused(monkeypatch, tmp_path, nothing_is_built, flag, match):
    """Every message names what to set instead."""
    from params.geometry_params import parse_geometry_params
    monkeypatch.setattr(sys, "argv", ["eval_geometry.py", "-model=DeepSense", "-dataset=MOD", "-learn_framework=FOCAL", flag])
    with pytest.raises(ValueError, match=r"eval_geometry\.py.*" + re.escape(match)):
        parse_geometry_params()
    name, value = flag[1:].split("=", 1)
    kind = {"geometry_split": str, "geometry_t": float, "geometry_max_rows": int}[name]
    with pytest.raises(ValueError, match=re.escape(match)):
        entry().evaluate_geometry(_run(tmp_path, **{name: kind(value)}))


def test_dataset_shape_is_refused(monkeypatch, tmp_path, nothing_is_built):
    from input_utils.yaml_utils import load_yaml
    from params.geometry_params import parse_geometry_params
    cfg = load_yaml(os.path.join(SRC, "data", "MOD.yaml"))
    assert cfg["vehicle_classification"]["num_classes"] == 7 and cfg["FOCAL"]["emb_dim"] == 256
    import yaml
    many = dict(cfg, vehicle_classification=dict(cfg["vehicle_classification"], num_classes=65))
    odd = dict(cfg, FOCAL=dict(cfg["FOCAL"], emb_dim=36))  # halves of 18 columns
    for name, bad, match in (("many.yaml", many, r"65 classes.*at most 64.*-task.*eval_knn\.py -model=DeepSense -dataset=MOD"),
                             ("odd.yaml", odd, r"emb_dim=36.*halves of 18.*multiple of 8")):
        path = tmp_path / name
        path.write_text(yaml.safe_dump(bad))
        monkeypatch.setattr(sys, "argv", ["eval_geometry.py", "-model=DeepSense", "-dataset=MOD", "-learn_framework=FOCAL", f"-config={path}"])
        with pytest.raises(ValueError, match=match):
            parse_geometry_params()
        with pytest.raises(ValueError, match=match):
            entry().evaluate_geometry(_run(tmp_path, model="DeepSense", dataset="MOD", task="vehicle_classification", dataset_config=bad))
    ok = dict(cfg, vehicle_classification=dict(cfg["vehicle_classification"], num_classes=64))
    from params.geometry_params import refuse_dataset_shape
    refuse_dataset_shape(_run(tmp_path), ok, "vehicle_classification")  # 64 classes pass


# ------------------------------------------------------------------------------------------ silhouette from sums
def sums_table(X, labels, G):
    """S[i, g] = the sum of float64 distances from row i to the rows of class g (its distance to itself is 0), and the class sizes."""
    d = np.sqrt(((X[:, None, :] - X[None, :, :]) ** 2).sum(-1))
    S = np.stack([d[:, labels == g].sum(1) for g in range(G)], axis=1)
    return S, np.bincount(labels, minlength=G)


def test_silhouette_from_sums_against_sklearn():
    from sklearn.metrics import silhouette_samples
    from train_utils.geometry import silhouette_from_sums
    r = np.random.default_rng(3)
    X = r.standard_normal((40, 5)) + 2.0 * r.integers(0, 3, 40)[:, None]
    labels = r.integers(0, 4, 40)
    labels[labels == 2] = 5   # class 2 is missing, and ids 4, 6 never occur: G = 7 with three empty classes
    labels[7] = 4             # ... and class 4 is a singleton
    labels[:4] = [0, 1, 3, 5]
    G = 7
    S, counts = sums_table(X, labels, G)
    assert counts[2] == 0 and counts[6] == 0 and counts[4] == 1
    s, mean, per_class = silhouette_from_sums(torch.from_numpy(S), torch.from_numpy(labels), torch.from_numpy(counts))
    want = silhouette_samples(X, labels)
    assert s.dtype == torch.float64 and np.allclose(s.numpy(), want, rtol=0, atol=1e-12)
    assert s[7] == 0.0  # the singleton
    assert mean == pytest.approx(want.mean(), abs=1e-12)
    per_class = per_class.numpy()
    for g in range(G):
        if counts[g]:
            assert per_class[g] == pytest.approx(want[labels == g].mean(), abs=1e-12)
        else:
            assert np.isnan(per_class[g])


def test_silhouette_of_coincident_rows_and_one_class():
    from sklearn.metrics import silhouette_samples
    from train_utils.geometry import group_counts, silhouette_from_sums
    # a = b = 0: rows 0 .. 3 are one point that is all of class 0 and all of class 1; class 2 lies elsewhere
    X = np.array([[1.0, 1.0]] * 4 + [[5.0, 1.0], [5.0, 2.0]])
    labels = np.array([0, 0, 1, 1, 2, 2])
    S, counts = sums_table(X, labels, 3)
    s, mean, _ = silhouette_from_sums(torch.from_numpy(S), torch.from_numpy(labels), torch.from_numpy(counts))
    want = silhouette_samples(X, labels)
    assert s[0] == 0.0 and s[1] == 0.0 and want[0] == 0.0
    assert np.allclose(s.numpy(), want, rtol=0, atol=1e-12) and mean == pytest.approx(want.mean(), abs=1e-12)
    # one class present: undefined
    labels = np.full(6, 1)
    S, counts = sums_table(X, labels, 3)
    s, mean, per_class = silhouette_from_sums(torch.from_numpy(S), torch.from_numpy(labels), torch.from_numpy(counts))
    assert np.isnan(mean) and torch.isnan(s).all() and torch.isnan(per_class).all()
    assert group_counts(torch.tensor([0, 2, 2]), 4).tolist() == [1, 0, 2, 0]
    with pytest.raises(ValueError, match=r"\[0, 3\)"):
        group_counts(torch.tensor([0, 3]), 3)
    with pytest.raises(ValueError, match=r"\[0, 3\)"):
        group_counts(torch.tensor([-1, 1]), 3)


# ------------------------------------------------------------------------------------------ effective rank, alignment
def rankme(X):
    X = X.astype(np.float64)
    sv = np.linalg.svd(X - X.mean(0), compute_uv=False)
    if sv.sum() == 0:
        return 1.0
    p = sv / sv.sum()
    p = p[p > 0]
    return float(np.exp(-(p * np.log(p)).sum()))


def test_effective_rank_against_svd():
    from train_utils.geometry import effective_rank
    r = np.random.default_rng(11)
    full = r.standard_normal((50, 12)).astype(np.float32)
    low = (r.standard_normal((50, 3)) @ r.standard_normal((3, 12))).astype(np.float32)
    one = (np.linspace(-1, 1, 30)[:, None] * r.standard_normal((1, 8))).astype(np.float32) + 4.0
    eye = np.eye(9, dtype=np.float32)
    # (the squared singular values are taken as eigenvalues of the scatter matrix: a direction of relative size e costs sqrt(e) there, so
    # rank-deficient inputs agree to about sqrt(2^-53 * condition), not to 1e-12)
    for X, tol in ((full, 1e-9), (low, 1e-5), (one, 1e-5), (eye, 1e-6)):
        got = effective_rank(torch.from_numpy(X))
        assert got == pytest.approx(rankme(X), rel=tol), X.shape
        assert effective_rank(torch.from_numpy(X), chunk=7) == pytest.approx(rankme(X), rel=tol)  # more than one chunk of rows
    assert effective_rank(torch.from_numpy(one)) == pytest.approx(1.0, abs=1e-5)
    assert effective_rank(torch.from_numpy(eye)) == pytest.approx(8.0, rel=1e-6)  # centring removes one direction of the identity
    assert effective_rank(torch.zeros(10, 4)) == 1.0
    assert effective_rank(torch.full((10, 4), 3.5)) == 1.0  # no variation at all


def test_alignment_against_numpy():
    from train_utils.geometry import alignment
    r = np.random.default_rng(2)
    a = r.standard_normal((33, 16)).astype(np.float32) * 5
    b = (a + r.standard_normal((33, 16))).astype(np.float32) * 0.1
    un = lambda x: x.astype(np.float64) / np.linalg.norm(x.astype(np.float64), axis=1, keepdims=True)
    want = ((un(a) - un(b)) ** 2).sum(1).mean()
    # (the rows are made unit length in fp32, as every tool here does: 2^-24 per component)
    assert alignment(torch.from_numpy(a), torch.from_numpy(b)) == pytest.approx(want, abs=1e-6)
    assert alignment(torch.from_numpy(a), torch.from_numpy(3 * a)) == pytest.approx(0.0, abs=1e-6)
    assert alignment(torch.from_numpy(a), torch.from_numpy(-a)) == pytest.approx(4.0, abs=1e-5)
    with pytest.raises(ValueError, match="one shape"):
        alignment(torch.zeros(3, 4), torch.zeros(4, 4))


# ------------------------------------------------------------------------------------------ declarations
def test_exports_are_declared_at_abi_14():
    from focal_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "focal_hip.h")).read()
    assert re.search(r"#define FOCAL_ABI_VERSION 14\b", hdr) and _lib.ABI_VERSION == 14
    assert re.search(r"typedef struct \{ int nq, nt, D, G, slices, fn, self_offset; float scale; \} focal_pairsum_desc;", hdr)
    assert re.search(r"enum \{ FOCAL_PAIR_SQDIST = 0, FOCAL_PAIR_DIST = 1, FOCAL_PAIR_GAUSS = 2 \};", hdr)
    assert re.search(r"size_t focal_pair_sums_workspace\(const focal_pairsum_desc\* d\);", hdr)
    assert re.search(r"int focal_pair_sums\(const focal_pairsum_desc\* d, const float\* q, const float\* t, const float\* t_sq, const int\* group,\s*"
                     r"float\* S, void\* ws,\s*size_t ws_bytes, void\* stream\);", hdr)
    assert len(_lib.PROTOTYPES["focal_pair_sums_workspace"][1]) == 1 and len(_lib.PROTOTYPES["focal_pair_sums"][1]) == 9
    assert [n for n, _ in _lib.PairSumDesc._fields_] == ["nq", "nt", "D", "G", "slices", "fn", "self_offset", "scale"]
    import ctypes
    assert ctypes.sizeof(_lib.PairSumDesc) == 32 and _lib.PairSumDesc.scale.offset == 28
    assert _lib.PAIR_FNS == {"sqdist": 0, "dist": 1, "gauss": 2} and _lib.PAIR_MAX_GROUPS == 64


def test_pairsum_source_is_built():
    mk = open(os.path.join(ROOT, "focal_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*=\s*(.*)$", mk, re.M).group(1).split()
    assert "pairsum.hip" in srcs and "rank.hip" in srcs
    assert os.path.isfile(os.path.join(ROOT, "focal_amd", "csrc", "pairsum.hip"))
