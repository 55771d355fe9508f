"""Host half of eval_tsne.py: what it refuses before anything is built, the seeded row subset, the PCA start, the plot, the exports'
declarations -- and the yardstick of tests/test_tsne_gpu.py (tests/tsne_reference.py) pinned to sklearn's own helpers.

The two facts the yardstick rests on, both taken on the CPU in float64:
* its gradient and KL are sklearn's `_kl_divergence` (the same formulas: agreement to rounding, asserted at 1e-12);
* its joint probabilities differ from sklearn's `_joint_probabilities` by about 8e-6 of max P, because sklearn stops each row's search at
  an entropy tolerance of 1e-5 and the yardstick takes 64 steps; the bound asserted is the 5e-5 the GPU test uses against sklearn."""
import argparse
import importlib.util
import os
import re
import sys

import numpy as np
import pytest
import torch

from tsne_reference import blobs, gradient, joint

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SRC = os.path.join(ROOT, "focal_amd", "src")
CASES = [(300, 32, 5, 1.5, 0), (257, 36, 4, 1.0, 0)]


def entry():
    spec = importlib.util.spec_from_file_location("focal_eval_tsne_entry", os.path.join(SRC, "eval_tsne.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _run(tmp_path, **kw):
    base = dict(dataset="HAR3LOC", model="SW_Transformer", task="activity_classification", learn_framework="FOCAL", stage="pretrain",
                label_ratio=1.0, model_weight=None, weight_folder=str(tmp_path / "weights" / "HAR3LOC_SW_Transformer"), tsne_split="test",
                tsne_perplexity=30.0, tsne_iters=1000, tsne_init="pca", tsne_seed=0, tsne_max_rows=16384, tsne_out=None, tsne_plot=False)
    base.update(kw)
    return argparse.Namespace(**base)


@pytest.fixture
def nothing_is_built(monkeypatch):
    """A loader, a model or a device selected during a refusal fails the test."""
    import input_utils.multi_modal_dataloader as loaders
    import params.params_util as util
    import train_utils.model_selection as selection

    def forbidden(*a, **k):
        raise AssertionError("built before the refusal")
    monkeypatch.setattr(loaders, "create_dataloader", forbidden)
    monkeypatch.setattr(selection, "init_backbone_model", forbidden)
    monkeypatch.setattr(util, "select_device", forbidden)
    monkeypatch.setattr(torch.cuda, "set_device", forbidden)
    monkeypatch.delenv("WORLD_SIZE", raising=False)


def test_other_frameworks_are_refused(monkeypatch, tmp_path, nothing_is_built):
    from params.tsne_params import parse_tsne_params
    monkeypatch.setattr(sys, "argv", ["eval_tsne.py", "-model=DeepSense", "-dataset=MOD", "-learn_framework=no"])
    with pytest.raises(ValueError, match=r"eval_tsne\.py.*test\.py -model=DeepSense -dataset=MOD -learn_framework=no"):
        parse_tsne_params()
    with pytest.raises(ValueError, match=r"test\.py"):
        entry().evaluate_tsne(_run(tmp_path, learn_framework="no", backbone_weight=str(tmp_path / "x.pt")))


def test_data_parallel_is_refused(monkeypatch, tmp_path, nothing_is_built):
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="one process"):
        entry().evaluate_tsne(_run(tmp_path, backbone_weight=str(tmp_path / "x.pt")))
    with pytest.raises(SystemExit, match="one process"):
        entry().main_eval_tsne()


def test_missing_checkpoint_is_refused(tmp_path, nothing_is_built):
    from params.knn_params import resolve_backbone_weight
    args = _run(tmp_path)
    args.backbone_weight = resolve_backbone_weight(args)
    with pytest.raises(FileNotFoundError, match=r"train\.py -model=SW_Transformer -dataset=HAR3LOC -learn_framework=FOCAL"):
        entry().evaluate_tsne(args)
    assert not hasattr(args, "classifier")


@pytest.mark.parametrize("name,flags", [("MOD_DeepSense_vehicle_classification_1.0_finetune_best.pt", "-learn_framework=FOCAL -stage=finetune"),
                                        ("MOD_DeepSense_vehicle_classification_best.pt", "-learn_framework=no")])
def test_classifier_checkpoint_is_refused(tmp_path, nothing_is_built, name, flags):
    path = tmp_path / name
    torch.save({"class_layer.0.weight": torch.zeros(2, 2)}, path)
    args = _run(tmp_path, model="DeepSense", dataset="MOD", task="vehicle_classification", model_weight=str(path), backbone_weight=str(path))
    with pytest.raises(ValueError, match=re.escape(f"test.py -model=DeepSense -dataset=MOD {flags}")):
        entry().evaluate_tsne(args)
    assert not hasattr(args, "classifier")


@pytest.mark.parametrize("flag,match", [("-tsne_perplexity=0.5", r"-tsne_perplexity >= 1"), ("-tsne_perplexity=nan", r"finite -tsne_perplexity"),
                                        ("-tsne_perplexity=inf", r"finite -tsne_perplexity"), ("-tsne_iters=0", r"-tsne_iters >= 1"),
                                        ("-tsne_max_rows=1", r"2 <= -tsne_max_rows <= 32768"),
                                        ("-tsne_max_rows=32769", r"2 <= -tsne_max_rows <= 32768")])
def test_settings_are_refused_before_anything_is_built(monkeypatch, tmp_path, nothing_is_built, flag, match):
    from params.tsne_params import parse_tsne_params
    monkeypatch.setattr(sys, "argv", ["eval_tsne.py", "-model=DeepSense", "-dataset=MOD", "-learn_framework=FOCAL", flag])
    with pytest.raises(ValueError, match=match):
        parse_tsne_params()
    name, value = flag[1:].split("=")
    kind = int if name != "tsne_perplexity" else float
    with pytest.raises(ValueError, match=match):  # the entry point refuses the same namespace, the checkpoint still unopened
        entry().evaluate_tsne(_run(tmp_path, backbone_weight=str(tmp_path / "absent.pt"), **{name: kind(value)}))


def test_plot_without_matplotlib_is_refused(monkeypatch, tmp_path, nothing_is_built):
    import params.tsne_params as tp
    real = importlib.util.find_spec
    monkeypatch.setattr(tp.importlib.util, "find_spec", lambda name, *a: None if name == "matplotlib" else real(name, *a))
    with pytest.raises(ValueError, match=r"without -tsne_plot"):
        entry().evaluate_tsne(_run(tmp_path, backbone_weight=str(tmp_path / "absent.pt"), tsne_plot=True))
    monkeypatch.setattr(sys, "argv", ["eval_tsne.py", "-model=DeepSense", "-dataset=MOD", "-learn_framework=FOCAL", "-tsne_plot"])
    with pytest.raises(ValueError, match=r"matplotlib"):
        tp.parse_tsne_params()


def test_perplexity_against_the_row_count():
    from params.tsne_params import refuse_perplexity_for_rows
    refuse_perplexity_for_rows(5.0, 16, "test")
    with pytest.raises(ValueError, match=r"-tsne_perplexity=30 needs more than 16 rows.*test split.*below 16"):
        refuse_perplexity_for_rows(30.0, 16, "test")
    with pytest.raises(ValueError, match=r"16 rows"):
        refuse_perplexity_for_rows(16.0, 16, "val")


def test_flags_parse_and_default_path(monkeypatch, tmp_path):
    from params.base_params import parse_base_args
    from params.tsne_params import resolve_tsne_out
    monkeypatch.setattr(sys, "argv", ["eval_tsne.py", "-learn_framework=FOCAL"])
    a = parse_base_args("eval_tsne")
    assert (a.tsne_split, a.tsne_perplexity, a.tsne_iters, a.tsne_init, a.tsne_seed, a.tsne_max_rows, a.tsne_out, a.tsne_plot) == \
        ("test", 30.0, 1000, "pca", 0, 16384, None, False)
    monkeypatch.setattr(sys, "argv", ["eval_tsne.py", "-tsne_split=val", "-tsne_perplexity=12.5", "-tsne_iters=60", "-tsne_init=random",
                                      "-tsne_seed=3", "-tsne_max_rows=100", "-tsne_out=/x/y.npz", "-tsne_plot"])
    a = parse_base_args("eval_tsne")
    assert (a.tsne_split, a.tsne_perplexity, a.tsne_iters, a.tsne_init, a.tsne_seed, a.tsne_max_rows, a.tsne_out, a.tsne_plot) == \
        ("val", 12.5, 60, "random", 3, 100, "/x/y.npz", True)
    args = _run(tmp_path, tsne_split="val")
    assert resolve_tsne_out(args) == os.path.join(args.weight_folder, "HAR3LOC_SW_Transformer_tsne_val.npz")
    assert resolve_tsne_out(_run(tmp_path, tsne_out="/somewhere/map.npz")) == "/somewhere/map.npz"


def test_seeded_subset():
    sub = entry().subset_rows
    a, b = sub(1000, 100, 7), sub(1000, 100, 7)
    assert torch.equal(a, b) and a.dtype == torch.int64 and a.numel() == 100
    assert torch.equal(a, a.sort().values) and a.unique().numel() == 100 and int(a.min()) >= 0 and int(a.max()) < 1000
    assert not torch.equal(a, sub(1000, 100, 8))
    assert torch.equal(sub(100, 100, 7), torch.arange(100)) and torch.equal(sub(37, 16384, 0), torch.arange(37))


def test_npz_bytes_repeat(tmp_path):
    e = entry()
    arrays = {"embedding": np.arange(6, dtype=np.float32).reshape(3, 2), "labels": np.array([0, 1, 0]), "kl": np.float64(0.5)}
    e.write_npz(str(tmp_path / "a.npz"), arrays)
    e.write_npz(str(tmp_path / "b.npz"), arrays)
    assert (tmp_path / "a.npz").read_bytes() == (tmp_path / "b.npz").read_bytes()
    back = np.load(str(tmp_path / "a.npz"))
    assert np.array_equal(back["embedding"], arrays["embedding"]) and back["embedding"].dtype == np.float32 and float(back["kl"]) == 0.5


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}x{c[1]}")
def test_pca_init_is_sklearns(case):
    """Up to the documented sign (largest-magnitude loading positive: sklearn's own svd_flip rule) and scale (first column's standard
    deviation 1e-4), to 1e-6 of the column norm."""
    from sklearn.decomposition import PCA
    from train_utils.tsne import pca_init
    X, _ = blobs(*case)
    got = pca_init(torch.from_numpy(np.array(X))).numpy().astype(np.float64)
    assert got.shape == (X.shape[0], 2) and abs(got[:, 0].std() - 1e-4) <= 1e-10
    pca = PCA(n_components=2, svd_solver="full").fit(X.astype(np.float64))
    want = pca.transform(X.astype(np.float64))
    for k in range(2):
        if pca.components_[k][np.abs(pca.components_[k]).argmax()] < 0:
            want[:, k] = -want[:, k]
    want = want / want[:, 0].std() * 1e-4
    for k in range(2):
        assert np.abs(got[:, k] - want[:, k]).max() <= 1e-6 * np.linalg.norm(want[:, k]), k


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}x{c[1]}")
def test_yardstick_is_sklearns(case):
    from scipy.spatial.distance import squareform
    from sklearn.manifold._t_sne import _joint_probabilities, _kl_divergence
    from tsne_reference import squared_distances
    X, _ = blobs(*case)
    n = X.shape[0]
    P, cond, beta = joint(X, 30.0)
    assert np.array_equal(P, P.T) and not P.diagonal().any() and abs(P.sum() - 1) <= 1e-12
    H = -(np.where(cond > 0, cond * np.log(np.where(cond > 0, cond, 1)), 0)).sum(1)
    assert np.abs(np.exp(H) - 30.0).max() <= 1e-9 * 30.0  # 64 steps: far below sklearn's tolerance
    sk = squareform(_joint_probabilities(squared_distances(X).astype(np.float32), 30.0, 0))
    gap = np.abs(P - sk).max() / P.max()
    print(f"yardstick against _joint_probabilities, n = {n}: {gap:.3e} of max P")
    assert gap <= 5e-5
    r = np.random.default_rng(5)
    for scale, e in ((1e-4, 1.0), (10.0, 1.0), (1e-4, 12.0), (10.0, 12.0)):
        Y = (r.standard_normal((n, 2)) * scale).astype(np.float32).astype(np.float64)
        g, kl, _ = gradient(Y, P, e)
        sk_kl, sk_g = _kl_divergence(Y.ravel(), squareform(e * P, checks=False), 1.0, n, 2)
        assert np.abs(g - sk_g.reshape(n, 2)).max() <= 1e-12 * np.abs(sk_g).max()
        if e == 1.0:  # (sklearn's value at 12 P is not a divergence; ours is that of P at every exaggeration)
            assert abs(kl - sk_kl) <= 1e-12 * max(1.0, abs(sk_kl))


def test_plot_writes_a_png(tmp_path):
    r = np.random.default_rng(0)
    path = entry().plot_embedding(str(tmp_path / "map.png"), r.standard_normal((60, 2)), np.arange(60) % 3, class_names=["walk", "run", "sit"],
                                  title="a title")
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n" and len(data) > 1000
    entry().plot_embedding(str(tmp_path / "bare.png"), r.standard_normal((10, 2)), np.arange(10) % 12)  # no names: the class indices
    assert os.path.getsize(tmp_path / "bare.png") > 1000


def test_exports_are_declared_at_abi_14():
    from focal_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "focal_hip.h")).read()
    assert re.search(r"#define FOCAL_ABI_VERSION 14\b", hdr) and _lib.ABI_VERSION == 14
    assert re.search(r"typedef struct \{ int n, D, slices; \} focal_tsne_desc;", hdr)
    for name, count in (("focal_tsne_dist", 5), ("focal_tsne_perplexity", 5), ("focal_tsne_symmetrize_workspace", 1),
                        ("focal_tsne_symmetrize", 6), ("focal_tsne_grad_workspace", 1), ("focal_tsne_grad", 7), ("focal_tsne_step", 14)):
        m = re.search(rf"^(?:int|size_t) {name}\(([^;]*)\);", hdr, re.M)
        assert m and len(m.group(1).split(",")) == count == len(_lib.PROTOTYPES[name][1]), name
    assert [n for n, _ in _lib.TsneDesc._fields_] == ["n", "D", "slices"]
    table = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(f"`{name}`" in table for name in ("focal_tsne_dist", "focal_tsne_perplexity", "focal_tsne_symmetrize", "focal_tsne_grad",
                                                 "focal_tsne_step"))
