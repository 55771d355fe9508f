"""Host half of eval_cluster.py: clustering_scores against sklearn, the flags, what is refused before anything is built, and the K-means
exports' declarations."""
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


def entry():
    spec = importlib.util.spec_from_file_location("focal_eval_cluster_entry", os.path.join(SRC, "eval_cluster.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _run(tmp_path, **kw):
    base = dict(dataset="HAR3LOC", model="SW_Transformer", task="activity_classification", learn_framework="FOCAL", stage="pretrain",
                label_ratio=1.0, model_weight=None, weight_folder=str(tmp_path / "weights" / "HAR3LOC_SW_Transformer"), n_clusters=None,
                cluster_n_init=10, cluster_max_iter=100, cluster_init="k-means++", cluster_seed=0)
    base.update(kw)
    return argparse.Namespace(**base)


# ------------------------------------------------------------------------------------------ scores
def _tables():
    r = np.random.default_rng(5)
    out = []
    for n_cls, n_clu, n in [(7, 7, 400), (7, 3, 400), (3, 12, 500), (10, 64, 3000), (2, 2, 9), (5, 5, 40)]:
        out.append((f"random {n_cls}x{n_clu}", r.integers(0, n_cls, n), r.integers(0, n_clu, n), n_cls, n_clu))
    y = r.integers(0, 6, 300)
    y[y == 2] = 3                                                       # an empty class row
    k = r.integers(0, 9, 300)
    k[(k == 0) | (k == 8)] = 4                                          # empty cluster columns, the first and the last
    out.append(("empty rows and columns", y, k, 6, 9))
    out.append(("one class", np.zeros(200, dtype=np.int64), r.integers(0, 5, 200), 4, 5))
    out.append(("one cluster", r.integers(0, 5, 200), np.full(200, 2), 5, 4))
    out.append(("one class, one cluster", np.full(50, 1), np.full(50, 3), 3, 5))
    y = r.integers(0, 7, 350)
    out.append(("perfect, relabelled", y, (y * 3 + 2) % 7, 7, 7))
    out.append(("each row its own cluster", np.zeros(6, dtype=np.int64), np.arange(6), 1, 6))
    out.append(("two rows", np.array([0, 1]), np.array([0, 0]), 2, 2))
    return out


@pytest.mark.parametrize("name,y,k,n_cls,n_clu", _tables(), ids=[t[0] for t in _tables()])
def test_clustering_scores_against_sklearn(name, y, k, n_cls, n_clu):
    from sklearn.metrics import adjusted_rand_score, normalized_mutual_info_score
    from train_utils.eval_functions import clustering_scores
    C = max(n_cls, n_clu)
    conf = np.zeros((C, C), dtype=np.int64)  # the square matrix ops.EvalState holds
    np.add.at(conf, (y, k), 1)
    ari, nmi = clustering_scores(conf, n_cls, n_clu)
    want = adjusted_rand_score(y, k), normalized_mutual_info_score(y, k)
    print(f"{name}: ARI {ari!r} (sklearn {want[0]!r}), NMI {nmi!r} (sklearn {want[1]!r})")
    assert isinstance(ari, float) and isinstance(nmi, float)
    assert abs(ari - want[0]) <= 1e-12 and abs(nmi - want[1]) <= 1e-12


def test_clustering_scores_degenerate_values():
    from train_utils.eval_functions import clustering_scores
    one = np.zeros((4, 4), dtype=np.int64)
    one[1, 3] = 50
    assert clustering_scores(one, 4, 4) == (1.0, 1.0)
    perfect = np.diag([5, 0, 9, 2]).astype(np.int64)
    ari, nmi = clustering_scores(perfect, 4, 4)
    assert ari == 1.0 and abs(nmi - 1.0) <= 1e-12
    one_cluster = np.zeros((3, 3), dtype=np.int64)
    one_cluster[:, 0] = [4, 5, 6]
    assert clustering_scores(one_cluster, 3, 1) == (0.0, 0.0)


# ------------------------------------------------------------------------------------------ flags
def test_cluster_flags_parse(monkeypatch):
    from params.base_params import parse_base_args
    monkeypatch.setattr(sys, "argv", ["eval_cluster.py", "-learn_framework=FOCAL"])
    a = parse_base_args("eval_cluster")
    assert (a.n_clusters, a.cluster_n_init, a.cluster_max_iter, a.cluster_init, a.cluster_seed) == (None, 10, 100, "k-means++", 0)
    monkeypatch.setattr(sys, "argv", ["eval_cluster.py", "-learn_framework=FOCAL", "-n_clusters=12", "-cluster_n_init=3", "-cluster_max_iter=20",
                                      "-cluster_init=random", "-cluster_seed=4"])
    a = parse_base_args("eval_cluster")
    assert (a.n_clusters, a.cluster_n_init, a.cluster_max_iter, a.cluster_init, a.cluster_seed) == (12, 3, 20, "random", 4)
    monkeypatch.setattr(sys, "argv", ["eval_cluster.py", "-learn_framework=FOCAL", "-cluster_init=farthest"])
    with pytest.raises(SystemExit):
        parse_base_args("eval_cluster")


def test_n_clusters_falls_back_to_num_classes():
    from params.cluster_params import resolve_n_clusters
    cfg = {"activity_classification": {"num_classes": 9}}
    assert resolve_n_clusters(argparse.Namespace(n_clusters=None, task="activity_classification", dataset_config=cfg)) == 9
    assert resolve_n_clusters(argparse.Namespace(n_clusters=4, task="activity_classification", dataset_config=cfg)) == 4
    with pytest.raises(ValueError, match=r"1 <= n_clusters <= 64"):
        resolve_n_clusters(argparse.Namespace(n_clusters=None, task="t", dataset_config={"t": {"num_classes": 70}}))


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


@pytest.mark.parametrize("n_clusters", [65, 0])
def test_cluster_count_is_refused(monkeypatch, tmp_path, nothing_is_built, n_clusters):
    from params.cluster_params import parse_cluster_params
    monkeypatch.setattr(sys, "argv", ["eval_cluster.py", "-model=DeepSense", "-dataset=MOD", "-learn_framework=FOCAL", f"-n_clusters={n_clusters}"])
    with pytest.raises(ValueError, match=r"1 <= n_clusters <= 64"):
        parse_cluster_params()
    path = tmp_path / "MOD_DeepSense_pretrain_best.pt"
    torch.save({}, path)
    with pytest.raises(ValueError, match=r"1 <= n_clusters <= 64"):
        entry().evaluate_cluster(_run(tmp_path, model="DeepSense", dataset="MOD", n_clusters=n_clusters, backbone_weight=str(path)))


# ------------------------------------------------------------------------------------------ refusals
def test_other_frameworks_are_refused(monkeypatch, tmp_path, nothing_is_built):
    from params.cluster_params import parse_cluster_params
    monkeypatch.setattr(sys, "argv", ["eval_cluster.py", "-model=DeepSense", "-dataset=MOD", "-learn_framework=no"])
    with pytest.raises(ValueError, match=r"eval_cluster\.py scores .* test\.py -model=DeepSense -dataset=MOD -learn_framework=no"):
        parse_cluster_params()
    with pytest.raises(ValueError, match=r"test\.py"):
        entry().evaluate_cluster(_run(tmp_path, learn_framework="no", backbone_weight=str(tmp_path / "x.pt")))


def test_data_parallel_is_refused(monkeypatch, tmp_path, nothing_is_built):
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="one process"):
        entry().evaluate_cluster(_run(tmp_path, backbone_weight=str(tmp_path / "x.pt")))
    with pytest.raises(SystemExit, match="one process"):
        entry().main_eval_cluster()


def test_missing_checkpoint_is_refused(tmp_path, nothing_is_built):
    from params.knn_params import resolve_backbone_weight
    args = _run(tmp_path)
    args.backbone_weight = resolve_backbone_weight(args)
    with pytest.raises(FileNotFoundError, match=r"train\.py -model=SW_Transformer -dataset=HAR3LOC -learn_framework=FOCAL"):
        entry().evaluate_cluster(args)
    assert not hasattr(args, "classifier")


@pytest.mark.parametrize("name,flags", [("MOD_DeepSense_vehicle_classification_1.0_finetune_best.pt", "-learn_framework=FOCAL -stage=finetune"),
                                        ("MOD_DeepSense_vehicle_classification_best.pt", "-learn_framework=no")])
def test_classifier_checkpoint_is_refused(tmp_path, nothing_is_built, name, flags):
    path = tmp_path / name
    torch.save({"class_layer.0.weight": torch.zeros(2, 2)}, path)
    args = _run(tmp_path, model="DeepSense", dataset="MOD", task="vehicle_classification", model_weight=str(path), backbone_weight=str(path))
    with pytest.raises(ValueError, match=re.escape(f"test.py -model=DeepSense -dataset=MOD {flags}")) as e:
        entry().evaluate_cluster(args)
    assert "eval_cluster.py scores what" in str(e.value) and "eval_knn.py" not in str(e.value)
    assert not hasattr(args, "classifier")


def test_pretraining_checkpoint_with_its_class_layer_is_taken(monkeypatch, tmp_path):
    """What pretraining saves holds the untrained class_layer.*: that file is read and the run goes on to build its loaders (where this test
    stops it)."""
    import input_utils.multi_modal_dataloader as loaders

    class Reached(Exception):
        pass

    def stop(*a, **k):
        raise Reached()
    monkeypatch.setattr(loaders, "create_dataloader", stop)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    path = tmp_path / "MOD_DeepSense_pretrain_best.pt"
    torch.save({"class_layer.0.weight": torch.zeros(2, 2), "mod_projectors.audio.0.bias": torch.zeros(4)}, path)
    args = _run(tmp_path, model="DeepSense", dataset="MOD", task="vehicle_classification", backbone_weight=str(path), batch_size=8, workers=0)
    with pytest.raises(Reached):
        entry().evaluate_cluster(args)


# ------------------------------------------------------------------------------------------ exports
def test_exports_are_declared_at_abi_14():
    from focal_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "focal_hip.h")).read()
    assert re.search(r"#define FOCAL_ABI_VERSION 14\b", hdr) and _lib.ABI_VERSION == 14
    assert re.search(r"typedef struct \{ int n, D, K, R, slices; \} focal_kmeans_desc;", hdr)
    assert re.search(r"int focal_kmeans_assign\(const focal_kmeans_desc\* d, const float\* x, const float\* c, const float\* c_sq, int\* labels,\s*"
                     r"float\* min_d2,\s*int\* changed, void\* stream\);", hdr)
    assert re.search(r"size_t focal_kmeans_update_workspace\(const focal_kmeans_desc\* d\);", hdr)
    assert re.search(r"int focal_kmeans_update\(const focal_kmeans_desc\* d, const float\* x, const int\* labels, const float\* min_d2, float\* c,\s*"
                     r"float\* c_sq,\s*int\* counts, float\* inertia, void\* ws, size_t ws_bytes, void\* stream\);", hdr)
    arity = {k: len(v[1]) for k, v in _lib.PROTOTYPES.items() if k.startswith("focal_kmeans_")}
    assert arity == {"focal_kmeans_assign": 8, "focal_kmeans_update_workspace": 1, "focal_kmeans_update": 11}
    assert [n for n, _ in _lib.KMeansDesc._fields_] == ["n", "D", "K", "R", "slices"]
    assert (_lib.KMEANS_MAX_K, _lib.KMEANS_MAX_CENTROIDS) == (64, 1024)


@pytest.mark.parametrize("D,K,R,match", [(34, 7, 10, "D % 4 == 0"), (0, 7, 1, "D >= 4"), (36, 0, 1, "1 <= K <= 64"), (36, 65, 1, "1 <= K <= 64"),
                                         (36, 7, 0, "R >= 1"), (36, 41, 25, "R * K <= 1024"), (36, 64, 17, "R * K <= 1024")])
def test_kmeans_check_limits_names_the_limit(D, K, R, match):
    from focal_amd import _lib, ops
    with pytest.raises(_lib.FocalHipError, match=re.escape(match)):
        ops.kmeans_check_limits(D, K, R)
    ops.kmeans_check_limits(36, 64, 16)  # 1024 centroids: the limit itself
    ops.kmeans_check_limits(4, 1, 1)
