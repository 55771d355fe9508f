"""Host half of eval_linear.py: the flags, what is refused before anything is built, the probe exports' declarations, and lbfgs_minimize
on a float64 numpy objective against sklearn's optimum."""
import argparse
import functools
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
    spec = importlib.util.spec_from_file_location("focal_eval_linear_entry", os.path.join(SRC, "eval_linear.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _run(tmp_path, **kw):
    base = dict(dataset="HAR3LOC", model="SW_Transformer", task="activity_classification", learn_framework="FOCAL", stage="pretrain",
                label_ratio=1.0, model_weight=None, weight_folder=str(tmp_path / "weights" / "HAR3LOC_SW_Transformer"),
                probe_l2="1e-4,1e-3,1e-2,1e-1", probe_max_iter=200, probe_tol=1e-5)
    base.update(kw)
    return argparse.Namespace(**base)


# ------------------------------------------------------------------------------------------ flags
def test_probe_flags_parse(monkeypatch):
    from params.base_params import parse_base_args
    from params.linear_params import parse_probe_l2
    monkeypatch.setattr(sys, "argv", ["eval_linear.py", "-learn_framework=FOCAL"])
    a = parse_base_args("eval_linear")
    assert (a.probe_l2, a.probe_max_iter, a.probe_tol) == ("1e-4,1e-3,1e-2,1e-1", 200, 1e-5)
    assert parse_probe_l2(a.probe_l2) == (1e-4, 1e-3, 1e-2, 1e-1)
    monkeypatch.setattr(sys, "argv", ["eval_linear.py", "-learn_framework=FOCAL", "-probe_l2=0.5, 2e-3", "-probe_max_iter=20", "-probe_tol=1e-3",
                                      "-label_ratio=0.1"])
    a = parse_base_args("eval_linear")
    assert (parse_probe_l2(a.probe_l2), a.probe_max_iter, a.probe_tol, a.label_ratio) == ((0.5, 2e-3), 20, 1e-3, 0.1)
    assert len(parse_probe_l2(",".join(["1e-3"] * 16))) == 16  # the limit itself


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


@pytest.mark.parametrize("text,match", [("", "no empty entry"), ("1e-3,,1e-2", "no empty entry"), ("1e-3,", "no empty entry"),
                                        ("0", "positive and finite"), ("1e-3,-1e-2", "positive and finite"), ("nan", "positive and finite"),
                                        ("1e-3,inf", "positive and finite"), ("abc", "comma list of positive strengths"),
                                        (",".join(["1e-3"] * 17), "at most 16")],
                         ids=["empty", "empty-entry", "trailing-comma", "zero", "negative", "nan", "inf", "word", "17-values"])
def test_probe_l2_is_refused(monkeypatch, tmp_path, nothing_is_built, text, match):
    from params.linear_params import parse_linear_params
    monkeypatch.setattr(sys, "argv", ["eval_linear.py", "-model=DeepSense", "-dataset=MOD", "-learn_framework=FOCAL", f"-probe_l2={text}"])
    with pytest.raises(ValueError, match=match) as e:
        parse_linear_params()
    assert "-probe_l2" in str(e.value) and "eval_linear.py" in str(e.value)
    path = tmp_path / "MOD_DeepSense_pretrain_best.pt"
    torch.save({}, path)
    with pytest.raises(ValueError, match=match):
        entry().evaluate_linear(_run(tmp_path, model="DeepSense", dataset="MOD", probe_l2=text, backbone_weight=str(path)))


# ------------------------------------------------------------------------------------------ refusals
def test_other_frameworks_are_refused(monkeypatch, tmp_path, nothing_is_built):
    from params.linear_params import parse_linear_params
    monkeypatch.setattr(sys, "argv", ["eval_linear.py", "-model=DeepSense", "-dataset=MOD", "-learn_framework=no"])
    with pytest.raises(ValueError, match=r"eval_linear\.py scores .* test\.py -model=DeepSense -dataset=MOD -learn_framework=no"):
        parse_linear_params()
    with pytest.raises(ValueError, match=r"test\.py"):
        entry().evaluate_linear(_run(tmp_path, learn_framework="no", backbone_weight=str(tmp_path / "x.pt")))


def test_data_parallel_is_refused(monkeypatch, tmp_path, nothing_is_built):
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="one process"):
        entry().evaluate_linear(_run(tmp_path, backbone_weight=str(tmp_path / "x.pt")))
    with pytest.raises(SystemExit, match="one process"):
        entry().main_eval_linear()


def test_missing_checkpoint_is_refused(tmp_path, nothing_is_built):
    from params.knn_params import resolve_backbone_weight
    args = _run(tmp_path)
    args.backbone_weight = resolve_backbone_weight(args)
    with pytest.raises(FileNotFoundError, match=r"train\.py -model=SW_Transformer -dataset=HAR3LOC -learn_framework=FOCAL"):
        entry().evaluate_linear(args)
    assert not hasattr(args, "classifier")


@pytest.mark.parametrize("name,flags", [("MOD_DeepSense_vehicle_classification_1.0_finetune_best.pt", "-learn_framework=FOCAL -stage=finetune"),
                                        ("MOD_DeepSense_vehicle_classification_best.pt", "-learn_framework=no")])
def test_classifier_checkpoint_is_refused(tmp_path, nothing_is_built, name, flags):
    path = tmp_path / name
    torch.save({"class_layer.0.weight": torch.zeros(2, 2)}, path)
    args = _run(tmp_path, model="DeepSense", dataset="MOD", task="vehicle_classification", model_weight=str(path), backbone_weight=str(path))
    with pytest.raises(ValueError, match=re.escape(f"test.py -model=DeepSense -dataset=MOD {flags}")) as e:
        entry().evaluate_linear(args)
    assert "eval_linear.py scores what" in str(e.value) and "eval_knn.py" not in str(e.value)
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
        entry().evaluate_linear(args)
    assert args.stage == "pretrain"


def test_chosen_strength_is_the_best_validation_accuracy_ties_to_the_larger():
    choose = entry().choose_l2
    assert choose((1e-4, 1e-3, 1e-2), [0.5, 0.7, 0.6]) == 1
    assert choose((1e-4, 1e-3, 1e-2), [0.7, 0.7, 0.6]) == 1
    assert choose((1e-2, 1e-3, 1e-4), [0.7, 0.7, 0.7]) == 0
    assert choose((1e-3,), [0.0]) == 0


# ------------------------------------------------------------------------------------------ exports
def test_exports_are_declared_at_abi_14():
    from focal_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "focal_hip.h")).read()
    assert re.search(r"#define FOCAL_ABI_VERSION 14\b", hdr) and _lib.ABI_VERSION == 14
    assert re.search(r"typedef struct \{ int n, D, C, R, slices; \} focal_probe_desc;", hdr)
    assert re.search(r"int focal_probe_forward\(const focal_probe_desc\* d, const float\* x, const float\* w, const float\* b, const int\* y,\s*"
                     r"float\* ce,\s*float\* g,\s*int\* preds, void\* stream\);", hdr)
    assert re.search(r"size_t focal_probe_grad_workspace\(const focal_probe_desc\* d\);", hdr)
    assert re.search(r"int focal_probe_grad\(const focal_probe_desc\* d, const float\* x, const float\* g, const float\* ce, const float\* w,\s*"
                     r"const float\* lam,\s*float\* gw, float\* gb, double\* f, void\* ws, size_t ws_bytes, void\* stream\);", hdr)
    arity = {k: len(v[1]) for k, v in _lib.PROTOTYPES.items() if k.startswith("focal_probe_")}
    assert arity == {"focal_probe_forward": 9, "focal_probe_grad_workspace": 1, "focal_probe_grad": 12}
    assert [n for n, _ in _lib.ProbeDesc._fields_] == ["n", "D", "C", "R", "slices"]
    assert (_lib.PROBE_MAX_C, _lib.PROBE_MAX_ROWS) == (64, 1024)
    table = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in arity:
        assert f"`{name}`" in table, name


@pytest.mark.parametrize("D,C,R,match", [(34, 7, 4, "D % 4 == 0"), (0, 7, 1, "D >= 4"), (36, 1, 1, "2 <= C <= 64"), (36, 65, 1, "2 <= C <= 64"),
                                         (36, 7, 0, "R >= 1"), (36, 41, 25, "R * C <= 1024"), (36, 64, 17, "R * C <= 1024")])
def test_probe_check_limits_names_the_limit(D, C, R, match):
    from focal_amd import _lib, ops
    with pytest.raises(_lib.FocalHipError, match=re.escape(match)):
        ops.probe_check_limits(D, C, R)
    ops.probe_check_limits(4, 2, 1)     # the limits themselves
    ops.probe_check_limits(36, 64, 16)  # 1024 weight rows


# ------------------------------------------------------------------------------------------ the minimiser
def recipe(n, D, C, seed):
    """Recipe R of the probe's tests: C Gaussian classes around centres of scale 0.35, labels a permutation of arange(n) % C."""
    r = np.random.default_rng(seed)
    cen = r.standard_normal((C, D)) * 0.35
    y = r.permutation(np.arange(n) % C)
    x = (cen[y] + r.standard_normal((n, D))).astype(np.float32)
    return x, y


def objective64(x, y, C, l2):
    """evaluate(theta [R, C * D + C]) -> (F [R], gradient [R, C * D + C]) of the probe's objective in float64 numpy."""
    n, D = x.shape
    onehot = np.eye(C)[y]

    def evaluate(theta):
        f, g = [], []
        for lam, t in zip(l2, theta):
            w, b = t[:C * D].reshape(C, D), t[C * D:]
            z = x @ w.T + b
            m = z.max(1, keepdims=True)
            lse = m[:, 0] + np.log(np.exp(z - m).sum(1))
            p = np.exp(z - lse[:, None])
            f.append((lse - z[np.arange(n), y]).mean() + 0.5 * lam * (w ** 2).sum())
            d = p - onehot
            g.append(np.concatenate([(d.T @ x / n + lam * w).ravel(), d.mean(0)]))
        return np.array(f), np.stack(g)
    return evaluate


L2 = (1e-3, 1e-2, 1e-1)


@functools.lru_cache(maxsize=None)
def case():
    n, D, C = 1000, 36, 7
    x, y = recipe(n, D, C, 5)
    x = x.astype(np.float64)
    x = (x - x.mean(0)) / x.std(0)
    return x, y, D, C


@functools.lru_cache(maxsize=None)
def together():
    from train_utils.linear_probe import lbfgs_minimize
    x, y, D, C = case()
    return lbfgs_minimize(objective64(x, y, C, L2), np.zeros((len(L2), C * D + C)), max_iter=5000, tol=1e-9, history=10)


def test_lbfgs_reaches_sklearns_optimum():
    from sklearn.linear_model import LogisticRegression
    x, y, D, C = case()
    n = x.shape[0]
    res = together()
    assert res["converged"].all(), res
    for r, lam in enumerate(L2):
        sk = LogisticRegression(C=1.0 / (lam * n), tol=1e-10, max_iter=20000).fit(x, y)
        theta = np.concatenate([sk.coef_.ravel(), sk.intercept_])[None]
        f_star = objective64(x, y, C, (lam,))(theta)[0][0]
        ours = objective64(x, y, C, (lam,))(res["theta"][r][None])[0][0]
        print(f"l2={lam:g}: F* {f_star!r}, ours {ours!r}, gap {ours - f_star:.3e}, {res['n_iter'][r]} steps, {res['n_eval']} evaluations in all")
        assert ours == pytest.approx(res["f"][r], abs=1e-15)
        assert ours - f_star <= 1e-9 * max(1.0, f_star)


def test_problems_in_lock_step_take_the_iterates_each_takes_alone():
    from train_utils.linear_probe import lbfgs_minimize
    x, y, D, C = case()
    res = together()
    for r, lam in enumerate(L2):
        trace = []

        def evaluate(theta, lam=lam, trace=trace):
            trace.append(theta[0].copy())
            return objective64(x, y, C, (lam,))(theta)
        alone = lbfgs_minimize(evaluate, np.zeros((1, C * D + C)), max_iter=5000, tol=1e-9, history=10)
        assert alone["theta"][0].tobytes() == res["theta"][r].tobytes()
        assert alone["f"][0] == res["f"][r] and alone["n_iter"][0] == res["n_iter"][r]
        assert alone["n_eval"] <= res["n_eval"]
    # every trial point, not only the last: the joint run's submissions for problem r are the lone run's, then its final point repeated
    joint = [[] for _ in L2]

    def evaluate_all(theta):
        for r in range(len(L2)):
            joint[r].append(theta[r].copy())
        return objective64(x, y, C, L2)(theta)
    lbfgs_minimize(evaluate_all, np.zeros((len(L2), C * D + C)), max_iter=5000, tol=1e-9, history=10)
    for r, lam in enumerate(L2):
        lone = []

        def evaluate(theta, lam=lam, lone=lone):
            lone.append(theta[0].copy())
            return objective64(x, y, C, (lam,))(theta)
        end = lbfgs_minimize(evaluate, np.zeros((1, C * D + C)), max_iter=5000, tol=1e-9, history=10)
        assert len(lone) <= len(joint[r])
        for a, b in zip(lone, joint[r]):
            assert a.tobytes() == b.tobytes()
        for b in joint[r][len(lone):]:
            assert b.tobytes() == end["theta"][0].tobytes()


def test_a_pair_with_negative_curvature_is_skipped_and_no_decrease_stops():
    """A concave stretch (s.y <= 0) must not enter the history; an evaluation that cannot decrease ends the problem unconverged."""
    from train_utils.linear_probe import lbfgs_minimize

    def evaluate(theta):  # f = sum(cos) on [0, pi]: concave near 0, minimum at pi
        return np.cos(theta).sum(1), -np.sin(theta)
    res = lbfgs_minimize(evaluate, np.full((1, 3), 0.3), max_iter=200, tol=1e-10)
    assert res["converged"].all() and np.allclose(np.abs(res["theta"]), np.pi, atol=1e-8)

    def flat(theta):  # the gradient promises a decrease that the value never shows
        return np.zeros(theta.shape[0]), np.ones_like(theta)
    res = lbfgs_minimize(flat, np.zeros((2, 3)), max_iter=50, tol=1e-10)
    assert not res["converged"].any() and (res["n_iter"] == 0).all() and (res["theta"] == 0).all()
