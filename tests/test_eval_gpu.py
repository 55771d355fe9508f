"""Evaluation on the device: the focal_eval_accumulate kernel (loss and confusion matrix of a batch, no host read), the evaluation
loop built on it (train_utils/eval_functions.py) against the reference's numbers, and the test.py entry point end to end."""
import copy
import importlib.util
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from sklearn.metrics import accuracy_score, confusion_matrix, f1_score

from conftest import make_args, no_dropout

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SRC = os.path.join(ROOT, "focal_amd", "src")
GOLD = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from focal_amd import ops as o
    return o


def batch(B, C, seed):
    """Seeded logits with ties (the row maximum copied into a later column in every third row) and labels."""
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(B, C, generator=g)
    for b in range(0, B, 3):
        first = int(logits[b].argmax())
        if first < C - 1:
            logits[b, first + 1 + (b % (C - 1 - first))] = logits[b, first]
    return logits, torch.randint(0, C, (B,), generator=g)


def new_state(C):
    return torch.zeros(2, dtype=torch.float64, device=DEV), torch.zeros(C * C + 1, dtype=torch.int32, device=DEV)


def sk_conf(labels, preds, C):
    return confusion_matrix(labels.numpy(), preds.numpy(), labels=list(range(C)))


# ------------------------------------------------------------------------------------------ 1-5: the kernel
@pytest.mark.parametrize("B,C", [(1, 2), (5, 7), (256, 7), (257, 7), (64, 64)])
def test_one_batch_logits_mode(ops, B, C):
    logits, labels = batch(B, C, seed=900 + B + C)
    assert (logits == logits.max(1, keepdim=True).values).sum(1).max() >= (2 if B > 1 else 1)  # there are ties
    acc, conf = new_state(C)
    preds_out = torch.full((B,), -7, dtype=torch.int64, device=DEV)
    ops.eval_accumulate(acc, conf, labels.to(DEV), logits=logits.to(DEV), preds_out=preds_out)
    loss = ops.cross_entropy(logits.to(DEV), labels.to(DEV))[0]
    acc, conf = acc.cpu(), conf.cpu()
    assert acc[0].item() == float(loss[0]), (acc[0].item(), float(loss[0]))  # bit-identical to focal_cross_entropy
    assert acc[1].item() == 1
    expect = torch.argmax(logits, dim=1)
    assert torch.equal(preds_out.cpu(), expect)
    assert np.array_equal(conf[:C * C].numpy().reshape(C, C), sk_conf(labels, expect, C))
    assert conf[C * C].item() == 0


def test_several_batches_into_one_state(ops):
    C, sizes = 7, (5, 256, 257, 1)
    state = ops.EvalState(C, DEV)
    losses, all_labels, all_preds = [], [], []
    for i, B in enumerate(sizes):
        logits, labels = batch(B, C, seed=930 + i)
        state.add(labels.to(DEV), logits=logits.to(DEV))
        losses.append(float(ops.cross_entropy(logits.to(DEV), labels.to(DEV))[0][0]))
        all_labels.append(labels)
        all_preds.append(torch.argmax(logits, dim=1))
    loss_sum, n_batches, conf = state.read()
    total = 0.0
    for v in losses:
        total += v  # fp64 adds of fp32 values, in launch order
    assert loss_sum == total and n_batches == 4
    assert conf.dtype == np.int64 and conf.shape == (C, C) and conf.sum() == 519
    assert np.array_equal(conf, sk_conf(torch.cat(all_labels), torch.cat(all_preds), C))


def test_strided_inputs_are_copied(ops):
    """labels / logits / preds may be views; the caller-owned accumulators may not."""
    from focal_amd._lib import FocalHipError
    B, C = 6, 5
    logits, labels = batch(B, C, seed=945)
    wide = torch.zeros(B, 2 * C)
    wide[:, ::2] = logits
    acc, conf = new_state(C)
    ops.eval_accumulate(acc, conf, labels.to(DEV), logits=wide.to(DEV)[:, ::2])
    assert acc.cpu()[0].item() == float(ops.cross_entropy(logits.to(DEV), labels.to(DEV))[0][0])
    assert np.array_equal(conf.cpu()[:C * C].numpy().reshape(C, C), sk_conf(labels, torch.argmax(logits, dim=1), C))
    with pytest.raises(FocalHipError):
        ops.eval_accumulate(acc, torch.zeros(2 * (C * C + 1), dtype=torch.int32, device=DEV)[::2], labels.to(DEV), logits=logits.to(DEV))


def test_prediction_mode(ops):
    B, C = 37, 4
    g = torch.Generator().manual_seed(940)
    labels, preds = torch.randint(0, C, (B,), generator=g), torch.randint(0, C, (B,), generator=g)
    acc, conf = new_state(C)
    ops.eval_accumulate(acc, conf, labels.to(DEV), preds=preds.to(DEV))
    assert acc.cpu().tolist() == [0.0, 0.0]
    conf = conf.cpu()
    assert np.array_equal(conf[:C * C].numpy().reshape(C, C), sk_conf(labels, preds, C)) and conf[C * C].item() == 0


def test_rejected_rows_touch_nothing_else(ops):
    """A guard that must hold: a label outside [0, C) is counted in the last word and nowhere else."""
    B, C = 9, 3
    logits, labels = batch(B, C, seed=950)
    labels[2], labels[6] = C, -1
    good = torch.tensor([b not in (2, 6) for b in range(B)])
    acc_big = torch.full((6,), -12345.0, dtype=torch.float64, device=DEV)
    conf_big = torch.full((C * C + 1 + 8,), -999, dtype=torch.int32, device=DEV)
    preds_big = torch.full((B + 8,), -77, dtype=torch.int64, device=DEV)
    acc, conf, preds_out = acc_big[2:4], conf_big[4:4 + C * C + 1], preds_big[4:4 + B]
    acc.zero_()
    conf.zero_()
    ops.eval_accumulate(acc, conf, labels.to(DEV), logits=logits.to(DEV), preds_out=preds_out)
    torch.cuda.synchronize()
    acc_big, conf_big, preds_big = acc_big.cpu(), conf_big.cpu(), preds_big.cpu()
    assert (acc_big[:2] == -12345.0).all() and (acc_big[4:] == -12345.0).all()
    assert (conf_big[:4] == -999).all() and (conf_big[4 + C * C + 1:] == -999).all()
    assert (preds_big[:4] == -77).all() and (preds_big[4 + B:] == -77).all()
    conf = conf_big[4:4 + C * C + 1]
    assert conf[C * C].item() == 2
    expect = torch.argmax(logits, dim=1)
    assert torch.equal(preds_big[4:4 + B], expect)
    assert np.array_equal(conf[:C * C].numpy().reshape(C, C), sk_conf(labels[good], expect[good], C))
    assert acc_big[3].item() == 1 and np.isfinite(acc_big[2].item())
    # a prediction outside [0, C) is rejected in the same way
    preds = expect.clone()
    preds[0] = C
    acc2, conf2 = new_state(C)
    ops.eval_accumulate(acc2, conf2, labels.clamp(0, C - 1).to(DEV), preds=preds.to(DEV))
    conf2 = conf2.cpu()
    assert conf2[C * C].item() == 1 and conf2[:C * C].sum().item() == B - 1
    state = ops.EvalState(C, DEV)
    state.add(labels.to(DEV), logits=logits.to(DEV))
    with pytest.raises(ValueError, match="outside"):
        state.read()


def test_limits(ops):
    from focal_amd._lib import FocalHipError
    logits, labels = batch(4, 65, seed=960)
    acc, conf = new_state(65)
    with pytest.raises(FocalHipError):
        ops.eval_accumulate(acc, conf, labels.to(DEV), logits=logits.to(DEV))
    logits, labels = batch(4, 3, seed=961)
    acc, conf = new_state(3)
    with pytest.raises(FocalHipError):
        ops.eval_accumulate(acc, conf, labels.to(DEV), logits=logits.to(DEV), preds=labels.to(DEV))
    with pytest.raises(FocalHipError):
        ops.eval_accumulate(acc, conf, labels.to(DEV))
    torch.cuda.synchronize()
    assert acc.cpu().tolist() == [0.0, 0.0] and conf.cpu().sum().item() == 0  # a refused call launches nothing


# ------------------------------------------------------------------------------------------ 6-7: the evaluation loop
class PassThroughAugmenter:
    """The loader already yields what the classifier takes."""

    def forward(self, option, inputs, labels=None):
        assert option == "no"
        return inputs if labels is None else (inputs, labels)


class Recording:
    """The classifier, keeping the logits it returned."""

    def __init__(self, net):
        self.net, self.logits = net, []

    def eval(self):
        self.net.eval()
        return self

    def __call__(self, x):
        self.logits.append(self.net(x))
        return self.logits[-1]


def build(cfg, model, ct):  # (as tests/test_finetune_gpu.py builds it)
    from oracle.weights import fill_state_dict_
    args = make_args(no_dropout(cfg), model, torch.device("cuda"), ct)
    args.stage = "finetune"
    if model == "SW_Transformer":
        from models.SW_Transformer import SW_Transformer as Net
    else:
        from models.DeepSense import DeepSense as Net
    net = Net(args)
    fill_state_dict_(net.state_dict())
    return args, net.to("cuda")


def host_triple(labels, preds):
    return accuracy_score(labels, preds), f1_score(labels, preds, average="macro", zero_division=1), confusion_matrix(labels, preds)


def same_triple(got, want):
    return got[0] == want[0] and got[1] == want[1] and got[2].shape == want[2].shape and np.array_equal(got[2], want[2])


@pytest.mark.parametrize("model", ["SW_Transformer", "DeepSense"])
@pytest.mark.parametrize("ct", ["fp32", "bf16"])
def test_eval_supervised_model_against_the_reference_fixture(cfg, model, ct):
    from models.loss import CrossEntropyLoss
    from oracle.weights import synthetic_freq_input
    from train_utils.eval_functions import eval_supervised_model
    fx = np.load(os.path.join(GOLD, f"finetune_{model}_b8.npz"))
    args, net = build(cfg, model, ct)
    x = synthetic_freq_input(cfg, 8, seed=303)
    labels, ref = torch.from_numpy(fx["labels"]), torch.from_numpy(fx["eval.logits"])
    cuts = [(0, 3), (3, 6), (6, 8)]  # a ragged last batch
    loader = [({l: {m: v[a:b].cuda() for m, v in mm.items()} for l, mm in x.items()}, labels[a:b].cuda()) for a, b in cuts]
    clf = Recording(net)
    loss, triple = eval_supervised_model(args, clf, PassThroughAugmenter(), loader, CrossEntropyLoss())
    tol = 1e-3 if ct == "fp32" else 3e-2
    want_loss = float(np.mean([F.cross_entropy(ref[a:b], labels[a:b]).item() for a, b in cuts]))
    print(f"{model} {ct}: loss {loss:.7f} fixture {want_loss:.7f}")
    assert abs(loss - want_loss) < tol * max(1.0, want_loss)
    own = torch.cat([t.float().cpu() for t in clf.logits])
    top2 = ref.topk(2, dim=1).values
    sure = (top2[:, 0] - top2[:, 1]) > 2 * tol * ref.abs().max()
    assert (~sure).sum().item() <= 2
    assert (~sure).sum().item() == (0 if ct == "fp32" else 2)
    assert torch.equal(own.argmax(1)[sure], ref.argmax(1)[sure])
    if ct == "fp32":
        assert same_triple(triple, host_triple(labels.numpy(), ref.argmax(1).numpy()))
    assert same_triple(triple, host_triple(labels.numpy(), own.argmax(1).numpy()))


class FixedLogits:
    def __init__(self, logits):
        self.logits = logits

    def eval(self):
        return self

    def __call__(self, x):
        return self.logits


def test_host_reads_do_not_scale_with_batches(cfg, monkeypatch):
    from models.loss import CrossEntropyLoss
    from train_utils.eval_functions import eval_supervised_model
    args = make_args(cfg, "DeepSense", torch.device("cuda"))
    logits, labels = batch(16, 7, seed=970)
    logits, labels = logits.to(DEV), labels.to(DEV)
    reads = {"n": 0}

    def counted(name):
        orig = getattr(torch.Tensor, name)

        def wrapper(self, *a, **k):
            reads["n"] += 1
            return orig(self, *a, **k)
        monkeypatch.setattr(torch.Tensor, name, wrapper)

    for name in ("item", "cpu", "numpy", "tolist"):
        counted(name)
    counts, results = [], []
    for n_batches in (2, 5):
        reads["n"] = 0
        results.append(eval_supervised_model(args, FixedLogits(logits), PassThroughAugmenter(), [(None, labels)] * n_batches, CrossEntropyLoss()))
        counts.append(reads["n"])
    print(f"host reads: {counts[0]} for 2 batches, {counts[1]} for 5 batches")
    assert counts[0] == counts[1], counts
    assert results[0][0] == results[1][0] and results[0][1][0] == results[1][1][0]  # the same batch again: same mean loss, same accuracy
    assert results[0][1][2].sum() == 32 and results[1][1][2].sum() == 80


def test_another_loss_is_refused(cfg):
    """The loop accumulates the project's cross-entropy; a loss with other semantics is not scored as if it were that one."""
    from train_utils.eval_functions import eval_supervised_model
    logits, labels = batch(4, 7, seed=975)
    with pytest.raises(TypeError, match="CrossEntropyLoss"):
        eval_supervised_model(make_args(cfg, "DeepSense", torch.device("cuda")), FixedLogits(logits.to(DEV)), PassThroughAugmenter(),
                              [(None, labels.to(DEV))], torch.nn.CrossEntropyLoss(label_smoothing=0.1))


def test_empty_loader_is_refused(cfg):
    from models.loss import CrossEntropyLoss
    from train_utils.eval_functions import eval_supervised_model
    with pytest.raises(ValueError, match="no batch"):
        eval_supervised_model(make_args(cfg, "DeepSense", torch.device("cuda")), FixedLogits(None), PassThroughAugmenter(), [], CrossEntropyLoss())


def test_eval_pretrained_model_takes_metrics_from_the_device_matrix(cfg, monkeypatch):
    """The KNN path of pretraining validation: predictions and labels through prediction mode, the per-batch losses read once.
    The encoder, the loss and the estimator are stubs; the numbers are held to the label / prediction form on the host."""
    from train_utils import eval_functions as ef
    args = make_args(cfg, "DeepSense", torch.device("cuda"))
    g = torch.Generator().manual_seed(980)
    sizes = (8, 8, 4)
    labels = [torch.randint(0, 7, (n,), generator=g) for n in sizes]
    onehot = [F.one_hot(y, 7).float() for y in labels]  # the file-backed loaders yield one-hot labels
    preds = torch.randint(0, 7, (sum(sizes),), generator=g)
    losses = [torch.rand((), generator=g).to(DEV) for _ in sizes]
    it = iter(losses)
    monkeypatch.setattr(ef, "calc_pretrain_loss", lambda *a: next(it))
    monkeypatch.setattr(ef, "extract_sample_features", lambda a, backbone, x: torch.zeros(len(x), 4, device=DEV))

    class Model:
        backbone = None

        def eval(self):
            return self

    class Estimator:
        def predict(self, feats):
            assert feats.shape == (sum(sizes), 4)
            return preds.to(DEV)

    loader = [(torch.zeros(n, 1), y) for n, y in zip(sizes, onehot)]
    loss, triple = ef.eval_pretrained_model(args, Model(), Estimator(), PassThroughAugmenter(), loader, None)
    assert loss == float(np.mean([v.item() for v in losses]))
    assert same_triple(triple, ef.eval_task_metrics(args, torch.cat(labels).numpy(), preds.numpy()))


# ------------------------------------------------------------------------------------------ 8: test.py
def entry():
    spec = importlib.util.spec_from_file_location("focal_test_entry", os.path.join(SRC, "test.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def parsed(monkeypatch, argv):
    from params.test_params import parse_test_params
    monkeypatch.setattr(sys, "argv", ["test.py"] + argv)
    return parse_test_params()


def write_seeded_checkpoint(args):
    """Name-seeded weights under the name the training loop would use; returns nothing the evaluation could reuse."""
    from oracle.weights import fill_state_dict_
    from train_utils.model_selection import init_backbone_model
    net = init_backbone_model(copy.copy(args))
    state = fill_state_dict_({k: v.detach().cpu().clone() for k, v in net.state_dict().items()})
    assert any(k.startswith("class_layer.") for k in state)
    torch.save(state, args.classifier_weight)


def parse_report(text):
    m = re.search(r"Test classifier loss:\s*([-\d.]+)\nTest acc:\s*([-\d.]+), test f1:\s*([-\d.]+)\nTest confusion matrix:\n(.*)", text, re.S)
    assert m, text[-2000:]
    return float(m.group(1)), float(m.group(2)), float(m.group(3)), [int(v) for v in re.findall(r"\d+", m.group(4))]


@pytest.mark.parametrize("model,flags,name", [
    ("DeepSense", ["-learn_framework=no"], "MOD_DeepSense_vehicle_classification_best.pt"),
    ("SW_Transformer", ["-learn_framework=FOCAL", "-stage=finetune"], "MOD_SW_Transformer_vehicle_classification_1.0_finetune_best.pt")])
def test_test_py_end_to_end(monkeypatch, tmp_path, capsys, model, flags, name):
    from input_utils.multi_modal_dataloader import create_dataloader
    argv = [f"-model={model}", "-dataset=MOD"] + flags + [f"-model_weight={tmp_path}", "-batch_size=8"]
    args = parsed(monkeypatch, argv)
    assert args.classifier_weight == os.path.join(str(tmp_path), name)
    write_seeded_checkpoint(args)
    # the logits the evaluation saw, kept on the device as the model returns them (a second forward would not do: SW_Transformer's
    # bf16 logits are not bit-repeatable from one forward to the next -- profiles/eval_on_device.txt)
    import train_utils.model_selection as selection
    seen, build_model = [], selection.init_backbone_model

    def recording_model(a):
        net = build_model(a)
        net.register_forward_hook(lambda module, inputs, out: seen.append(out.detach().clone()))
        return net
    monkeypatch.setattr(selection, "init_backbone_model", recording_model)
    capsys.readouterr()
    loss, acc, f1 = entry().test(args)
    printed = parse_report(capsys.readouterr().out)
    # what was scored is the checkpoint, head included: models initialise unseeded, so a load that was skipped, pointed at another file
    # or made without the class layer leaves tensors that differ from the file
    saved = torch.load(args.classifier_weight, map_location="cpu")
    loaded = {k: v.detach().cpu() for k, v in args.classifier.state_dict().items()}
    assert set(loaded) == set(saved) and any(k.startswith("class_layer.") for k in saved)
    for k, v in saved.items():
        assert loaded[k].dtype == v.dtype and torch.equal(loaded[k], v), k
    # the host's recomputation: the same model and weights, the same synthetic test loader, logits to the CPU
    losses, labels, preds = [], [], []
    batches = list(create_dataloader("test", args, batch_size=args.batch_size, workers=args.workers))
    assert len(batches) == len(seen) >= 1
    for (_, y), logits in zip(batches, seen):
        logits = logits.float().cpu()
        assert logits.shape == (8, 7)
        losses.append(F.cross_entropy(logits.double(), y).item())
        labels.append(y.numpy())
        preds.append(logits.argmax(1).numpy())
    want_loss = float(np.mean(losses))
    want = host_triple(np.concatenate(labels), np.concatenate(preds))
    print(f"{model}: loss {loss:.9f} host {want_loss:.9f}")
    assert abs(loss - want_loss) / abs(want_loss) < 1e-6  # (the bound test_gru_gpu.py::test_cross_entropy holds focal_cross_entropy to)
    assert acc == want[0] and f1 == want[1]
    assert printed[3] == want[2].ravel().tolist()
    assert abs(printed[0] - loss) <= 5.1e-6 and abs(printed[1] - acc) <= 5.1e-6 and abs(printed[2] - f1) <= 5.1e-6  # five decimals
    if model == "DeepSense":  # the same command as a fresh process
        r = subprocess.run([sys.executable, os.path.join(SRC, "test.py")] + argv, capture_output=True, text=True, timeout=300, cwd=SRC)
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
        assert parse_report(r.stdout) == printed


def test_test_py_refusals(monkeypatch, tmp_path):
    with pytest.raises(ValueError, match="-stage=finetune"):
        parsed(monkeypatch, ["-model=SW_Transformer", "-dataset=MOD", "-learn_framework=FOCAL", f"-model_weight={tmp_path}"])
    mod = entry()
    args = parsed(monkeypatch, ["-model=DeepSense", "-dataset=MOD", "-learn_framework=no", f"-model_weight={tmp_path}"])
    with pytest.raises(FileNotFoundError, match="train.py -model=DeepSense"):
        mod.test(args)
    assert not hasattr(args, "classifier")  # refused before a model was built
    # a checkpoint without class-layer tensors (what pretraining writes) would leave the head at its random initialisation
    torch.save({"mod_projectors.audio.0.bias": torch.zeros(4)}, args.classifier_weight)
    with pytest.raises(ValueError, match="class_layer"):
        mod.test(args)
    assert not hasattr(args, "classifier")
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit):
        mod.test(args)
