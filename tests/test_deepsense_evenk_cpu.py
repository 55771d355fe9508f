"""DeepSense with even convolution lengths, on the host: the oracle reproduces the reference fixture tests/golden/DeepSense_evenk_b8.npz
(gen_golden_deepsense_evenk.py) and the fixture's gradients are exactly the parameters the HIP model trains."""
import copy
import os

import numpy as np
import pytest
import torch

from conftest import make_args, no_dropout

GOLD = os.path.join(os.path.dirname(__file__), "golden")
EVEN_LENS = {"audio": [[1, 80], [1, 4], [1, 4]], "seismic": [[1, 4], [1, 4], [1, 4]]}


@pytest.fixture(scope="module")
def ecfg(cfg):
    c = no_dropout(cfg)
    c["DeepSense"]["loc_mod_conv_lens"] = copy.deepcopy(EVEN_LENS)
    return c


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLD, "DeepSense_evenk_b8.npz"))


def _state(cfg):
    from oracle import weights as ow
    st = {}
    for k, shp in ow.deepsense_state_spec(cfg).items():
        st[k] = torch.zeros(shp, dtype=torch.long) if k.endswith("num_batches_tracked") else ow.seeded_values(k, shp)
    return st


def scale_err(a, ref):
    return ((a - ref).abs().max() / ref.abs().max()).item()


def test_oracle_reproduces_the_even_length_fixture(ecfg, fx):
    from oracle import weights as ow
    from oracle.deepsense import deepsense_forward
    from oracle.step import OracleTrainer
    st = _state(ecfg)
    assert st["loc_mod_extractors.shake.seismic.conv_layer_in.conv.weight"].shape[-1] == 4
    assert st["loc_mod_extractors.shake.audio.conv_layers_inter.0.conv.weight"].shape[-1] == 4
    x1, x2 = ow.synthetic_freq_input(ecfg, 8, seed=101), ow.synthetic_freq_input(ecfg, 8, seed=202)
    tr = OracleTrainer("DeepSense", ecfg, st)
    terms, f1, f2, grads = tr.loss_and_grads(x1, x2)
    for m in f1:
        assert scale_err(f1[m].detach(), torch.from_numpy(fx[f"train.emb1.{m}"])) < 2e-5, m
        assert scale_err(f2[m].detach(), torch.from_numpy(fx[f"train.emb2.{m}"])) < 2e-5, m
    for k in ("shared", "private", "orth", "rank", "total"):
        ref = float(fx[f"train.loss.{k}"])
        assert abs(float(terms[k]) - ref) < 2e-5 * max(1.0, abs(ref)), k
    for n, ref in zip(fx["train.grad_names"], fx["train.grad_norms"]):
        got = grads[str(n)].double().norm().item()
        assert abs(got - ref) < 5e-4 * ref + 1e-5, (n, got, ref)
    for k in fx.files:
        if k.startswith("train.buf."):
            name = k[len("train.buf."):]
            assert (tr.P[name] - torch.from_numpy(fx[k])).abs().max().item() < 1e-5 * max(1.0, float(np.abs(fx[k]).max())), name
    # eval mode on the statistics the reference settled by itself
    for k in fx.files:
        if k.startswith("settled.buffer."):
            st[k[len("settled.buffer."):]] = torch.from_numpy(fx[k])
    with torch.no_grad():
        emb = deepsense_forward(st, ecfg, x1, proj_head=True, train=False)
        feat = deepsense_forward(st, ecfg, x1, proj_head=False, train=False)
    for m in emb:
        assert scale_err(emb[m], torch.from_numpy(fx[f"settled.eval.emb.{m}"])) < 2e-5, m
        assert scale_err(feat[m], torch.from_numpy(fx[f"settled.eval.feat.{m}"])) < 2e-5, m


def test_fixture_gradients_are_the_models_hot_set(ecfg, fx):
    from focal_amd.arena import layout
    from models.DeepSense import DeepSense
    net = DeepSense(make_args(ecfg, "DeepSense", torch.device("cpu"), "fp32"))
    index, _ = layout(net, net._hot)
    assert set(index) == {str(n) for n in fx["train.grad_names"]}
    params = dict(net.named_parameters())
    for n in index:
        assert fx[f"train.gradslice.{n}"].shape == (min(16, params[n].numel()),), n
    for mods in net.geometry.values():
        for mod, g in mods.items():
            assert g["k"] == 4 and g["k_in"] == EVEN_LENS[mod][0][1], (mod, g)
            assert g["pad_in"] == (0 if mod == "audio" else 1), (mod, g)
