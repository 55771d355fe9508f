#!/usr/bin/env python3
"""DeepSense with EVEN convolution lengths: the parity fixture of the config capability (tests/test_deepsense_evenk_*.py).

The config is the reference's own MOD.yaml with only the filter lengths changed, in memory:

    loc_mod_conv_lens: {audio: [[1, 80], [1, 4], [1, 4]], seismic: [[1, 4], [1, 4], [1, 4]]}

i.e. every 'same' convolution of the model has an even length, which torch pads asymmetrically (k - 1 zeros in all, (k - 1) // 2 on the
left, the rest on the right).  Run where the reference is importable (gen_golden.py: REF), never on the GPU box:

    python tests/golden/gen_golden_deepsense_evenk.py        ->  tests/golden/DeepSense_evenk_b8.npz

Stored (B = 8, name-seeded weights of oracle/weights.py, synthetic_freq_input seeds 101 / 202, dropout off), from the REFERENCE model:
  train.*    what DeepSense_b8.npz holds for a FOCAL training step: embeddings of both views, the five loss terms, the names, norms and
             strided slices of every parameter gradient, the BatchNorm running buffers after the step;
  adamw.*    the loss of three AdamW steps on that batch and a probe of one weight after them;
  settled.*  eval mode on running statistics the reference settled by itself (40 train-mode passes, as gen_golden_deepsense_settled.py):
             the buffers, and the embeddings / un-projected features of the held-out batch.
The oracle (oracle/deepsense.py, oracle/step.py) is checked against the reference on all of it before anything is written (< 2e-5 of scale
on every embedding)."""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G  # noqa: E402  (install_reference, ref_args, no_dropout, sub)

EVEN_LENS = {"audio": [[1, 80], [1, 4], [1, 4]], "seismic": [[1, 4], [1, 4], [1, 4]]}


def even_lens(cfg):
    cfg = copy.deepcopy(cfg)
    cfg["DeepSense"]["loc_mod_conv_lens"] = copy.deepcopy(EVEN_LENS)
    return cfg


def scale_err(a, ref):
    return ((a - ref).abs().max() / ref.abs().max()).item()


def main():
    G.install_reference()
    import yaml
    from oracle import weights as ow
    from oracle.config import load_config
    from oracle.deepsense import deepsense_forward
    from oracle.step import OracleTrainer
    from models.DeepSense import DeepSense
    from models.FOCALModules import FOCAL
    from models.loss import FOCALLoss
    from general_utils.weight_utils import freeze_patch_embedding

    torch.manual_seed(0)
    cfg = even_lens(G.no_dropout(yaml.safe_load(open(os.path.join(G.REF, "data", "MOD.yaml")))))
    my_cfg = even_lens(G.no_dropout(load_config()))
    args = G.ref_args("DeepSense", cfg)
    B = 8
    x1 = ow.synthetic_freq_input(my_cfg, B, seed=101)
    x2 = ow.synthetic_freq_input(my_cfg, B, seed=202)
    fix = {}

    net = DeepSense(args)
    ow.fill_state_dict_(net.state_dict())
    state0 = {k: v.clone() for k, v in net.state_dict().items()}
    spec = ow.deepsense_state_spec(my_cfg)
    assert list(spec.keys()) == list(state0.keys()), "oracle key list differs from the reference"
    for k, v in state0.items():
        assert tuple(v.shape) == tuple(spec[k]), (k, tuple(v.shape), spec[k])

    # ---------------------------------------------------------------- train mode: FOCAL(view 1, view 2) -> loss -> backward
    net.train()
    focal = freeze_patch_embedding(args, FOCAL(args, net))
    loss_fn = FOCALLoss(args)
    f1, f2 = focal(x1, x2, proj_head=True)
    loss = loss_fn(f1, f2)
    loss.backward()
    tr = OracleTrainer("DeepSense", my_cfg, state0)
    terms, o1, o2, grads = tr.loss_and_grads(x1, x2)
    assert abs(float(terms["total"]) - float(loss)) < 1e-4 * max(1.0, abs(float(loss))), (float(terms["total"]), float(loss))
    worst = 0.0
    for m in f1:
        e1, e2 = scale_err(o1[m], f1[m].detach()), scale_err(o2[m], f2[m].detach())
        assert max(e1, e2) < 2e-5, (m, "train", e1, e2)
        worst = max(worst, e1, e2)
        fix[f"train.emb1.{m}"] = f1[m].detach().numpy()
        fix[f"train.emb2.{m}"] = f2[m].detach().numpy()
    for k in ("shared", "private", "orth", "rank", "total"):
        fix[f"train.loss.{k}"] = np.array(float(terms[k]))
    fix["train.loss.reference_total"] = np.array(float(loss))
    names, norms = [], []
    for k, p in net.named_parameters():
        if p.grad is None:
            continue
        assert k in grads, f"reference has a gradient for {k} that the oracle treats as dead"
        gerr = (p.grad - grads[k]).norm().item()
        assert gerr < 5e-4 * p.grad.norm().item() + 1e-5, (k, gerr, p.grad.norm().item())
        names.append(k)
        norms.append(p.grad.double().norm().item())
        fix[f"train.gradslice.{k}"] = G.sub(p.grad, 16)
    dead = [k for k, p in net.named_parameters() if p.grad is None]
    assert sorted(dead) == sorted(k for k, _ in net.named_parameters() if k not in tr.train_keys), "dead-param set differs"
    fix["train.grad_names"] = np.array(names)
    fix["train.grad_norms"] = np.array(norms)
    for k, v in net.state_dict().items():
        if k.endswith(("running_mean", "running_var")) and k.startswith("loc_mod_extractors"):
            assert (v - tr.P[k]).abs().max().item() < 1e-5 * max(1.0, v.abs().max().item()), k
            fix[f"train.buf.{k}"] = v.numpy()

    # ---------------------------------------------------------------- three AdamW steps on the fixed batch
    net2 = DeepSense(args)
    net2.load_state_dict(state0)
    net2.train()
    focal2 = FOCAL(args, net2)
    oc = cfg["FOCAL"]["pretrain_optimizer"]
    opt = torch.optim.AdamW(focal2.parameters(), lr=oc["start_lr"], weight_decay=oc["weight_decay"])
    focal2 = freeze_patch_embedding(args, focal2)
    tr2 = OracleTrainer("DeepSense", my_cfg, state0)
    traj = []
    for it in range(3):
        opt.zero_grad()
        a, b = focal2(x1, x2, proj_head=True)
        l = loss_fn(a, b)
        l.backward()
        opt.step()
        mine = tr2.step(freq_pair=(x1, x2))
        assert abs(mine["total"] - float(l)) < 2e-3 * max(1.0, abs(float(l))), (it, mine["total"], float(l))
        traj.append(float(l))
    fix["adamw.loss_traj"] = np.array(traj)
    fix["adamw.probe_after3"] = G.sub(dict(net2.named_parameters())["mod_projectors.audio.2.weight"], 32)

    # ---------------------------------------------------------------- eval mode on statistics the reference settled by itself
    net3 = DeepSense(args)
    net3.load_state_dict(state0)
    net3.train()
    with torch.no_grad():
        for it in range(40):
            net3(ow.synthetic_freq_input(my_cfg, B, seed=5000 + it), class_head=False, proj_head=True)
    net3.eval()
    with torch.no_grad():
        emb = net3(x1, class_head=False, proj_head=True)
        feat = net3(x1, class_head=False, proj_head=False)
    state = {k: v.detach().clone() for k, v in net3.state_dict().items()}
    o_emb = deepsense_forward(state, my_cfg, x1, proj_head=True, train=False)
    o_feat = deepsense_forward(state, my_cfg, x1, proj_head=False, train=False)
    for m in emb:
        e, f = scale_err(o_emb[m], emb[m]), scale_err(o_feat[m], feat[m])
        assert e < 2e-5 and f < 2e-5, (m, "settled eval", e, f)
        worst = max(worst, e, f)
        fix[f"settled.eval.emb.{m}"] = emb[m].numpy()
        fix[f"settled.eval.feat.{m}"] = feat[m].numpy()
    for k, v in state.items():
        if k.endswith(("running_mean", "running_var", "num_batches_tracked")):
            fix[f"settled.buffer.{k}"] = v.numpy()
    fix["oracle_err"] = np.float64(worst)

    out = os.path.join(HERE, "DeepSense_evenk_b8.npz")
    np.savez_compressed(out, **fix)
    size, cap = os.path.getsize(out), os.path.getsize(os.path.join(HERE, "DeepSense_b8.npz"))
    assert size <= cap, (size, cap)
    print(f"wrote DeepSense_evenk_b8.npz: {size} bytes (DeepSense_b8.npz: {cap}), loss {float(loss):.6f}, traj {traj}, "
          f"oracle within {worst:.2e} of the reference")


if __name__ == "__main__":
    main()
