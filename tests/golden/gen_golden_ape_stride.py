#!/usr/bin/env python3
"""Generate the parity fixtures of SW_Transformer's `APE` and `in_stride` switches by IMPORTING THE REFERENCE in the build container.

Run here only (needs the reference checkout; never on the GPU box):   python tests/golden/gen_golden_ape_stride.py

Uses gen_golden.py's stand-ins for the third-party packages (nothing from the reference is copied).  Builds the reference
SW_Transformer + FOCAL + FOCALLoss on focal_amd/src/data/MOD.yaml with every dropout / drop-path rate overridden to 0 and
  SW_Transformer_ape_b8.npz      APE: true
  SW_Transformer_stride_b8.npz   APE: true, in_stride: {audio: 2, seismic: 1} (audio: image width 800, 4 input channels, 20 patches)
fills the state dict with oracle.weights.fill_state_dict_ (which makes the position embedding non-zero), runs synthetic_freq_input at
B = 8 and writes, per file: projected embeddings and pre-projector features of both views in eval and train mode (pass.*), the FOCAL
step's embeddings (train.emb*), the five loss terms, the gradient norm of every parameter that receives one, 16-element slices of the
absolute_pos_embed.* gradients, a 3-step AdamW loss trajectory and a probe on a position embedding.  Also
  manifest_SW_Transformer_stride.json   the reference's state-dict names and shapes at stride 2
Nothing is written unless the oracle (oracle/swt.py + oracle/loss.py, differentiated here with the position embeddings among the
leaves: oracle/step.py's own parameter filter is the APE-off one) agrees with the reference: 2e-5 on embeddings and loss, 5e-4 on
the gradients.
"""
import json
import os
import sys

import numpy as np
import torch
import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as gg  # noqa: E402

OUT = gg.OUT
B = 8
APE = "absolute_pos_embed."


def variant_cfg(base, stride):
    cfg = gg.no_dropout(base)
    cfg["SW_Transformer"]["APE"] = True
    if stride:
        cfg["SW_Transformer"]["in_stride"] = {"audio": 2, "seismic": 1}
    return cfg


def fixture(tag, cfg, seeds, manifest=None):
    from oracle import weights as ow
    from oracle.loss import focal_loss_terms
    from oracle.step import pretrain_param_filter
    from oracle.swt import swt_forward

    from general_utils.weight_utils import freeze_patch_embedding
    from models.FOCALModules import FOCAL
    from models.loss import FOCALLoss
    from models.SW_Transformer import SW_Transformer

    torch.manual_seed(0)
    args = gg.ref_args("SW_Transformer", cfg)
    net = SW_Transformer(args)
    sd = net.state_dict()
    if manifest:
        with open(os.path.join(OUT, manifest), "w") as f:
            json.dump([[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in sd.items()], f, indent=0)
    ow.fill_state_dict_(sd)
    state0 = {k: v.clone() for k, v in net.state_dict().items()}
    ape_keys = [k for k in state0 if k.startswith(APE)]
    assert ape_keys and all(state0[k].abs().max().item() > 1e-3 for k in ape_keys), "the position embedding must be non-zero"
    x1, x2 = ow.synthetic_freq_input(cfg, B, seed=seeds[0]), ow.synthetic_freq_input(cfg, B, seed=seeds[1])
    fix = {}

    # both views, eval and train mode (dropout 0: the modes differ only in which code path runs); the oracle must agree
    for mode in ("eval", "train"):
        net.train(mode == "train")
        with torch.no_grad():
            for v, x in (("1", x1), ("2", x2)):
                emb = net(x, class_head=False, proj_head=True)
                feat = net(x, class_head=False, proj_head=False)
                mine, mine_f = swt_forward(state0, cfg, x, proj_head=True), swt_forward(state0, cfg, x, proj_head=False)
                for m in cfg["modality_names"]:
                    for ref, got in ((emb[m], mine[m]), (feat[m], mine_f[m])):
                        err = (ref - got).abs().max().item()
                        assert err < 2e-5 * max(1.0, ref.abs().max().item()), (tag, mode, v, m, err)
                    fix[f"pass.{mode}.emb{v}.{m}"] = emb[m].numpy()
                    fix[f"pass.{mode}.feat{v}.{m}"] = feat[m].numpy()

    net.train()
    focal = freeze_patch_embedding(args, FOCAL(args, net))
    loss_fn = FOCALLoss(args)
    f1, f2 = focal(x1, x2, proj_head=True)
    loss = loss_fn(f1, f2)
    loss.backward()
    # the oracle's step with the position embeddings among the leaves
    P = {k: v.clone() for k, v in state0.items()}
    keys = [k for k, v in P.items() if v.is_floating_point() and (pretrain_param_filter("SW_Transformer", k) or k.startswith(APE))
            and not k.endswith(("running_mean", "running_var", "attn_mask"))]
    for k in keys:
        P[k].requires_grad_(True)
    o1, o2 = swt_forward(P, cfg, x1, proj_head=True), swt_forward(P, cfg, x2, proj_head=True)
    terms = focal_loss_terms(o1, o2, cfg, "SW_Transformer")
    grads = dict(zip(keys, torch.autograd.grad(terms["total"], [P[k] for k in keys], allow_unused=True)))
    assert abs(float(terms["total"]) - float(loss)) < 2e-5 * max(1.0, abs(float(loss))), (float(terms["total"]), float(loss))
    for k in ("shared", "private", "orth", "rank", "total"):
        fix[f"train.loss.{k}"] = np.array(float(terms[k]))
    for m in f1:
        assert (f1[m] - o1[m]).abs().max().item() < 2e-5 * max(1.0, f1[m].abs().max().item()), (tag, m, "train view1")
        fix[f"train.emb1.{m}"] = f1[m].detach().numpy()
        fix[f"train.emb2.{m}"] = f2[m].detach().numpy()
    names, norms = [], []
    for k, p in net.named_parameters():
        if p.grad is None:
            continue
        assert grads.get(k) is not None, f"reference has a gradient for {k} that the oracle does not produce"
        gerr = (p.grad - grads[k]).norm().item()
        assert gerr < 5e-4 * p.grad.norm().item() + 1e-5, (tag, k, gerr, p.grad.norm().item())
        names.append(k)
        norms.append(p.grad.double().norm().item())
        if k.startswith(APE):
            fix[f"train.gradslice.{k}"] = gg.sub(p.grad, 16)
    assert sorted(names) == sorted(k for k in keys if grads[k] is not None), "hot sets differ"
    assert set(ape_keys) <= set(names), "APE trains in FOCAL pretraining (freeze_patch_embedding matches patch_embed only)"
    fix["train.grad_names"] = np.array(names)
    fix["train.grad_norms"] = np.array(norms)

    # three AdamW steps on the same pair of views
    net2 = SW_Transformer(args)
    net2.load_state_dict(state0)
    net2.train()
    focal2 = FOCAL(args, net2)
    oc = cfg["FOCAL"]["pretrain_optimizer"]
    opt = torch.optim.AdamW(focal2.parameters(), lr=oc["start_lr"], weight_decay=oc["weight_decay"])
    focal2 = freeze_patch_embedding(args, focal2)
    traj = []
    for _ in range(3):
        opt.zero_grad()
        a, b = focal2(x1, x2, proj_head=True)
        l_ = loss_fn(a, b)
        l_.backward()
        opt.step()
        traj.append(float(l_))
    fix["adamw.loss_traj"] = np.array(traj)
    probe = f"{APE}{cfg['location_names'][0]}.audio"
    fix["adamw.probe_name"] = np.array(probe)
    fix["adamw.probe_before"] = gg.sub(state0[probe], 32)
    fix["adamw.probe_after3"] = gg.sub(dict(net2.named_parameters())[probe], 32)
    assert np.abs(fix["adamw.probe_after3"] - fix["adamw.probe_before"]).max() > 1e-4, "the probe must move"
    path = os.path.join(OUT, f"SW_Transformer_{tag}_b{B}.npz")
    np.savez_compressed(path, **fix)
    assert os.path.getsize(path) < 1 << 20
    return {"loss": float(loss), "traj": traj, "hot": len(names), "bytes": os.path.getsize(path)}


def main():
    gg.install_reference()
    with open(os.path.join(gg.REPO, "focal_amd", "src", "data", "MOD.yaml")) as f:
        base = yaml.safe_load(f)
    out = {"ape": fixture("ape", variant_cfg(base, False), (707, 808)),
           "stride": fixture("stride", variant_cfg(base, True), (909, 1010), manifest="manifest_SW_Transformer_stride.json")}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
