#!/usr/bin/env python3
"""Generate the multi-location SW_Transformer parity fixture by IMPORTING THE REFERENCE in the build container.

Run here only (needs the reference checkout; never on the GPU box):   python tests/golden/gen_golden_multiloc.py

Uses gen_golden.py's stand-ins for the third-party packages (nothing from the reference is copied).  Builds the reference
SW_Transformer + FOCAL + FOCALLoss on focal_amd/src/data/HAR3LOC.yaml (3 locations x 2 modalities) with every dropout / drop-path rate
overridden to 0, fills the state dict with oracle.weights.fill_state_dict_, runs synthetic_freq_input at B = 8 and writes
  SW_Transformer_3loc_b8.npz         projected embeddings and pre-projector features of both views in eval and train mode
                                     (pass.*), the FOCAL step's embeddings (train.emb*), the five loss terms, the gradient norm of every parameter that receives one (each loc_* tensor
                                     included), gradient slices of the location layers, a 3-step AdamW loss trajectory and a probe
  manifest_SW_Transformer_3loc.json  the reference's state-dict names and shapes
The loss terms are split by the oracle's loss head (oracle/loss.py, which is location-agnostic) and checked against the reference's total.
"""
import copy
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


def main():
    gg.install_reference()
    from oracle import weights as ow
    from oracle.loss import focal_loss_terms

    from general_utils.weight_utils import freeze_patch_embedding
    from models.FOCALModules import FOCAL
    from models.loss import FOCALLoss
    from models.SW_Transformer import SW_Transformer

    torch.manual_seed(0)
    with open(os.path.join(gg.REPO, "focal_amd", "src", "data", "HAR3LOC.yaml")) as f:
        cfg = gg.no_dropout(yaml.safe_load(f))
    args = gg.ref_args("SW_Transformer", cfg)
    args.dataset, args.task = "HAR3LOC", "activity_classification"
    net = SW_Transformer(args)
    sd = net.state_dict()
    manifest = [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in sd.items()]
    with open(os.path.join(OUT, "manifest_SW_Transformer_3loc.json"), "w") as f:
        json.dump(manifest, f, indent=0)
    ow.fill_state_dict_(sd)
    state0 = {k: v.clone() for k, v in net.state_dict().items()}
    x1, x2 = ow.synthetic_freq_input(cfg, B, seed=505), ow.synthetic_freq_input(cfg, B, seed=606)
    fix = {}

    # both views, eval and train mode (dropout 0: the modes differ only in which code path runs): projected embeddings and the
    # pre-projector features (the location-fusion output)
    for mode in ("eval", "train"):
        net.train(mode == "train")
        with torch.no_grad():
            for v, x in (("1", x1), ("2", x2)):
                emb = net(x, class_head=False, proj_head=True)
                feat = net(x, class_head=False, proj_head=False)
                for m in cfg["modality_names"]:
                    fix[f"pass.{mode}.emb{v}.{m}"] = emb[m].numpy()
                    fix[f"pass.{mode}.feat{v}.{m}"] = feat[m].numpy()

    net.train()
    focal = freeze_patch_embedding(args, FOCAL(args, net))
    loss_fn = FOCALLoss(args)
    f1, f2 = focal(x1, x2, proj_head=True)
    loss = loss_fn(f1, f2)
    loss.backward()
    terms = focal_loss_terms({m: v.detach() for m, v in f1.items()}, {m: v.detach() for m, v in f2.items()}, cfg, "SW_Transformer")
    assert abs(float(terms["total"]) - float(loss)) < 1e-4 * max(1.0, abs(float(loss))), (float(terms["total"]), float(loss))
    for k in ("shared", "private", "orth", "rank", "total"):
        fix[f"train.loss.{k}"] = np.array(float(terms[k]))
    for m in f1:
        fix[f"train.emb1.{m}"] = f1[m].detach().numpy()
        fix[f"train.emb2.{m}"] = f2[m].detach().numpy()
    names, norms = [], []
    for k, p in net.named_parameters():
        if p.grad is None:
            continue
        names.append(k)
        norms.append(p.grad.double().norm().item())
        if k.startswith(("loc_context_layers.", "loc_fusion_layer.")) and k.endswith("weight"):
            fix[f"train.gradslice.{k}"] = gg.sub(p.grad, 16)
    assert any(n.startswith("loc_context_layers.") for n in names) and any(n.startswith("loc_fusion_layer.") for n in names)
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
    probe = f"loc_fusion_layer.{cfg['modality_names'][0]}.mha.out_proj.weight"
    fix["adamw.probe_name"] = np.array(probe)
    fix["adamw.probe_after3"] = gg.sub(dict(net2.named_parameters())[probe], 32)
    path = os.path.join(OUT, f"SW_Transformer_3loc_b{B}.npz")
    np.savez_compressed(path, **fix)
    print(json.dumps({"loss": float(loss), "traj": traj, "params": int(sum(p.numel() for p in net.parameters())),
                      "hot": len(names), "bytes": os.path.getsize(path)}, indent=1))


if __name__ == "__main__":
    main()
