#!/usr/bin/env python3
"""Multi-location DeepSense: the parity fixture of FOCAL pretraining on focal_amd/src/data/HAR3LOC.yaml (3 locations x 2 modalities),
written by IMPORTING THE REFERENCE in the build container (gen_golden.py: REF and its stand-ins; nothing of the reference is copied).
Run where the reference is importable, never on the GPU box:

    python tests/golden/gen_golden_deepsense_multiloc.py   ->  tests/golden/DeepSense_3loc_b8.npz, manifest_DeepSense_3loc.json

The reference runs, per modality, one ConvBlock per location, the mean of their outputs (MeanFusionBlock) and a second ConvBlock
(mod_extractors.{mod}: one input channel, spectrum = loc_mod_out_channels) in front of the GRU.  oracle/deepsense.py is single-location
and cannot cross-check it; the location-agnostic helpers do their part (fill_state_dict_, synthetic_freq_input, focal_loss_terms).

Stored (B = 8, name-seeded weights, synthetic_freq_input seeds 311 / 312, dropout off), from the REFERENCE model:
  train.*    a FOCAL training step: embeddings of both views, the five loss terms (split by oracle.loss.focal_loss_terms, checked against
             the reference's total to 1e-4), names / norms / a 16-element strided slice of every parameter gradient, every BatchNorm
             running buffer under loc_mod_extractors. AND mod_extractors. after the step;
  adamw.*    the loss of three AdamW steps on that batch at learning rate adamw.lr = 1e-4 and a probe of
             mod_extractors.acc.conv_layers_inter.0.conv.weight after them -- a trajectory the reference itself keeps under gradient noise and
             under bf16 autocast (checked before writing, see main());
  settled.*  eval mode on running statistics the reference settled by itself (40 train-mode passes on seeds 5000 ...): the buffers and
             the embeddings / un-projected features of view 1.

Seeds: before anything is written the step is repeated under CPU bf16 autocast (a harsher rounding than the HIP path's: nothing stays in
fp32) and must stay inside the bf16 test's own bounds -- no gradient norm off by more than 6e-2, loss terms within 1e-2 -- i.e. no ranking
hinge of the loss sits at its kink on this batch and the test's outlier allowance is not consumed by the reference itself."""
import json
import os
import sys
import warnings

import numpy as np
import torch
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G  # noqa: E402  (install_reference, ref_args, no_dropout, sub)

B = 8
SEEDS = (311, 312)
PROBE = "mod_extractors.acc.conv_layers_inter.0.conv.weight"
ADAMW_LR = 1e-4


def main():
    G.install_reference()
    from oracle import weights as ow
    from oracle.loss import focal_loss_terms
    from general_utils.weight_utils import freeze_patch_embedding
    from models.DeepSense import DeepSense
    from models.FOCALModules import FOCAL
    from models.loss import FOCALLoss

    torch.manual_seed(0)
    with open(os.path.join(G.REPO, "focal_amd", "src", "data", "HAR3LOC.yaml")) as f:
        cfg = G.no_dropout(yaml.safe_load(f))
    args = G.ref_args("DeepSense", cfg)
    args.dataset, args.task = "HAR3LOC", "activity_classification"
    x1, x2 = ow.synthetic_freq_input(cfg, B, seed=SEEDS[0]), ow.synthetic_freq_input(cfg, B, seed=SEEDS[1])
    loss_fn = FOCALLoss(args)
    fix = {}

    net = DeepSense(args)
    sd = net.state_dict()
    manifest = [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in sd.items()]
    ow.fill_state_dict_(sd)
    state0 = {k: v.clone() for k, v in net.state_dict().items()}

    def step(model, autocast=False):
        model.train()
        focal = freeze_patch_embedding(args, FOCAL(args, model))
        if autocast:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                with torch.autocast("cpu", dtype=torch.bfloat16):
                    f1, f2 = focal(x1, x2, proj_head=True)
            f1, f2 = {m: v.float() for m, v in f1.items()}, {m: v.float() for m, v in f2.items()}
        else:
            f1, f2 = focal(x1, x2, proj_head=True)
        loss = loss_fn(f1, f2)
        loss.backward()
        terms = focal_loss_terms({m: v.detach() for m, v in f1.items()}, {m: v.detach() for m, v in f2.items()}, cfg, "DeepSense")
        return f1, f2, loss, {k: float(v) for k, v in terms.items()}

    # ---------------------------------------------------------------- train mode: FOCAL(view 1, view 2) -> loss -> backward
    f1, f2, loss, terms = step(net)
    assert abs(terms["total"] - float(loss)) < 1e-4 * max(1.0, abs(float(loss))), (terms["total"], float(loss))
    for m in f1:
        fix[f"train.emb1.{m}"] = f1[m].detach().numpy()
        fix[f"train.emb2.{m}"] = f2[m].detach().numpy()
    for k in ("shared", "private", "orth", "rank", "total"):
        fix[f"train.loss.{k}"] = np.array(terms[k])
    fix["train.loss.reference_total"] = np.array(float(loss))
    names, norms = [], []
    for k, p in net.named_parameters():
        if p.grad is None:
            continue
        names.append(k)
        norms.append(p.grad.double().norm().item())
        fix[f"train.gradslice.{k}"] = G.sub(p.grad, 16)
    dead = sorted({k.split(".")[0] for k, p in net.named_parameters() if p.grad is None})
    assert dead == ["class_layer"], dead
    assert sum(k.startswith("mod_extractors.") for k in names) == 36, "the second ConvBlocks must train"
    fix["train.grad_names"] = np.array(names)
    fix["train.grad_norms"] = np.array(norms)
    for k, v in net.state_dict().items():
        if k.endswith(("running_mean", "running_var")) and k.startswith(("loc_mod_extractors.", "mod_extractors.")):
            fix[f"train.buf.{k}"] = v.numpy()

    # ---------------------------------------------------------------- the batch is no bf16 trap: the same step under CPU bf16 autocast
    net_b = DeepSense(args)
    net_b.load_state_dict(state0)
    g1, g2, _, terms_b = step(net_b, autocast=True)
    drift_terms = max(abs(terms_b[k] - terms[k]) / max(1.0, abs(terms[k])) for k in terms)
    drift_emb = max(((a[m].detach() - b[m].detach()).abs().max() / b[m].detach().abs().max()).item() for a, b in ((g1, f1), (g2, f2)) for m in f1)
    ref_norm = dict(zip(names, norms))
    rel = {k: abs(p.grad.double().norm().item() - ref_norm[k]) / max(ref_norm[k], 1e-6) for k, p in net_b.named_parameters()
           if p.grad is not None and not (k.endswith("conv.bias") and ref_norm[k] < 1e-5)}
    over = {k: v for k, v in rel.items() if v > 6e-2}
    assert not over and drift_terms < 1e-2, (over, drift_terms)
    fix["bf16_autocast.grad_norm_worst_rel"] = np.float64(max(rel.values()))
    fix["bf16_autocast.terms_rel"] = np.float64(drift_terms)
    fix["bf16_autocast.emb_rel"] = np.float64(drift_emb)

    # ---------------------------------------------------------------- three AdamW steps on the fixed batch
    # At the FOCAL section's start_lr (1e-3) the reference's own trajectory on this model is no yardstick: AdamW's first updates are
    # sign-like, the loss falls 26 -> 7.6 in two of them, and gradient noise of 1e-6 of each tensor's maximum moves the third loss by up to
    # 5e-2, CPU bf16 autocast by 15 % -- on every seed pair tried (311 / 312, 505 / 606, 101 / 202, 707 / 808).  At ADAMW_LR = 1e-4 (the
    # DeepSense section's own optimizer.start_lr) the same batch descends as steeply (26 -> 13.7 -> 5.6) and the trajectory is stable.
    # That is checked here before anything is written: perturbed runs of the REFERENCE must stay within a quarter of the bounds the GPU test
    # asserts (fp32: 2e-3 per loss, 2e-4 on the probe; bf16: 1e-2 on the first loss, 15 % on the others).
    oc = cfg["FOCAL"]["pretrain_optimizer"]

    def trajectory(noise=0.0, noise_seed=0, autocast=False):
        net2 = DeepSense(args)
        net2.load_state_dict(state0)
        net2.train()
        focal2 = FOCAL(args, net2)
        opt = torch.optim.AdamW(focal2.parameters(), lr=ADAMW_LR, weight_decay=oc["weight_decay"])
        focal2 = freeze_patch_embedding(args, focal2)
        g = torch.Generator().manual_seed(noise_seed)
        out = []
        for _ in range(3):
            opt.zero_grad()
            if autocast:
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    with torch.autocast("cpu", dtype=torch.bfloat16):
                        a, b = focal2(x1, x2, proj_head=True)
                a, b = {m: v.float() for m, v in a.items()}, {m: v.float() for m, v in b.items()}
            else:
                a, b = focal2(x1, x2, proj_head=True)
            l_ = loss_fn(a, b)
            l_.backward()
            if noise:  # Gaussian, `noise` of each gradient tensor's largest element: what a kernel's summation order does, and harsher
                with torch.no_grad():
                    for p in net2.parameters():
                        if p.grad is not None:
                            p.grad.add_(torch.randn(p.grad.shape, generator=g) * noise * p.grad.abs().max())
            opt.step()
            out.append(float(l_.detach()))
        return out, G.sub(dict(net2.named_parameters())[PROBE], 32)

    traj, probe = trajectory()
    assert traj[2] < 0.5 * traj[0], traj  # the steps do move the loss: the bounds below are small against the descent
    worst_loss, worst_probe = 0.0, 0.0
    for noise_seed in (1, 2, 3):
        t, pr = trajectory(noise=1e-6, noise_seed=noise_seed)
        worst_loss = max(worst_loss, max(abs(a - b) / abs(b) for a, b in zip(t, traj)))
        worst_probe = max(worst_probe, float(np.abs(np.asarray(pr) - np.asarray(probe)).max()))
    assert worst_loss < 2e-3 / 4 and worst_probe < 2e-4 / 4, (worst_loss, worst_probe)
    tb, _ = trajectory(autocast=True)
    drift_traj = [abs(a - b) / abs(b) for a, b in zip(tb, traj)]
    assert drift_traj[0] < 1e-2 / 4 and max(drift_traj[1:]) < 0.15 / 4, drift_traj
    fix["adamw.lr"] = np.float64(ADAMW_LR)
    fix["adamw.loss_traj"] = np.array(traj)
    fix["adamw.probe_name"] = np.array(PROBE)
    fix["adamw.probe_after3"] = probe
    fix["adamw.reference_under_noise.loss_rel"] = np.float64(worst_loss)
    fix["adamw.reference_under_noise.probe_abs"] = np.float64(worst_probe)
    fix["adamw.reference_bf16_autocast.loss_rel"] = np.array(drift_traj)

    # ---------------------------------------------------------------- eval mode on statistics the reference settled by itself
    net3 = DeepSense(args)
    net3.load_state_dict(state0)
    net3.train()
    with torch.no_grad():
        for it in range(40):
            net3(ow.synthetic_freq_input(cfg, B, seed=5000 + it), class_head=False, proj_head=True)
    net3.eval()
    with torch.no_grad():
        emb = net3(x1, class_head=False, proj_head=True)
        feat = net3(x1, class_head=False, proj_head=False)
    for m in emb:
        fix[f"settled.eval.emb.{m}"] = emb[m].numpy()
        fix[f"settled.eval.feat.{m}"] = feat[m].numpy()
    for k, v in net3.state_dict().items():
        if k.endswith(("running_mean", "running_var", "num_batches_tracked")):
            fix[f"settled.buffer.{k}"] = v.numpy()

    with open(os.path.join(HERE, "manifest_DeepSense_3loc.json"), "w") as f:
        json.dump(manifest, f, indent=0)
    out = os.path.join(HERE, f"DeepSense_3loc_b{B}.npz")
    np.savez_compressed(out, **fix)
    size, cap = os.path.getsize(out), os.path.getsize(os.path.join(HERE, "augment_b2_seed77.npz"))
    assert size <= cap, (size, cap)
    print(json.dumps({"loss": float(loss), "terms": terms, "traj": traj, "keys": len(manifest),
                      "params": int(sum(p.numel() for p in net.parameters())), "hot": len(names),
                      "bf16_autocast": {"grad_norm_worst_rel": max(rel.values()), "terms_rel": drift_terms, "emb_rel": drift_emb},
                      "adamw_reference": {"noise_loss_rel": worst_loss, "noise_probe_abs": worst_probe, "bf16_autocast_loss_rel": drift_traj},
                      "bytes": size, "cap": cap}, indent=1))


if __name__ == "__main__":
    main()
