"""Entry point [build extension]: `python eval_retrieval.py -model=SW_Transformer -dataset=HAR3LOC -learn_framework=FOCAL
[-model_weight=PATH] [-retrieval_split=test|val|train] [-retrieval_k=1,5,10]`: cross-modal retrieval on the tensors the FOCAL loss trains --
the per-modality PROJECTED embeddings (`backbone(x, class_head=False, proj_head=True)`), cut into a shared and a private half as the loss
cuts them (models/FOCALModules.py: split_features).  For each space (shared, private, full) and each ordered modality pair a -> b, the
embedding of window i in modality a queries all n embeddings of modality b and the place of window i itself is reported: recall@k, mean
reciprocal rank, median rank, and the mean count of exact ties (a collapsed projector ties with everything).  Beside them the cosines the
loss's orthogonality term sees.  The shared space should retrieve, the private space should not, and the cosines should be near zero.
No label is read and no file is written.  The checkpoint, the way the backbone is built and the refusals are eval_knn.py's; one process."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from params.knn_params import pretraining_command, refuse_classifier_checkpoint, refuse_other_frameworks  # noqa: E402
from params.retrieval_params import (SCORE, TOOL, parse_retrieval_params, refuse_dataset_shape,  # noqa: E402
                                     refuse_retrieval_settings)

SPACES = ("shared", "private", "full")


def refuse_data_parallel():
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit(f"{TOOL} ranks on one device: launch it as one process (ranks of such a job would each score the same "
                         f"checkpoint on the same split); `python {TOOL} ...` without torchrun")


def load_backbone_weight(args):
    """The checkpoint's state dict, read to host memory.  Refused: no checkpoint (nothing is scored at a random initialisation)."""
    import torch
    path = args.backbone_weight
    if not os.path.isfile(path):
        raise FileNotFoundError(f"no backbone checkpoint at {path}: `{pretraining_command(args)}` writes it (or name the folder or the "
                                "file that holds it with -model_weight)")
    return torch.load(path, map_location="cpu")


def split_projections(args, backbone, augmenter, loader):
    """Projected embeddings {mod: [n, emb_dim] fp32} and class indices [n] of one split, on the device."""
    import torch
    mods = args.dataset_config["modality_names"]
    feats, labels = {m: [] for m in mods}, []
    with torch.no_grad():
        for time_loc_inputs, y in loader:
            freq_loc_inputs, _ = augmenter.forward("no", time_loc_inputs, y)
            out = backbone(freq_loc_inputs, class_head=False, proj_head=True)
            for m in mods:
                feats[m].append(out[m].detach().float())
            labels.append(y.argmax(dim=1) if y.dim() > 1 else y)
    if not labels:
        raise ValueError("eval_retrieval: the loader yielded no batch")
    proj = {m: torch.cat(feats[m]).contiguous() for m in mods}
    return proj, torch.cat(labels).to(proj[mods[0]].device).long()


def space_columns(width):
    h = width // 2
    return {"shared": slice(0, h), "private": slice(h, 2 * h), "full": slice(0, width)}


def evaluate_retrieval(args, keep=False):
    """Score `args.backbone_weight`; returns {"retrieval": {space: {(a, b): metrics}}, "orthogonality": ..., "n": rows, "chance": {k: k / n}}
    (metrics: train_utils/retrieval.py: retrieval_metrics).  keep=True: also, as a second value, {"projections": {mod: [n, emb_dim]},
    "labels", "ranks": {space: {(a, b): int64 [n]}}, "tied": the same} -- the very tensors that were scored."""
    refuse_data_parallel()
    refuse_other_frameworks(args, TOOL, SCORE)
    ks = refuse_retrieval_settings(args)
    refuse_dataset_shape(args, args.dataset_config)
    refuse_classifier_checkpoint(args, args.backbone_weight, TOOL)
    state_dict = load_backbone_weight(args)
    from data_augmenter.Augmenter import Augmenter
    from input_utils.multi_modal_dataloader import create_dataloader
    from train_utils.model_selection import init_backbone_model
    from train_utils.retrieval import cross_modal_ranks, orthogonality, retrieval_metrics
    split = getattr(args, "retrieval_split", "test")
    loader = create_dataloader(split, args, batch_size=args.batch_size, workers=args.workers)
    augmenter = Augmenter(args)
    args.augmenter = augmenter
    backbone = init_backbone_model(args)
    backbone.load_state_dict(state_dict, strict=True)
    args.classifier = backbone
    backbone.eval()
    proj, labels = split_projections(args, backbone, augmenter, loader)
    mods = list(args.dataset_config["modality_names"])
    n, width = proj[mods[0]].shape
    out = {"retrieval": {s: {} for s in SPACES}, "n": n, "chance": {k: min(k, n) / n for k in ks}}
    kept = {"projections": proj, "labels": labels, "ranks": {s: {} for s in SPACES}, "tied": {s: {} for s in SPACES}}
    for space, cols in space_columns(width).items():
        for a in mods:
            for b in mods:
                if a == b:
                    continue
                # (the fused form, not fused=False: profiles/retrieval_fused.txt)
                ranks, tied, _, _ = cross_modal_ranks(proj[a][:, cols], proj[b][:, cols])
                kept["ranks"][space][(a, b)], kept["tied"][space][(a, b)] = ranks, tied
                m = out["retrieval"][space][(a, b)] = retrieval_metrics(ranks, tied, ks)
                recalls = ", ".join(f"R@{k} {m['recall'][k]:.5f}" for k in ks)
                print(f"Retrieval [{space}] {a} -> {b} (n={n}): {recalls}, MRR {m['mrr']:.5f}, median rank {m['median_rank']:.1f}, "
                      f"mean tied {m['mean_tied']:.3f}")
    print("chance: " + ", ".join(f"R@{k} = {min(k, n)} / {n} = {out['chance'][k]:.5f}" for k in ks))
    out["orthogonality"] = orth = orthogonality(proj, mods)
    for mod, (mean, hinge) in orth["shared_private"].items():
        print(f"Orthogonality shared . private [{mod}]: mean cos {mean: .5f}, mean max(0, cos) {hinge:.5f}")
    for (a, b), (mean, hinge) in orth["private_private"].items():
        print(f"Orthogonality private . private [{a}, {b}]: mean cos {mean: .5f}, mean max(0, cos) {hinge:.5f}")
    return (out, kept) if keep else out


def main_eval_retrieval():
    refuse_data_parallel()
    evaluate_retrieval(parse_retrieval_params())


if __name__ == "__main__":
    main_eval_retrieval()
