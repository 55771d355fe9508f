"""Entry point [build extension]: `python eval_geometry.py -model=SW_Transformer -dataset=HAR3LOC -learn_framework=FOCAL
[-model_weight=PATH] [-geometry_split=test|val|train] [-geometry_t=2.0] [-geometry_max_rows=65536] [-geometry_seed=0]`: the numbers that
tell whether an embedding space is healthy, for a saved FOCAL backbone -- the first thing to look at when eval_knn.py's accuracy stalls.
Of the un-projected features: the silhouette against the class labels (sklearn's definition, overall and per class), the uniformity on
the sphere (Wang & Isola: log mean exp(-t d^2) over all pairs) and the effective rank (RankMe).  Of each modality's projected embedding,
cut into the shared and the private half as the loss cuts it: uniformity and effective rank, and per modality pair the alignment of the
positive pairs (the mean squared distance of one window's two embeddings).  A collapsing projector shows as a uniformity near 0 and an
effective rank near 1 before it shows in accuracy.  Only the silhouette reads a label.  No file is written.  The checkpoint, the way the
backbone is built and the refusals are eval_knn.py's; one process; two runs on one checkpoint print the same numbers."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from params.geometry_params import (SCORE, TOOL, default_task, parse_geometry_params, refuse_dataset_shape,  # noqa: E402
                                    refuse_geometry_settings)
from params.knn_params import pretraining_command, refuse_classifier_checkpoint, refuse_other_frameworks  # noqa: E402

HALVES = ("shared", "private")


def refuse_data_parallel():
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit(f"{TOOL} scores on one device: launch it as one process (ranks of such a job would each score the same "
                         f"checkpoint on the same split); `python {TOOL} ...` without torchrun")


def load_backbone_weight(args):
    """The checkpoint's state dict, read to host memory.  Refused: no checkpoint (nothing is scored at a random initialisation)."""
    import torch
    path = args.backbone_weight
    if not os.path.isfile(path):
        raise FileNotFoundError(f"no backbone checkpoint at {path}: `{pretraining_command(args)}` writes it (or name the folder or the "
                                "file that holds it with -model_weight)")
    return torch.load(path, map_location="cpu")


def class_names(args, n_cls):
    task = args.dataset_config.get(args.task)
    names = task.get("class_names") if isinstance(task, dict) else None
    return [str(names[c]) if names is not None and c < len(names) else str(c) for c in range(n_cls)]


def evaluate_geometry(args, keep=False):
    """Score `args.backbone_weight`; returns {"n", "features": {"silhouette", "silhouette_by_class", "uniformity", "effective_rank", "D"},
    "embeddings": {(mod, half): {"uniformity", "effective_rank", "D"}}, "alignment": {half: {(a, b): value}}}.  keep=True: also, as a
    second value, {"features", "labels", "projections": {mod: [n, emb_dim]}, "silhouettes": float64 [n], "sums": {"silhouette": S [n,
    classes], "uniformity": {"features" | (mod, half): S [n, 1]}}} -- the very tensors that were scored."""
    refuse_data_parallel()
    refuse_other_frameworks(args, TOOL, SCORE)
    refuse_geometry_settings(args)
    refuse_dataset_shape(args, args.dataset_config, default_task(args))
    refuse_classifier_checkpoint(args, args.backbone_weight, TOOL)
    state_dict = load_backbone_weight(args)
    from data_augmenter.Augmenter import Augmenter
    from eval_knn import split_features
    from eval_retrieval import space_columns, split_projections
    from eval_tsne import subset_rows
    from input_utils.multi_modal_dataloader import create_dataloader
    from train_utils.geometry import alignment, effective_rank, silhouette, uniformity
    from train_utils.model_selection import init_backbone_model
    split = getattr(args, "geometry_split", "test")
    t = float(getattr(args, "geometry_t", 2.0))
    seed = int(getattr(args, "geometry_seed", 0))
    loader = create_dataloader(split, args, batch_size=args.batch_size, workers=args.workers)
    augmenter = Augmenter(args)
    args.augmenter = augmenter
    backbone = init_backbone_model(args)
    backbone.load_state_dict(state_dict, strict=True)
    args.classifier = backbone
    backbone.eval()
    feats, labels = split_features(args, backbone, augmenter, loader)
    proj, _ = split_projections(args, backbone, augmenter, loader)
    feats = feats.float().contiguous()
    N = feats.shape[0]
    rows = subset_rows(N, int(getattr(args, "geometry_max_rows", 65536)), seed)
    n = rows.numel()
    if n < N:
        print(f"Geometry scores {n} of {N} rows of the {split} split (seed {seed})")
        pick = rows.to(feats.device)
        feats, labels = feats[pick].contiguous(), labels[pick].contiguous()
        proj = {m: p[pick].contiguous() for m, p in proj.items()}
    if n < 2:
        raise ValueError(f"{TOOL}: the {split} split has {n} row; every score is over pairs of rows: score a larger split with "
                         "-geometry_split")
    n_cls = int(args.dataset_config[args.task]["num_classes"])
    D = feats.shape[1]
    # (per score, by the measurement in profiles/geometry_fused.txt: the silhouette in its torch form, which is the faster one at
    # 65 536 x 1024; the uniformity in its fused form)
    sil, sil_mean, sil_class, S_sil = silhouette(feats, labels, n_cls, fused=False, return_sums=True)
    uni, S_uni = uniformity(feats, t=t, return_sums=True)
    rank = effective_rank(feats)
    out = {"n": n, "features": {"silhouette": sil_mean, "silhouette_by_class": sil_class.cpu().tolist(), "uniformity": uni,
                                "effective_rank": rank, "D": D},
           "embeddings": {}, "alignment": {h: {} for h in HALVES}}
    kept = {"features": feats, "labels": labels, "projections": proj, "silhouettes": sil,
            "sums": {"silhouette": S_sil, "uniformity": {"features": S_uni}}}
    print(f"Geometry [features] (split={split}, n={n}, D={D}): silhouette {sil_mean: .5f}, uniformity (t={t:g}) {uni: .5f}, "
          f"effective rank {rank:.3f} of {min(n - 1, D)}")
    if sil_mean != sil_mean:
        print(f"Silhouette is undefined: fewer than two of the task's {n_cls} classes occur among these {n} rows")
    else:
        names = class_names(args, n_cls)
        print("Silhouette by class: " + ", ".join(f"{names[c]} {v: .5f}" for c, v in enumerate(out["features"]["silhouette_by_class"])
                                                   if v == v))
    mods = list(args.dataset_config["modality_names"])
    cols = space_columns(proj[mods[0]].shape[1])
    for m in mods:
        for h in HALVES:
            z = proj[m][:, cols[h]].contiguous()
            u, S = uniformity(z, t=t, return_sums=True)
            r = effective_rank(z)
            out["embeddings"][(m, h)] = {"uniformity": u, "effective_rank": r, "D": z.shape[1]}
            kept["sums"]["uniformity"][(m, h)] = S
            print(f"Geometry [{m} {h}] (n={n}, D={z.shape[1]}): uniformity (t={t:g}) {u: .5f}, effective rank {r:.3f} of "
                  f"{min(n - 1, z.shape[1])}")
    for i, a in enumerate(mods):
        for b in mods[i + 1:]:
            parts = []
            for h in HALVES:
                v = out["alignment"][h][(a, b)] = alignment(proj[a][:, cols[h]], proj[b][:, cols[h]])
                parts.append(f"Alignment [{h}] {a} <-> {b}: {v:.5f}")
            print("      ".join(parts))
    return (out, kept) if keep else out


def main_eval_geometry():
    refuse_data_parallel()
    evaluate_geometry(parse_geometry_params())


if __name__ == "__main__":
    main_eval_geometry()
