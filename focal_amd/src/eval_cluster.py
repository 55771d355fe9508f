"""Entry point [build extension]: `python eval_cluster.py -model=SW_Transformer -dataset=HAR3LOC -learn_framework=FOCAL [-model_weight=PATH]
[-n_clusters=N] [-cluster_n_init=10] [-cluster_max_iter=100] [-cluster_init=k-means++|random] [-cluster_seed=0]`: the clustering quality of
a pretrained backbone's un-projected features -- K-means fitted on the training split's features (train_utils/kmeans.py: GpuKMeans, all
restarts in one pass per Lloyd iteration), the validation and test rows assigned to the fitted centroids and scored against their class
labels by the adjusted Rand index and the normalised mutual information.  It answers what eval_knn.py's accuracy does not: whether the
classes form compact groups.  The checkpoint, the way the backbone is built and the refusals are eval_knn.py's; an empty cluster keeps its
centroid (sklearn relocates it), and two runs on one checkpoint print the same numbers."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from params.cluster_params import (SCORE, TOOL, parse_cluster_params, refuse_cluster_settings, resolve_n_clusters)  # noqa: E402
from params.knn_params import pretraining_command, refuse_classifier_checkpoint, refuse_other_frameworks  # noqa: E402


def refuse_data_parallel():
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit(f"{TOOL} scores on one device: launch it as one process (ranks of such a job would each score the same "
                         f"checkpoint on the same splits); `python {TOOL} ...` without torchrun")


def load_backbone_weight(args):
    """The checkpoint's state dict, read to host memory.  Refused: no checkpoint (nothing is scored at a random initialisation)."""
    import torch
    path = args.backbone_weight
    if not os.path.isfile(path):
        raise FileNotFoundError(f"no backbone checkpoint at {path}: `{pretraining_command(args)}` writes it (or name the folder or the "
                                "file that holds it with -model_weight)")
    return torch.load(path, map_location="cpu")


def evaluate_cluster(args, keep=False):
    """Score `args.backbone_weight`; returns {"inertia": the fit's, "val": (ARI, NMI), "test": (ARI, NMI)}.  keep=True: also, as a second
    value, {"train": (features, labels, cluster ids), "val" / "test": (features, labels, cluster ids), "centers": [K, D], "estimator",
    "conf": {"val" / "test": matrix [num_classes, n_clusters]}} -- the very tensors that were scored."""
    refuse_data_parallel()
    refuse_other_frameworks(args, TOOL, SCORE)
    refuse_cluster_settings(args)
    refuse_classifier_checkpoint(args, args.backbone_weight, TOOL)
    state_dict = load_backbone_weight(args)
    from data_augmenter.Augmenter import Augmenter
    from eval_knn import split_features
    from input_utils.multi_modal_dataloader import create_dataloader
    from train_utils.eval_functions import clustering_scores
    from train_utils.kmeans import GpuKMeans
    from train_utils.model_selection import init_backbone_model
    from focal_amd import ops
    loaders = {split: create_dataloader(split, args, batch_size=args.batch_size, workers=args.workers) for split in ("train", "val", "test")}
    augmenter = Augmenter(args)
    args.augmenter = augmenter
    backbone = init_backbone_model(args)
    backbone.load_state_dict(state_dict, strict=True)
    args.classifier = backbone
    backbone.eval()
    n_cls = int(args.dataset_config[args.task]["num_classes"])
    K = resolve_n_clusters(args)
    x, y = split_features(args, backbone, augmenter, loaders["train"])
    # (the fused form, not fit(fused=False): profiles/kmeans_fused.txt)
    estimator = GpuKMeans(K, n_init=int(getattr(args, "cluster_n_init", 10)), max_iter=int(getattr(args, "cluster_max_iter", 100)),
                          init=getattr(args, "cluster_init", "k-means++"), seed=int(getattr(args, "cluster_seed", 0))).fit(x)
    kept = {"train": (x, y, estimator.labels_), "centers": estimator.cluster_centers_, "estimator": estimator, "conf": {}}
    width, states = max(n_cls, K), {}
    for split in ("val", "test"):
        feats, labels = split_features(args, backbone, augmenter, loaders[split])
        ids = estimator.predict(feats)
        states[split] = ops.EvalState(width, feats.device)
        states[split].add(labels, preds=ids)
        kept[split] = (feats, labels, ids)
    out = {"inertia": estimator.inertia_}
    for split in ("val", "test"):  # the host reads each matrix once (read() refuses a nonzero out-of-range word)
        conf = states[split].read()[2]
        out[split] = clustering_scores(conf, n_cls, K)
        kept["conf"][split] = conf[:n_cls, :K]
    print(f"K-means (K={K}, n_init={estimator.R}) train inertia: {out['inertia']: .5f}")
    print(f"K-means (K={K}) val ARI: {out['val'][0]: .5f}, val NMI: {out['val'][1]: .5f}")
    print(f"K-means (K={K}) test ARI: {out['test'][0]: .5f}, test NMI: {out['test'][1]: .5f}")
    print(f"Val contingency matrix (classes x clusters):\n {kept['conf']['val']}")
    print(f"Test contingency matrix (classes x clusters):\n {kept['conf']['test']}")
    return (out, kept) if keep else out


def main_eval_cluster():
    refuse_data_parallel()
    evaluate_cluster(parse_cluster_params())


if __name__ == "__main__":
    main_eval_cluster()
