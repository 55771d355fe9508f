"""Parameters of `eval_cluster.py` [build extension]: the checkpoint is resolved and refused as `eval_knn.py`'s is (params/knn_params.py);
the cluster count is settled here, before anything is built."""
from params.base_params import parse_base_args
from params.knn_params import refuse_classifier_checkpoint, refuse_other_frameworks, resolve_backbone_weight
from params.params_util import set_auto_params

TOOL = "eval_cluster.py"
SCORE = "the K-means ARI / NMI of its features"
MAX_CLUSTERS = 64  # focal_kmeans_assign's limit on K (include/focal_hip.h)


def refuse_cluster_count(n_clusters):
    """`-n_clusters` outside the assignment kernel's range, or restarts / iterations that are none.  n_clusters None (the flag not given:
    the task's num_classes, known once the dataset's configuration is read) passes."""
    if n_clusters is not None and not 1 <= int(n_clusters) <= MAX_CLUSTERS:
        raise ValueError(f"{TOOL}: need 1 <= n_clusters <= {MAX_CLUSTERS} (got -n_clusters={n_clusters}): the assignment kernel holds a "
                         f"restart's centroids in one pass of at most {MAX_CLUSTERS} columns")


def refuse_cluster_settings(args):
    refuse_cluster_count(getattr(args, "n_clusters", None))
    n_init, max_iter = int(getattr(args, "cluster_n_init", 10)), int(getattr(args, "cluster_max_iter", 100))
    if n_init < 1 or max_iter < 1:
        raise ValueError(f"{TOOL}: need -cluster_n_init >= 1 and -cluster_max_iter >= 1 (got {n_init}, {max_iter})")


def resolve_n_clusters(args):
    """`-n_clusters`, or the task's num_classes."""
    chosen = getattr(args, "n_clusters", None)
    n = int(chosen) if chosen is not None else int(args.dataset_config[args.task]["num_classes"])
    refuse_cluster_count(n)
    return n


def parse_cluster_params():
    base = parse_base_args("eval_cluster")
    refuse_other_frameworks(base, TOOL, SCORE)  # before the device is selected
    refuse_cluster_settings(base)
    base.stage = "pretrain"                     # the backbone is built as pretraining builds it: multi-location configurations included
    args = set_auto_params(base)
    args.backbone_weight = resolve_backbone_weight(args)
    refuse_classifier_checkpoint(args, args.backbone_weight, TOOL)
    args.n_clusters = resolve_n_clusters(args)
    return args
