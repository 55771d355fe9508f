"""Parameters of `eval_geometry.py` [build extension]: the checkpoint is resolved and refused as `eval_knn.py`'s is
(params/knn_params.py); the geometry settings and the dataset's shape are refused here, before anything is built."""
import math
import os

from input_utils.yaml_utils import load_yaml
from params.base_params import parse_base_args
from params.knn_params import refuse_classifier_checkpoint, refuse_other_frameworks, resolve_backbone_weight
from params.params_util import set_auto_params

TOOL = "eval_geometry.py"
SCORE = "the silhouette, uniformity, alignment and effective rank of its features and embeddings"
SPLITS = ("test", "val", "train")
MAX_CLASSES = 64  # focal_pair_sums' limit on G (include/focal_hip.h)


def refuse_geometry_settings(args):
    """An unknown split, a -geometry_t that is no positive number, a row cap below 2 -- each before a loader or a model exists."""
    split = getattr(args, "geometry_split", "test")
    if split not in SPLITS:
        raise ValueError(f"{TOOL}: -geometry_split is one of {', '.join(SPLITS)} (got {split}); the default is -geometry_split=test")
    t = float(getattr(args, "geometry_t", 2.0))
    if not math.isfinite(t) or t <= 0:
        raise ValueError(f"{TOOL}: need a finite -geometry_t > 0 (got {t}); the default is -geometry_t=2 (Wang & Isola's)")
    max_rows = int(getattr(args, "geometry_max_rows", 65536))
    if max_rows < 2:
        raise ValueError(f"{TOOL}: need -geometry_max_rows >= 2 (got {max_rows}): every score is over pairs of rows; the default is "
                         "-geometry_max_rows=65536 (a larger split is cut to a seeded subset)")


def refuse_dataset_shape(args, dataset_config, task):
    """The pair-sum kernel takes at most 64 groups and feature widths that are multiples of 4: a task with more classes or an embedding
    whose half is no such width is refused with what to use instead."""
    n_cls = int(dataset_config[task]["num_classes"])
    if n_cls > MAX_CLASSES:
        raise ValueError(f"{TOOL}: task {task} of -dataset={args.dataset} has {n_cls} classes; the silhouette's pair-sum kernel takes at "
                         f"most {MAX_CLASSES} groups: name a task with fewer classes with -task, or score the backbone with "
                         f"`python eval_knn.py -model={args.model} -dataset={args.dataset} -learn_framework=FOCAL`")
    emb_dim = int(dataset_config["FOCAL"]["emb_dim"])
    if emb_dim < 8 or (emb_dim // 2) % 4 or emb_dim % 2:
        raise ValueError(f"{TOOL}: FOCAL.emb_dim={emb_dim} gives shared / private halves of {emb_dim // 2} columns; the pair-sum kernel "
                         "takes a width that is a multiple of 4: set FOCAL.emb_dim to a multiple of 8 in the dataset's YAML (every "
                         "shipped configuration uses 256) and pretrain with it")


def dataset_yaml(args):
    here = os.path.dirname(os.path.abspath(__file__))
    return getattr(args, "config", None) or os.path.join(here, "..", "data", f"{args.dataset}.yaml")


def default_task(args):
    from params.params_util import _DEFAULT_TASK
    return args.task if getattr(args, "task", None) is not None else _DEFAULT_TASK[args.dataset]


def parse_geometry_params():
    base = parse_base_args("eval_geometry")
    refuse_other_frameworks(base, TOOL, SCORE)  # before the device is selected
    refuse_geometry_settings(base)
    refuse_dataset_shape(base, load_yaml(dataset_yaml(base)), default_task(base))
    base.stage = "pretrain"                     # the backbone is built as pretraining builds it: multi-location configurations included
    args = set_auto_params(base)
    args.backbone_weight = resolve_backbone_weight(args)
    refuse_classifier_checkpoint(args, args.backbone_weight, TOOL)
    return args
