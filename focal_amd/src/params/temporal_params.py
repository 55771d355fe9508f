"""Parameters of `eval_temporal.py` [build extension]: the checkpoint is resolved and refused as `eval_knn.py`'s is
(params/knn_params.py); the temporal settings and the dataset's shape are refused here, before anything is built."""
import math
import os

from input_utils.yaml_utils import load_yaml
from params.base_params import parse_base_args
from params.knn_params import refuse_classifier_checkpoint, refuse_other_frameworks, resolve_backbone_weight
from params.params_util import set_auto_params

TOOL = "eval_temporal.py"
SCORE = "the temporal ranking constraint on its projected embeddings"
SPLITS = ("test", "val", "train")
MAX_KS = 8
SEQ_LENGTHS = (2, 4, 8, 16)  # focal_seq_rank's limit on L (include/focal_hip.h)


def parse_temporal_ks(text):
    """`-temporal_k=1,5,10` -> [1, 5, 10].  Refused: an empty entry, something that is no integer, a value below 1, more than 8 values."""
    entries = [e.strip() for e in str(text).split(",")]
    if any(e == "" for e in entries):
        raise ValueError(f"{TOOL}: -temporal_k={text} has an empty entry; write the k of recall@k as -temporal_k=1,5,10")
    try:
        ks = [int(e) for e in entries]
    except ValueError:
        raise ValueError(f"{TOOL}: -temporal_k={text} holds something that is no integer; write -temporal_k=1,5,10") from None
    if any(k < 1 for k in ks):
        raise ValueError(f"{TOOL}: every k of -temporal_k must be >= 1 (got {text}); the default is -temporal_k=1,5,10")
    if len(ks) > MAX_KS:
        raise ValueError(f"{TOOL}: -temporal_k takes at most {MAX_KS} values (got {len(ks)}); run it again for the others")
    return ks


def refuse_temporal_settings(args):
    """An unknown split, a margin that is not finite, a malformed -temporal_k -- each before a loader or a model exists.  Returns the
    parsed ks."""
    split = getattr(args, "temporal_split", "test")
    if split not in SPLITS:
        raise ValueError(f"{TOOL}: -temporal_split is one of {', '.join(SPLITS)} (got {split}); the default is -temporal_split=test")
    margin = getattr(args, "temporal_margin", None)
    if margin is not None and not math.isfinite(float(margin)):
        raise ValueError(f"{TOOL}: need a finite -temporal_margin (got {margin}); leave it out to score at FOCAL.inter_rank_margin of "
                         "the dataset's YAML, the margin the loss trains with")
    return parse_temporal_ks(getattr(args, "temporal_k", "1,5,10"))


def refuse_dataset_shape(args, dataset_config):
    """The block-pool kernel takes sequence lengths that divide its 64-row tile and feature widths that are multiples of 4, and a split
    has to hold two subsequences at least: anything else is refused with what to set."""
    seq_len = int(dataset_config["seq_len"])
    if seq_len not in SEQ_LENGTHS:
        raise ValueError(f"{TOOL}: seq_len={seq_len} of -dataset={args.dataset}; the block-pool kernel takes seq_len in "
                         f"{{{', '.join(str(v) for v in SEQ_LENGTHS)}}} (a block of seq_len x seq_len distances must not straddle a tile): "
                         "set seq_len to one of these in the dataset's YAML (every shipped configuration uses 4) and pretrain with it")
    max_rows = int(getattr(args, "temporal_max_rows", 65536))
    if max_rows < 2 * seq_len:
        raise ValueError(f"{TOOL}: need -temporal_max_rows >= 2 * seq_len = {2 * seq_len} (got {max_rows}): the constraint ranks a "
                         "subsequence against another; the default is -temporal_max_rows=65536 (a larger split is cut to a seeded "
                         "subset of whole subsequences)")
    emb_dim = int(dataset_config["FOCAL"]["emb_dim"])
    if emb_dim < 4 or emb_dim % 4:
        raise ValueError(f"{TOOL}: FOCAL.emb_dim={emb_dim}; the block-pool kernel takes a width that is a multiple of 4: set "
                         "FOCAL.emb_dim to a multiple of 4 in the dataset's YAML (every shipped configuration uses 256) and pretrain "
                         "with it")


def dataset_yaml(args):
    here = os.path.dirname(os.path.abspath(__file__))
    return getattr(args, "config", None) or os.path.join(here, "..", "data", f"{args.dataset}.yaml")


def parse_temporal_params():
    base = parse_base_args("eval_temporal")
    refuse_other_frameworks(base, TOOL, SCORE)  # before the device is selected
    base.temporal_ks = refuse_temporal_settings(base)
    refuse_dataset_shape(base, load_yaml(dataset_yaml(base)))
    base.stage = "pretrain"                     # the backbone and the loader are built as pretraining builds them: whole subsequences
    args = set_auto_params(base)
    args.backbone_weight = resolve_backbone_weight(args)
    refuse_classifier_checkpoint(args, args.backbone_weight, TOOL)
    return args
