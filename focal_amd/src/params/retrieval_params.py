"""Parameters of `eval_retrieval.py` [build extension]: the checkpoint is resolved and refused as `eval_knn.py`'s is
(params/knn_params.py); the retrieval settings and the dataset's shape are refused here, before anything is built."""
import os

from input_utils.yaml_utils import load_yaml
from params.base_params import parse_base_args
from params.knn_params import refuse_classifier_checkpoint, refuse_other_frameworks, resolve_backbone_weight
from params.params_util import set_auto_params

TOOL = "eval_retrieval.py"
SCORE = "cross-modal retrieval on its projected embeddings"
SPLITS = ("test", "val", "train")
MAX_KS = 8


def parse_retrieval_ks(text):
    """`-retrieval_k=1,5,10` -> [1, 5, 10].  Refused: an empty entry, something that is no integer, a value below 1, more than 8 values."""
    entries = [e.strip() for e in str(text).split(",")]
    if any(e == "" for e in entries):
        raise ValueError(f"{TOOL}: -retrieval_k={text} has an empty entry; write the k of recall@k as -retrieval_k=1,5,10")
    try:
        ks = [int(e) for e in entries]
    except ValueError:
        raise ValueError(f"{TOOL}: -retrieval_k={text} holds something that is no integer; write -retrieval_k=1,5,10") from None
    if any(k < 1 for k in ks):
        raise ValueError(f"{TOOL}: every k of -retrieval_k must be >= 1 (got {text}); the default is -retrieval_k=1,5,10")
    if len(ks) > MAX_KS:
        raise ValueError(f"{TOOL}: -retrieval_k takes at most {MAX_KS} values (got {len(ks)}); run it again for the others")
    return ks


def refuse_retrieval_settings(args):
    """An unknown split or a malformed -retrieval_k, before a loader or a model exists.  Returns the parsed ks."""
    split = getattr(args, "retrieval_split", "test")
    if split not in SPLITS:
        raise ValueError(f"{TOOL}: -retrieval_split is one of {', '.join(SPLITS)} (got {split})")
    return parse_retrieval_ks(getattr(args, "retrieval_k", "1,5,10"))


def refuse_dataset_shape(args, dataset_config):
    """Retrieval crosses modalities, and the kernel takes feature widths that are multiples of 4: a dataset with one modality or an
    embedding whose half is no such width is refused with what to use instead."""
    mods = list(dataset_config.get("modality_names", []))
    if len(mods) < 2:
        raise ValueError(f"{TOOL}: -dataset={args.dataset} has {len(mods)} modality ({', '.join(mods) or 'none'}): retrieval ranks one "
                         "modality's embeddings against another's; score such a backbone with "
                         f"`python eval_knn.py -model={args.model} -dataset={args.dataset} -learn_framework=FOCAL`")
    emb_dim = int(dataset_config["FOCAL"]["emb_dim"])
    if emb_dim < 8 or (emb_dim // 2) % 4 or emb_dim % 2:
        raise ValueError(f"{TOOL}: FOCAL.emb_dim={emb_dim} gives shared / private halves of {emb_dim // 2} columns; the rank kernel takes "
                         "a width that is a multiple of 4: set FOCAL.emb_dim to a multiple of 8 in the dataset's YAML (every shipped "
                         "configuration uses 256) and pretrain with it")


def dataset_yaml(args):
    here = os.path.dirname(os.path.abspath(__file__))
    return getattr(args, "config", None) or os.path.join(here, "..", "data", f"{args.dataset}.yaml")


def parse_retrieval_params():
    base = parse_base_args("eval_retrieval")
    refuse_other_frameworks(base, TOOL, SCORE)  # before the device is selected
    base.retrieval_ks = refuse_retrieval_settings(base)
    refuse_dataset_shape(base, load_yaml(dataset_yaml(base)))
    base.stage = "pretrain"                     # the backbone is built as pretraining builds it: multi-location configurations included
    args = set_auto_params(base)
    args.backbone_weight = resolve_backbone_weight(args)
    refuse_classifier_checkpoint(args, args.backbone_weight, TOOL)
    return args
