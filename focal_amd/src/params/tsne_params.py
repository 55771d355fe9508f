"""Parameters of `eval_tsne.py` [build extension]: the checkpoint is resolved and refused as `eval_knn.py`'s is (params/knn_params.py);
the map's settings are refused here, before anything is built."""
import importlib.util
import math
import os

from params.base_params import parse_base_args
from params.knn_params import refuse_classifier_checkpoint, refuse_other_frameworks, resolve_backbone_weight
from params.params_util import set_auto_params

TOOL = "eval_tsne.py"
SCORE = "the t-SNE map of its features"
MAX_ROWS = 32768  # focal_tsne_perplexity's limit on n (include/focal_hip.h): a row of distances is held in LDS
SPLITS = ("test", "val", "train")


def refuse_tsne_settings(args):
    """A perplexity that is not a number >= 1, no iteration, a row cap outside the kernel's range, an unknown split, and -tsne_plot
    without matplotlib -- each before a loader or a model exists."""
    perplexity = float(getattr(args, "tsne_perplexity", 30.0))
    if not math.isfinite(perplexity) or perplexity < 1:
        raise ValueError(f"{TOOL}: need a finite -tsne_perplexity >= 1 (got {perplexity}); the default is -tsne_perplexity=30")
    iters = int(getattr(args, "tsne_iters", 1000))
    if iters < 1:
        raise ValueError(f"{TOOL}: need -tsne_iters >= 1 (got {iters}); the default is -tsne_iters=1000")
    max_rows = int(getattr(args, "tsne_max_rows", 16384))
    if not 2 <= max_rows <= MAX_ROWS:
        raise ValueError(f"{TOOL}: need 2 <= -tsne_max_rows <= {MAX_ROWS} (got {max_rows}): the exact method holds a row of the [n, n] "
                         f"distance matrix in LDS; set -tsne_max_rows={MAX_ROWS} at the most (a larger split is cut to a seeded subset)")
    split = getattr(args, "tsne_split", "test")
    if split not in SPLITS:
        raise ValueError(f"{TOOL}: -tsne_split is one of {', '.join(SPLITS)} (got {split})")
    if getattr(args, "tsne_plot", False) and importlib.util.find_spec("matplotlib") is None:
        raise ValueError(f"{TOOL}: -tsne_plot draws with matplotlib, which cannot be imported here: run without -tsne_plot and plot the "
                         "`embedding` and `labels` arrays of the .npz it writes")


def refuse_perplexity_for_rows(perplexity, n, split):
    """Once the features exist: the conditional distribution of a row has n - 1 entries, so its perplexity is below n."""
    if not perplexity < n:
        raise ValueError(f"{TOOL}: -tsne_perplexity={perplexity:g} needs more than {n} rows, which is all the {split} split has: set "
                         f"-tsne_perplexity below {n} or map a larger split with -tsne_split")


def resolve_tsne_out(args):
    """`-tsne_out`, or `{dataset}_{model}_tsne_{split}.npz` in the weight folder."""
    chosen = getattr(args, "tsne_out", None)
    if chosen is not None:
        return chosen
    return os.path.join(args.weight_folder, f"{args.dataset}_{args.model}_tsne_{getattr(args, 'tsne_split', 'test')}.npz")


def parse_tsne_params():
    base = parse_base_args("eval_tsne")
    refuse_other_frameworks(base, TOOL, SCORE)  # before the device is selected
    refuse_tsne_settings(base)
    base.stage = "pretrain"                     # the backbone is built as pretraining builds it: multi-location configurations included
    args = set_auto_params(base)
    args.backbone_weight = resolve_backbone_weight(args)
    refuse_classifier_checkpoint(args, args.backbone_weight, TOOL)
    args.tsne_out = resolve_tsne_out(args)
    return args
