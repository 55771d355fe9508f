"""Parameters of `eval_linear.py` [build extension]: the checkpoint is resolved and refused as `eval_knn.py`'s is (params/knn_params.py);
the regularisation grid is settled here, before anything is built."""
import math

from params.base_params import parse_base_args
from params.knn_params import refuse_classifier_checkpoint, refuse_other_frameworks, resolve_backbone_weight
from params.params_util import set_auto_params

TOOL = "eval_linear.py"
SCORE = "the linear-probe accuracy of its features"
MAX_L2 = 16  # problems of one fit: 16 x 64 classes is focal_probe_forward's limit on the weight rows (include/focal_hip.h)
DEFAULT_L2 = "1e-4,1e-3,1e-2,1e-1"


def parse_probe_l2(text):
    """`-probe_l2` as a tuple of positive floats.  Refused: an empty list or entry, a value that is no number, not positive or not finite,
    more than MAX_L2 values."""
    if isinstance(text, (tuple, list)):
        values = [float(v) for v in text]
    else:
        fields = [f.strip() for f in str(text if text is not None else "").split(",")]
        if not fields or any(f == "" for f in fields):
            raise ValueError(f"{TOOL}: -probe_l2 is a comma list of positive strengths with no empty entry (got {text!r}); the default is "
                             f"-probe_l2={DEFAULT_L2}")
        try:
            values = [float(f) for f in fields]
        except ValueError:
            raise ValueError(f"{TOOL}: -probe_l2 is a comma list of positive strengths (got {text!r}); the default is "
                             f"-probe_l2={DEFAULT_L2}") from None
    if not values:
        raise ValueError(f"{TOOL}: -probe_l2 is a comma list of positive strengths with no empty entry (got {text!r}); the default is "
                         f"-probe_l2={DEFAULT_L2}")
    for v in values:
        if math.isnan(v) or math.isinf(v) or not v > 0:
            raise ValueError(f"{TOOL}: every -probe_l2 strength is positive and finite (got {v!r} in {text!r}): the unregularised problem has "
                             f"no minimum on separable features; use a small strength such as -probe_l2=1e-6")
    if len(values) > MAX_L2:
        raise ValueError(f"{TOOL}: at most {MAX_L2} -probe_l2 strengths fit one pass (got {len(values)}): run the grid in parts of {MAX_L2}")
    return tuple(values)


def refuse_probe_settings(args):
    """Returns the parsed grid."""
    l2 = parse_probe_l2(getattr(args, "probe_l2", DEFAULT_L2))
    max_iter, tol = int(getattr(args, "probe_max_iter", 200)), float(getattr(args, "probe_tol", 1e-5))
    if max_iter < 1 or not tol >= 0:
        raise ValueError(f"{TOOL}: need -probe_max_iter >= 1 and -probe_tol >= 0 (got {max_iter}, {tol})")
    return l2


def parse_linear_params():
    base = parse_base_args("eval_linear")
    refuse_other_frameworks(base, TOOL, SCORE)  # before the device is selected
    l2 = refuse_probe_settings(base)
    base.stage = "pretrain"                     # the backbone is built as pretraining builds it: multi-location configurations included
    args = set_auto_params(base)
    args.backbone_weight = resolve_backbone_weight(args)
    refuse_classifier_checkpoint(args, args.backbone_weight, TOOL)
    args.probe_l2_values = l2
    return args
