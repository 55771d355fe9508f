"""Entry point: `python test.py -model=DeepSense -dataset=MOD -learn_framework=no [-stage=finetune] [-model_weight=PATH]`
(reference: src/test.py:16-58): loss, accuracy, macro-F1 and confusion matrix of a saved classifier on the test split.  The
checkpoint is the `*_best.pt` of the matching `train.py` run (params/test_params.py: resolve_classifier_weight); one process, the
first listed device."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from params.test_params import parse_test_params, refuse_pretrain_stage  # noqa: E402


def refuse_data_parallel():
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit("test.py evaluates on one device: launch it as one process (ranks of such a job would each score the same "
                         "checkpoint on the same test split)")


def training_command(args):
    stage = " -stage=finetune" if args.learn_framework == "FOCAL" else ""
    return f"python train.py -model={args.model} -dataset={args.dataset} -learn_framework={args.learn_framework}{stage}"


def load_classifier_weight(args):
    """The checkpoint's state dict, loaded once.  Refused: what would score a randomly initialised class layer -- no checkpoint, or
    one without class-layer tensors (which load_model_weight would skip without a word)."""
    import torch
    path = args.classifier_weight
    if not os.path.isfile(path):
        raise FileNotFoundError(f"no classifier checkpoint at {path}: `{training_command(args)}` writes it (or name the folder or "
                                "the file that holds it with -model_weight)")
    state = torch.load(path, map_location=args.device)
    if not any(k.startswith("class_layer.") for k in state):
        raise ValueError(f"{path} holds no class_layer.* tensor (a pretraining checkpoint?): its classifier would be scored at its "
                         f"random initialisation; evaluate what `{training_command(args)}` writes")
    return state


def test(args):
    """Evaluate `args.classifier_weight` on the test split; returns (loss, accuracy, macro-F1)."""
    refuse_data_parallel()
    refuse_pretrain_stage(args)
    state = load_classifier_weight(args)
    from general_utils.weight_utils import load_model_weight
    from input_utils.multi_modal_dataloader import create_dataloader
    from models.loss import CrossEntropyLoss
    from train_utils.eval_functions import eval_supervised_model
    from train_utils.model_selection import init_backbone_model
    test_dataloader = create_dataloader("test", args, batch_size=args.batch_size, workers=args.workers)
    from data_augmenter.Augmenter import Augmenter
    augmenter = Augmenter(args)
    args.augmenter = augmenter
    classifier = init_backbone_model(args)
    classifier = load_model_weight(args, classifier, state, load_class_layer=True)
    args.classifier = classifier
    test_loss, test_metrics = eval_supervised_model(args, classifier, augmenter, test_dataloader, CrossEntropyLoss())
    print(f"Test classifier loss: {test_loss: .5f}")
    print(f"Test acc: {test_metrics[0]: .5f}, test f1: {test_metrics[1]: .5f}")
    print(f"Test confusion matrix:\n {test_metrics[2]}")
    return test_loss, test_metrics[0], test_metrics[1]


def main_test():
    refuse_data_parallel()
    test(parse_test_params())


if __name__ == "__main__":
    main_test()
