"""Supervised training of a backbone from scratch (reference: train_utils/supervised_train.py:18-108; `train.py -learn_framework=no`):
every parameter goes to the optimizer, batches pass through the `fixed` augmentation pipeline (Mixup in the time domain, phase
shift after the transform -- data_augmenter/Augmenter.py), the loss is cross-entropy on `backbone(freq_x)` logits, validation every 5
epochs keeps the latest / best weights.  On the HIP path the backward runs through the classifier head (focal_amd/head_engine.py)
into the same encoder kernels pretraining uses; the patch embedding, frozen in pretraining, is trained here."""
import logging
import os
import sys

import numpy as np
import torch

from general_utils.time_utils import time_sync
from train_utils.eval_functions import val_and_logging
from train_utils.lr_scheduler import define_lr_scheduler
from train_utils.optimizer import define_optimizer, log_clip_stats

_ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "..", ".."))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)
from focal_amd.graph_step import CapturedClassifierStep  # noqa: E402


def classifier_step_form(args, augmenter, option):
    """(graph, host_draws) of a classifier stage: -no_graph launches every kernel eagerly; -host_draws (FOCAL_HOST_DRAWS=1), or a `fixed`
    pipeline the device draws do not cover, keeps the augmenter eager and host-drawn in front of the step."""
    graph = not getattr(args, "no_graph", False)
    host = bool(getattr(args, "host_draws", False)) or os.environ.get("FOCAL_HOST_DRAWS") == "1"
    if option == "fixed" and not augmenter.fixed_device_draws_supported():
        host = True
    return graph, host


def run_classifier_epoch(graphed, augmenter, train_dataloader, option, graph, host_draws, parent_step):
    """One epoch of classifier steps -> the list of their losses.  Three forms: the captured step with the augmenter inside it (device
    draws); the captured body behind the eager, host-drawn augmenter; and, with both switches, `parent_step`, the plain eager loop body.
    The loss of a step is read when the next one is about to go out (train_utils/pretrain.py's `pending`), not right behind its own."""
    losses, pending = [], None
    for time_loc_inputs, labels in train_dataloader:
        if not graph and host_draws:
            losses.append(parent_step(time_loc_inputs, labels))
            graphed.eager_steps += 1
            continue
        if host_draws:
            augmenter.static_fixed = graphed.enabled  # the captured body reads the spectra at fixed addresses
            try:
                freq_x, labels = augmenter.forward(option, time_loc_inputs, labels)
            finally:
                augmenter.static_fixed = False
            if pending is not None:
                losses.append(pending.item())
            pending = graphed(freq_x, labels)
        else:
            time_loc_inputs, labels = augmenter.move_to_target_device(time_loc_inputs, labels)
            if pending is not None:
                losses.append(pending.item())
            pending = graphed.step_from_inputs(augmenter, time_loc_inputs, labels, option)
    if pending is not None:
        losses.append(pending.item())
    return losses


def supervised_train(args, classifier, augmenter, train_dataloader, val_dataloader, test_dataloader, loss_func, num_batches):
    classifier_config = args.dataset_config[args.model]
    optimizer = define_optimizer(args, classifier.parameters())
    lr_scheduler = define_lr_scheduler(args, optimizer)
    logging.info("---------------------------Start Pretraining Classifier-------------------------------")
    start = time_sync()
    best_val_acc = 0
    best_weight = os.path.join(args.weight_folder, f"{args.dataset}_{args.model}_{args.task}_best.pt")
    latest_weight = os.path.join(args.weight_folder, f"{args.dataset}_{args.model}_{args.task}_latest.pt")
    val_epochs = 5
    epochs = getattr(args, "epochs", None) or classifier_config["lr_scheduler"]["train_epochs"]
    # the step [zero_grad -> fixed pipeline -> classifier -> cross-entropy -> backward -> AdamW] is replayed from a hipGraph once its shapes
    # have repeated, with Mixup and the phase shift drawn on the device inside it (focal_amd/graph_step.py: CapturedClassifierStep)
    graph, host_draws = classifier_step_form(args, augmenter, "fixed")
    graphed = CapturedClassifierStep(classifier, loss_func, optimizer, enabled=graph)
    logging.info(f"classifier step: {'replayed from a hipGraph' if graph else 'launched eagerly'}; fixed pipeline drawn on the "
                 f"{'host, in front of the step' if host_draws else 'device, inside the step'}")

    def parent_step(time_loc_inputs, labels):
        aug_freq_loc_inputs, labels = augmenter.forward("fixed", time_loc_inputs, labels)
        optimizer.zero_grad()  # (the reference zeroes between forward and backward; gradients accumulate in the arena only in backward)
        logits = classifier(aug_freq_loc_inputs)
        loss = loss_func(logits, labels)
        loss.backward()
        optimizer.step()
        return loss.item()

    for epoch in range(epochs):
        if epoch > 0:
            logging.info("-" * 40 + f"Epoch {epoch}" + "-" * 40)
        classifier.train()
        args.epoch = epoch
        train_loss_list = run_classifier_epoch(graphed, augmenter, train_dataloader, "fixed", graph, host_draws, parent_step)
        logging.info(f"epoch {epoch}: {graphed.replays} graph replays, {graphed.eager_steps} eager steps so far")
        log_clip_stats(optimizer, epoch)
        if epoch % val_epochs == 0:
            val_metric, val_loss = val_and_logging(args, epoch, classifier, augmenter, val_dataloader, test_dataloader, loss_func,
                                                  float(np.mean(train_loss_list)))
            torch.save(classifier.state_dict(), latest_weight)
            if val_metric > best_val_acc:
                best_val_acc = val_metric
                torch.save(classifier.state_dict(), best_weight)
        lr_scheduler.step(epoch)
    end = time_sync()
    logging.info("------------------------------------------------------------------------")
    logging.info(f"Total processing time: {(end - start): .3f} s")
    return classifier
