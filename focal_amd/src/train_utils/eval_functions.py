"""Validation (reference: train_utils/eval_functions.py:10-137): under pretraining the mean pretraining loss plus accuracy /
macro-F1 / confusion matrix of the KNN estimator on the backbone features; under finetuning the classifier's own loss and metrics."""
import logging

import numpy as np
import torch
from sklearn.metrics import accuracy_score, confusion_matrix, f1_score

from train_utils.knn import extract_sample_features
from train_utils.loss_calc_utils import calc_pretrain_loss

from focal_amd import ops  # noqa: E402  (train_utils.knn has put the repository root on sys.path)


def eval_task_metrics(args, labels, predictions):
    if args.task in {"distance_classification", "speed_classification"}:
        num_classes = args.dataset_config[args.task]["num_classes"]
        mean_acc = 1 - (np.abs(labels - predictions) / np.maximum(labels, (num_classes - 1) - labels))
        mean_acc = np.nan_to_num(mean_acc, nan=1.0).mean()
    else:
        mean_acc = accuracy_score(labels, predictions)
    mean_f1 = f1_score(labels, predictions, average="macro", zero_division=1)
    try:
        conf = confusion_matrix(labels, predictions)
    except Exception:  # noqa: BLE001
        conf = []
    return mean_acc, mean_f1, conf


def metrics_from_confusion(args, conf):
    """`eval_task_metrics` from the confusion matrix alone (conf[label, prediction] counts over ALL classes of the task, pure numpy):
    the classes that count are the ones seen as a label or as a prediction -- sklearn's sorted union --, macro-F1 is taken over them
    and the returned matrix is `conf` restricted to them."""
    conf = np.asarray(conf, dtype=np.int64)
    total = conf.sum()
    true_sum, pred_sum, tp = conf.sum(axis=1), conf.sum(axis=0), np.diag(conf)
    if args.task in {"distance_classification", "speed_classification"}:
        num_classes = args.dataset_config[args.task]["num_classes"]
        lab = np.arange(conf.shape[0], dtype=np.float64)[:, None]
        pred = np.arange(conf.shape[1], dtype=np.float64)[None, :]
        with np.errstate(divide="ignore", invalid="ignore"):
            cell = 1 - (np.abs(lab - pred) / np.maximum(lab, (num_classes - 1) - lab))
        mean_acc = float((np.nan_to_num(cell, nan=1.0) * conf)[conf > 0].sum() / total)
    else:
        mean_acc = float(tp.sum() / total)
    seen = np.flatnonzero(true_sum + pred_sum)
    mean_f1 = float(np.average(2.0 * tp[seen] / (true_sum[seen] + pred_sum[seen])))  # (zero_division never applies to a seen class)
    return mean_acc, mean_f1, conf[np.ix_(seen, seen)]


def clustering_scores(conf, n_classes, n_clusters):
    """(adjusted Rand index, normalised mutual information) of a clustering against the class labels, from the integer contingency
    matrix alone: conf[label, cluster] counts, of which the leading [n_classes, n_clusters] block is read (ops.EvalState's matrix is
    square, max(n_classes, n_clusters) wide).  float64 on the host; empty rows and columns are allowed.  sklearn's conventions
    (adjusted_rand_score; normalized_mutual_info_score with its default arithmetic-mean normalisation): ARI from the pair counts, 1.0
    when no pair is split either way; NMI 1.0 when one class meets one cluster (or there is no row), 0.0 when the mutual information
    is 0."""
    m = np.asarray(conf, dtype=np.int64)[:int(n_classes), :int(n_clusters)]
    n = int(m.sum())
    n_c, n_k = m.sum(axis=1), m.sum(axis=0)
    # pairs: together in both (tp), in the clustering only (fp), in the classes only (fn), in neither (tn) -- exact integers
    sum_sq = int((m.astype(object) ** 2).sum()) if m.size else 0
    tp = sum_sq - n
    fp = int((n_k.astype(object) ** 2).sum()) - sum_sq
    fn = int((n_c.astype(object) ** 2).sum()) - sum_sq
    tn = n * n - fp - fn - sum_sq
    if fn == 0 and fp == 0:
        ari = 1.0
    else:
        tp, fp, fn, tn = float(tp), float(fp), float(fn), float(tn)
        ari = 2.0 * (tp * tn - fn * fp) / ((tp + fn) * (fn + tn) + (tp + fp) * (fp + tn))
    pi, pj = n_c[n_c > 0].astype(np.float64), n_k[n_k > 0].astype(np.float64)
    if pi.size == pj.size == 1 or pi.size == pj.size == 0:
        return ari, 1.0
    nzx, nzy = np.nonzero(m)
    nz = m[nzx, nzy].astype(np.float64)
    outer = n_c[nzx].astype(np.int64) * n_k[nzy].astype(np.int64)
    log_outer = -np.log(outer.astype(np.float64)) + np.log(pi.sum()) + np.log(pj.sum())
    terms = (nz / n) * (np.log(nz) - np.log(float(n))) + (nz / n) * log_outer
    terms = np.where(np.abs(terms) < np.finfo(terms.dtype).eps, 0.0, terms)
    mi = float(np.clip(terms.sum(), 0.0, None))
    if mi == 0.0:
        return ari, 0.0

    def entropy(p):
        return 0.0 if p.size == 1 else float(-np.sum((p / p.sum()) * (np.log(p) - np.log(p.sum()))))
    return ari, float(mi / (0.5 * (entropy(pi) + entropy(pj))))


def eval_supervised_model(args, classifier, augmenter, dataloader, loss_func):
    """Loss and task metrics of a classifier (reference :29-62).  Loss and confusion matrix stay on the device (ops.EvalState: one
    launch per batch, whose batch loss is `CrossEntropyLoss`'s bit for bit); the host reads them once, after the loop.
    `loss_func` is not called: it names the loss, and the one built is the project's `models.loss.CrossEntropyLoss` (mean reduction, no
    class weights, no label smoothing), which is what init_loss_func hands the finetune / supervised stages.  Anything else is refused,
    never scored as plain cross-entropy."""
    from models.loss import CrossEntropyLoss
    if not isinstance(loss_func, CrossEntropyLoss):
        raise TypeError(f"eval_supervised_model accumulates models.loss.CrossEntropyLoss on the device; {type(loss_func).__name__} is not built")
    classifier.eval()
    state = None
    with torch.no_grad():
        for time_loc_inputs, labels in dataloader:
            freq_loc_inputs, labels = augmenter.forward("no", time_loc_inputs, labels)
            logits = classifier(freq_loc_inputs)
            labels = labels.argmax(dim=1) if labels.dim() > 1 else labels
            if state is None:
                state = ops.EvalState(logits.shape[1], logits.device)
            state.add(labels.to(logits.device), logits=logits)
    if state is None:
        raise ValueError("eval_supervised_model: the loader yielded no batch")
    loss_sum, n_batches, conf = state.read()
    return loss_sum / n_batches, metrics_from_confusion(args, conf)


def eval_pretrained_model(args, default_model, estimator, augmenter, dataloader, loss_func):
    default_model.eval()
    feats, labels, losses = [], [], []
    with torch.no_grad():
        for time_loc_inputs, label in dataloader:
            labels.append(label.argmax(dim=1) if label.dim() > 1 else label)
            losses.append(calc_pretrain_loss(args, default_model, augmenter, loss_func, time_loc_inputs).detach().reshape(1))
            feats.append(extract_sample_features(args, default_model.backbone, augmenter.forward("no", time_loc_inputs)))
    if not feats:
        raise ValueError("eval_pretrained_model: the loader yielded no batch")
    predictions = estimator.predict(torch.cat(feats))
    state = ops.EvalState(args.dataset_config[args.task]["num_classes"], predictions.device)
    state.add(torch.cat(labels).to(predictions.device), preds=predictions)
    mean_loss = float(np.mean(torch.cat(losses).double().cpu().numpy()))  # the per-batch losses: one read, averaged in fp64
    return mean_loss, metrics_from_confusion(args, state.read()[2])


def val_and_logging(args, epoch, model, augmenter, val_loader, test_loader, loss_func, train_loss, estimator=None):
    if args.train_mode in {"contrastive"} and args.stage == "pretrain":
        logging.info(f"Train {args.train_mode} loss: {train_loss: .5f} \n")
    else:
        logging.info(f"Training loss: {train_loss: .5f} \n")
    if args.train_mode == "supervised" or args.stage == "finetune":
        val_loss, val_metrics = eval_supervised_model(args, model, augmenter, val_loader, loss_func)
        test_loss, test_metrics = eval_supervised_model(args, model, augmenter, test_loader, loss_func)
    else:
        val_loss, val_metrics = eval_pretrained_model(args, model, estimator, augmenter, val_loader, loss_func)
        test_loss, test_metrics = eval_pretrained_model(args, model, estimator, augmenter, test_loader, loss_func)
    logging.info(f"Val loss: {val_loss: .5f}")
    logging.info(f"Val acc: {val_metrics[0]: .5f}, val f1: {val_metrics[1]: .5f}")
    logging.info(f"Val confusion matrix:\n {val_metrics[2]} \n")
    logging.info(f"Test loss: {test_loss: .5f}")
    logging.info(f"Test acc: {test_metrics[0]: .5f}, test f1: {test_metrics[1]: .5f}")
    logging.info(f"Test confusion matrix:\n {test_metrics[2]} \n")
    return val_metrics[0], val_loss
