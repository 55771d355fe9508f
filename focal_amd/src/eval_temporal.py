"""Entry point [build extension]: `python eval_temporal.py -model=SW_Transformer -dataset=HAR3LOC -learn_framework=FOCAL
[-model_weight=PATH] [-temporal_split=test|val|train] [-temporal_margin=M] [-temporal_k=1,5,10] [-temporal_max_rows=65536]
[-temporal_seed=0]`: does a saved FOCAL backbone satisfy the loss's temporal constraint on held-out data?  The loss's fourth term
(models/loss.py: forward_temporal_inter_ranking_loss) asks that the windows of one subsequence lie closer to each other than to the
windows of any other subsequence, by `inter_rank_margin`; during training only the step's batch sees it.  Here every subsequence of the
split is ranked against every other one: the term's own value over the whole split, the share of ordered pairs of subsequences whose
hinge is inactive, the share that is ordered at all, the mean distances within and across subsequences, and per window where its nearest
sibling lands among all other windows (recall@k, MRR, median rank).  Scored: each modality's full projected embedding, un-normalised, as
the loss reads it, and the un-projected features.  No label is read and no file is written.  The checkpoint, the way the backbone is built
and the refusals are eval_knn.py's; one process; two runs on one checkpoint print the same numbers."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from params.knn_params import pretraining_command, refuse_classifier_checkpoint, refuse_other_frameworks  # noqa: E402
from params.temporal_params import (SCORE, TOOL, parse_temporal_params, refuse_dataset_shape,  # noqa: E402
                                    refuse_temporal_settings)

# (the form sequence_ranking takes here, by the measurement in profiles/temporal_fused.txt)
FUSED = True


def refuse_data_parallel():
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit(f"{TOOL} ranks on one device: launch it as one process (ranks of such a job would each score the same "
                         f"checkpoint on the same split); `python {TOOL} ...` without torchrun")


def load_backbone_weight(args):
    """The checkpoint's state dict, read to host memory.  Refused: no checkpoint (nothing is scored at a random initialisation)."""
    import torch
    path = args.backbone_weight
    if not os.path.isfile(path):
        raise FileNotFoundError(f"no backbone checkpoint at {path}: `{pretraining_command(args)}` writes it (or name the folder or the "
                                "file that holds it with -model_weight)")
    return torch.load(path, map_location="cpu")


def subset_sequences(N, seq_len, max_rows, seed):
    """The rows of a split of N = S seq_len that are scored: all of them, or the rows of a random subset of max_rows // seq_len WHOLE
    subsequences from a generator seeded with `seed`, sorted (int64, host)."""
    import torch
    from eval_tsne import subset_rows
    L = int(seq_len)
    if N % L:
        raise ValueError(f"{TOOL}: {N} rows are not whole subsequences of {L} windows")
    seqs = subset_rows(N // L, int(max_rows) // L, seed)
    return (seqs[:, None] * L + torch.arange(L)[None, :]).reshape(-1)


def seeded_pass(seed, fn, *a):
    """fn(*a) with Python's generator seeded (the file-backed sequence sampler shuffles with it, and the float sums of a sequence depend
    on the order of the others in their last bits), and the generator's state put back afterwards."""
    import random
    state = random.getstate()
    random.seed(int(seed))
    try:
        return fn(*a)
    finally:
        random.setstate(state)


def evaluate_temporal(args, keep=False):
    """Score `args.backbone_weight`; returns {"n", "N", "seq_len", "margin", "temporal": {name: temporal_metrics + "D"}, "neighbours":
    {name: retrieval_metrics}, "chance": {k: k / (n - 1)}} with name = each modality and "features".  keep=True: also, as a second value,
    {"scored": {name: [n, D]}, "ranking": {name: sequence_ranking's tensors}, "ranks" / "tied" / "pos": {name: int64 [n]}} -- the very
    tensors that were scored."""
    refuse_data_parallel()
    refuse_other_frameworks(args, TOOL, SCORE)
    ks = refuse_temporal_settings(args)
    refuse_dataset_shape(args, args.dataset_config)
    refuse_classifier_checkpoint(args, args.backbone_weight, TOOL)
    state_dict = load_backbone_weight(args)
    from data_augmenter.Augmenter import Augmenter
    from eval_knn import split_features
    from eval_retrieval import split_projections
    from input_utils.multi_modal_dataloader import create_dataloader
    from train_utils.model_selection import init_backbone_model
    from train_utils.retrieval import retrieval_metrics
    from train_utils.temporal import neighbour_ranks, sequence_ranking, temporal_metrics
    split = getattr(args, "temporal_split", "test")
    seed = int(getattr(args, "temporal_seed", 0))
    L = int(args.dataset_config["seq_len"])
    margin = getattr(args, "temporal_margin", None)
    margin = float(args.dataset_config["FOCAL"]["inter_rank_margin"] if margin is None else margin)
    if not (getattr(args, "sequence_sampler", False) and args.stage == "pretrain"):
        raise ValueError(f"{TOOL}: the loader yields whole subsequences at stage pretrain with the sequence sampler on only (got "
                         f"stage={args.stage}, sequence_sampler={getattr(args, 'sequence_sampler', False)}): parse the arguments with "
                         "params/temporal_params.py: parse_temporal_params")
    loader = create_dataloader(split, args, batch_size=args.batch_size, workers=args.workers)
    augmenter = Augmenter(args)
    args.augmenter = augmenter
    backbone = init_backbone_model(args)
    backbone.load_state_dict(state_dict, strict=True)
    args.classifier = backbone
    backbone.eval()
    # every loader kind yields batches of whole subsequences (the synthetic one whole multiples of seq_len rows, the packed and the
    # file-backed one the sampler's subsequences, the last one padded by repeating its final sample): rows k L .. k L + L - 1 of the
    # concatenated split are one subsequence, in either pass
    feats, _ = seeded_pass(seed, split_features, args, backbone, augmenter, loader)
    proj, _ = seeded_pass(seed, split_projections, args, backbone, augmenter, loader)
    mods = list(args.dataset_config["modality_names"])
    scored = {m: proj[m].float().contiguous() for m in mods}
    scored["features"] = feats.float().contiguous()
    N = scored["features"].shape[0]
    if N % L or any(z.shape[0] != N for z in scored.values()):
        raise ValueError(f"{TOOL}: the {split} split came as {N} rows, which are not whole subsequences of seq_len={L} windows: the "
                         "loader did not batch by subsequence")
    rows = subset_sequences(N, L, int(getattr(args, "temporal_max_rows", 65536)), seed)
    n = rows.numel()
    if n < N:
        print(f"Temporal scores {n} of {N} rows of the {split} split ({n // L} whole subsequences, seed {seed})")
        pick = rows.to(scored["features"].device)
        scored = {name: z[pick].contiguous() for name, z in scored.items()}
    if n < 2 * L:
        raise ValueError(f"{TOOL}: the {split} split has {n // L} subsequence; the constraint ranks one against another: score a larger "
                         "split with -temporal_split")
    out = {"n": n, "N": N, "seq_len": L, "margin": margin, "temporal": {}, "neighbours": {},
           "chance": {k: min(k, n - 1) / (n - 1) for k in ks}}
    kept = {"scored": scored, "ranking": {}, "ranks": {}, "tied": {}, "pos": {}}
    for name in mods + ["features"]:
        z = scored[name]
        rank = kept["ranking"][name] = sequence_ranking(z, L, margin, fused=FUSED)
        t = out["temporal"][name] = dict(temporal_metrics(rank, L), D=z.shape[1])
        print(f"Temporal [{name}] (split={split}, sequences={t['sequences']}, seq_len={L}, D={z.shape[1]}): ranking loss "
              f"{t['ranking_loss']:.5f} (margin {margin:g}), margin satisfied {t['margin_satisfied']:.5f}, ordered {t['ordered']:.5f}, "
              f"mean intra {t['mean_intra']:.5f}, mean inter {t['mean_inter']:.5f}, ratio {t['ratio']:.5f}")
        ranks, tied, pos = neighbour_ranks(z, L, rank["intra_d2"])
        kept["ranks"][name], kept["tied"][name], kept["pos"][name] = ranks, tied, pos
        m = out["neighbours"][name] = retrieval_metrics(ranks, tied, ks)
        recalls = ", ".join(f"R@{k} {m['recall'][k]:.5f}" for k in ks)
        print(f"Temporal neighbours [{name}] (n={n}): {recalls}, MRR {m['mrr']:.5f}, median rank {m['median_rank']:.1f}")
    print("chance: " + ", ".join(f"R@{k} = {min(k, n - 1)} / {n - 1} = {out['chance'][k]:.5f}" for k in ks))
    return (out, kept) if keep else out


def main_eval_temporal():
    refuse_data_parallel()
    evaluate_temporal(parse_temporal_params())


if __name__ == "__main__":
    main_eval_temporal()
