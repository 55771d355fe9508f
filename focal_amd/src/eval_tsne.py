"""Entry point [build extension]: `python eval_tsne.py -model=SW_Transformer -dataset=HAR3LOC -learn_framework=FOCAL [-model_weight=PATH]
[-tsne_split=test|val|train] [-tsne_perplexity=30] [-tsne_iters=1000] [-tsne_init=pca|random] [-tsne_seed=0] [-tsne_max_rows=16384]
[-tsne_out=PATH] [-tsne_plot]`: the t-SNE map of a pretrained backbone's un-projected features, coloured by class -- the picture the FOCAL
paper draws of its frozen features, and the first thing to open when eval_knn.py's number looks wrong.  The exact method with sklearn's
defaults (train_utils/tsne.py: GpuTSNE; no Barnes-Hut approximation, at most 32 768 rows, a larger split is cut to a seeded subset); the
map and everything needed to redraw it go to an .npz, with -tsne_plot also to a PNG.  The checkpoint, the way the backbone is built and
the refusals are eval_knn.py's; two runs on one checkpoint write the same bytes.  Transductive: it maps the rows it is given and has no
`transform` for others."""
import io
import os
import sys
import zipfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from params.knn_params import pretraining_command, refuse_classifier_checkpoint, refuse_other_frameworks  # noqa: E402
from params.tsne_params import (SCORE, TOOL, parse_tsne_params, refuse_perplexity_for_rows, refuse_tsne_settings,  # noqa: E402
                                resolve_tsne_out)


def refuse_data_parallel():
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit(f"{TOOL} maps on one device: launch it as one process (ranks of such a job would each map the same "
                         f"checkpoint on the same split); `python {TOOL} ...` without torchrun")


def load_backbone_weight(args):
    """The checkpoint's state dict, read to host memory.  Refused: no checkpoint (nothing is mapped at a random initialisation)."""
    import torch
    path = args.backbone_weight
    if not os.path.isfile(path):
        raise FileNotFoundError(f"no backbone checkpoint at {path}: `{pretraining_command(args)}` writes it (or name the folder or the "
                                "file that holds it with -model_weight)")
    return torch.load(path, map_location="cpu")


def subset_rows(N, max_rows, seed):
    """The rows of a split of N that are mapped: all of them, or a random subset of max_rows from a generator seeded with `seed`, sorted
    (int64, host)."""
    import torch
    if N <= max_rows:
        return torch.arange(N)
    gen = torch.Generator().manual_seed(int(seed))
    return torch.randperm(N, generator=gen)[:max_rows].sort().values


def write_npz(path, arrays):
    """numpy's .npz layout (np.load reads it) with fixed member timestamps: the same arrays give the same bytes."""
    import numpy as np
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:
        for name, value in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(value), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue())


def plot_embedding(path, embedding, labels, class_names=None, title=None):
    """A scatter of the map coloured by class, written as a PNG on the Agg backend."""
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    import numpy as np
    embedding, labels = np.asarray(embedding), np.asarray(labels)
    fig, ax = plt.subplots(figsize=(7, 6), dpi=120)
    classes = np.unique(labels)
    cmap = plt.get_cmap("tab10" if len(classes) <= 10 else "tab20")
    for k, c in enumerate(classes):
        rows = labels == c
        name = class_names[int(c)] if class_names is not None and 0 <= int(c) < len(class_names) else str(int(c))
        ax.scatter(embedding[rows, 0], embedding[rows, 1], s=6, color=cmap(k % cmap.N), label=str(name), linewidths=0)
    ax.legend(markerscale=2.5, fontsize=8, loc="best")
    ax.set_xticks([])
    ax.set_yticks([])
    if title:
        ax.set_title(title, fontsize=9)
    fig.savefig(path, format="png", metadata={"Software": None})
    plt.close(fig)
    return path


def evaluate_tsne(args, keep=False):
    """Map the chosen split of `args.backbone_weight`; returns {"kl": KL(P || Q) of the map, "n": rows mapped, "path": the .npz}.
    keep=True: also, as a second value, {"features", "labels", "rows": the tensors that were mapped, "estimator": the GpuTSNE}."""
    refuse_data_parallel()
    refuse_other_frameworks(args, TOOL, SCORE)
    refuse_tsne_settings(args)
    refuse_classifier_checkpoint(args, args.backbone_weight, TOOL)
    state_dict = load_backbone_weight(args)
    import numpy as np
    from data_augmenter.Augmenter import Augmenter
    from eval_knn import split_features
    from input_utils.multi_modal_dataloader import create_dataloader
    from train_utils.model_selection import init_backbone_model
    from train_utils.tsne import GpuTSNE
    split = getattr(args, "tsne_split", "test")
    loader = create_dataloader(split, args, batch_size=args.batch_size, workers=args.workers)
    augmenter = Augmenter(args)
    args.augmenter = augmenter
    backbone = init_backbone_model(args)
    backbone.load_state_dict(state_dict, strict=True)
    args.classifier = backbone
    backbone.eval()
    feats, labels = split_features(args, backbone, augmenter, loader)
    N = feats.shape[0]
    rows = subset_rows(N, int(getattr(args, "tsne_max_rows", 16384)), int(getattr(args, "tsne_seed", 0)))
    n = rows.numel()
    if n < N:
        print(f"t-SNE maps {n} of {N} rows of the {split} split (seed {int(getattr(args, 'tsne_seed', 0))})")
        pick = rows.to(feats.device)
        feats, labels = feats[pick].contiguous(), labels[pick].contiguous()
    perplexity = float(getattr(args, "tsne_perplexity", 30.0))
    refuse_perplexity_for_rows(perplexity, n, split)
    # (the fused form, not fit(fused=False): profiles/tsne_fused.txt)
    estimator = GpuTSNE(perplexity=perplexity, n_iter=int(getattr(args, "tsne_iters", 1000)), init=getattr(args, "tsne_init", "pca"),
                        seed=int(getattr(args, "tsne_seed", 0))).fit(feats)
    kl = estimator.kl_divergence_
    print(f"t-SNE (perplexity={perplexity:g}, n={n}, iterations={estimator.n_iter_}) KL divergence: {kl: .5f}")
    path = getattr(args, "tsne_out", None) or resolve_tsne_out(args)
    embedding, host_labels = estimator.embedding_.cpu().numpy(), labels.cpu().numpy()
    write_npz(path, {"embedding": embedding.astype(np.float32), "labels": host_labels, "rows": rows.numpy(),
                     "betas": estimator.betas_.cpu().numpy(), "kl": np.float64(kl), "perplexity": np.float64(perplexity),
                     "n_iter": np.int64(estimator.n_iter_)})
    print(f"t-SNE map written to {path}")
    out = {"kl": kl, "n": n, "path": path}
    if getattr(args, "tsne_plot", False):
        names = args.dataset_config.get(args.task, {}).get("class_names") if isinstance(args.dataset_config.get(args.task), dict) else None
        out["plot"] = plot_embedding(os.path.splitext(path)[0] + ".png", embedding, host_labels, class_names=names,
                                     title=f"{args.dataset} {args.model} {split}: t-SNE, perplexity {perplexity:g}, KL {kl:.3f}")
        print(f"t-SNE plot written to {out['plot']}")
    kept = {"features": feats, "labels": labels, "rows": rows, "estimator": estimator}
    return (out, kept) if keep else out


def main_eval_tsne():
    refuse_data_parallel()
    evaluate_tsne(parse_tsne_params())


if __name__ == "__main__":
    main_eval_tsne()
