"""SW_Transformer backbone -- same constructor contract, forward signature, module tree and state_dict as the
reference (models/SW_Transformer.py), executed on the MI355X HIP kernels.

`forward(freq_x, class_head=False, proj_head=...)` is the FOCAL pretraining path (reference :210-268, :294-304).
The classifier path (`class_head=True`: TransformerFusionBlock over the modality tokens + class layer, reference :244-276) runs for
the finetune stage (frozen encoders, head trained) and for supervised training from scratch (gradient flows on into the encoders and
the patch embedding).  On a multi-location dataset the FOCAL pretraining path runs the reference's location fusion (:126-150,
:226-242: per modality, loc_context_layers + loc_fusion_layer over the L location features) as one HIP stage per modality
(focal_amd/loc_engine.py); the classifier path on such a dataset raises.  The section's `APE` and `in_stride` switches (reference
:184-208, :222-224) run inside the patch-embedding kernel (focal_amd/swin_engine.py, csrc/embed.hip) on every one of these paths.
"""
import os
import sys

import torch
import torch.nn as nn

_ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "..", ".."))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

from focal_amd import runtime  # noqa: E402
from focal_amd.backbone import HipBackbone, run_stage  # noqa: E402
from focal_amd.head_engine import ClassifierHead  # noqa: E402
from focal_amd.loc_engine import LocFusionStage  # noqa: E402
from focal_amd.swin_engine import ProjectorHead, SwinModEncoder  # noqa: E402
from input_utils.padding_utils import get_padded_size  # noqa: E402
from models.FusionModules import LocContextLayer, TransformerFusionBlock  # noqa: E402
from models.SwinModules import BasicLayer, PatchEmbed, PatchMerging  # noqa: E402


class SW_Transformer(HipBackbone):
    def __init__(self, args) -> None:
        super().__init__()
        self.args = args
        self.config = args.dataset_config["SW_Transformer"]
        self.modalities = args.dataset_config["modality_names"]
        self.locations = args.dataset_config["location_names"]
        self.num_segments = args.dataset_config["num_segments"]
        self.drop_rate = self.config["dropout_ratio"]
        self.attn_drop_rate = self.config["attn_drop_rate"]
        self.norm_layer = nn.LayerNorm
        # No batch statistics anywhere in this backbone: FOCAL may run both views as one batch of 2B
        # (FOCALModules.FOCAL.forward).  Measured r1: 9.48 ms (two passes on 4 streams) -> 9.12 ms (one pass, 2 streams);
        # cutting the heavier modality back into batch chunks to balance the streams was slower again (9.34 ms).
        # (one pass per view on four streams -- halved kernels, doubled launches -- cost 14 %: DESIGN 4; the switch was removed in round 4)
        self.views_share_pass = True
        self._init_hip(args)
        self.init_encoder()

    def init_encoder(self) -> None:
        cfg, dcfg = self.config, self.args.dataset_config
        if len(self.locations) * len(self.modalities) > 8:
            # the encoder index is a 3-bit field of every Swin dropout stream id (swin_engine: ((view * 8 + index) * 64 + block) * 8 + site):
            # a ninth encoder would draw the masks of the next view's first encoder
            raise NotImplementedError(f"at most 8 (location, modality) encoders (got {len(self.locations)} x {len(self.modalities)})")
        if len(self.locations) > 1 and (self.supervised or getattr(self.args, "stage", "pretrain") == "finetune"):
            raise NotImplementedError("class_head=True on a multi-location dataset needs location fusion in the classifier head "
                                      "(focal_amd/head_engine.py); only FOCAL pretraining runs it (focal_amd/loc_engine.py)")
        self.freq_interval_layers = nn.ModuleDict()
        self.patch_embed = nn.ModuleDict()
        self.absolute_pos_embed = nn.ModuleDict()
        self.mod_patch_embed = nn.ModuleDict()
        self.mod_in_layers = nn.ModuleDict()
        self.geometry, self.block_windows, self.drop_path_rates = {}, {}, {}
        c0 = cfg["time_freq_out_channels"]
        for loc in self.locations:
            self.freq_interval_layers[loc] = nn.ModuleDict()
            self.patch_embed[loc] = nn.ModuleDict()
            self.absolute_pos_embed[loc] = nn.ParameterDict()
            self.mod_in_layers[loc] = nn.ModuleDict()
            self.geometry[loc] = {}
            for mod in self.modalities:
                stride = cfg["in_stride"][mod]
                spectrum = dcfg["loc_mod_spectrum_len"][loc][mod]
                if stride < 1 or spectrum % stride != 0:
                    # (the reference's reshape [b, i, s, c] -> [b, i, s // stride, c * stride] fails on such a spectrum at the first batch)
                    raise ValueError(f"SW_Transformer.in_stride[{mod}] = {stride} does not divide loc_mod_spectrum_len[{loc}][{mod}] = {spectrum}")
                window, patch = list(cfg["window_size"][mod]), list(cfg["patch_size"]["freq"][mod])
                depths = list(cfg["time_freq_block_num"][mod])
                padded = get_padded_size((self.num_segments, spectrum // stride), window, patch, len(depths))
                pe = PatchEmbed(img_size=padded, patch_size=patch, in_chans=dcfg["loc_mod_in_freq_channels"][loc][mod] * stride,
                                embed_dim=c0, norm_layer=self.norm_layer)
                self.patch_embed[loc][mod] = pe
                grid = pe.patches_resolution
                self.absolute_pos_embed[loc][mod] = nn.Parameter(torch.zeros(1, pe.num_patches, c0))
                nn.init.trunc_normal_(self.absolute_pos_embed[loc][mod], std=0.02)
                dpr = [x.item() for x in torch.linspace(0, cfg["drop_path_rate"], sum(depths))]
                self.drop_path_rates[mod] = dpr
                layers, stages = nn.ModuleList(), []
                for i, depth in enumerate(depths):
                    res, dim = (grid[0] // 2 ** i, grid[1] // 2 ** i), c0 * 2 ** i
                    layer = BasicLayer(dim=dim, input_resolution=res, num_heads=cfg["time_freq_head_num"],
                                       window_size=list(window), depth=depth, drop=self.drop_rate,
                                       attn_drop=self.attn_drop_rate, drop_path=dpr[sum(depths[:i]):sum(depths[:i + 1])],
                                       norm_layer=self.norm_layer, downsample=PatchMerging if i < len(depths) - 1 else None)
                    layers.append(layer)
                    stages.append(dict(H=res[0], W=res[1], C=dim, depth=depth, downsample=i < len(depths) - 1))
                    for bi, blk in enumerate(layer.blocks):
                        self.block_windows[(loc, mod, i, bi)] = (*blk.window_size, *blk.shift_size)
                self.freq_interval_layers[loc][mod] = layers
                last = stages[-1]
                self.mod_in_layers[loc][mod] = nn.Linear(last["H"] * last["W"] * last["C"], cfg["loc_out_channels"])
                self.geometry[loc][mod] = dict(grid=grid, patch=patch, window=window, stages=stages,
                                               heads=cfg["time_freq_head_num"], pad_img=padded, stride=stride)
                if (spectrum // stride) // patch[1] > grid[1] or self.num_segments > grid[0]:
                    raise ValueError("padded patch grid smaller than the input")
        if len(self.locations) > 1:
            # location fusion, as the reference builds it: per modality loc_block_num encoder layers + one attention fusion block
            self.loc_context_layers = nn.ModuleDict()
            self.loc_fusion_layer = nn.ModuleDict()
            E = cfg["loc_out_channels"]
            for mod in self.modalities:
                self.loc_context_layers[mod] = nn.Sequential(*[
                    LocContextLayer(d_model=E, nhead=cfg["loc_head_num"], dim_feedforward=E, dropout=cfg["dropout_ratio"], batch_first=True)
                    for _ in range(cfg["loc_block_num"])])
                self.loc_fusion_layer[mod] = TransformerFusionBlock(E, cfg["loc_head_num"], cfg["dropout_ratio"], cfg["dropout_ratio"])
        out_dim = dcfg["FOCAL"]["emb_dim"]
        self.mod_projectors = nn.ModuleDict()
        for mod in self.modalities:
            self.mod_projectors[mod] = nn.Sequential(nn.Linear(cfg["loc_out_channels"], out_dim), nn.ReLU(),
                                                     nn.Linear(out_dim, out_dim))
        self.mod_fusion_layers = TransformerFusionBlock(cfg["loc_out_channels"], cfg["loc_head_num"],
                                                        cfg["dropout_ratio"], cfg["dropout_ratio"])
        self.sample_dim = cfg["loc_out_channels"]
        n_cls = dcfg[self.args.task]["num_classes"]
        if self.args.train_mode == "supervised" or cfg["pretrained_head"] == "linear":
            self.class_layer = nn.Sequential(nn.Linear(self.sample_dim, n_cls))
        else:
            self.class_layer = nn.Sequential(nn.Linear(self.sample_dim, cfg["fc_dim"]), nn.GELU(), nn.Linear(cfg["fc_dim"], n_cls))
        # (the encoder index keys the dropout streams: location-major, so a single-location dataset keeps index = modality index)
        M = len(self.modalities)
        self._encoders = {(loc, mod): SwinModEncoder(self, loc, mod, li * M + mi)
                          for li, loc in enumerate(self.locations) for mi, mod in enumerate(self.modalities)}
        self._loc_stages = ({mod: LocFusionStage(self, mod, mi) for mi, mod in enumerate(self.modalities)}
                            if len(self.locations) > 1 else {})
        self._heads = {mod: ProjectorHead(self, mod) for mod in self.modalities}
        self._class_head = ClassifierHead(self, "mod_fusion_layers", cfg["loc_head_num"], cfg["dropout_ratio"])

    def _run_encoders(self, freq_x, proj_head, view, dev, cur, point, view_index, views_in_batch):
        """(view_index, views_in_batch: no batch statistics here, the two views are two batches or one batch of 2B alike)"""
        loc = self.locations[0]
        out = {}
        # The heaviest modality is enqueued first: the order of enqueueing is the order of the nodes in the captured step, and what the
        # runtime dispatches first gets a head start on the stream that ends the step (audio has 2/3 of the MOD step's work).  Autograd
        # then reaches the heaviest encoder's backward pass last; that order was measured not to matter.  +1.4 % on the step
        # (profiles/r3_heavy_first_ab.txt).
        order = list(range(len(self.modalities)))
        tokens = [self.geometry[loc][m]["stages"][0]["H"] * self.geometry[loc][m]["stages"][0]["W"] for m in self.modalities]
        order.sort(key=lambda i: -tokens[i])  # (stable: equal modalities keep the configuration order)
        if self._loc_stages:
            self._forward_locations(freq_x, proj_head, view, dev, cur, point, order, out)
        for mi in (order if not self._loc_stages else ()):
            mod = self.modalities[mi]
            # stream per modality; with one backbone pass per view the two passes of a step alternate between two sets of streams so
            # that they overlap.  One pass per step (views_share_pass) always uses the same set -- the first modality stays on the
            # caller's stream: alternating there only doubled the streams every join has to wait for (-1.6 % on the step,
            # profiles/r3_encoder_streams_ab.txt)
            slot = 0 if self.views_share_pass else view % 2
            st = runtime.fork_from(dev, slot * len(self.modalities) + mi, point)
            with torch.cuda.stream(st):
                f = run_stage(self, self._encoders[(loc, mod)], freq_x[loc][mod], view, self.training)
                out[mod] = run_stage(self, self._heads[mod], f) if proj_head else f
                out[mod].record_stream(cur)
        return out

    def _forward_locations(self, freq_x, proj_head, view, dev, cur, point, order, out):
        """Multi-location dataset: the L*M encoders fork from one point, each on its own stream; a modality's location fusion waits for
        its own L encoders and runs, with the projector after it, on the caller's stream.  (Not on one of the encoders' side streams:
        a side stream joined into another side stream inside a captured step makes hipStreamEndCapture fault -- forked streams join the
        capture's origin only, docs/DESIGN_rounds_1_4.md.  The fusion stages of the M modalities are a few dozen small launches each.)"""
        M = len(self.modalities)
        for mi in order:
            mod = self.modalities[mi]
            feats = []
            for li, loc in enumerate(self.locations):
                st = runtime.fork_from(dev, li * M + mi, point)
                with torch.cuda.stream(st):
                    feats.append(run_stage(self, self._encoders[(loc, mod)], freq_x[loc][mod], view, self.training))
                if st != cur:
                    cur.wait_stream(st)  # (an event on st now: that stream carries this one encoder)
            f = run_stage(self, self._loc_stages[mod], feats, view, self.training, input_grads=True)
            out[mod] = run_stage(self, self._heads[mod], f) if proj_head else f

    def _join_features(self, feats):
        return torch.stack(feats, dim=1)  # [b, M, c] (the reference's [b, 1, M, c] with i = 1) for the modality fusion block
