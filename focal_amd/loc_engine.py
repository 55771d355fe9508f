"""Location fusion of SW_Transformer on a multi-location dataset, per modality, as one autograd node (reference:
models/SW_Transformer.py:126-150 construction, :226-242 forward; models/FusionModules.py:61-140).

The L encoders of a modality (one per location) give [N, E] features each (N = 2B: both views share one pass).  In location order they
form N sequences of L tokens that run through `loc_block_num` nn.TransformerEncoderLayer(E, loc_head_num, dim_feedforward=E,
dropout=p, batch_first=True) -- torch defaults: post-norm, ReLU, eps 1e-5 -- and one TransformerFusionBlock (LayerNorm, the mean of
the L tokens as the single query of nn.MultiheadAttention over them), giving [N, E] for the projector.

Per encoder layer (R = N*L rows, fp32 activations):
  forward   qkv = x Win^T + b . o, P, W = attention core (focal_loc_attn_fwd: softmax(q k^T / 8), dropout on the weights) .
            y1 = x + drop1(o Wout^T + b) (residual epilogue) . x1 = LN1(y1) . r = relu(x1 W1^T + b) . h = drop(r) .
            y2 = x1 + drop2(h W2^T + b) . x2 = LN2(y2)                                    7 launches, 8 with dropout on
  backward  LN2 (and the drop2 mask of its output) . dW2 . dh (relu mask from h) . drop . dW1 . dx1 . + residual . LN1 . dWout, do
            (drop1 mask in the GEMM loader) . dqkv (focal_loc_attn_bwd) . dWin . dx . + residual               13 launches, 14
The fusion block (head_engine.FusionBlock): LN . mean . q / kv projections . focal_fusion_attn_fwd . out_proj -- 6 launches;
backward 9.  With the stack, 60 launches per modality and step with dropout on (kernel trace: profiles/multiloc_loc_stage_kernel_stats.csv).
The stage input is ONE stack copy of the L features (focal_loc_stack: the split-K mod_in GEMMs write a plain [N, E] row block);
the last residual add of the backward pass writes the L input gradients location-major (focal_loc_unstack_add), each a contiguous
[N, E] block handed to its encoder as is.

The GEMMs multiply fp32 operands in both compute modes: the bf16 GEMM family has no fp32-activation residual epilogue (an extra cast
launch per product would be needed), and at R = 1 536 rows the products run on small grids.  The stage itself then adds no bf16
rounding: the bf16 step's deviation from the reference is the six bf16 encoders' (DESIGN, location fusion).

Dropout masks come from the device counter RNG (the same `rng_state` words as every Swin / fusion site) with a stream id per
(view, modality, layer, site), in a range of its own (LOC_STREAM_BASE): no two sites share a mask, and a captured replay draws fresh
masks every step because the seed word advances on the device.
"""
import torch

from . import ops
from ._lib import ACT_RELU_OUT, EPI_NONE, EPI_RELU, EPI_RESIDUAL
from .head_engine import FusionBlock, lin, lin_bwd

LOC_STREAM_BASE = 0x40000000  # above every Swin / DeepSense stream id ((view * 8 + encoder) * 64 + block) * 8 + site < 2^28)
SITE_ATTN, SITE_DROP1, SITE_HIDDEN, SITE_DROP2 = range(4)
FUSION_LAYER = 7              # the fusion block's "layer" in the stream id: encoder layers are 0 .. 6
LOC_MAX_L = 8


class LocFusionStage:
    def __init__(self, backbone, mod, mod_index):
        cfg = backbone.config
        self.bb, self.mod, self.mi = backbone, mod, mod_index
        self.L = len(backbone.locations)
        self.E = cfg["loc_out_channels"]
        self.heads = cfg["loc_head_num"]
        self.blocks = cfg["loc_block_num"]
        self.p = float(cfg["dropout_ratio"])
        if not (2 <= self.L <= LOC_MAX_L and self.E == 64 * self.heads and self.E <= 256 and 1 <= self.blocks < FUSION_LAYER):
            raise NotImplementedError(f"location fusion covers 2..{LOC_MAX_L} locations, loc_out_channels = 64 * loc_head_num <= 256 and "
                                      f"1 <= loc_block_num < {FUSION_LAYER} (got L={self.L} E={self.E} heads={self.heads} "
                                      f"blocks={self.blocks})")
        self.ctx = f"loc_context_layers.{mod}"
        self.fusion = FusionBlock(backbone, f"loc_fusion_layer.{mod}", self.heads, fp32_operands=True)

    def stream_id(self, view, layer, site):
        return LOC_STREAM_BASE + ((((view & 0xFFFF) * 8 + self.mi) * 8 + layer) * 8 + site)

    # ------------------------------------------------------------------------------------------------ forward
    def forward(self, feats, view, training):
        """feats: L fp32 [N, E] features in location order -> (fused [N, E] fp32, saved state for backward)."""
        ar = self.bb.arena()
        L, E, H = self.L, self.E, self.heads
        N = feats[0].shape[0]
        R = N * L
        dev = feats[0].device
        p = self.p if training else 0.0
        rng = self.bb.rng_state() if p > 0 else None
        W, f32 = ar.master, ops.code(torch.float32)
        xs = torch.empty(N, L, E, dtype=torch.float32, device=dev)
        ops.loc_stack([f if f.dtype == torch.float32 and f.is_contiguous() else f.float().contiguous() for f in feats], xs)
        x = xs.view(R, E)
        layers = []
        for li in range(self.blocks):
            pre = f"{self.ctx}.{li}"
            qkv, d_qkv = lin(f32, x, W(f"{pre}.self_attn.in_proj_weight"), W(f"{pre}.self_attn.in_proj_bias"))
            o = torch.empty(R, E, dtype=torch.float32, device=dev)
            probs = torch.empty(N, H, L, L, dtype=torch.float32, device=dev)
            weights = torch.empty_like(probs)
            ops.loc_attn_fwd(N, L, E, H, qkv, o, probs, weights, rng, self.stream_id(view, li, SITE_ATTN), p)
            drop1 = ops.drop_desc(rng, self.stream_id(view, li, SITE_DROP1), p) if p > 0 else None
            y1, d_o = lin(f32, o, W(f"{pre}.self_attn.out_proj.weight"), W(f"{pre}.self_attn.out_proj.bias"), EPI_RESIDUAL, x, drop1)
            x1, st1 = ops.layernorm_fwd(y1, W(f"{pre}.norm1.weight"), W(f"{pre}.norm1.bias"), torch.float32)
            F = ar.index[f"{pre}.linear1.weight"][2][0]
            r, _ = lin(f32, x1, W(f"{pre}.linear1.weight"), W(f"{pre}.linear1.bias"), EPI_RELU)
            h = ops.dropout(r, rng, self.stream_id(view, li, SITE_HIDDEN), p) if p > 0 else r
            drop2 = ops.drop_desc(rng, self.stream_id(view, li, SITE_DROP2), p) if p > 0 else None
            y2, d_2 = lin(f32, h, W(f"{pre}.linear2.weight"), W(f"{pre}.linear2.bias"), EPI_RESIDUAL, x1, drop2)
            x2, st2 = ops.layernorm_fwd(y2, W(f"{pre}.norm2.weight"), W(f"{pre}.norm2.bias"), torch.float32)
            layers.append(dict(x=x, qkv=qkv, d_qkv=d_qkv, o=o, probs=probs, weights=weights, d_o=d_o, y1=y1, st1=st1, x1=x1, h=h, F=F,
                               d_2=d_2, drop2=drop2, y2=y2, st2=st2))
            x = x2
        # TransformerFusionBlock: LayerNorm, query = mean of the L normalised tokens, nn.MultiheadAttention over them (head_engine.FusionBlock)
        y, fs = self.fusion.forward(x, N, L, p, rng, self.stream_id(view, FUSION_LAYER, SITE_ATTN))
        saved = dict(N=N, R=R, rng=rng, p=p, view=view, layers=layers, fusion=fs)
        return y, saved

    # ------------------------------------------------------------------------------------------------ backward
    def backward(self, sv, dy):
        """dy [N, E] -> the L input gradients ([N, E] each, contiguous views of one [L, N, E] buffer); parameter gradients accumulate
        into the arena."""
        ar = self.bb.arena()
        L, E, H = self.L, self.E, self.heads
        N, R, rng, p, view = sv["N"], sv["R"], sv["rng"], sv["p"], sv["view"]
        W, G = ar.master, ar.g
        dev = dy.device
        f32 = ops.code(torch.float32)
        g = self.fusion.backward(sv["fusion"], dy)
        grads = None
        for li in reversed(range(self.blocks)):
            s, pre = sv["layers"][li], f"{self.ctx}.{li}"
            # x2 = LN2(y2), y2 = x1 + drop2(h W2^T + b2): dy2 feeds the residual, dy2 * mask2 the product
            dy2 = torch.empty(R, E, dtype=torch.float32, device=dev)
            gm = torch.empty_like(dy2) if s["drop2"] is not None else None
            ops.layernorm_bwd(g, s["y2"], s["st2"], W(f"{pre}.norm2.weight"), dy2, False, G(f"{pre}.norm2.weight"), G(f"{pre}.norm2.bias"),
                              dx_masked=gm, mask=s["drop2"])
            gm = dy2 if gm is None else gm
            F = s["F"]
            d2 = ops.linear_desc(f32, R, E, F, f32, f32, ACT_RELU_OUT, EPI_NONE)
            ops.linear_bwd_weight(d2, gm, s["h"], G(f"{pre}.linear2.weight"), G(f"{pre}.linear2.bias"))
            dh = torch.empty(R, F, dtype=torch.float32, device=dev)
            ops.linear_bwd_data(d2, gm, W(f"{pre}.linear2.weight"), s["h"], dh)  # zero where h = 0: relu off or dropped
            dz = ops.dropout(dh, rng, self.stream_id(view, li, SITE_HIDDEN), p) if p > 0 else dh  # x mask: 1 / (1 - p) where kept
            d1 = ops.linear_desc(f32, R, F, E, f32, f32)
            t = lin_bwd(d1, dz, s["x1"], W(f"{pre}.linear1.weight"), G(f"{pre}.linear1.weight"), G(f"{pre}.linear1.bias"))
            ops.axpy(1.0, dy2, t)  # + the residual path around the feed-forward block
            dy1 = torch.empty(R, E, dtype=torch.float32, device=dev)
            ops.layernorm_bwd(t, s["y1"], s["st1"], W(f"{pre}.norm1.weight"), dy1, False, G(f"{pre}.norm1.weight"), G(f"{pre}.norm1.bias"))
            # y1 = x + drop1(o Wout^T + b): the residual-epilogue descriptor masks dy1 in the GEMM loaders
            do = lin_bwd(s["d_o"], dy1, s["o"], W(f"{pre}.self_attn.out_proj.weight"), G(f"{pre}.self_attn.out_proj.weight"),
                         G(f"{pre}.self_attn.out_proj.bias"))
            dqkv = torch.empty(R, 3 * E, dtype=torch.float32, device=dev)
            ops.loc_attn_bwd(N, L, E, H, s["qkv"], s["probs"], s["weights"], do, dqkv)
            tx = lin_bwd(s["d_qkv"], dqkv, s["x"], W(f"{pre}.self_attn.in_proj_weight"), G(f"{pre}.self_attn.in_proj_weight"),
                         G(f"{pre}.self_attn.in_proj_bias"))
            if li > 0:
                ops.axpy(1.0, dy1, tx)
                g = tx
            else:
                grads = torch.empty(L, N, E, dtype=torch.float32, device=dev)
                ops.loc_unstack_add(dy1.view(N, L, E), tx.view(N, L, E), list(grads))
        return list(grads)
