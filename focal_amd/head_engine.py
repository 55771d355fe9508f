"""Classifier head of the finetuning path (`backbone(freq_x, class_head=True)`), as one engine object for backbone.StageFn.

SW_Transformer (models/SW_Transformer.py:269-276): stack the per-modality features [B, M, E] -> TransformerFusionBlock
(models/FusionModules.py:61-140: LayerNorm, query = mean over the M tokens, nn.MultiheadAttention over them) -> class layer.
DeepSense (models/DeepSense.py:154-157): concatenate the features -> class layer.
Finetuning trains exactly these parameters (general_utils/weight_utils.py:61-80); the encoders run forward-only in front.
Everything here is fp32 (activations of a few hundred KB); the products run on the GEMM family with `compute` operands."""
import torch

from . import ops
from ._lib import ACT_NONE, EPI_GELU, EPI_NONE


def lin(code, x, w, b, epilogue=EPI_NONE, resid=None, drop=None):
    """y [rows, n_out] fp32 = epilogue(x w^T + b), fp32 activations, `code` operands -> (y, the product's descriptor)."""
    f32 = ops.code(torch.float32)
    d = ops.linear_desc(code, x.shape[0], w.shape[0], x.shape[1], f32, f32, ACT_NONE, epilogue, out_drop=drop)
    y = torch.empty(x.shape[0], w.shape[0], dtype=torch.float32, device=x.device)
    ops.linear_fwd(d, x, w, b, resid, y)
    return y, d


def lin_bwd(d, dy, x, w, gw, gb, need_dx=True):
    """Weight and bias gradients of lin() into gw / gb (the arena); -> dx, or None where nothing flows further."""
    ops.linear_bwd_weight(d, dy, x, gw, gb)
    if not need_dx:
        return None
    dx = torch.empty_like(x)
    ops.linear_bwd_data(d, dy, w, None, dx)
    return dx


class FusionBlock:
    """TransformerFusionBlock (models/FusionModules.py:61-140) on the HIP kernels, forward and backward: LayerNorm over the M tokens of a
    sample, query = the mean of the normalised tokens, nn.MultiheadAttention (head_dim 64) of that one query over them, out_proj.
    Shared by the classifier head (M modality tokens; `compute` operands) and the location fusion of a multi-location dataset
    (focal_amd/loc_engine.py: M = L location tokens; fp32 operands).  x [B*M, E] fp32 -> y [B, E] fp32."""

    def __init__(self, backbone, prefix, heads, fp32_operands=False):
        self.bb, self.pre, self.heads, self.fp32_operands = backbone, prefix, heads, fp32_operands

    def _code(self):
        return ops.code(torch.float32 if self.fp32_operands else self.bb.compute_dtype)

    def _w(self, ar, name):
        return ar.master(name) if self.fp32_operands else ar.operand(name)

    def forward(self, x, B, M, p_attn, rng, stream_id):
        ar, pre, E = self.bb.arena(), self.pre, x.shape[1]
        xn, st = ops.layernorm_fwd(x, ar.master(f"{pre}.norm1.weight"), ar.master(f"{pre}.norm1.bias"), torch.float32)
        qin = ops.mean_time(xn, B, M, E)
        # nn.MultiheadAttention packs W_q | W_k | W_v as in_proj_weight [3E, E]: row slices of the arena, no copies
        w_in, b_in = self._w(ar, f"{pre}.mha.in_proj_weight"), ar.master(f"{pre}.mha.in_proj_bias")
        q, d_q = lin(self._code(), qin, w_in[:E], b_in[:E])
        kv, d_kv = lin(self._code(), xn, w_in[E:], b_in[E:])
        o = torch.empty(B, E, dtype=torch.float32, device=x.device)
        probs = torch.empty(B, self.heads, M, dtype=torch.float32, device=x.device)
        weights = torch.empty_like(probs)
        ops.fusion_attn_fwd(B, M, E, self.heads, q, kv, o, probs, weights, rng, stream_id, p_attn)
        y, d_out = lin(self._code(), o, self._w(ar, f"{pre}.mha.out_proj.weight"), ar.master(f"{pre}.mha.out_proj.bias"))
        return y, dict(x=x, st=st, xn=xn, qin=qin, q=q, d_q=d_q, kv=kv, d_kv=d_kv, o=o, probs=probs, weights=weights, d_out=d_out,
                       B=B, M=M, E=E)

    def backward(self, sv, dy):
        """dy [B, E] fp32 -> dx [B*M, E]; the block's parameter gradients accumulate into the arena."""
        ar, pre, B, M, E = self.bb.arena(), self.pre, sv["B"], sv["M"], sv["E"]
        do = lin_bwd(sv["d_out"], dy, sv["o"], self._w(ar, f"{pre}.mha.out_proj.weight"), ar.g(f"{pre}.mha.out_proj.weight"),
                     ar.g(f"{pre}.mha.out_proj.bias"))
        dq = torch.empty(B, E, dtype=torch.float32, device=dy.device)
        dkv = torch.empty(B * M, 2 * E, dtype=torch.float32, device=dy.device)
        ops.fusion_attn_bwd(B, M, E, self.heads, sv["q"], sv["kv"], sv["probs"], sv["weights"], do, dq, dkv)
        w_in, gw, gb = self._w(ar, f"{pre}.mha.in_proj_weight"), ar.g(f"{pre}.mha.in_proj_weight"), ar.g(f"{pre}.mha.in_proj_bias")
        dqin = lin_bwd(sv["d_q"], dq, sv["qin"], w_in[:E], gw[:E], gb[:E])
        dxn = lin_bwd(sv["d_kv"], dkv, sv["xn"], w_in[E:], gw[E:], gb[E:])
        ops.loc_mean_bwd_add(dqin, dxn.view(B, M, E))  # the query is the mean of the M normalised tokens: dxn += dqin / M
        dx = torch.empty_like(sv["x"])
        ops.layernorm_bwd(dxn, sv["x"], sv["st"], ar.master(f"{pre}.norm1.weight"), dx, False, ar.g(f"{pre}.norm1.weight"),
                          ar.g(f"{pre}.norm1.bias"))
        return dx


class ClassifierHead:
    def __init__(self, backbone, fusion_prefix=None, heads=0, p_attn=0.0):
        self.bb, self.fusion, self.heads, self.p_attn = backbone, fusion_prefix, heads, p_attn
        self.block = FusionBlock(backbone, fusion_prefix, heads) if fusion_prefix is not None else None

    # ------------------------------------------------------------------------------------------------ forward
    def forward(self, feats, training):
        """feats: [B, M, E] (fusion) or [B, sum E_m] (concatenation) fp32 -> logits [B, n_cls]."""
        bb, ar = self.bb, self.bb.arena()
        sv = {"training": training}
        if self.fusion is not None:
            B, M, E = feats.shape
            p = self.p_attn if training else 0.0
            h, fs = self.block.forward(feats.reshape(B * M, E).contiguous(), B, M, p, bb.rng_state() if p > 0 else None, 0x7F00)
            sv["fusion"] = fs
        else:
            h = feats.contiguous()
        sv["h_in"] = h
        if "class_layer.2.weight" in ar.index:
            # Linear -> GELU -> Linear (`pretrained_head` != "linear", models/SW_Transformer.py:175-181): the hidden layer on the exact-fp32
            # GEMM with the GELU epilogue (value and derivative from one launch), the few-column output layer as for the linear head
            f32 = ops.code(torch.float32)
            Bn, K = h.shape
            N = ar.index["class_layer.0.weight"][2][0]
            d0 = ops.linear_desc(f32, Bn, N, K, f32, f32, ACT_NONE, EPI_GELU)
            h1, g1 = torch.empty(Bn, N, dtype=torch.float32, device=h.device), torch.empty(Bn, N, dtype=torch.float32, device=h.device)
            ops.linear_fwd(d0, h, ar.master("class_layer.0.weight"), ar.master("class_layer.0.bias"), None, h1, g1)
            sv.update(d0=d0, h1=h1, g1=g1)
            logits = ops.small_linear_fwd(h1, ar.master("class_layer.2.weight"), ar.master("class_layer.2.bias"))
            return logits, sv
        logits = ops.small_linear_fwd(h, ar.master("class_layer.0.weight"), ar.master("class_layer.0.bias"))
        return logits, sv

    # ------------------------------------------------------------------------------------------------ backward
    def backward(self, sv, dlogits):
        ar = self.bb.arena()
        if dlogits.dtype != torch.float32 or not dlogits.is_contiguous():
            dlogits = dlogits.float().contiguous()
        train_encoders = getattr(self.bb, "supervised", False)  # supervised training: the gradient continues into the encoders
        need_dx = self.fusion is not None or train_encoders
        if "d0" in sv:
            dh1 = ops.small_linear_bwd(dlogits, sv["h1"], ar.master("class_layer.2.weight"), ar.g("class_layer.2.weight"),
                                       ar.g("class_layer.2.bias"), True)
            ops.mul_(dh1, sv["g1"])  # through the GELU: the derivative saved by the forward epilogue
            ops.linear_bwd_weight(sv["d0"], dh1, sv["h_in"], ar.g("class_layer.0.weight"), ar.g("class_layer.0.bias"))
            dh = None
            if need_dx:
                dh = torch.empty_like(sv["h_in"])
                d0b = ops.linear_desc(sv["d0"].dtype, sv["d0"].M, sv["d0"].N, sv["d0"].K, sv["d0"].x_dtype, sv["d0"].y_dtype)
                ops.linear_bwd_data(d0b, dh1, ar.master("class_layer.0.weight"), None, dh)
        else:
            dh = ops.small_linear_bwd(dlogits, sv["h_in"], ar.master("class_layer.0.weight"), ar.g("class_layer.0.weight"),
                                      ar.g("class_layer.0.bias"), need_dx)
        if self.fusion is None:
            return dh if train_encoders else None  # finetuning: the encoders in front are frozen
        fs = sv["fusion"]
        dx = self.block.backward(fs, dh)  # gradient w.r.t. the features (propagated further in supervised training only)
        return dx.view(fs["B"], fs["M"], fs["E"]) if train_encoders else None
