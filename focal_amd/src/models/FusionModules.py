"""Fusion blocks of the reference (models/FusionModules.py).  They are parameter containers with the reference's names and
shapes (checkpoint interchange); their arithmetic runs in the HIP engines -- TransformerFusionBlock in focal_amd/head_engine.py
(class_head=True) and in focal_amd/loc_engine.py (location fusion of a multi-location dataset), the encoder layers of the
location context in focal_amd/loc_engine.py.  Calling a module here is an error rather than a silent eager path."""
import torch.nn as nn


class MeanFusionBlock(nn.Module):
    def forward(self, *a, **k):
        raise NotImplementedError("MeanFusionBlock is a parameterless container: the mean over the locations runs in "
                                  "focal_amd/deepsense_engine.py (DeepSenseMultiLocEncoder, focal_rows_mean), not as a torch module")


class TransformerFusionBlock(nn.Module):
    def __init__(self, embed_dim, num_heads, dropout_rate, attention_dropout_rate):
        super().__init__()
        self.norm1 = nn.LayerNorm(embed_dim)
        self.mha = nn.MultiheadAttention(embed_dim, num_heads, dropout=attention_dropout_rate, batch_first=True)

    def forward(self, *a, **k):
        raise NotImplementedError("TransformerFusionBlock runs in focal_amd/head_engine.py / loc_engine.py, not as a torch module")


class LocContextLayer(nn.TransformerEncoderLayer):
    """torch.nn.TransformerEncoderLayer(d_model, nhead, dim_feedforward, dropout, batch_first=True) as the reference builds it for
    loc_context_layers (post-norm, ReLU, layer_norm_eps 1e-5): same parameters and names; executed by focal_amd/loc_engine.py."""

    def forward(self, *a, **k):
        raise NotImplementedError("the location-context encoder layer runs in focal_amd/loc_engine.py, not as a torch module")
