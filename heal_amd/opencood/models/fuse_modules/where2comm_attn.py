"""EncodeLayer of Where2comm (reference: opencood/models/fuse_modules/where2comm_attn.py:64-103): multi-head attention of a query
over a short sequence, a residual LayerNorm, a two-layer feed-forward net and a second residual LayerNorm.  Plain torch layers with
the reference's attribute names, so a reference checkpoint's keys load strictly: this is the CPU, gradient and unsupported-shape
arithmetic of Where2commFusion (fusion_in_one.py); inference on the device reads the parameters and runs heal_conv1x1,
heal_warp_mha_fuse and heal_layernorm_nchw instead."""
import torch.nn as nn


class EncodeLayer(nn.Module):
    def __init__(self, channels, n_head=8, dropout=0):
        super().__init__()
        self.attn = nn.MultiheadAttention(channels, n_head, dropout)
        self.linear1 = nn.Linear(channels, channels)
        self.linear2 = nn.Linear(channels, channels)
        self.norm1 = nn.LayerNorm(channels)
        self.norm2 = nn.LayerNorm(channels)
        self.dropout1 = nn.Dropout(dropout)
        self.dropout2 = nn.Dropout(dropout)
        self.relu = nn.ReLU()

    def forward(self, q, k, v):
        """(seq, batch, feature) order: q [1, HW, C], k and v [n, HW, C] -> [1, HW, C]."""
        context, _ = self.attn(q, k, v)
        output1 = self.norm1(q + self.dropout1(context))
        context = self.linear2(self.relu(self.linear1(output1)))
        return self.norm2(output1 + self.dropout2(context))
