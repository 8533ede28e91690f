"""TEST SCAFFOLDING (not the product): containers with the attribute names and call conventions of the Swin3D model classes
(model/swin3d_transformer.py: WindowAttention :94, SwinTransformerBlock :180, BasicLayer :214), written from the model's formulas on
this package's operator API, so that layers.patch_swin_classes() can be compared with an unpatched run on the GPU box, where the
reference itself cannot travel.  Unlike tests/model_standin.py these classes HAVE forwards of their own - the comparison's other side:

    WindowAttention.forward   qkv, q * scale, A1 + rel-pos bias (index = difference of the quantised in-window coordinates + qgl - 1, by
                              torch ops), softmax per query, A4 with the value table, proj
    BasicLayer.forward        the pair lists of the plain and the shifted windows (index_build.swin_stage_index_hip without plans: its
                              pair lists are pinned bit for bit by tests/golden/swin3d_window_attention.npz), blocks alternate, shift
                              0.0 / half a window; no downsample
"""
import torch
from torch import nn

from stratified_transformer_amd import index_build
from stratified_transformer_amd import pointops as P
from stratified_transformer_amd.standin import Mlp


class WindowAttention(nn.Module):
    def __init__(self, dim, window_size, num_heads, quant_size):
        super().__init__()
        self.dim, self.num_heads, self.window_size, self.quant_size = dim, num_heads, window_size, quant_size
        self.scale = (dim // num_heads) ** -0.5
        self.rel_query = self.rel_key = self.rel_value = True
        self.quant_grid_length = int(window_size / quant_size)
        shape = (2 * self.quant_grid_length - 1, num_heads, dim // num_heads, 3)
        self.relative_pos_query_table = nn.Parameter(torch.zeros(shape))
        self.relative_pos_key_table = nn.Parameter(torch.zeros(shape))
        self.relative_pos_value_table = nn.Parameter(torch.zeros(shape))
        self.qkv, self.proj, self.proj_drop = nn.Linear(dim, 3 * dim), nn.Linear(dim, dim), nn.Dropout(0.0)

    def forward(self, feats, xyz, index_0, index_0_offsets, n_max, index_1, shift_size):
        N, C = feats.shape
        h = self.num_heads
        qkv = self.qkv(feats).reshape(N, 3, h, C // h).permute(1, 0, 2, 3).contiguous()
        query, key, value = qkv[0] * self.scale, qkv[1], qkv[2]
        offs, i1 = index_0_offsets.int(), index_1.int()
        quant = ((xyz - xyz.min(0)[0] + shift_size) % self.window_size) // self.quant_size
        rel = (quant[index_0.long()] - quant[index_1.long()] + self.quant_grid_length - 1).int()
        logits = P.attention_step1_v2(query.float(), key.float(), i1, offs, n_max)
        logits = logits + P.dot_prod_with_idx_v3(query.float(), offs, n_max, key.float(), i1, self.relative_pos_query_table.float(),
                                                 self.relative_pos_key_table.float(), rel)
        weights = P.segment_softmax(logits, offs)
        x = P.attention_step2_with_rel_pos_value_v2(weights, value.float(), offs, n_max, i1, self.relative_pos_value_table.float(), rel)
        return self.proj_drop(self.proj(x.view(N, C)))


class SwinTransformerBlock(nn.Module):
    def __init__(self, dim, num_heads, window_size, quant_size, mlp_ratio=4.0):
        super().__init__()
        self.norm1, self.norm2 = nn.LayerNorm(dim), nn.LayerNorm(dim)
        self.attn = WindowAttention(dim, window_size, num_heads, quant_size)
        self.drop_path = nn.Identity()
        self.mlp = Mlp(dim, int(dim * mlp_ratio))

    def forward(self, feats, xyz, index_0, index_0_offsets, n_max, index_1, shift_size):
        feats = feats + self.drop_path(self.attn(self.norm1(feats), xyz, index_0, index_0_offsets, n_max, index_1, shift_size))
        return feats + self.drop_path(self.mlp(self.norm2(feats)))


class BasicLayer(nn.Module):
    def __init__(self, depth, channel, num_heads, window_size, quant_size):
        super().__init__()
        self.depth, self.window_size = depth, window_size
        self.blocks = nn.ModuleList([SwinTransformerBlock(channel, num_heads, window_size, quant_size) for _ in range(depth)])
        self.downsample = None

    def forward(self, feats, xyz, offset):
        even, odd, _ = index_build.swin_stage_index_hip(xyz, offset, float(self.window_size), float(self.blocks[0].attn.quant_size))
        shift_size = 1 / 2 * torch.tensor([self.window_size] * 3).type_as(xyz).to(xyz.device)
        for i, blk in enumerate(self.blocks):
            bi = even if i % 2 == 0 else odd
            feats = blk(feats, xyz, bi.index_0, bi.offsets, bi.n_max, bi.index_1, 0.0 if i % 2 == 0 else shift_size)
        return feats, xyz, offset, None, None, None
