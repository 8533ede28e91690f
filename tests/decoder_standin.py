"""TEST / BENCH SCAFFOLDING (not the product): a container with the attribute names and state-dict keys of the reference's decoder class
(model/stratified_transformer.py: Upsample :329-342), written from its published structure as stratified_transformer_amd/standin.py was,
so that layers.upsample_forward can be installed, exercised and timed where the reference cannot travel.  The forward keeps the
reference's call structure on the operator API - two Sequential(LayerNorm, Linear), `pointops.interpolation` with its default k, one add
- because that is the path the installed forward is compared with; golden parameters load by name.
"""
from torch import nn


class Upsample(nn.Module):
    def __init__(self, k, in_channels, out_channels, bn_momentum=0.02):
        super().__init__()
        self.k, self.in_channels, self.out_channels = k, in_channels, out_channels
        self.linear1 = nn.Sequential(nn.LayerNorm(out_channels), nn.Linear(out_channels, out_channels))
        self.linear2 = nn.Sequential(nn.LayerNorm(in_channels), nn.Linear(in_channels, out_channels))

    def forward(self, feats, xyz, support_xyz, offset, support_offset, support_feats=None):
        from stratified_transformer_amd import pointops
        skip = self.linear1(support_feats)
        coarse = pointops.interpolation(xyz, support_xyz, self.linear2(feats), offset, support_offset)
        return skip + coarse, support_xyz, support_offset
