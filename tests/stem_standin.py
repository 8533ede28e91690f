"""The stem and the heads as the model composes them (model/stratified_transformer.py:344-392, 406-443), restated small for the tests of
layers.fuse_batch_norms: KPConvSimpleBlock, KPConvResBlock with the reference's forward signature (feats, xyz, batch, neighbor_idx), the
classifier and the regressor.  `conv` makes the convolution: compat.KPConvLayer on the GPU, MeanConv (same call signature, plain torch)
where there is none."""
import torch
from torch import nn

from stratified_transformer_amd.compat import FastBatchNorm1d

GRID = 0.04


class MeanConv(nn.Module):
    """a convolution with KPConvLayer's call signature in plain torch: a Linear on the mean of the neighbours' rows (index < 0: row 0)"""

    def __init__(self, c_in, c_out, point_influence=GRID, add_one=False):
        super().__init__()
        self.weight = nn.Parameter(torch.randn(c_in, c_out) * (2.0 / (c_in + c_out)) ** 0.5)

    def forward(self, query_points, support_points, neighbors, x):
        return x[neighbors.clamp(min=0).long()].mean(1) @ self.weight


def kp_conv(c_in, c_out, point_influence=GRID, add_one=False):
    from stratified_transformer_amd.compat import KPConvLayer
    return KPConvLayer(c_in, c_out, point_influence=point_influence, add_one=add_one)


class Simple(nn.Module):
    """KPConvSimpleBlock (:344-359)"""

    def __init__(self, c_in, c_out, conv, momentum=0.02):
        super().__init__()
        self.kpconv = conv(c_in, c_out, point_influence=GRID * 1.0, add_one=False)
        self.bn = FastBatchNorm1d(c_out, momentum=momentum)
        self.activation = nn.LeakyReLU(negative_slope=0.2)

    def forward(self, feats, xyz, batch, neighbor_idx):
        feats = self.kpconv(xyz, xyz, neighbor_idx, feats)
        feats = self.activation(self.bn(feats))
        return feats


class Res(nn.Module):
    """KPConvResBlock (:362-392); in_channels == out_channels is the model's use (:414): the shortcut is the identity"""

    def __init__(self, c_in, c_out, conv, momentum=0.02):
        super().__init__()
        d_2 = c_out // 4
        activation = nn.LeakyReLU(negative_slope=0.2)
        self.unary_1 = nn.Sequential(nn.Linear(c_in, d_2, bias=False), FastBatchNorm1d(d_2, momentum=momentum), activation)
        self.unary_2 = nn.Sequential(nn.Linear(d_2, c_out, bias=False), FastBatchNorm1d(c_out, momentum=momentum), activation)
        self.kpconv = conv(d_2, d_2, point_influence=GRID * 1.0, add_one=False)
        self.bn = FastBatchNorm1d(c_out, momentum=momentum)
        self.activation = activation
        if c_in != c_out:
            self.shortcut_op = nn.Sequential(nn.Linear(c_in, c_out, bias=False), FastBatchNorm1d(c_out, momentum=momentum))
        else:
            self.shortcut_op = nn.Identity()

    def forward(self, feats, xyz, batch, neighbor_idx):
        shortcut = feats
        feats = self.unary_1(feats)
        feats = self.kpconv(xyz, xyz, neighbor_idx, feats)
        feats = self.unary_2(feats)
        shortcut = self.shortcut_op(shortcut)
        feats += shortcut
        return feats


class StemHeads(nn.Module):
    """stem_layer, classifier and regressor of Stratified (:412-415, :426-443, activation='Tanh') without the transformer between them"""

    def __init__(self, conv, c_in=3, c=48, num_classes=19):
        super().__init__()
        self.stem_layer = nn.ModuleList([Simple(c_in, c, conv), Res(c, c, conv)])
        self.classifier = nn.Sequential(nn.Linear(c, c), nn.BatchNorm1d(c), nn.ReLU(inplace=True), nn.Linear(c, num_classes))
        self.regressor = nn.Sequential(nn.Linear(c, c), nn.BatchNorm1d(c), nn.Tanh(), nn.Linear(c, 3))

    def forward(self, feats, xyz, batch, neighbor_idx):
        for layer in self.stem_layer:
            feats = layer(feats, xyz, batch, neighbor_idx)
        return self.classifier(feats), self.regressor(feats)


def shake_norms(model, seed):
    """affine parameters and running statistics away from their defaults, so that every one of them matters"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, nn.modules.batchnorm._BatchNorm):
                if m.affine:
                    m.weight.copy_(1 + 0.2 * torch.randn(m.weight.shape, generator=g))
                    m.bias.copy_(0.2 * torch.randn(m.bias.shape, generator=g))
                if m.running_mean is not None:
                    m.running_mean.copy_(0.1 * torch.randn(m.running_mean.shape, generator=g))
                    m.running_var.copy_(1 + 0.3 * torch.rand(m.running_var.shape, generator=g))
    return model
