"""Golden vectors of the DECODER layer, produced by EXECUTING THE REFERENCE'S OWN `Upsample` on CPU in float32 (build container only;
same shims as make_golden.py, nothing of the reference is copied):

  model/stratified_transformer.py  Upsample.__init__/forward (:329-342: two Sequential(LayerNorm, Linear), the interpolation, the add)

`pointops.interpolation`, whose own form allocates on the GPU, is bound to a torch restatement of lib/pointops2/functions/pointops.py:756-770
(inverse-distance weights, a zero tensor, k gather-multiply-adds in order) over the CPU oracle's kNN (oracle/pointops_oracle.c); the
indices and weights it used are stored beside the result, so that the interpolation term can be restated from them.

Two batch elements, 64 coarse and 257 fine points (the coarse points are every fourth fine point, as a sampler would leave
them: each has a fine point at distance 0), in_channels 32, out_channels 16, k = 3.

    python tests/golden/make_golden_upsample.py   ->  tests/golden/upsample_reference.npz
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", ".."))
import make_golden as mg  # noqa: E402
from oracle import pointops_ref as ref  # noqa: E402

USED = {}


def t_interpolation(xyz, new_xyz, feat, offset, new_offset, k=3):
    idx, dist = ref.knnquery(k, xyz.detach().numpy(), new_xyz.detach().numpy(), offset.numpy().astype(np.int32),
                             new_offset.numpy().astype(np.int32))
    idx, dist = torch.from_numpy(idx), torch.from_numpy(dist)
    dist_recip = 1.0 / (dist + 1e-8)
    weight = dist_recip / torch.sum(dist_recip, dim=1, keepdim=True)
    new_feat = torch.zeros(new_xyz.shape[0], feat.shape[1])
    for i in range(k):
        new_feat = new_feat + feat[idx[:, i].long(), :] * weight[:, i].unsqueeze(-1)
    USED.update(idx=idx, weight=weight, term=new_feat.detach(), linear2_out=feat.detach())
    return new_feat


def main():
    mg.install_shims()
    root = os.path.realpath(os.path.join(HERE, "..", ".."))
    sys.path[:] = [p for p in sys.path if os.path.realpath(p or ".") != root]  # `lib.pointops2...` must be the reference's here
    assert "lib" not in sys.modules
    sys.path.insert(0, mg.REF)
    import model.stratified_transformer as st  # the reference
    assert os.path.realpath(st.pointops.__file__).startswith(mg.REF), st.pointops.__file__
    st.pointops.interpolation = t_interpolation

    C_in, C_out, k = 32, 16, 3
    fine = [mg.synthetic_room(120, 31), mg.synthetic_room(137, 32, box=(0.7, 0.6, 0.5))]
    coarse = [fine[0][::4], fine[1][::4][:34]]
    support_xyz, xyz = torch.cat(fine).contiguous(), torch.cat(coarse).contiguous()
    support_offset = torch.tensor([120, 257], dtype=torch.int32)
    offset = torch.tensor([30, 64], dtype=torch.int32)
    assert xyz.shape[0] == 64 and support_xyz.shape[0] == 257
    torch.manual_seed(7)
    up = st.Upsample(k, C_in, C_out)
    with torch.no_grad():  # O(1) parameters so that every term matters
        for name, p in up.named_parameters():
            if name.endswith("weight") and p.dim() == 2:
                p.copy_(torch.randn(p.shape) * (1.0 / p.shape[1] ** 0.5))
            elif name.endswith("bias"):
                p.copy_(torch.randn(p.shape) * 0.1)
            elif name.endswith("weight") and p.dim() == 1:
                p.copy_(1.0 + 0.1 * torch.randn(p.shape))
    feats = torch.randn(64, C_in, requires_grad=True)
    support_feats = torch.randn(257, C_out, requires_grad=True)
    out, s_xyz, s_off = up(feats, xyz, support_xyz, offset, support_offset, support_feats)
    assert s_xyz is support_xyz and s_off is support_offset and out.dtype == torch.float32
    grad_out = torch.randn(out.shape, generator=torch.Generator().manual_seed(9))
    out.backward(grad_out)
    data = dict(xyz=xyz.numpy(), support_xyz=support_xyz.numpy(), offset=offset.numpy(), support_offset=support_offset.numpy(),
                feats=feats.detach().numpy(), support_feats=support_feats.detach().numpy(), grad_out=grad_out.numpy(),
                knn_idx=USED["idx"].numpy(), knn_weight=USED["weight"].numpy(), interpolated=USED["term"].numpy(),
                linear2_out=USED["linear2_out"].numpy(), out=out.detach().numpy(), grad_feats=feats.grad.numpy(),
                grad_support_feats=support_feats.grad.numpy(), config=np.array([k, C_in, C_out], dtype=np.int32))
    for name, p in up.named_parameters():
        data["param." + name] = p.detach().numpy()
        data["grad." + name] = p.grad.numpy()
    path = os.path.join(HERE, "upsample_reference.npz")
    np.savez_compressed(path, **data)
    print("wrote", path, os.path.getsize(path), "bytes;  |out| =", float(out.detach().abs().max()), " |grad_feats| =", float(feats.grad.abs().max()))


if __name__ == "__main__":
    main()
