"""GPU: operands on a device that is not the current one - _lib.call makes it current for the launch and gives it back."""
import pytest
import torch

from stratified_transformer_amd import dataprep, pointops

pytestmark = pytest.mark.gpu


def _run(dev):
    """voxel keys of 1000 points; segment softmax of [300, 3] logits over 40 segments, forward and backward (one launch each, no
    side streams, no large LDS)"""
    g = torch.Generator().manual_seed(5)
    coord = (torch.rand(1000, 3, generator=g) * 4).to(dev)
    keys = dataprep.voxel_keys(coord, 0.04)
    cuts = torch.sort(torch.randperm(299, generator=g)[:39] + 1)[0]   # 40 non-empty segments of 300 rows
    offsets = torch.cat([torch.zeros(1, dtype=torch.long), cuts, torch.tensor([300])]).int().to(dev)
    src = torch.randn(300, 3, generator=g).to(dev).requires_grad_()
    out = pointops.segment_softmax(src, offsets)
    out.backward(torch.randn(300, 3, generator=g).to(dev))
    return [t.cpu() for t in (keys, out.detach(), src.grad)]


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs a second device that is not the current one")
def test_operands_on_a_device_that_is_not_current():
    torch.cuda.set_device(0)
    want = _run(torch.device("cuda", 0))
    got = _run(torch.device("cuda", 1))
    assert torch.cuda.current_device() == 0
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and torch.equal(a, b)
    assert want[1].sum(0).sub(40).abs().max() < 1e-4   # (softmax rows were written at all: each segment sums to 1 per head)
