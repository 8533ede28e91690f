"""The cases of the gather-add tests (tests/test_gather_add_cpu.py, tests/test_gather_add_hip.py): seeded operands as torch CPU tensors.

SHAPES (n fine rows, m source rows, k, c) puts every value of c in {1, 3, 4, 8, 12, 48, 52, 1024}, n in {1, 63, 64, 65, 257}, m in {1, 2,
64} and k in {1, 3, 16, 64} on the kernels at least once, with the channel counts spread over the paths they select: c % 8 == 0 is
chunked for every row type, c % 4 == 0 only for fp32 feat (one element per lane for the halves), odd c one element per lane always;
c = 1024 is the row of more than 64 chunks (several chunks per lane under one walk of the indices); n = 63 / 64 / 65 / 257 with few
chunks fills, over-fills and leaves partly empty the rows of a wave, and several workgroups.  Every shape runs with every pair of
row types.
"""
import itertools

import torch

FEAT_DTYPES = (torch.float32, torch.float16, torch.bfloat16)
BASE_DTYPES = (None, torch.float32, torch.float16, torch.bfloat16)
DTYPE_PAIRS = tuple(itertools.product(FEAT_DTYPES, BASE_DTYPES))

SHAPES = (
    (1, 1, 1, 1),
    (63, 2, 3, 3),
    (64, 64, 3, 4),
    (65, 64, 16, 8),
    (257, 64, 3, 12),
    (257, 64, 3, 48),
    (65, 2, 64, 52),
    (63, 64, 16, 1024),
    (257, 1, 3, 8),       # every fine row on source row 0: n * k = 771 pairs on one row
    (64, 2, 64, 48),
    (257, 64, 1, 8),
)


def operands(n, m, k, c, feat_dtype=torch.float32, base_dtype=None, seed=0, invalid=0.1):
    """-> dict(feat [m, c], idx [n, k] int32, weight [n, k] f32, base [n, c] or None, grad_out [n, c] f32).  About `invalid` of the idx
    entries are -1 or m (skipped); indices repeat inside a row whenever k > m.  Values are O(1) with both signs."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * n + 11 * m + 13 * k + c)
    feat = torch.randn((m, c), generator=g).to(feat_dtype)
    idx = torch.randint(0, max(m, 1), (n, k), generator=g, dtype=torch.int32)
    if invalid > 0:
        u = torch.rand((n, k), generator=g)
        idx = torch.where(u < invalid / 2, torch.full_like(idx, -1), idx)
        idx = torch.where(u > 1 - invalid / 2, torch.full_like(idx, m), idx)
    if m == 0:
        idx = torch.full_like(idx, -1)
    weight = torch.rand((n, k), generator=g) + 0.05
    weight = weight / weight.sum(1, keepdim=True)
    base = None if base_dtype is None else torch.randn((n, c), generator=g).to(base_dtype)
    grad_out = torch.randn((n, c), generator=g)
    return dict(feat=feat, idx=idx, weight=weight, base=base, grad_out=grad_out)
