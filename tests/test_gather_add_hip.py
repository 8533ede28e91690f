"""GPU (-m gpu): the gather-add on csrc/upsample.hip - pointops.gather_add / interpolate_add and the installed Upsample.forward - against the
fp32 oracle of tests/gather_add_oracle.py evaluated on the CPU, the parent's interpolation path and the reference's own decoder
(tests/golden/upsample_reference.npz).

Bars.  The operator, forward and backward: bit-identical to the oracle (the same fp32 operations in the same order; one rounding to
feat's row type in the backward), on every shape of tests/gather_add_cases.py with every pair of row types.  Against the parent's
_WeightedGather + base: 2 k eps sum_i |w_i f_i| per element.  The layer: the UNPATCHED stand-in's maximum error against the golden
on this GPU is measured first, per tensor (output, both feature gradients, every parameter gradient), and the installed forward is
held to twice that figure; under autocast the unpatched autocast error against the fp32 golden is the yardstick.

Every test prints its figures (pytest -s).
"""
import os

import numpy as np
import pytest
import torch

from tests import decoder_standin
from tests import gather_add_cases as cases
from tests import gather_add_oracle as O

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "upsample_reference.npz")
EPS = float(np.finfo(np.float32).eps)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from stratified_transformer_amd import pointops
    pointops.clear_caches()


@pytest.fixture(scope="module")
def P():
    from stratified_transformer_amd import pointops
    return pointops


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same_bits(got, want):
    return got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape) and torch.equal(_bits(got), _bits(want))


def _run(P, feat, idx, weight, base, grad_out):
    """operands on the CPU -> (out, grad_feat, grad_base) from the GPU, on the CPU"""
    f = feat.cuda().requires_grad_(True)
    b = None if base is None else base.cuda().requires_grad_(True)
    out = P.gather_add(f, idx.cuda(), weight.cuda(), b)
    out.backward(grad_out.cuda())
    torch.cuda.synchronize()
    return out.detach().cpu(), f.grad.cpu(), None if b is None else b.grad.cpu()


@pytest.mark.parametrize("shape", cases.SHAPES, ids=lambda s: "n%d_m%d_k%d_c%d" % s)
def test_forward_and_backward_are_the_oracle_bit_for_bit(P, shape):
    n, m, k, c = shape
    p = cases.operands(n, m, k, c, torch.float32, torch.float32)
    grad32 = O.backward(p["grad_out"], p["idx"], p["weight"], m)             # fp32 sums: one per shape, rounded per feat dtype below
    for fd, bd in cases.DTYPE_PAIRS:
        feat, base = p["feat"].to(fd), None if bd is None else p["base"].to(bd)
        out, grad_feat, grad_base = _run(P, feat, p["idx"], p["weight"], base, p["grad_out"])
        want = torch.from_numpy(O.forward(feat, p["idx"], p["weight"], base))
        assert _same_bits(out, want), (fd, bd, float((out - want).abs().max()))
        assert _same_bits(grad_feat, grad32.to(fd)), (fd, bd)
        if bd is not None:
            assert _same_bits(grad_base, p["grad_out"].to(bd)), (fd, bd)


def test_int64_indices_are_clamped_and_narrowed(P):
    p = cases.operands(65, 64, 3, 8)
    idx = p["idx"].long()
    idx[0, 0], idx[1, 1] = 2 ** 40, -2 ** 40
    out = P.gather_add(p["feat"].cuda(), idx.cuda(), p["weight"].cuda()).cpu()
    assert _same_bits(out, torch.from_numpy(O.forward(p["feat"], idx.clamp(-1, 64), p["weight"])))


def test_skipped_entries_invalid_rows_and_repeats(P):
    n, m, k, c = 9, 5, 4, 8
    p = cases.operands(n, m, k, c, torch.float16, torch.bfloat16, invalid=0.0)
    idx = p["idx"]
    idx[0] = torch.tensor([-1, m, -1, m])           # no valid entry: base or 0, no gradient
    idx[1] = torch.tensor([-1, 2, m, 2])            # skipped entries between valid ones, a repeat
    idx[2] = torch.tensor([3, 3, 3, 3])             # one source row four times
    idx[3:] = idx[3:].clamp(0, 3)                   # source row 4 is referenced by nobody
    for base in (p["base"], None):
        out, grad_feat, _ = _run(P, p["feat"], idx, p["weight"], base, p["grad_out"])
        assert _same_bits(out, torch.from_numpy(O.forward(p["feat"], idx, p["weight"], base)))
        assert _same_bits(out[0], torch.zeros(c) if base is None else base[0].float())
        assert _same_bits(grad_feat, O.backward(p["grad_out"], idx, p["weight"], m, torch.float16))
        assert (_bits(grad_feat[4]) == 0).all()
    # the all-invalid row carries no gradient: changing its grad_out changes nothing
    go = p["grad_out"].clone()
    go[0] = 1e30
    assert _same_bits(_run(P, p["feat"], idx, p["weight"], None, go)[1], grad_feat)


def test_every_fine_row_on_source_row_zero(P):
    n, m, k, c = 257, 1, 3, 8
    p = cases.operands(n, m, k, c, invalid=0.0)
    assert int((p["idx"] == 0).sum()) == 771
    out, grad_feat, _ = _run(P, p["feat"], p["idx"], p["weight"], None, p["grad_out"])
    assert _same_bits(out, torch.from_numpy(O.forward(p["feat"], p["idx"], p["weight"])))
    assert _same_bits(grad_feat, O.backward(p["grad_out"], p["idx"], p["weight"], m))


@pytest.mark.parametrize("dtype,c", [(torch.float32, 8), (torch.float16, 8), (torch.bfloat16, 5)])
def test_unreferenced_source_rows_get_exact_zeros(P, dtype, c):
    """grad_feat is allocated by the operator (torch.empty); the block it is likely to be handed is filled with NaN first"""
    from stratified_transformer_amd import pointops2_cuda
    n, m, k = 65, 64, 3
    p = cases.operands(n, m, k, c, dtype, invalid=0.0)
    idx = p["idx"] // 2 * 2                          # odd source rows are referenced by nobody
    f = p["feat"].cuda().requires_grad_(True)
    out = P.gather_add(f, idx.cuda(), p["weight"].cuda())
    junk = torch.full((m, c), float("nan"), dtype=dtype, device="cuda")
    del junk
    out.backward(p["grad_out"].cuda())
    assert (_bits(f.grad[1::2]) == 0).all() and _same_bits(f.grad, O.backward(p["grad_out"], idx, p["weight"], m, dtype))
    # and the launcher itself, on a buffer that held NaN
    keys = idx.cuda().view(-1)
    rows = torch.arange(0, n * k + 1, k, dtype=torch.int32, device="cuda")
    src_offsets, src_pair, _ = P._csc_build(rows, keys, m + 1)
    grad_feat = torch.full((m, c), float("nan"), dtype=dtype, device="cuda")
    pointops2_cuda.gather_add_backward(n, m, k, c, p["grad_out"].cuda(), p["weight"].cuda(), src_offsets[:m + 1], src_pair, grad_feat)
    assert _same_bits(grad_feat, f.grad)


def test_empty_operands(P):
    w0, i0 = torch.zeros(0, 3, device="cuda"), torch.zeros(0, 3, dtype=torch.int32, device="cuda")
    # n = 0
    f = torch.randn(6, 8, device="cuda", requires_grad=True)
    out = P.gather_add(f, i0, w0, torch.zeros(0, 8, device="cuda"))
    assert tuple(out.shape) == (0, 8) and out.dtype == torch.float32
    out.sum().backward()
    assert tuple(f.grad.shape) == (6, 8) and (_bits(f.grad) == 0).all()
    # m = 0: base, or zeros
    f = torch.zeros(0, 8, device="cuda", dtype=torch.float16, requires_grad=True)
    idx = torch.tensor([[0, -1, 5]] * 7, dtype=torch.int32, device="cuda")
    w = torch.rand(7, 3, device="cuda")
    base = torch.randn(7, 8, device="cuda").bfloat16()
    assert (_bits(P.gather_add(f, idx, w)) == 0).all()
    out = P.gather_add(f, idx, w, base)
    assert _same_bits(out, base.float())
    out.sum().backward()
    assert tuple(f.grad.shape) == (0, 8) and f.grad.dtype == torch.float16


@pytest.mark.parametrize("dtype,c,how", [(torch.float32, 3, "rows"), (torch.float16, 5, "rows"), (torch.bfloat16, 7, "rows"),
                                         (torch.float16, 4, "rows"), (torch.float32, 8, "flat"), (torch.float16, 8, "flat")])
def test_misaligned_views_give_the_bits_of_the_aligned_copy(P, dtype, c, how):
    """feat[1:] / base[1:] of a row-major buffer with odd c (and, `flat`, a chunkable c one element into its storage) start off the
    16-byte grid: the element path must give the chunked path's bits"""
    n, m, k = 65, 64, 3
    p = cases.operands(n, m, k, c, dtype, dtype)
    idx, w, go = p["idx"].cuda(), p["weight"].cuda(), p["grad_out"].cuda()

    def shifted(t):
        if how == "rows":
            return torch.cat([t[:1], t]).cuda()[1:]
        flat = torch.cat([t.reshape(-1)[:1], t.reshape(-1)]).cuda()
        return flat[1:].view(t.shape)
    feat_v, base_v, go_v = shifted(p["feat"]), shifted(p["base"]), shifted(p["grad_out"])
    assert feat_v.is_contiguous() and feat_v.data_ptr() % 16 != 0 and base_v.data_ptr() % 16 != 0
    got = {}
    for name, (f, b, g) in dict(view=(feat_v, base_v, go_v), copy=(p["feat"].cuda(), p["base"].cuda(), go)).items():
        f = f.detach().requires_grad_(True)
        out = P.gather_add(f, idx, w, b)
        out.backward(g)
        got[name] = (out.detach(), f.grad)
    assert _same_bits(got["view"][0], got["copy"][0]) and _same_bits(got["view"][1], got["copy"][1])
    assert _same_bits(got["copy"][0], torch.from_numpy(O.forward(p["feat"], p["idx"], p["weight"], p["base"])))


@pytest.mark.parametrize("dtype,c", [(torch.float32, 8), (torch.float16, 16), (torch.bfloat16, 3)])
def test_non_finite_rows_stay_where_the_oracle_puts_them(P, dtype, c):
    n, m, k = 65, 16, 3
    p = cases.operands(n, m, k, c, dtype, torch.float32)
    feat = p["feat"].clone()
    feat[3], feat[7] = float("inf"), float("nan")
    feat[3, ::2] = float("-inf")
    out, _, _ = _run(P, feat, p["idx"], p["weight"], p["base"], p["grad_out"])
    want = torch.from_numpy(O.forward(feat, p["idx"], p["weight"], p["base"]))
    touched = ((p["idx"] == 3) | (p["idx"] == 7)).any(1)
    assert torch.equal(torch.isnan(out), torch.isnan(want)) and torch.equal(torch.isinf(out), torch.isinf(want))
    assert torch.isfinite(out[~touched]).all() and (~torch.isfinite(out[touched])).all(1).all()
    assert _same_bits(torch.nan_to_num(out, nan=0.0), torch.nan_to_num(want, nan=0.0))
    # the gradient of feat: non-finite where a non-finite grad_out row is gathered, and only there
    grad_out = out.clone()
    got = _run(P, feat, p["idx"], p["weight"], p["base"], grad_out)[1]
    want_g = O.backward(grad_out, p["idx"], p["weight"], m, dtype)
    assert torch.equal(torch.isnan(got), torch.isnan(want_g)) and torch.equal(torch.isinf(got), torch.isinf(want_g))
    assert _same_bits(torch.nan_to_num(got, nan=0.0), torch.nan_to_num(want_g, nan=0.0))
    valid = (p["idx"] >= 0) & (p["idx"] < m)
    reached = torch.zeros(m, dtype=torch.bool)
    reached[p["idx"][touched][valid[touched]].long()] = True
    assert torch.isfinite(got[~reached].float()).all() and (~torch.isfinite(got.float())).any()


def test_backward_is_reproducible_at_any_address(P):
    n, m, k, c = 257, 64, 16, 48
    p = cases.operands(n, m, k, c, torch.float16, torch.float16)
    first = _run(P, p["feat"], p["idx"], p["weight"], p["base"], p["grad_out"])[1]
    second = _run(P, p["feat"], p["idx"], p["weight"], p["base"], p["grad_out"])[1]
    pad = [torch.empty(12345, device="cuda") for _ in range(3)]     # moves what the third run allocates
    third = _run(P, p["feat"].clone(), p["idx"].clone(), p["weight"].clone(), p["base"].clone(), p["grad_out"].clone())[1]
    del pad
    assert _same_bits(first, second) and _same_bits(first, third)
    assert _same_bits(first, O.backward(p["grad_out"], p["idx"], p["weight"], m, torch.float16))


@pytest.mark.parametrize("shape", [(257, 64, 3, 48), (65, 64, 16, 8), (63, 2, 3, 3)], ids=lambda s: "n%d_m%d_k%d_c%d" % s)
def test_against_the_parents_weighted_gather_plus_base(P, shape):
    n, m, k, c = shape
    p = cases.operands(n, m, k, c, torch.float32, torch.float32, invalid=0.0)   # (the parent's kernel follows every index)
    feat, idx, w, base = (p[x].cuda() for x in ("feat", "idx", "weight", "base"))
    got = P.gather_add(feat, idx, w, base).cpu().double()
    parent = (P._WeightedGather.apply(feat, idx, w) + base).cpu().double()
    terms = sum((p["feat"][p["idx"][:, i].long()].double() * p["weight"][:, i:i + 1].double()).abs() for i in range(k))
    bound = 2 * k * EPS * terms
    err = (got - parent).abs()
    print("gather_add vs _WeightedGather + base: max err %.3e, max err / bound %.3f" % (float(err.max()), float((err / bound).max())))
    assert (err <= bound).all()


# ---- the layer ----
def _golden():
    g = np.load(GOLDEN)
    return {k: g[k] for k in g.files}


def _layer_run(g, autocast):
    """the stand-in decoder (as patched or not at this moment) on the golden's inputs -> dict of tensors on the CPU, the saved tensors'
    (shape, dtype) list, and the identity of the returned support objects"""
    up = decoder_standin.Upsample(int(g["config"][0]), int(g["config"][1]), int(g["config"][2])).cuda()
    up.load_state_dict({k[6:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("param.")})
    feats = torch.from_numpy(g["feats"]).cuda().requires_grad_(True)
    support_feats = torch.from_numpy(g["support_feats"]).cuda().requires_grad_(True)
    xyz, support_xyz = torch.from_numpy(g["xyz"]).cuda(), torch.from_numpy(g["support_xyz"]).cuda()
    offset, support_offset = torch.from_numpy(g["offset"]).cuda(), torch.from_numpy(g["support_offset"]).cuda()
    saved = []

    def pack(t):
        saved.append((tuple(t.shape), t.dtype))
        return t
    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        with torch.autocast("cuda", dtype=autocast or torch.float16, enabled=autocast is not None):
            out, s_xyz, s_off = up(feats, xyz, support_xyz, offset, support_offset, support_feats)
    assert out.dtype == torch.float32
    out.backward(torch.from_numpy(g["grad_out"]).cuda())
    torch.cuda.synchronize()
    res = {"out": out.detach().cpu(), "grad_feats": feats.grad.cpu(), "grad_support_feats": support_feats.grad.cpu()}
    for name, prm in up.named_parameters():
        res["grad." + name] = prm.grad.cpu()
    return res, saved, (s_xyz is support_xyz and s_off is support_offset)


def _errors(res, g):
    return {k: float((v.double() - torch.from_numpy(g[k]).double()).abs().max()) for k, v in res.items()}


@pytest.mark.parametrize("autocast", [None, torch.float16, torch.bfloat16], ids=["fp32", "autocast_f16", "autocast_bf16"])
def test_installed_decoder_against_the_reference_layer(P, autocast):
    """Measured on one MI355X, max abs error against the reference's fp32 CPU run, unpatched / installed (the bar is twice the first):
    see DESIGN.md 4.24 for the recorded figures of every tensor."""
    from stratified_transformer_amd import layers
    g = _golden()
    assert decoder_standin.Upsample.forward is not layers.upsample_forward
    off, saved_off, same_off = _layer_run(g, autocast)
    before = P.GATHER_ADD_VIEWS
    try:
        assert layers.install_fast_decoder(decoder_standin) == [decoder_standin.Upsample]
        on, saved_on, same_on = _layer_run(g, autocast)
    finally:
        layers.uninstall_fast_layers()
    assert P.GATHER_ADD_VIEWS == before + 1                 # the installed forward ran gather_add, and built its view in the forward
    err_off, err_on = _errors(off, g), _errors(on, g)
    for k in err_off:
        print("%-14s %-28s unpatched %.3e   installed %.3e" % ("fp32" if autocast is None else str(autocast), k, err_off[k], err_on[k]))
    assert same_off and same_on                              # support_xyz / support_offset are returned as passed in
    m, c = g["feats"].shape[0], int(g["config"][2])
    assert ((m, c), torch.float32) in saved_off              # the parent's path keeps (under autocast: makes) an fp32 [m, c] copy of linear2's rows
    assert ((m, c), torch.float32) not in saved_on and ((m, c), torch.float16) not in saved_on   # the installed one saves no [m, c] rows at all
    bad = {k: (err_on[k], err_off[k]) for k in err_off if not err_on[k] <= 2 * err_off[k]}
    assert not bad, bad
