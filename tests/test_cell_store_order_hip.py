"""GPU (-m gpu): the query loops of the cell attention walkers store a query's results one iteration late (at the top of the next
iteration, the last query's after the loop) and the key-side flush takes all its key ids before its first atomic (csrc/cell_attn.hip,
DESIGN.md 4.6).  What that can break: the first and the last query of a piece (pieces of exactly 1, 2 and `cap` queries), the lane that
straddles the end of a row (`nvalid`: cells with nk % 16 == 1 and == 15), and the chunks after the first, which read what an earlier
chunk of the same wave stored (cells of more than 48 keys in the backward, of more than 128 in the forward).  Every test asserts on the
plan that its scene holds the case before it compares anything.

Scenes: a sparse cloud of _N points (h = 2, L = 64, pieces of at most 4 queries) for the edge pieces; the `two_chunks_L80_h8_cap8`
scene of tests/cell_edges.py for the chunks.  The forward of fp32 operands below n * h = 96000 is the matrix-core kernel
(pointops2_cell_forward_variant), so on the sparse cloud the fp32 launch reaches the VALU BACKWARD and the bf16-storage launch the VALU
forward and backward; the fp32 VALU forward runs on the two-chunk scene (valu80 on both patterns), whose plan holds pieces of 1, 2 and
cap queries and both row remainders as well.  Bars: FTOL / GTOL / TTOL of tests/cell_edges.py, as tests/test_cell_qkv_hip.py.
"""
import functools

import numpy as np
import pytest
import torch

from tests.cell_edges import (_CELL_GRADS, _SCALES, _cell_nk, _cell_nq, _cell_operands, _cell_scene, _np, _oracle_attention, _oracle_operands,
                              _packed_operands, _pair_list, _qkv_launch, _variant_scene, FTOL, GTOL, TTOL)
from tests.util import dev

pytestmark = pytest.mark.gpu

_N, _SEED, _H, _L, _CAP = 600, 1, 2, 64, 4
_TABLES = ("table_q", "table_k", "table_v")
PATTERNS = ("even", "odd")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from stratified_transformer_amd import pointops
    pointops.clear_caches()


@functools.lru_cache(maxsize=None)
def _sparse_blocks():
    _, _, even, odd = _cell_scene(_N, 1, 0.16, 0.01, _SEED, _L, _CAP)
    return dict(even=even, odd=odd)


@functools.lru_cache(maxsize=None)
def _chunk_blocks():
    blocks, variants, L, h = _variant_scene("two_chunks_L80_h8_cap8")
    assert variants == ("valu80", "valu80")
    return dict(zip(PATTERNS, blocks)), L, h


def _assert_edge_pieces(plan, cap):
    """pieces of exactly 1, 2 and cap queries; a row that ends one slot into a 16-key pass and one that ends one slot short of it"""
    nq, nk = _cell_nq(plan), _cell_nk(plan)
    assert nq.max() <= cap
    for want in (1, 2, cap):
        assert (nq == want).any(), f"no piece of exactly {want} queries"
    for rem in (1, 15):
        assert (nk % 16 == rem).any(), f"no cell with nk % 16 == {rem}"


def _launch(plan, ops, L, go):
    """tests.cell_edges._cell_launch that also returns the weight planes: out, pbuf, gsbuf and the six gradients (fp32 or bf16 storage)"""
    from stratified_transformer_amd import _lib
    n, h, _ = ops[0].shape
    sfx = "_bf16" if ops[0].dtype == torch.bfloat16 else ""
    f32 = dict(dtype=torch.float32, device="cuda")
    out, ml, pbuf = torch.empty(n, h, 16, **f32), torch.empty(n, h, 2, **f32), torch.zeros(h, max(plan.n_pairs, 1), **f32)
    ptrs = [_lib.ptr(t) for t in ops]
    _lib.call(f"cell_attention_forward{sfx}_launcher", plan.c_arg(), h, 16, L, *ptrs, _lib.ptr(out), _lib.ptr(ml), _lib.ptr(pbuf), device=out.device)
    gsbuf = torch.zeros_like(pbuf)
    grads = [torch.empty(n, h, 16, **f32)] + [torch.zeros(t.shape, **f32) for t in ops[1:]]  # grad_q fully written, the rest accumulated
    _lib.call(f"cell_attention_backward{sfx}_launcher", plan.c_arg(), h, 16, L, _lib.ptr(dev(go)), *ptrs[:3], _lib.ptr(out), *ptrs[3:], _lib.ptr(pbuf),
              _lib.ptr(gsbuf), *[_lib.ptr(g) for g in grads], device=out.device)
    return out, pbuf, gsbuf, dict(zip(_CELL_GRADS, grads))


def _check_against_oracle(what, out, grads, want, wgrads):
    np.testing.assert_allclose(_np(out), want, err_msg=f"{what} forward", **FTOL)
    for name in _CELL_GRADS:
        tol = TTOL if name.startswith("table") else GTOL
        s = max(1.0, float(np.abs(wgrads[name]).max())) if name.startswith("table") else 1.0
        np.testing.assert_allclose(_np(grads[name]) / s, wgrads[name] / s, err_msg=f"{what} grad {name}", **tol)


def _vs_oracle_twice(blk, L, h, bf16, expect, seed):
    """forward and the six gradients against the oracle; out, pbuf, gsbuf and grad_q bit for bit over two launches; the rows of
    grad_k / grad_v of a point that is a key of no cell stay zero"""
    from stratified_transformer_amd import _lib
    plan = blk.cells
    assert _lib.cell_forward_variant(plan, h, L, bf16=bf16) == expect
    p, go = _cell_operands(plan.n_points, h, L, seed)
    ops = [dev(p[x]) for x in _CELL_GRADS]
    if bf16:
        ops = [t.bfloat16() for t in ops]
        p = {x: _np(t.float()) for x, t in zip(_CELL_GRADS, ops)}
    out, pbuf, gsbuf, grads = _launch(plan, ops, L, go)
    _, i1, offs, rel = _pair_list(blk, L)
    want, wgrads = _oracle_attention(p, i1, offs, rel, go)
    what = f"{expect} {'bf16' if bf16 else 'fp32'}"
    _check_against_oracle(what, out, grads, want, wgrads)
    out2, pbuf2, gsbuf2, grads2 = _launch(plan, ops, L, go)
    for name, a, b in (("out", out, out2), ("pbuf", pbuf, pbuf2), ("gsbuf", gsbuf, gsbuf2), ("grad_q", grads["q"], grads2["q"])):
        assert torch.equal(a, b), f"{what}: {name} differs over two launches by {float((a - b).abs().max())}"
    nk_total = int(_np(plan.cell_kbase)[plan.n_cells])
    no_key = np.setdiff1d(np.arange(plan.n_points), _np(plan.cell_keys)[:nk_total])
    for name in ("k", "v"):
        assert not _np(grads[name])[no_key].any(), f"{what}: grad_{name} of a point that is no key was written"


@pytest.mark.parametrize("pattern", PATTERNS)
def test_edge_pieces_fp32_backward_and_bf16_walkers(pattern):
    """Pieces of exactly 1, 2 and cap queries, rows with nk % 16 == 1 and 15: the fp32 backward (behind the matrix-core forward) and the
    VALU forward and backward on bf16 storage, against the oracle and themselves."""
    blk = _sparse_blocks()[pattern]
    _assert_edge_pieces(blk.cells, _CAP)
    _vs_oracle_twice(blk, _L, _H, False, "mfma64", seed=31)
    _vs_oracle_twice(blk, _L, _H, True, "valu80", seed=32)


@pytest.mark.parametrize("pattern", PATTERNS)
def test_chunks_after_the_first_fp32_valu_forward_and_backward(pattern):
    """Cells of more than 48 keys (backward chunks) and of more than 128 (forward chunks: running max / sum, logits parked in pbuf, out
    and grad_q read back and added to) on the fp32 VALU forward and the backward; the plan also holds the edge pieces."""
    blocks, L, h = _chunk_blocks()
    blk = blocks[pattern]
    nk = _cell_nk(blk.cells)
    assert (nk > 48).any() and (nk > 128).any(), nk.max()
    _assert_edge_pieces(blk.cells, 8)
    _vs_oracle_twice(blk, L, h, False, "valu80", seed=33)


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_edge_pieces_packed_rows(dtype):
    """The packed (PK) instances share the sweeps: fp16 and bf16 rows of a packed qkv on the sparse cloud, both patterns, forward and
    backward against the oracle; grad_qkv[:, 0] is scale * the oracle's grad_q."""
    td = dict(float16=torch.float16, bfloat16=torch.bfloat16)[dtype]
    scale = _SCALES[dtype]
    for pattern in PATTERNS:
        blk = _sparse_blocks()[pattern]
        plan = blk.cells
        _assert_edge_pieces(plan, _CAP)
        qkv, tabs, go = _packed_operands(plan.n_points, _H, _L, 34, td)
        out, _, grads = _qkv_launch(plan, qkv, scale, tabs, _L, go)
        _, i1, offs, rel = _pair_list(blk, _L)
        want, wgrads = _oracle_attention(_oracle_operands(qkv, scale, tabs), i1, offs, rel, go)
        wgrads["q"] = np.float32(scale) * wgrads["q"]
        g_qkv = grads["qkv"]
        got = dict(q=g_qkv[:, 0], k=g_qkv[:, 1], v=g_qkv[:, 2], **{t: grads[t] for t in _TABLES})
        _check_against_oracle(f"packed {dtype} {pattern}", out, got, want, wgrads)
