"""GPU (-m gpu): the deterministic backward of the cell attention (csrc/cell_det.hip, the DET instances of csrc/cell_attn.hip):
the two reduce kernels alone on handcrafted input, the three composite launchers against their own partial buffers and against the
oracle, repeatability of fused.cell_attention / cell_attention_qkv over runs whose buffers land at other addresses, and the switches.

"Bitwise" below means equal as 32-bit patterns.  The expected sums are tests/cell_det.py's numpy restatement of the order the
C header states: a point's key slots in the order of the plan's key-major view, the table partial rows in ascending order."""
import functools

import numpy as np
import pytest
import torch

from tests import cell_det
from tests.cell_det import GUARD_ROWS, _cell_det_launch, _qkv_det_launch
from tests.cell_edges import (GTOL, TTOL, _SCALES, _cell_operands, _np, _oracle_attention, _oracle_operands, _packed_operands, _pair_list,
                              _variant_scene)
from tests.util import dev

pytestmark = pytest.mark.gpu

_TABLES = ("table_q", "table_k", "table_v")
_DTYPES = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from stratified_transformer_amd import pointops
    pointops.clear_caches()


@functools.lru_cache(maxsize=None)
def _scene(case):
    """(even, odd) blocks of a variant scene, L, h - built once for all tests of this module"""
    blocks, _, L, h = _variant_scene(case)
    return blocks, L, h


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


# ---- 1. the two reduces alone ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", [1, 3])
def test_key_reduce_follows_the_order_it_is_given(h):
    """six points with 0, 1, 3, 0, 130 and 2 slots; `order` a seeded permutation of the 136 slots cut into the points' runs (NOT sorted
    inside a run: the kernel must follow `order`); partial rows scaled by 2^+-20.  The plain layout [n, h, 16] and the k and v thirds of
    a packed [n, 3, h, 16] buffer, all NaN before: the sequential fp32 sum bit for bit, zeros for the empty points, the q third
    untouched."""
    from stratified_transformer_amd import _lib
    rng = np.random.default_rng(100 + h)
    counts = np.array([0, 1, 3, 0, 130, 2])
    n, K = counts.shape[0], int(counts.sum())
    assert K == 136
    offsets = np.r_[0, np.cumsum(counts)].astype(np.int32)
    order = rng.permutation(K).astype(np.int32)
    pk, pv = cell_det.scaled_normals(rng, (K, h, 16)), cell_det.scaled_normals(rng, (K, h, 16))
    want_k, want_v = cell_det.sequential_sum(pk, offsets, order), cell_det.sequential_sum(pv, offsets, order)
    d_off, d_ord, d_pk, d_pv = dev(offsets), dev(order), dev(pk), dev(pv)
    plain = _nan(n, h, 16)
    _lib.call("cell_key_grads_reduce_launcher", n, h, _lib.ptr(d_off), _lib.ptr(d_ord), _lib.ptr(d_pk), _lib.ptr(plain), h * 16, device=plain.device)
    assert np.array_equal(_bits(_np(plain)), _bits(want_k))
    assert not _np(plain)[[0, 3]].any()
    packed = _nan(n, 3, h, 16)
    third = h * 16 * 4  # bytes from a point's q row to its k row
    for t, part in ((1, d_pk), (2, d_pv)):
        _lib.call("cell_key_grads_reduce_launcher", n, h, _lib.ptr(d_off), _lib.ptr(d_ord), _lib.ptr(part), _lib.ptr(packed) + t * third, 3 * h * 16,
                  device=packed.device)
    got = _np(packed)
    assert np.isnan(got[:, 0]).all(), "the q third was written"
    assert np.array_equal(_bits(got[:, 1]), _bits(want_k)) and np.array_equal(_bits(got[:, 2]), _bits(want_v))
    assert not np.isnan(got[:, 1:]).any()


@pytest.mark.parametrize("L", [64, 80])
@pytest.mark.parametrize("rows", [1, 2, 37])
def test_table_reduce_adds_the_partial_rows_in_ascending_order(rows, L):
    from stratified_transformer_amd import _lib
    h = 3
    rng = np.random.default_rng(rows * 100 + L)
    parts = cell_det.scaled_normals(rng, (3 * rows, h, L * 48)).reshape(3, rows, h, L * 48)
    d_parts = dev(parts)
    grads = [_nan(L, h, 16, 3) for _ in range(3)]
    _lib.call("cell_table_grads_reduce_launcher", rows, h, L, _lib.ptr(d_parts), *[_lib.ptr(g) for g in grads], device=d_parts.device)
    for t, g in enumerate(grads):
        want = cell_det.table_from_images(cell_det.ascending_sum(parts[t]), L)
        assert not np.isnan(_np(g)).any()
        assert np.array_equal(_bits(_np(g)), _bits(want)), _TABLES[t]


def test_the_reduce_launchers_record_errors():
    from stratified_transformer_amd import _lib
    x, i = _nan(8, 16), dev(np.zeros(9, np.int32))
    with pytest.raises(RuntimeError, match="row_stride"):
        _lib.call("cell_key_grads_reduce_launcher", 8, 1, _lib.ptr(i), _lib.ptr(i), _lib.ptr(x), _lib.ptr(x), 8, device=x.device)
    with pytest.raises(RuntimeError, match="NULL"):
        _lib.call("cell_key_grads_reduce_launcher", 8, 1, None, _lib.ptr(i), _lib.ptr(x), _lib.ptr(x), 16, device=x.device)
    with pytest.raises(RuntimeError, match="partial_rows"):
        _lib.call("cell_table_grads_reduce_launcher", 0, 1, 1, _lib.ptr(x), _lib.ptr(x), _lib.ptr(x), _lib.ptr(x), device=x.device)
    torch.cuda.synchronize()
    assert bool(torch.isnan(x).all())


# ---- 2. the composite launchers against their own partials ----------------------------------------------------------------------
def _check_partials(plan, h, L, parts, grad_k, grad_v, grad_tabs, what):
    """no NaN in the partials proper, the guard rows intact, and the gradients = the fixed-order sums of those partials, bitwise"""
    K, rows = plan.n_keyslots, parts["rows"]
    kp, tp = _np(parts["key"]), _np(parts["table"])
    assert kp.shape[0] == 2 * K + GUARD_ROWS and tp.shape[0] == 3 * rows * h + GUARD_ROWS
    assert not np.isnan(kp[: 2 * K]).any(), f"{what}: {int(np.isnan(kp[: 2 * K]).any(axis=(1, 2)).sum())} of {2 * K} key partial rows hold a NaN"
    assert np.isnan(kp[2 * K:]).all(), f"{what}: a store behind the end of the key partials"
    assert not np.isnan(tp[: 3 * rows * h]).any(), f"{what}: table partials hold a NaN"
    assert np.isnan(tp[3 * rows * h:]).all(), f"{what}: a store behind the end of the table partials"
    offsets, order = (_np(t) for t in cell_det.key_view(plan))
    assert offsets.shape[0] == plan.n_points + 1 and offsets[-1] == K and np.array_equal(np.sort(order), np.arange(K))
    for name, got, plane in (("k", grad_k, kp[:K]), ("v", grad_v, kp[K: 2 * K])):
        assert not np.isnan(got).any(), f"{what} grad {name}"
        assert np.array_equal(_bits(got), _bits(cell_det.sequential_sum(plane, offsets, order))), f"{what} grad {name}: not the sequential sum of its partials"
    images = tp[: 3 * rows * h].reshape(3, rows, h, L * 48)
    for t, name in enumerate(_TABLES):
        assert not np.isnan(grad_tabs[name]).any(), f"{what} grad {name}"
        want = cell_det.table_from_images(cell_det.ascending_sum(images[t]), L)
        assert np.array_equal(_bits(grad_tabs[name]), _bits(want)), f"{what} grad {name}: not the ascending sum of its partials"


def _check_oracle(got, want, what, q_scale=1.0):
    np.testing.assert_allclose(got["q"], np.float32(q_scale) * want["q"], err_msg=f"{what} grad q", **GTOL)
    for x in ("k", "v"):
        np.testing.assert_allclose(got[x], want[x], err_msg=f"{what} grad {x}", **GTOL)
    for name in _TABLES:
        s = max(1.0, float(np.abs(want[name]).max()))
        np.testing.assert_allclose(got[name] / s, want[name] / s, err_msg=f"{what} grad {name}", **TTOL)


@pytest.mark.parametrize("case,storage", [("mfma64_h1", "float32"), ("mfma80_h3", "float32"), ("mfma80_h3", "bfloat16"),
                                          ("two_chunks_L80_h8_cap8", "float32")])
def test_unpacked_launchers_sum_their_own_partials(case, storage):
    """cell_attention_det_backward_launcher / _bf16_launcher, even and odd pattern: every output and both partial buffers NaN before
    the launch.  Afterwards grad_k / grad_v are the sequential sums of the launcher's own key partials through the plan's key-major
    view and the table gradients the ascending sums of its table partials, bit for bit; nothing behind the buffers' ends was written;
    all six gradients meet the standing bars against the oracle (bf16 storage: the oracle on the rounded operands)."""
    blocks, L, h = _scene(case)
    for pattern, blk in zip(("even", "odd"), blocks):
        plan = blk.cells
        p, go = _cell_operands(plan.n_points, h, L, seed=h + 7)
        names = ("q", "k", "v") + _TABLES
        ops = [dev(p[x]).to(_DTYPES[storage]).contiguous() for x in names]
        p = {x: _np(t.float()) for x, t in zip(names, ops)}
        _, grads, parts = _cell_det_launch(plan, ops, L, go)
        got = {x: _np(g) for x, g in grads.items()}
        what = f"{case} {storage} {pattern}"
        assert not np.isnan(got["q"]).any(), what
        _check_partials(plan, h, L, parts, got["k"], got["v"], got, what)
        _, i1, offs, rel = _pair_list(blk, L)
        _, want = _oracle_attention(p, i1, offs, rel, go)
        _check_oracle(got, want, what)


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_packed_launcher_sums_its_own_partials(dtype):
    """the same for cell_attention_qkv_det_backward_launcher on mfma64_h1, half and bf16 rows: the k and v thirds of grad_qkv (rows
    3 * h * 16 floats apart) are the sequential sums, the q third is written for every query"""
    blocks, L, h = _scene("mfma64_h1")
    scale = _SCALES[dtype]
    for pattern, blk in zip(("even", "odd"), blocks):
        plan = blk.cells
        qkv, tabs, go = _packed_operands(plan.n_points, h, L, 40, _DTYPES[dtype])
        _, grads, parts = _qkv_det_launch(plan, qkv, scale, tabs, L, go)
        g_qkv = _np(grads["qkv"])
        got = dict(q=g_qkv[:, 0], k=g_qkv[:, 1], v=g_qkv[:, 2], **{t: _np(grads[t]) for t in _TABLES})
        what = f"packed {dtype} {pattern}"
        assert not np.isnan(g_qkv).any(), what
        _check_partials(plan, h, L, parts, got["k"], got["v"], got, what)
        _, i1, offs, rel = _pair_list(blk, L)
        _, want = _oracle_attention(_oracle_operands(qkv, scale, tabs), i1, offs, rel, go)
        _check_oracle(got, want, what, q_scale=scale)


# ---- 3. repeatability -----------------------------------------------------------------------------------------------------------
def _three_runs(run):
    """run() three times with a scratch tensor of another size alive in between, so that the buffers land at other addresses"""
    results, scratch = [], []
    for i in range(3):
        results.append(run())
        scratch.append(torch.empty((i + 1) * 1_000_003, dtype=torch.uint8, device="cuda"))
    torch.cuda.synchronize()
    return results


def test_cell_attention_repeats_itself_bit_for_bit():
    from stratified_transformer_amd import fused
    blocks, L, h = _scene("two_chunks_L80_h8_cap8")
    plan = blocks[1].cells
    plan.key_view = None
    views = fused.CELL_KEY_VIEWS
    p, go = _cell_operands(plan.n_points, h, L, seed=3)
    ops = [dev(p[x]) for x in ("q", "k", "v") + _TABLES]
    d_go = dev(go)

    def run():
        leaves = [t.clone().requires_grad_(True) for t in ops]
        out = fused.cell_attention(*leaves, plan, deterministic=True)
        out.backward(d_go)
        return [out.detach()] + [t.grad for t in leaves]
    first, *others = _three_runs(run)
    assert fused.CELL_KEY_VIEWS == views + 1, "the plan's key-major view was not built exactly once"
    assert all(bool(torch.isfinite(t).all()) for t in first)
    for other in others:
        for name, a, b in zip(("out", "q", "k", "v") + _TABLES, first, other):
            assert a.data_ptr() != b.data_ptr()
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), name


def test_cell_attention_qkv_repeats_itself_bit_for_bit():
    from stratified_transformer_amd import fused
    blocks, L, h = _scene("mfma64_h1")
    plan = blocks[0].cells
    plan.key_view = None
    views = fused.CELL_KEY_VIEWS
    qkv, tabs, go = _packed_operands(plan.n_points, h, L, 41, torch.float16)
    d_go = dev(go)

    def run():
        leaf = qkv.clone().requires_grad_(True)
        tl = [t.clone().requires_grad_(True) for t in tabs]
        out = fused.cell_attention_qkv(leaf, _SCALES["float16"], *tl, plan, deterministic=True)
        out.backward(d_go)
        assert leaf.grad.dtype == torch.float16
        return [out.detach(), leaf.grad.float()] + [t.grad for t in tl]
    first, *others = _three_runs(run)
    assert fused.CELL_KEY_VIEWS == views + 1
    assert all(bool(torch.isfinite(t).all()) for t in first)
    for other in others:
        for name, a, b in zip(("out", "qkv") + _TABLES, first, other):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), name


# ---- 4. the switches ------------------------------------------------------------------------------------------------------------
def test_the_module_switch_takes_the_new_path(monkeypatch):
    """deterministic=None follows fused.DETERMINISTIC: with it on, the backward calls the deterministic launcher (and only then)"""
    from stratified_transformer_amd import _lib, fused
    blocks, L, h = _scene("mfma64_h1")
    plan = blocks[0].cells
    p, go = _cell_operands(plan.n_points, h, L, seed=9)
    ops = [dev(p[x]) for x in ("q", "k", "v") + _TABLES]
    called = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a, **kw: (called.append(name), real(name, *a, **kw))[1])

    def backward_launcher():
        del called[:]
        leaves = [t.clone().requires_grad_(True) for t in ops]
        fused.cell_attention(*leaves, plan).backward(dev(go))
        return [c for c in called if "backward" in c]
    assert backward_launcher() == ["cell_attention_backward_launcher"]
    try:
        fused.DETERMINISTIC = True
        assert backward_launcher() == ["cell_attention_det_backward_launcher"]
    finally:
        fused.DETERMINISTIC = False
    assert backward_launcher() == ["cell_attention_backward_launcher"]


@pytest.mark.parametrize("amp", [False, True])
def test_the_installed_layer_switch(amp):
    """layers.DETERMINISTIC_ATTENTION on a stand-in WindowAttention with a block's plan attached (fp32: fused.cell_attention; under
    autocast: fused.cell_attention_qkv on the half qkv): two backward passes give the same bits in qkv.weight.grad and the three
    table gradients"""
    from stratified_transformer_amd import layers, standin
    blocks, L, h = _scene("mfma80_h3")
    blk = blocks[1]
    n = blk.cells.n_points
    torch.manual_seed(12)
    attn = standin.WindowAttention(h * 16, 0.1, h, 0.005).cuda()
    assert attn.relative_pos_query_table.shape[0] == L
    with torch.no_grad():
        for t in (attn.relative_pos_query_table, attn.relative_pos_key_table, attn.relative_pos_value_table):
            t.normal_(std=0.5)
    attn._sta_block = blk
    feats = torch.randn(n, h * 16, device="cuda")
    go = torch.randn(n, h * 16, device="cuda")
    n_max = (blk.offsets[1:] - blk.offsets[:-1]).max()
    params = dict(qkv=attn.qkv.weight, table_q=attn.relative_pos_query_table, table_k=attn.relative_pos_key_table, table_v=attn.relative_pos_value_table)

    def run():
        attn.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.float16, enabled=amp):
            out = layers.window_attention_forward(attn, feats, None, blk.index_0, blk.index_1, blk.offsets, n_max)
        (out.float() * go).sum().backward()
        return {k: v.grad.clone() for k, v in params.items()}
    try:
        layers.DETERMINISTIC_ATTENTION = True
        a = run()
        scratch = torch.empty(3_000_001, dtype=torch.uint8, device="cuda")  # noqa: F841 (other addresses for the second pass)
        b = run()
    finally:
        layers.DETERMINISTIC_ATTENTION = False
    for name in params:
        assert bool(torch.isfinite(a[name]).all()) and float(a[name].abs().max()) > 0, name
        assert torch.equal(a[name].view(torch.int32), b[name].view(torch.int32)), name


def test_a_partial_plan_is_refused():
    """deterministic=True on plan.share(0, 2) raises; the C launcher records an error for such a plan and writes nothing"""
    from stratified_transformer_amd import fused
    blocks, L, h = _scene("mfma64_h1")
    plan = blocks[0].cells
    share = plan.share(0, 2)
    assert share.partial
    p, go = _cell_operands(plan.n_points, h, L, seed=11)
    ops = [dev(p[x]) for x in ("q", "k", "v") + _TABLES]
    with pytest.raises(RuntimeError, match="partial plan"):
        fused.cell_attention(*ops, share, deterministic=True)
    qkv, tabs, _ = _packed_operands(plan.n_points, h, L, 42, torch.float32)
    with pytest.raises(RuntimeError, match="partial plan"):
        fused.cell_attention_qkv(qkv, 0.25, *tabs, share, deterministic=True)
    fused.cell_attention(*ops, share, deterministic=False)  # the default mode still serves a share
    # the C entry points themselves: the forward serves the share, the deterministic backward records an error ...
    with pytest.raises(RuntimeError, match="cell_attention_det_backward_launcher.*share of the cells"):
        _cell_det_launch(share, ops, L, go)
    with pytest.raises(RuntimeError, match="cell_attention_qkv_det_backward_launcher.*share of the cells"):
        _qkv_det_launch(share, qkv, 0.25, tabs, L, go)
    # ... and writes nothing: the same call by hand, keeping the NaN-filled outputs
    from stratified_transformer_amd import _lib
    n = plan.n_points
    f32 = dict(dtype=torch.float32, device="cuda")
    out, pbuf = torch.zeros(n, h, 16, **f32), torch.zeros(h, plan.n_pairs, **f32)
    grads = [_nan(*t.shape) for t in ops]
    offsets, order = cell_det.key_view(plan)
    kp, tp, _, kfloats, tfloats = cell_det._det_buffers(plan, h, L)
    with pytest.raises(RuntimeError, match="share of the cells"):
        _lib.call("cell_attention_det_backward_launcher", share.c_arg(), h, 16, L, _lib.ptr(dev(go)), *[_lib.ptr(t) for t in ops[:3]], _lib.ptr(out),
                  *[_lib.ptr(t) for t in ops[3:]], _lib.ptr(pbuf), _lib.ptr(pbuf.clone()), *[_lib.ptr(g) for g in grads], _lib.ptr(offsets), _lib.ptr(order),
                  _lib.ptr(kp), kfloats, _lib.ptr(tp), tfloats, device=out.device)
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in grads + [kp, tp])
