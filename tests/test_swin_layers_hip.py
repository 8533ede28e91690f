"""GPU (-m gpu): the installable Swin3D layers (layers.patch_swin_classes: swin_basic_layer_forward, swin_window_attention_forward) under
the stand-in classes of tests/swin_standin.py, against the SAME classes unpatched (operators + torch rel-pos chain) on the same weights.
Bar: the installed-layer comparison of tests/test_hip_parity.py - every tensor within 1e-3 of its scale."""
import copy

import numpy as np
import pytest
import torch

from tests.util import dev

pytestmark = pytest.mark.gpu

N_SIZES, W, QUANT, C, H, DEPTH = [900, 500], 0.16, 0.01, 48, 3, 2


def _np(t):
    return t.detach().float().cpu().numpy()


@pytest.fixture(scope="module")
def problem():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from stratified_transformer_amd import pointops, scene
    from tests import swin_standin as sw
    pointops.clear_caches()
    xyz, offset = scene.make_batch(N_SIZES, seed=11)
    torch.manual_seed(5)
    layer = sw.BasicLayer(DEPTH, C, H, W, QUANT).cuda()
    with torch.no_grad():
        for blk in layer.blocks:
            for t in (blk.attn.relative_pos_query_table, blk.attn.relative_pos_key_table, blk.attn.relative_pos_value_table):
                t.normal_(std=0.2)
    g = torch.Generator().manual_seed(6)
    feats = torch.randn(xyz.shape[0], C, generator=g)
    go = torch.randn(xyz.shape[0], C, generator=g)
    return dict(sw=sw, layer=layer, xyz=dev(xyz), offset=dev(offset), feats=feats.cuda(), go=go.cuda(), ref={})


def _run(p, layer, amp):
    feats = p["feats"].clone().requires_grad_(True)
    layer.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=torch.float16, enabled=amp):
        f, x, o, f_down, x_down, o_down = layer(feats, p["xyz"], p["offset"])
    assert x is p["xyz"] and o is p["offset"] and f_down is None and x_down is None and o_down is None
    (f.float() * p["go"]).sum().backward()
    torch.cuda.synchronize()
    res = {"out": _np(f), "grad_feats": _np(feats.grad)}
    res.update({"grad." + n: _np(t.grad) for n, t in layer.named_parameters()})
    return res


def _unpatched(p, amp):
    """the stand-in's own forward (operators + torch chain): computed once per mode and kept"""
    if amp not in p["ref"]:
        sw = p["sw"]
        assert sw.BasicLayer.forward.__module__ == sw.__name__ and sw.WindowAttention.forward.__module__ == sw.__name__
        p["ref"][amp] = _run(p, p["layer"], amp)
    return p["ref"][amp]


def _close(got, want):
    assert got.keys() == want.keys()
    for name in want:
        tol = 1e-3 * max(float(np.abs(want[name]).max()), 1e-6)
        diff = float(np.abs(got[name] - want[name]).max())
        assert got[name].shape == want[name].shape and diff <= tol, (name, diff, tol)


@pytest.mark.parametrize("amp", [False, True], ids=["fp32", "autocast"])
def test_patched_swin_layer_equals_the_unpatched_classes_on_the_plan(problem, amp):
    from stratified_transformer_amd import fused, layers
    sw = problem["sw"]
    want = _unpatched(problem, amp)
    calls = {"cell": 0, "qkv": 0, "dtypes": set(), "rows": set()}
    real, real_qkv = fused.cell_attention, fused.cell_attention_qkv

    def spy(q, k, v, tq, tk, tv, plan):
        calls["cell"] += 1
        calls["rows"].add(plan.table_rows)
        return real(q, k, v, tq, tk, tv, plan)

    def spy_qkv(qkv, scale, tq, tk, tv, plan):
        calls["qkv"] += 1
        calls["dtypes"].add(qkv.dtype)
        calls["rows"].add(plan.table_rows)
        return real_qkv(qkv, scale, tq, tk, tv, plan)
    fused.cell_attention, fused.cell_attention_qkv = spy, spy_qkv
    try:
        classes = [sw.BasicLayer, sw.WindowAttention]
        assert layers.patch_swin_classes(*classes) == classes
        assert sw.BasicLayer.forward is layers.swin_basic_layer_forward and sw.WindowAttention.forward is layers.swin_window_attention_forward
        got = _run(problem, problem["layer"], amp)
    finally:
        fused.cell_attention, fused.cell_attention_qkv = real, real_qkv
        layers.uninstall_fast_layers()
    # uninstall restores the originals
    assert sw.BasicLayer.forward.__module__ == sw.__name__ and sw.WindowAttention.forward.__module__ == sw.__name__
    assert not layers._ORIGINAL
    # the plan path was taken: one fused function per block, on 31-row plans; under autocast on the half qkv where the Linear left it
    assert calls["rows"] == {31}
    if amp:
        assert calls["qkv"] == DEPTH and calls["cell"] == 0 and calls["dtypes"] == {torch.float16}
    else:
        assert calls["cell"] == DEPTH and calls["qkv"] == 0
    _close(got, want)


def test_patched_window_attention_alone_runs_on_the_pair_list(problem):
    """WindowAttention rebound without the layer (no `_sta_block`): fused.window_attention on the pair list it is given, rel-pos index by
    the torch chain; same numbers as the unpatched classes."""
    from stratified_transformer_amd import fused, layers
    sw = problem["sw"]
    want = _unpatched(problem, False)
    calls = {"window": 0, "cell": 0}
    real, real_cell = fused.window_attention, fused.cell_attention

    def spy(*a):
        calls["window"] += 1
        return real(*a)

    def spy_cell(*a):
        calls["cell"] += 1
        return real_cell(*a)
    fused.window_attention, fused.cell_attention = spy, spy_cell
    try:
        assert layers.patch_swin_classes(window_attention_cls=sw.WindowAttention) == [sw.WindowAttention]
        got = _run(problem, problem["layer"], False)
    finally:
        fused.window_attention, fused.cell_attention = real, real_cell
        layers.uninstall_fast_layers()
    assert calls == {"window": DEPTH, "cell": 0}
    _close(got, want)


def test_a_stratified_stand_in_patched_in_the_same_process_is_unaffected(problem):
    """Both variants installed at once: each class keeps its own forwards, the Stratified layer computes what it computes alone, and one
    uninstall restores both."""
    import model_standin as ms
    from stratified_transformer_amd import layers
    sw = problem["sw"]
    torch.manual_seed(9)
    strat = ms.BasicLayer(8, 2, C, H, W, QUANT).cuda()
    feats = problem["feats"]

    def run_strat():
        layers.forget_clouds()
        f = strat(feats, problem["xyz"], problem["offset"])[0]
        torch.cuda.synchronize()
        return _np(f)
    strat_classes, swin_classes = [ms.BasicLayer, ms.WindowAttention], [sw.BasicLayer, sw.WindowAttention]
    try:
        assert layers.patch_classes(*strat_classes) == strat_classes
        alone = run_strat()
        assert layers.patch_swin_classes(*swin_classes) == swin_classes
        assert ms.BasicLayer.forward is layers.basic_layer_forward and ms.WindowAttention.forward is layers.window_attention_forward
        assert sw.BasicLayer.forward is layers.swin_basic_layer_forward
        swin_out = _np(copy.deepcopy(problem["layer"])(feats, problem["xyz"], problem["offset"])[0])
        both = run_strat()
    finally:
        layers.uninstall_fast_layers()
    assert ms.BasicLayer.forward is not layers.basic_layer_forward and sw.BasicLayer.forward is not layers.swin_basic_layer_forward
    tol = 1e-3 * max(float(np.abs(alone).max()), 1e-6)
    assert float(np.abs(both - alone).max()) <= tol
    _close({"out": swin_out}, {"out": _unpatched(problem, False)["out"]})
