"""Helpers of the deterministic cell-attention tests (tests/test_cell_det_*.py): the sequential fp32 sums the two reduce kernels
must reproduce bit for bit, restated in numpy, and launch helpers for the deterministic launchers of the C ABI, next to
tests/cell_edges.py's _cell_launch / _qkv_launch.  Nothing here needs a GPU to be imported."""
import numpy as np

from tests.cell_edges import _CELL_GRADS

GUARD_ROWS = 64  # NaN rows behind the end of each partial buffer: a store past the end shows


def sequential_sum(partials, offsets, order):
    """out[i] = ((0 + partials[order[a]]) + partials[order[a + 1]]) + ... over a .. b - 1 = offsets[i] .. offsets[i + 1] - 1, in fp32:
    a loop over the position inside a key, vectorised over the keys.  partials [K, ...] float32 -> [len(offsets) - 1, ...] float32."""
    assert partials.dtype == np.float32
    offsets, order = np.asarray(offsets, np.int64), np.asarray(order, np.int64)
    counts = np.diff(offsets)
    out = np.zeros((counts.shape[0],) + partials.shape[1:], np.float32)
    for j in range(int(counts.max()) if counts.size else 0):
        live = np.flatnonzero(counts > j)
        out[live] = out[live] + partials[order[offsets[live] + j]]  # one rounding to fp32 per add
    return out


def sequential_sum_loop(partials, offsets, order):
    """the same as a plain Python loop, one add at a time"""
    out = np.zeros((len(offsets) - 1,) + partials.shape[1:], np.float32)
    for i in range(len(offsets) - 1):
        s = np.zeros(partials.shape[1:], np.float32)
        for e in range(int(offsets[i]), int(offsets[i + 1])):
            s = (s + partials[int(order[e])]).astype(np.float32)
        out[i] = s
    return out


def ascending_sum(rows):
    """((0 + rows[0]) + rows[1]) + ... in fp32 over axis 0"""
    assert rows.dtype == np.float32
    s = np.zeros(rows.shape[1:], np.float32)
    for r in rows:
        s = s + r
    return s


def table_from_images(images, L):
    """the table gradient [L, h, 16, 3] that the summed images [h, L * 48] of the table bodies stand for"""
    h = images.shape[0]
    return np.ascontiguousarray(images.reshape(h, L, 16, 3).transpose(1, 0, 2, 3))


def scaled_normals(rng, shape):
    """standard normals times 2^+-20 per leading row: a sum of such rows shows any other order of its adds"""
    x = rng.standard_normal(shape, dtype=np.float32)
    s = np.float32(2.0) ** rng.choice(np.array([-20, 20]), size=shape[0]).astype(np.float32)
    return x * s.reshape((-1,) + (1,) * (len(shape) - 1))


def key_view(plan):
    """(slot_offsets, slot_order) of a plan, device tensors (the package's own, built once per plan)"""
    from stratified_transformer_amd import fused
    return fused._cell_key_view(plan)


def _nan(*shape):
    import torch
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def _det_buffers(plan, h, L):
    """NaN-filled key partials [2 * K + GUARD_ROWS, h, 16] and table partials [3 * rows * h + GUARD_ROWS, L * 48], and the sizes (in
    floats, without the guard rows) the launchers are told"""
    from stratified_transformer_amd import _lib
    rows = int(_lib.lib().pointops2_cell_table_partial_rows(plan.c_arg(), h))
    K = plan.n_keyslots
    kp, tp = _nan(2 * K + GUARD_ROWS, h, 16), _nan(3 * rows * h + GUARD_ROWS, L * 48)
    return kp, tp, rows, 2 * K * h * 16, 3 * rows * h * L * 48


def _cell_det_launch(plan, ops, L, go):
    """The cell forward and the DETERMINISTIC backward through the C ABI, fp32 or bf16 storage by the operands' dtype.  Every output
    and both partial buffers start as NaN.  Returns out, the six gradients, and dict(key=[2 K + guard rows, h, 16] (dK then dV),
    table=[3 rows h + guard rows, L * 48], rows=the table partial rows)."""
    import torch
    from stratified_transformer_amd import _lib
    from tests.util import dev
    n, h, _ = ops[0].shape
    sfx = "_bf16" if ops[0].dtype == torch.bfloat16 else ""
    f32 = dict(dtype=torch.float32, device="cuda")
    out, ml, pbuf = torch.empty(n, h, 16, **f32), torch.empty(n, h, 2, **f32), torch.empty(h, max(plan.n_pairs, 1), **f32)
    ptrs = [_lib.ptr(t) for t in ops]
    _lib.call(f"cell_attention_forward{sfx}_launcher", plan.c_arg(), h, 16, L, *ptrs, _lib.ptr(out), _lib.ptr(ml), _lib.ptr(pbuf), device=out.device)
    gsbuf = torch.empty_like(pbuf)
    grads = [_nan(*t.shape) for t in ops]
    offsets, order = key_view(plan)
    kp, tp, rows, kfloats, tfloats = _det_buffers(plan, h, L)
    _lib.call(f"cell_attention_det_backward{sfx}_launcher", plan.c_arg(), h, 16, L, _lib.ptr(dev(go)), *ptrs[:3], _lib.ptr(out), *ptrs[3:], _lib.ptr(pbuf),
              _lib.ptr(gsbuf), *[_lib.ptr(g) for g in grads], _lib.ptr(offsets), _lib.ptr(order), _lib.ptr(kp), kfloats, _lib.ptr(tp), tfloats,
              device=out.device)
    return out, dict(zip(_CELL_GRADS, grads)), dict(key=kp, table=tp, rows=rows)


def _qkv_det_launch(plan, qkv, scale, tabs, L, go):
    """The packed forward and the DETERMINISTIC packed backward through the C ABI: out, dict(qkv=grad_qkv [n, 3, h, 16], table_q, ..),
    the partials as _cell_det_launch returns them.  Every output and both partial buffers start as NaN."""
    import torch
    from stratified_transformer_amd import _lib
    from tests.util import dev
    n, _, h, _ = qkv.shape
    f32 = dict(dtype=torch.float32, device="cuda")
    out, ml, pbuf = torch.empty(n, h, 16, **f32), torch.empty(n, h, 2, **f32), torch.zeros(h, max(plan.n_pairs, 1), **f32)
    rt = _lib.ROW_TYPES[qkv.dtype]
    tpt = [_lib.ptr(t) for t in tabs]
    _lib.call("cell_attention_qkv_forward_launcher", plan.c_arg(), h, 16, L, _lib.ptr(qkv), rt, float(scale), *tpt, _lib.ptr(out), _lib.ptr(ml),
              _lib.ptr(pbuf), device=out.device)
    gsbuf = torch.empty_like(pbuf)
    g_qkv = _nan(n, 3, h, 16)
    g_tabs = [_nan(*t.shape) for t in tabs]
    offsets, order = key_view(plan)
    kp, tp, rows, kfloats, tfloats = _det_buffers(plan, h, L)
    _lib.call("cell_attention_qkv_det_backward_launcher", plan.c_arg(), h, 16, L, _lib.ptr(dev(go)), _lib.ptr(qkv), rt, float(scale), _lib.ptr(out), *tpt,
              _lib.ptr(pbuf), _lib.ptr(gsbuf), _lib.ptr(g_qkv), *[_lib.ptr(g) for g in g_tabs], _lib.ptr(offsets), _lib.ptr(order), _lib.ptr(kp), kfloats,
              _lib.ptr(tp), tfloats, device=out.device)
    return out, dict(qkv=g_qkv, table_q=g_tabs[0], table_k=g_tabs[1], table_v=g_tabs[2]), dict(key=kp, table=tp, rows=rows)
