"""Optional fused fast path of WindowAttention.forward's operator sequence.

The reference model calls five operators per attention block
(model/stratified_transformer.py:183-208: attention_step1_v2, dot_prod_with_idx_v3, `+`, scatter_softmax,
attention_step2_with_rel_pos_value_v2).  `window_attention` below is ONE autograd function for the whole
sequence.  It is an addition, not a replacement: the model file runs unmodified on the operator API without
it; a caller that owns its attention module can call it instead and gets

  * forward: logits + softmax in one kernel (`window_logits_softmax_forward_launcher`: the key rows are
    gathered once instead of twice, the three [M, h] intermediates a1, a2, a1+a2 never exist), then the
    A4 kernel; only the softmax output [M, h] is kept for the backward;
  * backward: two walks over the pair list instead of seven (`window_attention_backward_launcher`: by query
    grad_attn -> softmax backward -> grad_logit and grad_q; by key grad_k and grad_v) plus the three table
    gradients; without a key-major view the operators' own backward launchers, in autograd's order;
  * the same numbers: every term is computed as the separate operators compute it (bit-identical for
    h = 3 or 4 heads, equal up to the order of the softmax sum otherwise).

d = 16 only (the shipped configs); other head dims: use the operators.
"""
import torch
from torch.autograd import Function

from . import _lib
from . import pointops as P
from . import pointops2_cuda as pointops_cuda
from ._lib import ptr


class WindowAttention(Function):
    @staticmethod
    def forward(ctx, q, k, v, table_q, table_k, table_v, index0_offsets, index1, rel_idx):
        for t in (q, k, v, table_q, table_k, table_v, index0_offsets, index1, rel_idx):
            assert t.is_contiguous()
        N, h, hdim = q.shape
        if hdim != 16:
            raise RuntimeError("window_attention: d != 16 (use the operators of pointops for other head dims)")
        M = index1.shape[0]
        L = table_q.shape[0]
        assert table_k.shape[0] == L and table_v.shape[0] == L
        P._check_pair_list("window_attention", N, index0_offsets, index1, rel_idx)
        _lib.check_tensors((q, torch.float32, "q"), (k, torch.float32, "k"), (v, torch.float32, "v"),
                           (table_q, torch.float32, "table_q"), (table_k, torch.float32, "table_k"), (table_v, torch.float32, "table_v"),
                           (index0_offsets, torch.int32, "index0_offsets"), (index1, torch.int32, "index1"), (rel_idx, torch.int32, "rel_idx"))
        attn = torch.empty((M, h), dtype=torch.float32, device=q.device)
        out = torch.zeros((N, h, hdim), dtype=torch.float32, device=q.device)
        opts = _lib.with_table_rows(P.pair_opts(index0_offsets, index1), L)  # (the pair walkers take their rows in window order, csrc/common.h)
        _lib.call("window_logits_softmax_forward_launcher", int(index0_offsets.shape[0]) - 1, M, h, hdim, ptr(q), ptr(index0_offsets), ptr(k),
                  ptr(index1), ptr(table_q), ptr(table_k), ptr(rel_idx), ptr(attn), device=q.device, opts=opts)
        pointops_cuda.attention_step2_with_rel_pos_value_forward_cuda_v2(N, M, h, hdim, 0, attn, v, index0_offsets, index1, table_v, rel_idx, out,
                                                                         opts=opts)
        ctx.save_for_backward(q, k, v, table_q, table_k, table_v, index0_offsets, index1, rel_idx, attn)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        q, k, v, table_q, table_k, table_v, offs, index1, rel_idx, attn = ctx.saved_tensors
        N, h, hdim = q.shape
        NK = k.shape[0]
        M = index1.shape[0]
        L = table_q.shape[0]
        dev = q.device
        grad_out = grad_out.contiguous()
        z = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)  # noqa: E731
        e = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)  # noqa: E731
        csc = P.csc_of(offs, index1, NK)
        opts = _lib.with_table_rows(P.pair_opts(offs, index1, csc=csc), L)  # (the same options serve every launch below: one L, one pair list)
        if csc is not None and L <= 80:
            # two walks (by query, by key) + the three table gradients: DESIGN.md 4.5
            grad_logit, grad_q, grad_k, grad_v = e(M, h), e(N, h, hdim), e(NK, h, hdim), e(v.shape[0], h, hdim)
            grad_tq, grad_tk, grad_tv = z(L, h, hdim, 3), z(L, h, hdim, 3), z(L, h, hdim, 3)
            _lib.check_tensors((grad_out, torch.float32, "grad_out"))
            _lib.call("window_attention_backward_launcher", int(offs.shape[0]) - 1, M, h, hdim, ptr(grad_out), ptr(q), ptr(k), ptr(v), ptr(attn),
                      ptr(offs), ptr(index1), ptr(table_q), ptr(table_k), ptr(table_v), ptr(rel_idx), ptr(grad_logit), ptr(grad_q), ptr(grad_k),
                      ptr(grad_v), ptr(grad_tq), ptr(grad_tk), ptr(grad_tv), device=dev, opts=opts)
            return grad_q, grad_k, grad_v, grad_tq, grad_tk, grad_tv, None, None, None
        # the operators' own backward launchers, in autograd's order
        grad_attn = e(M, h)
        grad_v, grad_tv = z(v.shape[0], h, hdim), z(L, h, hdim, 3)
        pointops_cuda.attention_step2_with_rel_pos_value_backward_cuda_v2(N, M, h, hdim, 0, grad_out, offs, index1, attn, v, table_v, rel_idx,
                                                                          grad_attn, grad_v, grad_tv, opts=opts)
        grad_logit = e(M, h)
        _lib.call("segment_softmax_backward_launcher", int(offs.shape[0]) - 1, M, h, ptr(attn), ptr(grad_attn), ptr(offs), ptr(grad_logit), device=dev)
        # A1 and A2 receive the same gradient; grad_k is accumulated by both into one buffer
        gq1, gq2 = e(N, h, hdim), e(N, h, hdim)
        grad_k = z(NK, h, hdim)
        grad_tq, grad_tk = z(L, h, hdim, 3), z(L, h, hdim, 3)
        pointops_cuda.attention_step1_backward_cuda_v2(int(offs.shape[0]) - 1, M, h, h * hdim, 0, grad_logit, offs, index1, q, k, gq1, grad_k,
                                                       opts=opts)
        pointops_cuda.dot_prod_with_idx_backward_cuda_v3(N, M, h, hdim, 0, grad_logit, q, offs, k, index1, table_q, table_k, rel_idx,
                                                         gq2, grad_k, grad_tq, grad_tk, opts=opts)
        return gq1.add_(gq2), grad_k, grad_v, grad_tq, grad_tk, grad_tv, None, None, None


def window_attention(q, k, v, table_q, table_k, table_v, index0_offsets, index1, rel_idx):
    """q, k, v [N, h, 16] f32 (q already scaled, as the model does at :181); tables [L, h, 16, 3]; the block's CSR
    pair list (index0_offsets [N+1], index1 [M] i32) and rel_idx [M, 3] i32  ->  [N, h, 16]"""
    return WindowAttention.apply(q, k, v, table_q, table_k, table_v, index0_offsets, index1, rel_idx)


def _cell_checks(plan, hdim, L, rows, needs_grad):
    """What both cell functions refuse before they launch; rows: the row counts of q, k, v."""
    if hdim != 16:
        raise RuntimeError("cell_attention: d != 16 (use the operators of pointops for other head dims)")
    if any(r != plan.n_points for r in rows):
        raise RuntimeError("cell_attention: the plan was built for %d points, q/k/v have %d/%d/%d rows" % (plan.n_points, *rows))
    # The plan's packed rel-pos indices were clamped to [0, plan.table_rows) when it was filled and the kernels take the
    # tables' L as the axis stride of their LDS image: any other L would index another axis / table (the model asserts the
    # index range instead, model/stratified_transformer.py:189-190).
    if L != plan.table_rows:
        raise RuntimeError("cell_attention: the plan was built for tables of %d rows (cell_table_rows), the tables have %d" % (plan.table_rows, L))
    if L > 80 and needs_grad:
        raise RuntimeError("cell_attention: the backward supports at most 80 table rows (L = %d): use the operators of pointops, "
                           "or run the forward under torch.no_grad()" % L)


def _cell_forward_buffers(plan, N, h, dev):
    """out [N, h, 16], ml [N, h, 2], pbuf [h, n_pairs], fp32."""
    # a plan restricted to a share of the cells (CellPlan.share: one scene over several ranks) leaves the other cells' rows and
    # tile entries untouched: they must read as zero (the ranks' outputs are summed; the key-side table gradient walks all cells)
    alloc = torch.zeros if plan.partial else torch.empty
    f32 = dict(dtype=torch.float32, device=dev)
    return alloc((N, h, 16), **f32), torch.empty((N, h, 2), **f32), alloc((h, max(plan.n_pairs, 1)), **f32)


def _cell_backward_buffers(plan, pbuf, *accumulated):
    """gsbuf like pbuf, and one zero-filled fp32 gradient per tensor of `accumulated`: views of ONE buffer, so that a block pays one
    fill kernel instead of one per gradient."""
    gsbuf = torch.zeros_like(pbuf) if plan.partial else torch.empty_like(pbuf)
    acc = torch.zeros(sum(t.numel() for t in accumulated), dtype=torch.float32, device=pbuf.device)
    return gsbuf, [g.view(t.shape) for g, t in zip(acc.split([t.numel() for t in accumulated]), accumulated)]


# The backward of cell_attention / cell_attention_qkv without float atomics (csrc/cell_det.hip): dK, dV and the table
# gradients are stored as partial sums and added per destination in a fixed order, so two runs of one build on one device model give
# the same bits.  What `deterministic=None` means at a call; the forward is the same kernel either way.
DETERMINISTIC = False
CELL_KEY_VIEWS = 0  # key-major views of a plan's key list built so far (tests: one per plan, not one per block)


def _cell_key_view(plan):
    """(slot_offsets [N + 1], slot_order [K]) of plan.cell_keys: per point its key slots, ascending.  Built once per plan."""
    if plan.key_view is None:
        global CELL_KEY_VIEWS
        CELL_KEY_VIEWS += 1
        K = plan.n_keyslots
        rows = torch.arange(K + 1, dtype=torch.int32, device=plan.cell_keys.device)
        offsets, order, _ = P._csc_build(rows, plan.cell_keys[:K], plan.n_points)
        plan.key_view = (offsets, order)
    return plan.key_view


def _deterministic(flag, plan, name):
    det = DETERMINISTIC if flag is None else bool(flag)
    if det and plan.partial:
        raise RuntimeError("%s: deterministic=True on a partial plan (CellPlan.share / with_tasks): the ranks' gradients are summed by an "
                           "all-reduce whose order this mode does not fix" % name)
    return det


def cell_partial_buffers(plan, h, L, dev):
    """The two workspaces of a deterministic backward, uninitialised: key partials [2, K, h, 16] (dK, dV per key slot) and table partials
    [3, rows, h, L * 48] (an image of each table per workgroup), fp32."""
    rows = int(_lib.lib().pointops2_cell_table_partial_rows(plan.c_arg(), int(h)))
    f32 = dict(dtype=torch.float32, device=dev)
    return torch.empty((2, max(plan.n_keyslots, 1), h, 16), **f32), torch.empty((3, rows, h, L * 48), **f32)


def _det_args(plan, h, L, dev):
    """the trailing arguments of the cell_attention_*det_backward launchers (and the tensors behind them, to be kept alive over the launch)"""
    offsets, order = _cell_key_view(plan)
    kp, tp = cell_partial_buffers(plan, h, L, dev)
    return (ptr(offsets), ptr(order), ptr(kp), kp.numel(), ptr(tp), tp.numel()), (kp, tp)


def _as_operand(dtype, *grads):
    """autograd wants a gradient of the operand's dtype; the kernels took the sums in fp32"""
    return grads if dtype == torch.float32 else tuple(g.to(dtype) for g in grads)


class CellAttention(Function):
    """The same operator sequence on a cell plan (index_build.CellPlan; csrc/cell_attn.hip): one wave per
    (cell, head) loads the cell's key / value rows once for all its queries; the backward keeps dK / dV of a cell in
    registers and takes the three table gradients from cell-ordered softmax weights / logit gradients."""

    @staticmethod
    def forward(ctx, q, k, v, table_q, table_k, table_v, plan, det=False):
        N, h, hdim = q.shape
        L = table_q.shape[0]
        _cell_checks(plan, hdim, L, (N, k.shape[0], v.shape[0]), any(ctx.needs_input_grad[:6]))
        st = q.dtype  # storage type of q / k / v / tables: fp32, or bf16 (fp32 arithmetic and outputs either way)
        if st not in (torch.float32, torch.bfloat16):
            raise TypeError("cell_attention: q / k / v / tables must all be float32 or all bfloat16, got %s" % st)
        _lib.check_tensors((q, st, "q"), (k, st, "k"), (v, st, "v"), (table_q, st, "table_q"), (table_k, st, "table_k"), (table_v, st, "table_v"))
        assert table_k.shape == table_q.shape and table_v.shape == table_q.shape
        out, ml, pbuf = _cell_forward_buffers(plan, N, h, q.device)
        _lib.call("cell_attention_forward_launcher" if st == torch.float32 else "cell_attention_forward_bf16_launcher", plan.c_arg(), h, hdim, L, ptr(q), ptr(k), ptr(v), ptr(table_q), ptr(table_k), ptr(table_v),
                  ptr(out), ptr(ml), ptr(pbuf), device=q.device)
        ctx.plan, ctx.det = plan, det
        ctx.save_for_backward(q, k, v, table_q, table_k, table_v, out, pbuf)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        q, k, v, table_q, table_k, table_v, out, pbuf = ctx.saved_tensors
        plan = ctx.plan
        N, h, hdim = q.shape
        L = table_q.shape[0]
        grad_out = grad_out.contiguous()
        _lib.check_tensors((grad_out, torch.float32, "grad_out"))
        if ctx.det:  # every gradient is fully written: nothing to zero-fill
            gsbuf = torch.empty_like(pbuf)
            grad_q, grad_k, grad_v, gtq, gtk, gtv = (torch.empty(t.shape, dtype=torch.float32, device=q.device) for t in (q, k, v, table_q, table_k, table_v))
            det_args, _keep = _det_args(plan, h, L, q.device)
            _lib.call("cell_attention_det_backward_launcher" if q.dtype == torch.float32 else "cell_attention_det_backward_bf16_launcher", plan.c_arg(), h, hdim, L,
                      ptr(grad_out), ptr(q), ptr(k), ptr(v), ptr(out), ptr(table_q), ptr(table_k), ptr(table_v), ptr(pbuf), ptr(gsbuf), ptr(grad_q), ptr(grad_k),
                      ptr(grad_v), ptr(gtq), ptr(gtk), ptr(gtv), *det_args, device=q.device)
            return (*_as_operand(q.dtype, grad_q, grad_k, grad_v, gtq, gtk, gtv), None, None)
        grad_q = (torch.zeros if plan.partial else torch.empty)(q.shape, dtype=torch.float32, device=q.device)
        gsbuf, (grad_k, grad_v, gtq, gtk, gtv) = _cell_backward_buffers(plan, pbuf, k, v, table_q, table_k, table_v)
        _lib.call("cell_attention_backward_launcher" if q.dtype == torch.float32 else "cell_attention_backward_bf16_launcher", plan.c_arg(), h, hdim, L, ptr(grad_out), ptr(q), ptr(k), ptr(v), ptr(out), ptr(table_q),
                  ptr(table_k), ptr(table_v), ptr(pbuf), ptr(gsbuf), ptr(grad_q), ptr(grad_k), ptr(grad_v), ptr(gtq), ptr(gtk), ptr(gtv),
                  device=q.device)
        return (*_as_operand(q.dtype, grad_q, grad_k, grad_v, gtq, gtk, gtv), None, None)


def cell_attention(q, k, v, table_q, table_k, table_v, plan, deterministic=None):
    """q, k, v [N, h, 16] f32 (q already scaled, :181); tables [L, h, 16, 3]; plan = BlockIndex.cells of the block's
    pattern (index_build.stage_index_hip(..., cell_table_rows=L))  ->  [N, h, 16], same numbers as the five operators
    up to the order of the sums.  deterministic (None: fused.DETERMINISTIC): the backward without float atomics - the same gradient
    bits from run to run on one device model, at the price of two partial buffers (cell_partial_buffers); not for a partial plan."""
    return CellAttention.apply(q, k, v, table_q, table_k, table_v, plan, _deterministic(deterministic, plan, "cell_attention"))


class CellAttentionQKV(Function):
    """CellAttention on the packed projection: the kernels read q, k, v rows out of qkv [N, 3, h, 16] where the model's qkv Linear
    left them (fp32, or fp16 / bf16 under autocast), scale q as they load it and write one fp32 gradient buffer of qkv's shape.
    Saved for the backward: qkv itself, the tables, out and pbuf - no [N, h, 16] copy of q, k or v."""

    @staticmethod
    def forward(ctx, qkv, scale, table_q, table_k, table_v, plan, det=False):
        if qkv.dim() != 4 or qkv.shape[1] != 3:
            raise RuntimeError("cell_attention_qkv: qkv must be [N, 3, h, 16], got %s" % (tuple(qkv.shape),))
        N, _, h, hdim = qkv.shape
        L = table_q.shape[0]
        _cell_checks(plan, hdim, L, (N, N, N), any(ctx.needs_input_grad[:5]))
        if qkv.dtype not in _lib.ROW_TYPES:
            raise TypeError("cell_attention_qkv: qkv must be float32, float16 or bfloat16, got %s" % qkv.dtype)
        f32 = torch.float32
        _lib.check_tensors((qkv, qkv.dtype, "qkv"), (table_q, f32, "table_q"), (table_k, f32, "table_k"), (table_v, f32, "table_v"))
        assert table_k.shape == table_q.shape and table_v.shape == table_q.shape
        out, ml, pbuf = _cell_forward_buffers(plan, N, h, qkv.device)
        _lib.call("cell_attention_qkv_forward_launcher", plan.c_arg(), h, hdim, L, ptr(qkv), _lib.ROW_TYPES[qkv.dtype], float(scale), ptr(table_q),
                  ptr(table_k), ptr(table_v), ptr(out), ptr(ml), ptr(pbuf), device=qkv.device)
        ctx.plan, ctx.scale, ctx.det = plan, float(scale), det
        ctx.save_for_backward(qkv, table_q, table_k, table_v, out, pbuf)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        qkv, table_q, table_k, table_v, out, pbuf = ctx.saved_tensors
        plan = ctx.plan
        N, _, h, hdim = qkv.shape
        L = table_q.shape[0]
        grad_out = grad_out.contiguous()
        _lib.check_tensors((grad_out, torch.float32, "grad_out"))
        if ctx.det:  # every gradient is fully written: nothing to zero-fill
            gsbuf = torch.empty_like(pbuf)
            grad_qkv, gtq, gtk, gtv = (torch.empty(t.shape, dtype=torch.float32, device=qkv.device) for t in (qkv, table_q, table_k, table_v))
            det_args, _keep = _det_args(plan, h, L, qkv.device)
            _lib.call("cell_attention_qkv_det_backward_launcher", plan.c_arg(), h, hdim, L, ptr(grad_out), ptr(qkv), _lib.ROW_TYPES[qkv.dtype], ctx.scale,
                      ptr(out), ptr(table_q), ptr(table_k), ptr(table_v), ptr(pbuf), ptr(gsbuf), ptr(grad_qkv), ptr(gtq), ptr(gtk), ptr(gtv), *det_args,
                      device=qkv.device)
            return (*_as_operand(qkv.dtype, grad_qkv), None, gtq, gtk, gtv, None, None)
        gsbuf, (grad_qkv, gtq, gtk, gtv) = _cell_backward_buffers(plan, pbuf, qkv, table_q, table_k, table_v)
        _lib.call("cell_attention_qkv_backward_launcher", plan.c_arg(), h, hdim, L, ptr(grad_out), ptr(qkv), _lib.ROW_TYPES[qkv.dtype], ctx.scale,
                  ptr(out), ptr(table_q), ptr(table_k), ptr(table_v), ptr(pbuf), ptr(gsbuf), ptr(grad_qkv), ptr(gtq), ptr(gtk), ptr(gtv), device=qkv.device)
        return (*_as_operand(qkv.dtype, grad_qkv), None, gtq, gtk, gtv, None, None)


def cell_attention_qkv(qkv, scale, table_q, table_k, table_v, plan, deterministic=None):
    """qkv [N, 3, h, 16] contiguous, f32 / f16 / bf16: the qkv Linear's output as it stands (`self.qkv(feats).view(N, 3, h, 16)`, under
    autocast too), q NOT yet scaled; scale: the model's `self.scale`; tables [L, h, 16, 3] f32; plan as for cell_attention
    ->  [N, h, 16] f32: what cell_attention returns for (qkv[:, 0] * scale).float(), qkv[:, 1].float(), qkv[:, 2].float().
    deterministic: as for cell_attention."""
    return CellAttentionQKV.apply(qkv, scale, table_q, table_k, table_v, plan, _deterministic(deterministic, plan, "cell_attention_qkv"))
