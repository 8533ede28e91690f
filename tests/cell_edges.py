"""Helpers shared by the cell-attention tests (tests/test_hip_parity.py, tests/test_cell_qkv_hip.py, tests/test_cell_edges_*.py):
the scene builders and C-ABI launch helpers of the variant tests, the oracle's operator chain, and what the edge tests add - a
float64 restatement of that chain in numpy, the non-finite row sets a poisoned operand row must produce (from the pair list alone),
and the conditions a saturated softmax has to meet.  Nothing here needs a GPU to be imported; the functions that launch kernels or
build a plan import torch / the package when they are called."""
import numpy as np

from oracle import pointops_ref as ref

_TABLES = ("table_q", "table_k", "table_v")
_CELL_GRADS = ("q", "k", "v", "table_q", "table_k", "table_v")
ROWS = ("out", "q", "k", "v")  # the per-point results: out and the three row gradients
TTOL = dict(rtol=2e-4, atol=2e-4)
FTOL = dict(rtol=2e-5, atol=1e-4)
GTOL = dict(rtol=2e-5, atol=2e-4)
# q's scale per row type of the packed launchers: the model's 16 ** -0.5 for fp32 rows; for the half types values that are no powers
# of two, so that the product q * scale is rounded (a `qk_scale` of the model's constructor)
_SCALES = {"float32": 0.25, "float16": 0.3, "bfloat16": 0.19}


def _dtypes():
    import torch
    return {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}


def _np(t):
    return t.detach().cpu().numpy()


# ---- scenes and plans -------------------------------------------------------------------------------------------------------
def _cell_plans(xyz_np, offset, w, quant, seed, L, cap=0):
    """even and odd block index (with their cell plans) of a cloud, on a seeded random downsample of n // 8 + b points"""
    from stratified_transformer_amd import index_build
    from tests.util import dev
    n, nbatch = xyz_np.shape[0], offset.shape[0]
    rng = np.random.default_rng(seed)
    ds = np.sort(rng.permutation(n)[: n // 8 + nbatch]).astype(np.int32)
    even, odd, _ = index_build.stage_index_hip(dev(xyz_np), dev(offset), w, quant, dev(ds), cell_table_rows=L, cell_max_queries=cap)
    return even, odd


def _cell_scene(n, nbatch, w, quant, seed, L, cap=0):
    from stratified_transformer_amd import scene
    sizes = [n // nbatch + (1 if i < n % nbatch else 0) for i in range(nbatch)]
    xyz_np, offset = scene.make_batch(sizes, seed=seed)
    even, odd = _cell_plans(xyz_np, offset, w, quant, seed, L, cap)
    return xyz_np, offset, even, odd


def _cell_nk(plan):
    return np.diff(_np(plan.cell_kbase)[: plan.n_cells + 1])


def _cell_nq(plan):
    return np.diff(_np(plan.cell_qstart)[: plan.n_cells + 1])


# name: (points per batch element, w, quant, h, cap (None: index_build.cell_query_cap, as the production pass), fp32 variant of the
# (even, odd) pattern, least keys of the largest cell).  L = 2 * int(2w / quant): 64, or 80 at w / quant = 20.
_CELL_VARIANT_SCENES = {
    "mfma64_h1": ([3000], 0.16, 0.01, 1, 16, ("mfma64", "mfma64"), 0),
    "mfma80_h3": ([4000], 0.1, 0.005, 3, 32, ("mfma80", "mfma80"), 0),
    # S3DIS stage 0 at n * h = 96000 with the production cut: the shifted pattern's small cells take the VALU forward
    "stage0_h12_production_cap": ([8000], 0.16, 0.01, 12, None, ("mfma64", "valu80"), 0),
    "stage0_h3_cap8": ([32000], 0.16, 0.01, 3, 8, ("valu80", "valu80"), 0),
    # big cells cut into pieces of 8 queries (each with the whole key list): n * h >= 96000 at an average below 15 queries, cells of
    # more than 128 keys (two or more register chunks: running max / sum in `ml`, logits parked in pbuf) ...
    "two_chunks_L80_h8_cap8": ([6000, 6000], 0.3, 0.015, 8, 8, ("valu80", "valu80"), 129),
    # ... and of more than 256 (three or more)
    "three_chunks_h12_cap8": ([8000], 0.32, 0.02, 12, 8, ("valu80", "valu80"), 257),
}


def _variant_scene(case):
    """(even, odd) block index of a scene of _CELL_VARIANT_SCENES, the fp32 variants it must reach, L, h"""
    from stratified_transformer_amd import index_build, scene
    sizes, w, quant, h, cap, variants, nk_least = _CELL_VARIANT_SCENES[case]
    L = 2 * int((2 * w + 1e-4) // quant)
    n = sum(sizes)
    cap = index_build.cell_query_cap(n, h) if cap is None else cap
    xyz_np, offset = scene.make_batch(sizes, seed=n + h)
    blocks = _cell_plans(xyz_np, offset, w, quant, n + h, L, cap)
    for blk in blocks:
        if nk_least:
            nk = _cell_nk(blk.cells)
            assert blk.cells.nk_max >= nk_least, blk.cells.nk_max
            assert ((nk > 128) & (nk % 16 != 0)).any(), blk.cells.nk_max
    return blocks, variants, L, h


def _expand_cells(plan):
    """the pair list a cell plan stands for, in (query, tile order): arrays (query, key, r0, r1, r2)"""
    nC = plan.n_cells
    qstart, kbase, pbase = (_np(t) for t in (plan.cell_qstart, plan.cell_kbase, plan.cell_pbase))
    order, keys, relp = _np(plan.cell_order), _np(plan.cell_keys), _np(plan.relp).view(np.uint32)
    rows = []
    for c in range(nC):
        nq, nk = qstart[c + 1] - qstart[c], kbase[c + 1] - kbase[c]
        tile = relp[pbase[c]: pbase[c] + nq * nk].reshape(nq, nk)
        qi = np.repeat(order[qstart[c]: qstart[c + 1]], nk).reshape(nq, nk)
        kj = np.tile(keys[kbase[c]: kbase[c + 1]], nq).reshape(nq, nk)
        keep = (tile >> 31) == 0
        rows.append(np.stack([qi[keep], kj[keep], tile[keep] & 255, (tile[keep] >> 8) & 255, (tile[keep] >> 16) & 255], 1))
    allp = np.concatenate(rows).astype(np.int64)
    return allp[np.argsort(allp[:, 0], kind="stable")]


def check_cell_plan_is_the_pair_list(blk, L, cap):
    """Every (query, key, rel-pos index clamped to [0, L)) of the block's CSR pair list appears exactly once in the cell tiles of its
    plan, in the same per-query order - a pair the list holds twice is there twice; each query and each cell id exactly once; the work
    order is a permutation, largest tile first; the pieces of a parent share one key list.  Returns the expanded tiles
    (query, key, r0, r1, r2), int64 [M, 5]."""
    plan = blk.cells
    n = plan.n_points
    if cap:
        assert np.diff(_np(plan.cell_qstart)[: plan.n_cells + 1]).max() <= cap
    got = _expand_cells(plan)
    i0, i1, rel = _np(blk.index_0).astype(np.int64), _np(blk.index_1).astype(np.int64), np.clip(_np(blk.rel_idx), 0, L - 1)
    assert got.shape[0] == i0.shape[0]
    assert np.array_equal(got[:, 0], i0) and np.array_equal(got[:, 1], i1) and np.array_equal(got[:, 2:], rel)
    assert np.array_equal(np.sort(_np(plan.cell_order)), np.arange(n))
    perm = _np(plan.cell_perm)[: plan.n_cells]
    assert np.array_equal(np.sort(perm), np.arange(plan.n_cells))
    tiles = np.diff(_np(plan.cell_pbase)[: plan.n_cells + 1])
    assert np.all(np.diff(tiles[perm]) <= 0) and tiles.sum() == plan.n_pairs
    assert np.diff(_np(plan.cell_kbase)[: plan.n_cells + 1]).max() == plan.nk_max
    # parents: the uncut cells; the pieces of a parent are consecutive cell ids with one key list (contiguous tiles)
    pf, kb, keys = _np(plan.parent_first)[: plan.n_parents + 1], _np(plan.cell_kbase), _np(plan.cell_keys)
    assert pf[0] == 0 and pf[-1] == plan.n_cells and np.all(np.diff(pf) > 0)
    if not cap:
        assert plan.n_parents == plan.n_cells
    for a, b in zip(pf[:-1], pf[1:]):
        for piece in range(a + 1, b):
            assert np.array_equal(keys[kb[piece]: kb[piece + 1]], keys[kb[a]: kb[a + 1]])
    return got


def _pair_list(blk, L):
    """index_0, index_1, offsets, rel_idx (clamped as the model asserts it) of a block, numpy"""
    return (_np(blk.index_0).astype(np.int32), _np(blk.index_1), _np(blk.offsets), np.clip(_np(blk.rel_idx), 0, L - 1).astype(np.int32))


# ---- the oracle's operator chain --------------------------------------------------------------------------------------------
def _oracle_softmax(p, i1, offs, rel):
    return ref.segment_softmax(ref.attention_step1_v2(p["q"], p["k"], i1, offs)
                               + ref.dot_prod_with_idx_v3(p["q"], offs, p["k"], i1, p["table_q"], p["table_k"], rel), offs)


def _oracle_attention(p, i1, offs, rel, go, sm=None):
    sm = _oracle_softmax(p, i1, offs, rel) if sm is None else sm
    out = ref.attention_step2_with_rel_pos_value_v2(sm, p["v"], offs, i1, p["table_v"], rel)
    if go is None:
        return out, None
    ga, gv, gtv = ref.attention_step2_with_rel_pos_value_v2_backward(go, sm, p["v"], offs, i1, p["table_v"], rel)
    gs = ref.segment_softmax_backward(sm, ga, offs)
    gq1, gk1 = ref.attention_step1_v2_backward(gs, p["q"], p["k"], i1, offs)
    gq2, gk2, gtq, gtk = ref.dot_prod_with_idx_v3_backward(gs, p["q"], offs, p["k"], i1, p["table_q"], p["table_k"], rel)
    return out, dict(q=gq1 + gq2, k=gk1 + gk2, v=gv, table_q=gtq, table_k=gtk, table_v=gtv)


# ---- operands and launches through the C ABI --------------------------------------------------------------------------------
def _cell_operands(n, h, L, seed):
    rng = np.random.default_rng(seed)
    p = {x: rng.standard_normal((n, h, 16), dtype=np.float32) for x in ("q", "k", "v")}
    for t in _TABLES:
        p[t] = rng.standard_normal((L, h, 16, 3), dtype=np.float32) * 0.5
    return p, rng.standard_normal((n, h, 16), dtype=np.float32)


def _cell_launch(plan, ops, L, go=None):
    """The cell forward (and with grad_out `go` its backward) through the C ABI, fp32 or bf16 storage by the operands' dtype:
    out, and the six gradients in fp32 as the kernels wrote them (fused.cell_attention casts a bf16 operand's to bf16)."""
    import torch
    from stratified_transformer_amd import _lib
    from tests.util import dev
    n, h, _ = ops[0].shape
    sfx = "_bf16" if ops[0].dtype == torch.bfloat16 else ""
    f32 = dict(dtype=torch.float32, device="cuda")
    out, ml, pbuf = torch.empty(n, h, 16, **f32), torch.empty(n, h, 2, **f32), torch.empty(h, max(plan.n_pairs, 1), **f32)
    ptrs = [_lib.ptr(t) for t in ops]
    _lib.call(f"cell_attention_forward{sfx}_launcher", plan.c_arg(), h, 16, L, *ptrs, _lib.ptr(out), _lib.ptr(ml), _lib.ptr(pbuf), device=out.device)
    if go is None:
        return out, None
    gsbuf = torch.empty_like(pbuf)
    grads = [torch.empty(n, h, 16, **f32)] + [torch.zeros(t.shape, **f32) for t in ops[1:]]  # grad_q fully written, the rest accumulated
    _lib.call(f"cell_attention_backward{sfx}_launcher", plan.c_arg(), h, 16, L, _lib.ptr(dev(go)), *ptrs[:3], _lib.ptr(out), *ptrs[3:], _lib.ptr(pbuf),
              _lib.ptr(gsbuf), *[_lib.ptr(g) for g in grads], device=out.device)
    return out, dict(zip(_CELL_GRADS, grads))


def _packed_operands(n, h, L, seed, dtype):
    """qkv [n, 3, h, 16] of `dtype` on the device, the three fp32 tables, grad_out (numpy)"""
    from tests.util import dev
    rng = np.random.default_rng(seed)
    qkv = dev(rng.standard_normal((n, 3, h, 16), dtype=np.float32)).to(dtype).contiguous()
    tabs = [dev(rng.standard_normal((L, h, 16, 3), dtype=np.float32) * np.float32(0.5)) for _ in _TABLES]
    return qkv, tabs, rng.standard_normal((n, h, 16), dtype=np.float32)


def _oracle_operands(qkv, scale, tabs):
    """what the model hands its operators: (query * scale).float(), key.float(), value.float() (:181-183), the product taken by torch
    in qkv's dtype"""
    p = dict(q=_np((qkv[:, 0] * scale).float().contiguous()), k=_np(qkv[:, 1].float().contiguous()), v=_np(qkv[:, 2].float().contiguous()))
    p.update({name: _np(t) for name, t in zip(_TABLES, tabs)})
    return p


def _qkv_launch(plan, qkv, scale, tabs, L, go=None):
    """The packed forward (and with grad_out `go` its backward) through the C ABI: out, pbuf, and the fp32 gradient buffers as the
    kernels wrote them (grad_qkv [n, 3, h, 16] and the three table gradients)."""
    import torch
    from stratified_transformer_amd import _lib
    from tests.util import dev
    n, _, h, _ = qkv.shape
    f32 = dict(dtype=torch.float32, device="cuda")
    out, ml, pbuf = torch.empty(n, h, 16, **f32), torch.empty(n, h, 2, **f32), torch.zeros(h, max(plan.n_pairs, 1), **f32)
    rt = _lib.ROW_TYPES[qkv.dtype]
    tp = [_lib.ptr(t) for t in tabs]
    _lib.call("cell_attention_qkv_forward_launcher", plan.c_arg(), h, 16, L, _lib.ptr(qkv), rt, float(scale), *tp, _lib.ptr(out), _lib.ptr(ml),
              _lib.ptr(pbuf), device=out.device)
    if go is None:
        return out, pbuf, None
    gsbuf = torch.empty_like(pbuf)
    g_qkv = torch.zeros(n, 3, h, 16, **f32)
    g_tabs = [torch.zeros(t.shape, **f32) for t in tabs]
    _lib.call("cell_attention_qkv_backward_launcher", plan.c_arg(), h, 16, L, _lib.ptr(dev(go)), _lib.ptr(qkv), rt, float(scale), _lib.ptr(out), *tp,
              _lib.ptr(pbuf), _lib.ptr(gsbuf), _lib.ptr(g_qkv), *[_lib.ptr(g) for g in g_tabs], device=out.device)
    return out, pbuf, dict(qkv=g_qkv, table_q=g_tabs[0], table_k=g_tabs[1], table_v=g_tabs[2])


# ---- float64 restatement of the chain (numpy only) ----------------------------------------------------------------------------
class _Scatter:
    """sums rows by an index: out[r] = sum of vals[m] over idx[m] == r (float64 [nrows, ...]); the sort is taken once"""

    def __init__(self, idx, nrows):
        self.nrows = nrows
        self.order = np.argsort(idx, kind="stable")
        si = idx[self.order]
        self.starts = np.flatnonzero(np.r_[True, si[1:] != si[:-1]]) if si.shape[0] else np.zeros(0, np.int64)
        self.rows = si[self.starts]

    def __call__(self, vals):
        out = np.zeros((self.nrows,) + vals.shape[1:], np.float64)
        x = np.take(vals, self.order, axis=0)
        ends = np.r_[self.starts[1:], x.shape[0]]
        for r, a, b in zip(self.rows, self.starts, ends):  # (block sums: np.add.reduceat along axis 0 of wide rows is several times slower)
            out[r] = x[a:b].sum(axis=0)
        return out


def _head_tables(tab, hd):
    """[3][L, 16] float64, contiguous: one head's rows of a table per axis"""
    return [np.ascontiguousarray(tab[:, hd, :, ax], dtype=np.float64) for ax in range(3)]


def _table_sum(rows, rel):
    """T(m) = sum over the axes of table[rel[m, ax], head, :, ax]: [M, 16]"""
    return np.take(rows[0], rel[:, 0], axis=0) + np.take(rows[1], rel[:, 1], axis=0) + np.take(rows[2], rel[:, 2], axis=0)


def _row_dot(a, b):
    return np.einsum("md,md->m", a, b)


def logits_f64(p, i0, i1, rel):
    """[M, h] float64: <q_i, k_j> + <q_i, Tq(m)> + <k_j, Tk(m)>,  T(m) = sum over the axes of table[rel[m, ax], :, :, ax]"""
    h = p["q"].shape[1]
    lg = np.empty((i0.shape[0], h), np.float64)
    for hd in range(h):
        qi = np.take(np.ascontiguousarray(p["q"][:, hd], dtype=np.float64), i0, axis=0)
        kj = np.take(np.ascontiguousarray(p["k"][:, hd], dtype=np.float64), i1, axis=0)
        lg[:, hd] = _row_dot(qi, kj + _table_sum(_head_tables(p["table_q"], hd), rel)) + _row_dot(kj, _table_sum(_head_tables(p["table_k"], hd), rel))
    return lg


def softmax_f64(lg, offs):
    """segment softmax over the rows of the CSR pair list (every segment holds at least its own point)"""
    starts = offs[:-1].astype(np.int64)
    assert (np.diff(offs) > 0).all()
    rep = np.repeat(np.arange(starts.shape[0]), np.diff(offs))
    e = np.exp(lg - np.maximum.reduceat(lg, starts, axis=0)[rep])
    return e / np.add.reduceat(e, starts, axis=0)[rep]


def attention_f64(p, i0, i1, offs, rel, go=None):
    """out, the six gradients (None without `go`) and the logits, all float64, written from the formulas of the operator chain:
       sm = softmax_i(logit);  out_i = sum_m sm (v_j + Tv(m));  ga = <go_i, v_j + Tv(m)>;  gs = sm (ga - sum_i sm ga)
       grad q_i = sum gs (k_j + Tq(m));  grad k_j = sum gs (q_i + Tk(m));  grad v_j = sum sm go_i
       grad table_q[r, :, :, ax] = sum over rel[m, ax] = r of gs q_i;  table_k: gs k_j;  table_v: sm go_i
    (numpy only; the heads are independent and run on a few threads)"""
    from concurrent.futures import ThreadPoolExecutor
    n, h, _ = p["q"].shape
    L = p["table_q"].shape[0]
    i0, i1, rel = i0.astype(np.int64), i1.astype(np.int64), rel.astype(np.int64)
    starts = offs[:-1].astype(np.int64)
    assert (np.diff(offs) > 0).all() and np.array_equal(np.repeat(np.arange(n), np.diff(offs)), i0)
    lg = np.empty((i0.shape[0], h), np.float64)
    out = np.empty((n, h, 16), np.float64)
    g = None
    if go is not None:
        g = {x: np.zeros(p[x].shape, np.float64) for x in _CELL_GRADS}
        by_key, by_rel = _Scatter(i1, n), [_Scatter(rel[:, ax], L) for ax in range(3)]

    def head(hd):
        qh, kh, vh = (np.ascontiguousarray(p[x][:, hd], dtype=np.float64) for x in ("q", "k", "v"))
        qi, kj = np.take(qh, i0, axis=0), np.take(kh, i1, axis=0)
        tqm, tkm = _table_sum(_head_tables(p["table_q"], hd), rel), _table_sum(_head_tables(p["table_k"], hd), rel)
        l = _row_dot(qi, kj + tqm) + _row_dot(kj, tkm)
        lg[:, hd] = l
        e = np.exp(l - np.take(np.maximum.reduceat(l, starts), i0))
        sm = e / np.take(np.add.reduceat(e, starts), i0)
        vt = np.take(vh, i1, axis=0) + _table_sum(_head_tables(p["table_v"], hd), rel)
        out[:, hd] = np.add.reduceat(sm[:, None] * vt, starts, axis=0)
        if go is None:
            return
        goi = np.take(np.ascontiguousarray(go[:, hd], dtype=np.float64), i0, axis=0)
        ga = _row_dot(goi, vt)
        gs = sm * (ga - np.take(np.add.reduceat(sm * ga, starts), i0))
        g["q"][:, hd] = np.add.reduceat(gs[:, None] * (kj + tqm), starts, axis=0)
        # (the sums over keys and over table rows take [M, 32] and [M, 48] rows at once: the reductions dominate the time)
        kv = by_key(np.concatenate([gs[:, None] * (qi + tkm), sm[:, None] * goi], axis=1))
        g["k"][:, hd], g["v"][:, hd] = kv[:, :16], kv[:, 16:]
        w = np.concatenate([gs[:, None] * qi, gs[:, None] * kj, sm[:, None] * goi], axis=1)
        for ax in range(3):
            t = by_rel[ax](w)
            g["table_q"][:, hd, :, ax], g["table_k"][:, hd, :, ax], g["table_v"][:, hd, :, ax] = t[:, :16], t[:, 16:32], t[:, 32:]

    with ThreadPoolExecutor(max_workers=min(h, 8)) as pool:
        list(pool.map(head, range(h)))
    return out, g, lg


# ---- A. non-finite rows -------------------------------------------------------------------------------------------------------
POISONS = ("v_inf", "k_nan", "q_nan", "go_inf")


def poison_value(kind):
    return np.float32(np.inf) if kind.endswith("inf") else np.float32(np.nan)


def poison(p, go, kind, r):
    """copies of the operand dict and grad_out with row r (every head) of one of them made non-finite"""
    p, go = dict(p), go.copy()
    name = kind.split("_")[0]
    if name == "go":
        go[r] = poison_value(kind)
    else:
        p[name] = p[name].copy()
        p[name][r] = poison_value(kind)
    return p, go


def predicted_nonfinite(n, i0, i1, kind, r):
    """The rows of out / grad_q / grad_k / grad_v (boolean [n] each) and the table gradients (a flag each) that are non-finite when
    row r of one operand is, from the pair list alone - provided no softmax weight is exactly 0 and every other value is finite:
      a non-finite v_r or k_r reaches the queries Q that hold key r; a non-finite q_r or grad_out_r reaches query r alone (Q = {r});
      out:     rows Q (v: weight * inf; k, q: the row's softmax is NaN); grad_out is no input of the forward
      grad_q:  rows Q (every logit gradient gs of such a row is NaN: it holds the row's sum over p * grad_attn)
      grad_k:  the keys of Q (gs of the row)
      grad_v:  sum of p * grad_out: the keys of Q where p or grad_out is non-finite (k, q, grad_out) - a v row does not enter
      tables:  grad table_q / table_k sum gs rows: always; grad table_v sums p * grad_out: not under a v poison"""
    name = kind.split("_")[0]
    Q = np.zeros(n, bool)
    if name in ("v", "k"):
        Q[i0[i1 == r]] = True
    else:
        Q[r] = True
    keys = np.zeros(n, bool)
    keys[i1[Q[i0]]] = True
    none = np.zeros(n, bool)
    rows = dict(out=none if name == "go" else Q, q=Q, k=keys, v=none if name == "v" else keys)
    tabs = dict(table_q=True, table_k=True, table_v=name != "v")
    return rows, tabs


def nonfinite_rows(a):
    """boolean [n]: rows of a [n, h, 16] array that hold a non-finite value"""
    return ~np.isfinite(a).all(axis=(1, 2))


def poison_rows(plan_nk, plan_kbase, plan_keys, n):
    """the rows to poison, by name: row 0 (what every padded slot reads), the last key of a cell whose key count is not a multiple of
    16 (the largest such cell), row n - 1"""
    ragged = np.flatnonzero(plan_nk % 16 != 0)
    assert ragged.size, "no cell with nk % 16 != 0"
    c = ragged[np.argmax(plan_nk[ragged])]
    return dict(row0=0, last_key_of_ragged_cell=int(plan_keys[plan_kbase[c] + plan_nk[c] - 1]), last_row=n - 1)


def check_poisoned(what, got_rows, got_tabs, want_rows, want_tabs, grad_rtol=None):
    """The contract of the non-finite tests.  got_rows / want_rows: out, q, k, v -> [n, h, 16]; *_tabs: the three table gradients.
    Row results: the set of non-finite rows equals the oracle's exactly, every other row is within the standing bars.  Table gradients
    (histogram x rows on the matrix cores: one NaN row legitimately spreads over a product tile, so no entry-wise masks): wholly finite
    and within TTOL over their scale where the oracle's is; at least one non-finite entry where the oracle's has one.  grad_rtol: the
    row gradients were rounded once to a half type (its unit roundoff instead of the standing rtol)."""
    for name in got_rows:
        got, want = got_rows[name], want_rows[name]
        gm, wm = nonfinite_rows(got), nonfinite_rows(want)
        extra, missing = np.flatnonzero(gm & ~wm), np.flatnonzero(wm & ~gm)
        assert extra.size == 0 and missing.size == 0, (
            f"{what} {name}: mask mismatch: {extra.size} rows wrongly non-finite (first {extra[:8].tolist()}), {missing.size} rows wrongly "
            f"finite (first {missing[:8].tolist()}); the oracle has {int(wm.sum())} non-finite rows")
        tol = FTOL if name == "out" else GTOL if grad_rtol is None else dict(GTOL, rtol=grad_rtol)
        np.testing.assert_allclose(got[~wm], want[~wm], err_msg=f"{what} {name}", **tol)
    for name in got_tabs:
        got, want = got_tabs[name], want_tabs[name]
        if np.isfinite(want).all():
            assert np.isfinite(got).all(), f"{what} grad {name}: {int((~np.isfinite(got)).sum())} non-finite entries, the oracle's is finite"
            s = max(1.0, float(np.abs(want).max()))
            np.testing.assert_allclose(got / s, want / s, err_msg=f"{what} grad {name}", **TTOL)
        else:
            assert not np.isfinite(got).all(), f"{what} grad {name}: finite, the oracle's has non-finite entries (a swallowed NaN)"


# ---- B. saturated softmax -----------------------------------------------------------------------------------------------------
CHUNK = 128  # keys of a register chunk of the forward kernels (16 * CA_NP, 16 * CM_NKT)
K_MARGIN = 4.0  # margin over the oracle's own rounding error against float64 (__expf, another summation order)


def pair_slots(plan):
    """For the pairs of a plan in CSR order (test_cell_plan_is_the_pair_list: query by query, in tile order): the pair's position in
    its cell's key list and the cell's key count.  numpy int64 [M] each."""
    nC = plan.n_cells
    qstart, kbase, pbase = (_np(t) for t in (plan.cell_qstart, plan.cell_kbase, plan.cell_pbase))
    order, relp = _np(plan.cell_order), _np(plan.relp).view(np.uint32)
    qi, slot, nks = [], [], []
    for c in range(nC):
        nq, nk = qstart[c + 1] - qstart[c], kbase[c + 1] - kbase[c]
        tile = relp[pbase[c]: pbase[c] + nq * nk].reshape(nq, nk)
        keep = (tile >> 31) == 0
        qi.append(np.repeat(order[qstart[c]: qstart[c + 1]], nk).reshape(nq, nk)[keep])
        slot.append(np.tile(np.arange(nk), nq).reshape(nq, nk)[keep])
        nks.append(np.full(int(keep.sum()), nk))
    qi, slot, nks = (np.concatenate(x).astype(np.int64) for x in (qi, slot, nks))
    o = np.argsort(qi, kind="stable")
    return slot[o], nks[o]


def saturation_conditions(lg, sm_oracle, offs, slot=None, nk=None):
    """What a saturated-softmax case must show, from the float64 logits `lg` [M, h], the oracle's weights and (multi-chunk scenes) the
    pairs' slots in their cells' key lists: a dict of measured figures; assert_saturated() holds them to the conditions."""
    starts = offs[:-1].astype(np.int64)
    res = dict(zero_fraction=float((sm_oracle == 0).mean()), one_hot_rows=int((np.maximum.reduceat(sm_oracle, starts, axis=0) >= 1 - 2.0 ** -20).sum()))
    if slot is None:
        return res
    rows = np.flatnonzero(np.minimum.reduceat(nk, starts) > CHUNK)  # (a row's pairs share one cell)
    first = last = jump = 0
    for i in rows:
        a, b = offs[i], offs[i + 1]
        ch = slot[a:b] // CHUNK
        nch = (int(nk[a]) + CHUNK - 1) // CHUNK
        for hd in range(lg.shape[1]):
            m = np.full(nch, -np.inf)
            np.maximum.at(m, ch, lg[a:b, hd])
            where = int(np.argmax(m))
            first += where == 0
            last += where == nch - 1
            run = np.maximum.accumulate(m)
            ok = np.isfinite(run[:-1])
            jump += bool((np.diff(run)[ok] > 88.0).any())
    res.update(multi_chunk_rows=int(rows.size) * lg.shape[1], max_in_first_chunk=int(first), max_in_last_chunk=int(last), rescale_underflows=int(jump))
    return res


def assert_saturated(res, multi_chunk):
    assert res["zero_fraction"] >= 0.25, res
    assert res["one_hot_rows"] >= 1, res
    if multi_chunk:
        assert res["max_in_first_chunk"] >= 1 and res["max_in_last_chunk"] >= 1 and res["rescale_underflows"] >= 1, res


def plant_late_maximum(p_k, plan, factor=8.0):
    """Scales, in place, the k row of the last key of the largest cell by `factor`: the rows of that cell whose logit with the key is
    large and positive find their maximum in the last chunk, more than 88 above the running maximum.  Returns the key."""
    nk = _cell_nk(plan)
    c = int(np.argmax(nk))
    kb = _np(plan.cell_kbase)
    key = int(_np(plan.cell_keys)[kb[c] + nk[c] - 1])
    p_k[key] *= factor
    return key


def check_against_f64(what, got, oracle, f64, bars, ratios=None):
    """max|kernel - f64| <= max(standing bar, K_MARGIN * max|oracle - f64|) per output; bars: name -> (rtol, atol, scale).  The
    standing bar is atol + rtol * |f64| per element, over the scale the standing comparison divides by.  Returns / fills the ratios
    max|kernel - f64| / max|oracle - f64|."""
    ratios = {} if ratios is None else ratios
    fails = []
    for name, (rtol, atol, scaled) in bars.items():
        assert np.isfinite(got[name]).all() and np.isfinite(oracle[name]).all(), f"{what} {name}: non-finite"
        s = max(1.0, float(np.abs(f64[name]).max())) if scaled else 1.0
        d_k = np.abs(got[name] - f64[name]) / s
        e_k, e_o = float(d_k.max()), float(np.abs(oracle[name] - f64[name]).max()) / s
        standing = atol + rtol * np.abs(f64[name]) / s  # element by element, as assert_allclose takes it
        ratios[name] = (e_k, e_o, e_k / max(e_o, 1e-30))
        print(f"{what} {name}: |kernel - f64| = {e_k:.3e}  |oracle - f64| = {e_o:.3e}  ratio {e_k / max(e_o, 1e-30):.2f}")
        if not (d_k <= np.maximum(standing, K_MARGIN * e_o)).all():
            fails.append((name, e_k, e_o))
    assert not fails, (what, fails)
    return ratios


def standing_bars(backward=True):
    bars = dict(out=(FTOL["rtol"], FTOL["atol"], False))
    if backward:
        bars.update({x: (GTOL["rtol"], GTOL["atol"], False) for x in ("q", "k", "v")})
        bars.update({t: (TTOL["rtol"], TTOL["atol"], True) for t in _TABLES})
    return bars
