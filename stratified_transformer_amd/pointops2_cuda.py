"""Stand-in for the reference's compiled extension module `pointops2_cuda`
(lib/pointops2/src/pointops_api.cpp:16-45): the same function names, positional arguments and
ownership rules (the caller allocates and zero-fills every output; functions return None), taking
torch tensors and forwarding their device pointers to the C ABI of libpointops2_hip.so.

`stratified_transformer_amd.install()` registers this module as `sys.modules["pointops2_cuda"]`, so
the reference's own `lib/pointops2/functions/pointops.py` (`import pointops2_cuda as pointops_cuda`,
pointops.py:11) binds to it unchanged.

Stricter than the reference shims (which validate nothing, e.g. attention_cuda_v2.cpp:7-16): dtype,
device and contiguity are checked, launches go to torch's current stream of the operands' device
(_lib.call makes it current), and native errors are raised as RuntimeError.

Every function takes a keyword-only `opts` (_lib.LaunchOpts, the launch options of this one call; the reference's
pointops.py passes none).  The rel-pos _v2 / _v3 functions add the tables' row count L themselves.
"""
import torch

from . import _lib
from ._lib import ptr

F32, I32 = torch.float32, torch.int32


_chk = _lib.check_tensors


def _call(name, ref, *args, opts=None):
    _lib.call(name, *args, device=ref.device, opts=opts)


# sampling/sampling_cuda.cpp
def furthestsampling_cuda(b, n, xyz, offset, new_offset, tmp, idx, *, opts=None):
    _chk((xyz, F32, "xyz"), (offset, I32, "offset"), (new_offset, I32, "new_offset"), (tmp, F32, "tmp"), (idx, I32, "idx"))
    _call("furthestsampling_cuda_launcher", xyz, int(b), int(n), ptr(xyz), ptr(offset), ptr(new_offset), ptr(tmp), ptr(idx), opts=opts)


# knnquery/knnquery_cuda.cpp
def knnquery_cuda(m, nsample, xyz, new_xyz, offset, new_offset, idx, dist2, *, opts=None):
    _chk((xyz, F32, "xyz"), (new_xyz, F32, "new_xyz"), (offset, I32, "offset"), (new_offset, I32, "new_offset"),
         (idx, I32, "idx"), (dist2, F32, "dist2"))
    _call("knnquery_cuda_launcher", xyz, int(m), int(nsample), ptr(xyz), ptr(new_xyz), ptr(offset), ptr(new_offset), ptr(idx), ptr(dist2), opts=opts)


# grouping/grouping_cuda.cpp
def grouping_forward_cuda(m, nsample, c, input, idx, output, *, opts=None):
    _chk((input, F32, "input"), (idx, I32, "idx"), (output, F32, "output"))
    _call("grouping_forward_cuda_launcher", input, int(m), int(nsample), int(c), ptr(input), ptr(idx), ptr(output), opts=opts)


def grouping_backward_cuda(m, nsample, c, grad_output, idx, grad_input, *, opts=None):
    _chk((grad_output, F32, "grad_output"), (idx, I32, "idx"), (grad_input, F32, "grad_input"))
    _call("grouping_backward_cuda_launcher", grad_output, int(m), int(nsample), int(c), ptr(grad_output), ptr(idx), ptr(grad_input), opts=opts)


# interpolation/interpolation_cuda.cpp
def interpolation_forward_cuda(n, c, k, input, idx, weight, output, *, opts=None):
    _chk((input, F32, "input"), (idx, I32, "idx"), (weight, F32, "weight"), (output, F32, "output"))
    _call("interpolation_forward_cuda_launcher", input, int(n), int(c), int(k), ptr(input), ptr(idx), ptr(weight), ptr(output), opts=opts)


def interpolation_backward_cuda(n, c, k, grad_output, idx, weight, grad_input, *, opts=None):
    _chk((grad_output, F32, "grad_output"), (idx, I32, "idx"), (weight, F32, "weight"), (grad_input, F32, "grad_input"))
    _call("interpolation_backward_cuda_launcher", grad_output, int(n), int(c), int(k), ptr(grad_output), ptr(idx), ptr(weight), ptr(grad_input), opts=opts)


# csrc/kpconv.hip (no counterpart in the reference's launcher set: the KPConv stem of torch_points3d)
def kpconv_aggregate_forward(n_q, n_s, n_nb, c, n_kp, query_xyz, support_xyz, neighbors, feat, k_points, extent, wf, *, opts=None):
    _chk((query_xyz, F32, "query_xyz"), (support_xyz, F32, "support_xyz"), (neighbors, I32, "neighbors"), (feat, F32, "feat"),
         (k_points, F32, "k_points"), (wf, F32, "wf"))
    _call("kpconv_aggregate_forward_launcher", query_xyz, int(n_q), int(n_s), int(n_nb), int(c), int(n_kp), ptr(query_xyz), ptr(support_xyz),
          ptr(neighbors), ptr(feat), ptr(k_points), float(extent), ptr(wf), opts=opts)


def kpconv_aggregate_backward(n_q, n_s, n_nb, c, n_kp, query_xyz, support_xyz, neighbors, k_points, extent, grad_wf, grad_feat, *, opts=None):
    _chk((query_xyz, F32, "query_xyz"), (support_xyz, F32, "support_xyz"), (neighbors, I32, "neighbors"), (k_points, F32, "k_points"),
         (grad_wf, F32, "grad_wf"), (grad_feat, F32, "grad_feat"))
    _call("kpconv_aggregate_backward_launcher", query_xyz, int(n_q), int(n_s), int(n_nb), int(c), int(n_kp), ptr(query_xyz), ptr(support_xyz),
          ptr(neighbors), ptr(k_points), float(extent), ptr(grad_wf), ptr(grad_feat), opts=opts)


# csrc/grouped_max.hip (no counterpart in the reference's launcher set: the max-pool of TransitionDown taken per source row)
def _row_type(t, name):
    if t.dtype not in _lib.ROW_TYPES:
        raise TypeError(f"{name}: expected torch.float32, torch.float16 or torch.bfloat16, got {t.dtype}")
    return _lib.ROW_TYPES[t.dtype]


def _shaped(t, shape, name):
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: expected shape {list(shape)}, got {list(t.shape)}")


def grouped_max_forward(m, n_s, k, c, feat, idx, out, arg, *, opts=None):
    """out [m,c] (feat's dtype), arg [m,c] uint8 or None <- feat [n_s,c] f32 / f16 / bf16, idx [m,k] int32"""
    m, n_s, k, c = int(m), int(n_s), int(k), int(c)
    rt = _row_type(feat, "feat")
    _chk((feat, feat.dtype, "feat"), (idx, I32, "idx"), (out, feat.dtype, "out"))
    _shaped(feat, (n_s, c), "feat"), _shaped(idx, (m, k), "idx"), _shaped(out, (m, c), "out")
    if arg is not None:
        _chk((arg, torch.uint8, "arg"))
        _shaped(arg, (m, c), "arg")
    _call("grouped_max_forward_launcher", feat, m, n_s, k, c, rt, ptr(feat), ptr(idx), ptr(out), ptr(arg), opts=opts)


def grouped_max_backward(m, n_s, k, c, grad_out, arg, src_offsets, src_pair, grad_feat, *, opts=None):
    """grad_feat [n_s,c] (fully written) <- grad_out [m,c] of the same dtype, arg [m,c] uint8, the key-major view of idx:
    src_offsets (n_s + 1 entries), src_pair (m * k entries), int32"""
    m, n_s, k, c = int(m), int(n_s), int(k), int(c)
    rt = _row_type(grad_out, "grad_out")
    _chk((grad_out, grad_out.dtype, "grad_out"), (arg, torch.uint8, "arg"), (src_offsets, I32, "src_offsets"), (src_pair, I32, "src_pair"),
         (grad_feat, grad_out.dtype, "grad_feat"))
    _shaped(grad_out, (m, c), "grad_out"), _shaped(arg, (m, c), "arg"), _shaped(grad_feat, (n_s, c), "grad_feat")
    if src_offsets.numel() != n_s + 1:
        raise ValueError(f"src_offsets: expected {n_s + 1} entries, got {src_offsets.numel()}")
    if src_pair.numel() != m * k:
        raise ValueError(f"src_pair: expected {m * k} entries, got {src_pair.numel()}")
    _call("grouped_max_backward_launcher", grad_out, m, n_s, k, c, rt, ptr(grad_out), ptr(arg), ptr(src_offsets), ptr(src_pair), ptr(grad_feat),
          opts=opts)


# csrc/upsample.hip (no counterpart in the reference's launcher set: Upsample's weighted sum of k gathered rows and its add, typed rows)
def gather_add_forward(n, m, k, c, feat, idx, weight, base, out, *, opts=None):
    """out [n,c] f32 (fully written) <- feat [m,c] f32 / f16 / bf16, idx [n,k] int32, weight [n,k] f32, base [n,c] f32 / f16 / bf16 or None"""
    n, m, k, c = int(n), int(m), int(k), int(c)
    rt = _row_type(feat, "feat")
    _chk((feat, feat.dtype, "feat"), (idx, I32, "idx"), (weight, F32, "weight"), (out, F32, "out"))
    _shaped(feat, (m, c), "feat"), _shaped(idx, (n, k), "idx"), _shaped(weight, (n, k), "weight"), _shaped(out, (n, c), "out")
    bt = 0
    if base is not None:
        bt = _row_type(base, "base")
        _chk((base, base.dtype, "base"))
        _shaped(base, (n, c), "base")
    _call("gather_add_forward_launcher", feat, n, m, k, c, rt, bt, ptr(feat), ptr(idx), ptr(weight), ptr(base), ptr(out), opts=opts)


def gather_add_backward(n, m, k, c, grad_out, weight, src_offsets, src_pair, grad_feat, *, opts=None):
    """grad_feat [m,c] f32 / f16 / bf16 (fully written) <- grad_out [n,c] f32, weight [n,k] f32, the key-major view of idx:
    src_offsets (m + 1 entries), src_pair (n * k entries), int32"""
    n, m, k, c = int(n), int(m), int(k), int(c)
    rt = _row_type(grad_feat, "grad_feat")
    _chk((grad_out, F32, "grad_out"), (weight, F32, "weight"), (src_offsets, I32, "src_offsets"), (src_pair, I32, "src_pair"),
         (grad_feat, grad_feat.dtype, "grad_feat"))
    _shaped(grad_out, (n, c), "grad_out"), _shaped(weight, (n, k), "weight"), _shaped(grad_feat, (m, c), "grad_feat")
    if src_offsets.numel() != m + 1:
        raise ValueError(f"src_offsets: expected {m + 1} entries, got {src_offsets.numel()}")
    if src_pair.numel() != n * k:
        raise ValueError(f"src_pair: expected {n * k} entries, got {src_pair.numel()}")
    _call("gather_add_backward_launcher", grad_out, n, m, k, c, rt, ptr(grad_out), ptr(weight), ptr(src_offsets), ptr(src_pair), ptr(grad_feat),
          opts=opts)


# csrc/rownorm.hip (no counterpart in the reference's launcher set: residual add, DropPath row scale and LayerNorm of a pre-norm block)
RESIDUAL_NORM_MAX_C = 1024
RESIDUAL_NORM_PARTIAL_ROWS = 1024  # most workgroups of the backward: one row of `partials` each


def _opt(t, dtype, shape, name):
    if t is not None:
        _chk((t, dtype, name))
        _shaped(t, shape, name)


def _residual_norm_sizes(n, c):
    n, c = int(n), int(c)
    if n < 0:
        raise ValueError(f"n: expected a row count >= 0, got {n}")
    if not 1 <= c <= RESIDUAL_NORM_MAX_C:
        raise ValueError(f"c: expected 1 <= c <= {RESIDUAL_NORM_MAX_C}, got {c}")
    return n, c


def residual_norm_forward(n, c, x, y, row_scale, weight, bias, eps, z, o, stat, *, opts=None):
    """z [n,c] f32 (or None: not wanted), o [n,c] f32 / f16 / bf16, stat [n,2] f32 <- x [n,c] f32, y [n,c] f32 / f16 / bf16 or None,
    row_scale [n] f32 or None, weight / bias [c] f32: z = x + row_scale[:, None] * y, o = LayerNorm(z), stat = (mean, rstd) per row"""
    n, c = _residual_norm_sizes(n, c)
    _chk((x, F32, "x"), (weight, F32, "weight"), (bias, F32, "bias"), (stat, F32, "stat"))
    _shaped(x, (n, c), "x"), _shaped(weight, (c,), "weight"), _shaped(bias, (c,), "bias"), _shaped(stat, (n, 2), "stat")
    ot = _row_type(o, "o")
    _opt(o, o.dtype, (n, c), "o")
    yt = _row_type(y, "y") if y is not None else _lib.ROW_TYPES[F32]
    _opt(y, None if y is None else y.dtype, (n, c), "y")
    _opt(row_scale, F32, (n,), "row_scale")
    _opt(z, F32, (n, c), "z")
    if row_scale is not None and y is None:
        raise ValueError("row_scale: given without y")
    _call("residual_norm_forward_launcher", x, n, c, yt, ot, ptr(x), ptr(y), ptr(row_scale), ptr(weight), ptr(bias), float(eps), ptr(z), ptr(o),
          ptr(stat), opts=opts)


def residual_norm_backward(n, c, grad_o, grad_z, z, stat, row_scale, weight, grad_x, grad_y, partials, grad_weight, grad_bias, *, opts=None):
    """grad_x [n,c] f32, grad_y [n,c] (y's dtype; None: not wanted), grad_weight / grad_bias [c] f32 (with partials, a
    [rows <= 1024, 2, c] f32 workspace; all three None: not wanted) <- grad_o [n,c] (o's dtype) or None, grad_z [n,c] f32 or None,
    z, stat, row_scale, weight of the forward.  Every output is fully written."""
    n, c = _residual_norm_sizes(n, c)
    _chk((z, F32, "z"), (stat, F32, "stat"), (weight, F32, "weight"), (grad_x, F32, "grad_x"))
    _shaped(z, (n, c), "z"), _shaped(stat, (n, 2), "stat"), _shaped(weight, (c,), "weight"), _shaped(grad_x, (n, c), "grad_x")
    ot = _row_type(grad_o, "grad_o") if grad_o is not None else _lib.ROW_TYPES[F32]
    _opt(grad_o, None if grad_o is None else grad_o.dtype, (n, c), "grad_o")
    yt = _row_type(grad_y, "grad_y") if grad_y is not None else _lib.ROW_TYPES[F32]
    _opt(grad_y, None if grad_y is None else grad_y.dtype, (n, c), "grad_y")
    _opt(grad_z, F32, (n, c), "grad_z")
    _opt(row_scale, F32, (n,), "row_scale")
    rows = _residual_norm_partial_rows(c, partials, grad_weight, grad_bias)
    _call("residual_norm_backward_launcher", z, n, c, yt, ot, ptr(grad_o), ptr(grad_z), ptr(z), ptr(stat), ptr(row_scale), ptr(weight),
          ptr(grad_x), ptr(grad_y), ptr(partials), rows, ptr(grad_weight), ptr(grad_bias), opts=opts)


def _residual_norm_partial_rows(c, partials, grad_weight, grad_bias):
    """the rows of the parameter gradients' workspace (0: none wanted), the three tensors checked"""
    rows = 0
    if partials is not None or grad_weight is not None or grad_bias is not None:
        for t, name in ((partials, "partials"), (grad_weight, "grad_weight"), (grad_bias, "grad_bias")):
            if t is None:
                raise ValueError(f"{name}: partials, grad_weight and grad_bias are given together or not at all")
        _chk((partials, F32, "partials"), (grad_weight, F32, "grad_weight"), (grad_bias, F32, "grad_bias"))
        _shaped(grad_weight, (c,), "grad_weight"), _shaped(grad_bias, (c,), "grad_bias")
        rows = int(partials.shape[0]) if partials.dim() == 3 else 0
        if not 1 <= rows <= RESIDUAL_NORM_PARTIAL_ROWS or tuple(partials.shape[1:]) != (2, c):
            raise ValueError(f"partials: expected shape [1 <= rows <= {RESIDUAL_NORM_PARTIAL_ROWS}, 2, {c}], got {list(partials.shape)}")
    return rows


def _stream_type(first, others):
    """the row type of the residual stream: `first` (name, tensor) names it, every other stream tensor given must share its dtype"""
    xt = _row_type(first[1], first[0])
    for name, t in others:
        if t is not None and t.dtype != first[1].dtype:
            raise TypeError(f"{name}: expected {first[1].dtype} like {first[0]} (the stream tensors share one dtype), got {t.dtype}")
    return xt


def residual_norm_stream_forward(n, c, x, y, row_scale, weight, bias, eps, z, o, stat, *, opts=None):
    """residual_norm_forward with x and z [n,c] of one dtype of f32 / f16 / bf16 (the residual stream): z = x + row_scale[:, None] * y
    rounded once to that dtype, o = LayerNorm(z as stored), stat = (mean, rstd) per row"""
    n, c = _residual_norm_sizes(n, c)
    xt = _stream_type(("x", x), (("z", z),))
    _chk((x, x.dtype, "x"), (weight, F32, "weight"), (bias, F32, "bias"), (stat, F32, "stat"))
    _shaped(x, (n, c), "x"), _shaped(weight, (c,), "weight"), _shaped(bias, (c,), "bias"), _shaped(stat, (n, 2), "stat")
    ot = _row_type(o, "o")
    _opt(o, o.dtype, (n, c), "o")
    yt = _row_type(y, "y") if y is not None else _lib.ROW_TYPES[F32]
    _opt(y, None if y is None else y.dtype, (n, c), "y")
    _opt(row_scale, F32, (n,), "row_scale")
    _opt(z, x.dtype, (n, c), "z")
    if row_scale is not None and y is None:
        raise ValueError("row_scale: given without y")
    _call("residual_norm_stream_forward_launcher", x, n, c, xt, yt, ot, ptr(x), ptr(y), ptr(row_scale), ptr(weight), ptr(bias), float(eps), ptr(z),
          ptr(o), ptr(stat), opts=opts)


def residual_norm_stream_backward(n, c, grad_o, grad_z, z, stat, row_scale, weight, grad_x, grad_y, partials, grad_weight, grad_bias, *, opts=None):
    """residual_norm_backward with z, grad_z (or None) and grad_x [n,c] of one dtype of f32 / f16 / bf16 (the residual stream); grad_x and
    grad_y are each rounded once from the fp32 gradient.  Every output is fully written."""
    n, c = _residual_norm_sizes(n, c)
    xt = _stream_type(("z", z), (("grad_z", grad_z), ("grad_x", grad_x)))
    _chk((z, z.dtype, "z"), (stat, F32, "stat"), (weight, F32, "weight"), (grad_x, z.dtype, "grad_x"))
    _shaped(z, (n, c), "z"), _shaped(stat, (n, 2), "stat"), _shaped(weight, (c,), "weight"), _shaped(grad_x, (n, c), "grad_x")
    ot = _row_type(grad_o, "grad_o") if grad_o is not None else _lib.ROW_TYPES[F32]
    _opt(grad_o, None if grad_o is None else grad_o.dtype, (n, c), "grad_o")
    yt = _row_type(grad_y, "grad_y") if grad_y is not None else _lib.ROW_TYPES[F32]
    _opt(grad_y, None if grad_y is None else grad_y.dtype, (n, c), "grad_y")
    _opt(grad_z, z.dtype, (n, c), "grad_z")
    _opt(row_scale, F32, (n,), "row_scale")
    rows = _residual_norm_partial_rows(c, partials, grad_weight, grad_bias)
    _call("residual_norm_stream_backward_launcher", z, n, c, xt, yt, ot, ptr(grad_o), ptr(grad_z), ptr(z), ptr(stat), ptr(row_scale), ptr(weight),
          ptr(grad_x), ptr(grad_y), ptr(partials), rows, ptr(grad_weight), ptr(grad_bias), opts=opts)


# csrc/linear_grads.hip (no counterpart in the reference's launcher set: grad_weight and grad_bias of a Linear over point rows)
LINEAR_GRADS_MAX_DIM = 1536
LINEAR_GRADS_ROWS = _lib.LINEAR_GRADS_ROWS  # rows of a chunk: one block of `partials` each


def _linear_grads_sizes(in_features, out_features):
    in_features, out_features = int(in_features), int(out_features)
    for name, v in (("in", in_features), ("out", out_features)):
        if not 1 <= v <= LINEAR_GRADS_MAX_DIM:
            raise ValueError(f"{name}: expected 1 <= {name} <= {LINEAR_GRADS_MAX_DIM}, got {v}")
    return in_features, out_features


def linear_grads_partial_rows(n, in_features, out_features):
    """blocks of the `partials` of n rows: ceil(n / LINEAR_GRADS_ROWS), 1 for n == 0; a function of n alone.  No launch, no GPU."""
    n = int(n)
    if n < 0:
        raise ValueError(f"n: expected a row count >= 0, got {n}")
    in_features, out_features = _linear_grads_sizes(in_features, out_features)
    return int(_lib.lib().pointops2_linear_grads_partial_rows(n, in_features, out_features))


def linear_grads_partial(n, in_features, out_features, x, g, partials, *, opts=None):
    """partials [G, out, in + 1] f32 (fully written; column `in` is the bias partial) <- x [n, in], g [n, out], each f32 / f16 / bf16;
    G = linear_grads_partial_rows(n, in, out)"""
    rows = linear_grads_partial_rows(n, in_features, out_features)
    n, (in_features, out_features) = int(n), _linear_grads_sizes(in_features, out_features)
    xt, gt = _row_type(x, "x"), _row_type(g, "g")
    _chk((x, x.dtype, "x"), (g, g.dtype, "g"), (partials, F32, "partials"))
    _shaped(x, (n, in_features), "x"), _shaped(g, (n, out_features), "g")
    if partials.dim() != 3 or tuple(partials.shape[1:]) != (out_features, in_features + 1):
        raise ValueError(f"partials: expected shape [rows, {out_features}, {in_features + 1}], got {list(partials.shape)}")
    # (a wrong row count is the library's own rejection: it knows G)
    _call("linear_grads_partial_launcher", partials, n, in_features, out_features, xt, gt, ptr(x), ptr(g), ptr(partials), int(partials.shape[0]),
          opts=opts)
    return rows


def linear_grads_reduce(in_features, out_features, partials, grad_weight, grad_bias, *, opts=None):
    """grad_weight [out, in] f32, grad_bias [out] f32 or None (fully written) <- partials [G, out, in + 1] f32, added in ascending order"""
    in_features, out_features = _linear_grads_sizes(in_features, out_features)
    _chk((partials, F32, "partials"), (grad_weight, F32, "grad_weight"))
    if partials.dim() != 3 or partials.shape[0] < 1 or tuple(partials.shape[1:]) != (out_features, in_features + 1):
        raise ValueError(f"partials: expected shape [rows >= 1, {out_features}, {in_features + 1}], got {list(partials.shape)}")
    _shaped(grad_weight, (out_features, in_features), "grad_weight")
    _opt(grad_bias, F32, (out_features,), "grad_bias")
    _call("linear_grads_reduce_launcher", partials, in_features, out_features, int(grad_bias is not None), ptr(partials), int(partials.shape[0]),
          ptr(grad_weight), ptr(grad_bias), opts=opts)


# csrc/batchnorm.hip (no counterpart in the reference's launcher set: BatchNorm1d + activation + residual add of the stem and the heads)
BATCH_NORM_MAX_C = 1024
BATCH_NORM_PARTIAL_ROWS = 1024  # most workgroups of the two reductions: one row of `partials` each


def _batch_norm_sizes(n, c):
    n, c = int(n), int(c)
    if n < 0:
        raise ValueError(f"n: expected a row count >= 0, got {n}")
    if not 1 <= c <= BATCH_NORM_MAX_C:
        raise ValueError(f"c: expected 1 <= c <= {BATCH_NORM_MAX_C}, got {c}")
    return n, c


def _batch_norm_act(act):
    if act not in _lib.ACTIVATIONS:
        raise ValueError(f"act: expected one of {sorted(_lib.ACTIVATIONS)}, got {act!r}")
    return _lib.ACTIVATIONS[act]


def _batch_norm_partials(partials, width, c):
    _chk((partials, F32, "partials"))
    rows = int(partials.shape[0]) if partials.dim() == 3 else 0
    if not 1 <= rows <= BATCH_NORM_PARTIAL_ROWS or tuple(partials.shape[1:]) != (width, c):
        raise ValueError(f"partials: expected shape [1 <= rows <= {BATCH_NORM_PARTIAL_ROWS}, {width}, {c}], got {list(partials.shape)}")
    return rows


def batch_norm_act_stats(n, c, x, partials, eps, momentum, running_mean, running_var, stat, *, opts=None):
    """stat [2,c] f32 = (mean, 1 / sqrt(biased variance + eps)) per channel <- x [n,c] f32 / f16 / bf16; running_mean / running_var [c] f32
    (both or neither) take torch's momentum update on the device; partials: a [1 <= rows <= 1024, 3, c] f32 workspace"""
    n, c = _batch_norm_sizes(n, c)
    xt = _row_type(x, "x")
    _chk((x, x.dtype, "x"), (stat, F32, "stat"))
    _shaped(x, (n, c), "x"), _shaped(stat, (2, c), "stat")
    rows = _batch_norm_partials(partials, 3, c)
    if (running_mean is None) != (running_var is None):
        raise ValueError(f"{'running_mean' if running_mean is None else 'running_var'}: running_mean and running_var are given together or not at all")
    _opt(running_mean, F32, (c,), "running_mean")
    _opt(running_var, F32, (c,), "running_var")
    _call("batch_norm_act_stats_launcher", x, n, c, xt, ptr(x), ptr(partials), rows, float(eps), float(momentum), ptr(running_mean),
          ptr(running_var), ptr(stat), opts=opts)


def batch_norm_act_forward(n, c, x, mean, scale, scale_is_var, eps, weight, bias, act, negative_slope, residual, o, stat_out, *, opts=None):
    """o [n,c] (x's dtype) = act(((x - mean) * rstd) * weight + bias) (+ residual [n,c] f32 / f16 / bf16 or None) <- x [n,c] f32 / f16 / bf16,
    mean / scale [c] f32 (scale: rstd, or the variance with scale_is_var), weight / bias [c] f32; stat_out [2,c] f32 or None receives
    (mean, rstd) as used"""
    n, c = _batch_norm_sizes(n, c)
    code = _batch_norm_act(act)
    xt = _row_type(x, "x")
    _chk((x, x.dtype, "x"), (mean, F32, "mean"), (scale, F32, "scale"), (weight, F32, "weight"), (bias, F32, "bias"), (o, x.dtype, "o"))
    _shaped(x, (n, c), "x"), _shaped(mean, (c,), "mean"), _shaped(scale, (c,), "scale"), _shaped(weight, (c,), "weight"), _shaped(bias, (c,), "bias")
    _shaped(o, (n, c), "o")
    rt = _row_type(residual, "residual") if residual is not None else _lib.ROW_TYPES[F32]
    _opt(residual, None if residual is None else residual.dtype, (n, c), "residual")
    _opt(stat_out, F32, (2, c), "stat_out")
    _call("batch_norm_act_forward_launcher", x, n, c, xt, rt, code, float(negative_slope), ptr(x), ptr(mean), ptr(scale), int(bool(scale_is_var)),
          float(eps), ptr(weight), ptr(bias), ptr(residual), ptr(o), ptr(stat_out), opts=opts)


def batch_norm_act_backward(n, c, x, grad_o, stat, weight, bias, act, negative_slope, training, partials, grad_weight, grad_bias, grad_x, *,
                            opts=None):
    """grad_weight / grad_bias [c] f32 - computed when partials (a [1 <= rows <= 1024, 2, c] f32 workspace) is given - and grad_x [n,c]
    (x's dtype; None: not wanted) <- x, grad_o [n,c] of one dtype, stat [2,c], weight, bias of the forward.  With `training` grad_x
    reads grad_weight / grad_bias, so they are given even where partials is None (an earlier call computed them).  Every output is
    fully written."""
    n, c = _batch_norm_sizes(n, c)
    code = _batch_norm_act(act)
    xt = _row_type(x, "x")
    _chk((x, x.dtype, "x"), (grad_o, x.dtype, "grad_o"), (stat, F32, "stat"), (weight, F32, "weight"), (bias, F32, "bias"))
    _shaped(x, (n, c), "x"), _shaped(grad_o, (n, c), "grad_o"), _shaped(stat, (2, c), "stat"), _shaped(weight, (c,), "weight"), _shaped(bias, (c,), "bias")
    _opt(grad_x, x.dtype, (n, c), "grad_x")
    _opt(grad_weight, F32, (c,), "grad_weight")
    _opt(grad_bias, F32, (c,), "grad_bias")
    rows = 0
    if partials is not None:
        rows = _batch_norm_partials(partials, 2, c)
    if partials is None and grad_x is None:
        raise ValueError("partials: neither partials nor grad_x is given: nothing to compute")
    if partials is not None or (grad_x is not None and training):
        for t, name in ((grad_weight, "grad_weight"), (grad_bias, "grad_bias")):
            if t is None:
                raise ValueError(f"{name}: needed by partials (the sums' destination) and by grad_x in training mode")
    _call("batch_norm_act_backward_launcher", x, n, c, xt, code, float(negative_slope), int(bool(training)), ptr(x), ptr(grad_o), ptr(stat),
          ptr(weight), ptr(bias), ptr(partials), rows, ptr(grad_weight), ptr(grad_bias), ptr(grad_x), opts=opts)


# the same norm over several ranks' rows (SyncBatchNorm in training mode): per-rank moments, the merge of the gathered rows, dx from the gathered sums
BATCH_NORM_MAX_WORLD = 1024
BATCH_NORM_MAX_ROWS = 2 ** 24  # counts travel as fp32


def _batch_norm_world(t, width, c, name):
    _chk((t, F32, name))
    world = int(t.shape[0]) if t.dim() == 3 else 0
    if not 1 <= world <= BATCH_NORM_MAX_WORLD or tuple(t.shape[1:]) != (width, c):
        raise ValueError(f"{name}: expected shape [1 <= world <= {BATCH_NORM_MAX_WORLD}, {width}, {c}], got {list(t.shape)}")
    return world


def batch_norm_act_moments(n, c, x, partials, row, *, opts=None):
    """row [3,c] f32 = this rank's (count, mean, M2) per channel <- x [n,c] f32 / f16 / bf16; partials: a [1 <= rows <= 1024, 3, c] f32
    workspace (None with n == 0, which writes a row of zeros)"""
    n, c = _batch_norm_sizes(n, c)
    xt = _row_type(x, "x")
    _chk((x, x.dtype, "x"), (row, F32, "row"))
    _shaped(x, (n, c), "x"), _shaped(row, (3, c), "row")
    rows = 0
    if partials is not None:
        rows = _batch_norm_partials(partials, 3, c)
    elif n > 0:
        raise ValueError("partials: needed by the row pass (n > 0)")
    _call("batch_norm_act_moments_launcher", x, n, c, xt, ptr(x), ptr(partials), rows, ptr(row), opts=opts)


def batch_norm_act_merge(world, c, rows, eps, momentum, running_mean, running_var, stat, total, *, opts=None):
    """stat [2,c] f32 = (mean, rstd) of all ranks' rows, total [1] f32 = their number <- rows [world,3,c] f32, merged in rank order;
    running_mean / running_var [c] f32 (both or neither) take torch's momentum update with the merged moments"""
    _, c = _batch_norm_sizes(0, c)
    if _batch_norm_world(rows, 3, c, "rows") != int(world):
        raise ValueError(f"rows: expected {int(world)} rows (world), got {list(rows.shape)}")
    _chk((stat, F32, "stat"), (total, F32, "total"))
    _shaped(stat, (2, c), "stat"), _shaped(total, (1,), "total")
    if (running_mean is None) != (running_var is None):
        raise ValueError(f"{'running_mean' if running_mean is None else 'running_var'}: running_mean and running_var are given together or not at all")
    _opt(running_mean, F32, (c,), "running_mean")
    _opt(running_var, F32, (c,), "running_var")
    _call("batch_norm_act_merge_launcher", rows, int(world), c, ptr(rows), float(eps), float(momentum), ptr(running_mean), ptr(running_var),
          ptr(stat), ptr(total), opts=opts)


def batch_norm_act_sync_backward(n, c, x, grad_o, stat, weight, bias, act, negative_slope, world, sums, total, grad_x, *, opts=None):
    """grad_x [n,c] (x's dtype, fully written) <- x, grad_o [n,c] of one dtype, stat [2,c], weight, bias of the forward, sums [world,2,c]
    f32 (every rank's (sum g * xhat, sum g), added in rank order) and total [1] f32 (the ranks' summed row count)"""
    n, c = _batch_norm_sizes(n, c)
    code = _batch_norm_act(act)
    xt = _row_type(x, "x")
    _chk((x, x.dtype, "x"), (grad_o, x.dtype, "grad_o"), (stat, F32, "stat"), (weight, F32, "weight"), (bias, F32, "bias"), (total, F32, "total"),
         (grad_x, x.dtype, "grad_x"))
    _shaped(x, (n, c), "x"), _shaped(grad_o, (n, c), "grad_o"), _shaped(stat, (2, c), "stat"), _shaped(weight, (c,), "weight"), _shaped(bias, (c,), "bias")
    _shaped(total, (1,), "total"), _shaped(grad_x, (n, c), "grad_x")
    if _batch_norm_world(sums, 2, c, "sums") != int(world):
        raise ValueError(f"sums: expected {int(world)} rows (world), got {list(sums.shape)}")
    _call("batch_norm_act_sync_backward_launcher", x, n, c, xt, code, float(negative_slope), ptr(x), ptr(grad_o), ptr(stat), ptr(weight), ptr(bias),
          int(world), ptr(sums), ptr(total), ptr(grad_x), opts=opts)


# csrc/seg_loss.hip (no counterpart in the reference's launcher set: the loss tail of tool/train.py - cross-entropy, L1 shift, IoU counts)
SEG_LOSS_MAX_C = 64
SEG_LOSS_PARTIAL_ROWS = 1024  # most workgroups of the forward: one row of `partials` each


def _seg_loss_sizes(n, c, smooth_eps, shift_pred, shift):
    n, c, smooth_eps = int(n), int(c), float(smooth_eps)
    if n < 0:
        raise ValueError(f"n: expected a row count >= 0, got {n}")
    if not 1 <= c <= SEG_LOSS_MAX_C:
        raise ValueError(f"c: expected 1 <= c <= {SEG_LOSS_MAX_C}, got {c}")
    if not 0.0 <= smooth_eps < 1.0 or (smooth_eps > 0.0 and c < 2):
        raise ValueError(f"smooth_eps: expected 0 <= smooth_eps < 1 (and c >= 2 when > 0), got {smooth_eps} with c = {c}")
    if (shift_pred is None) != (shift is None):
        raise ValueError(f"{'shift' if shift is None else 'shift_pred'}: shift_pred and shift are given together or not at all")
    return n, c, smooth_eps


def _seg_loss_inputs(n, c, logits, target, shift_pred, shift):
    lt = _row_type(logits, "logits")
    _chk((logits, logits.dtype, "logits"), (target, torch.int64, "target"))
    _shaped(logits, (n, c), "logits"), _shaped(target, (n,), "target")
    st = _row_type(shift_pred, "shift_pred") if shift_pred is not None else _lib.ROW_TYPES[F32]
    _opt(shift_pred, None if shift_pred is None else shift_pred.dtype, (n, 3), "shift_pred")
    _opt(shift, F32, (n, 3), "shift")
    return lt, st


def seg_loss_forward(n, c, logits, target, shift_pred, shift, ignore_index, smooth_eps, offset_weight, stat, partials, counts, rows, losses, *,
                     opts=None):
    """losses [3] f32 = (ce, l1, total), stat [n,2] f32 = (row maximum, log of the row's sum of exponentials), counts [3,c] and rows [2]
    int64 (ACCUMULATED: zero-fill them) <- logits [n,c] f32 / f16 / bf16, target [n] int64, shift_pred [n,3] f32 / f16 / bf16 with
    shift [n,3] f32, or both None; partials: a [1 <= rows <= 1024, 2] float64 workspace"""
    n, c, smooth_eps = _seg_loss_sizes(n, c, smooth_eps, shift_pred, shift)
    lt, st = _seg_loss_inputs(n, c, logits, target, shift_pred, shift)
    _chk((stat, F32, "stat"), (partials, torch.float64, "partials"), (counts, torch.int64, "counts"), (rows, torch.int64, "rows"), (losses, F32, "losses"))
    _shaped(stat, (n, 2), "stat"), _shaped(counts, (3, c), "counts"), _shaped(rows, (2,), "rows"), _shaped(losses, (3,), "losses")
    prows = int(partials.shape[0]) if partials.dim() == 2 else 0
    if not 1 <= prows <= SEG_LOSS_PARTIAL_ROWS or tuple(partials.shape[1:]) != (2,):
        raise ValueError(f"partials: expected shape [1 <= rows <= {SEG_LOSS_PARTIAL_ROWS}, 2], got {list(partials.shape)}")
    _call("seg_loss_forward_launcher", logits, n, c, lt, st, ptr(logits), ptr(target), ptr(shift_pred), ptr(shift), int(ignore_index), smooth_eps,
          float(offset_weight), ptr(stat), ptr(partials), prows, ptr(counts), ptr(rows), ptr(losses), opts=opts)


def seg_loss_backward(n, c, logits, target, stat, shift_pred, shift, grad_losses, rows, ignore_index, smooth_eps, offset_weight, grad_logits,
                      grad_shift_pred, *, opts=None):
    """grad_logits [n,c] (logits' dtype) and grad_shift_pred [n,3] (shift_pred's dtype), each fully written or None (not wanted) <-
    grad_losses [3] f32 and the forward's rows [2] int64, both read on the device, and logits, target, stat, shift_pred, shift"""
    n, c, smooth_eps = _seg_loss_sizes(n, c, smooth_eps, shift_pred, shift)
    lt, st = _seg_loss_inputs(n, c, logits, target, shift_pred, shift)
    _chk((stat, F32, "stat"), (grad_losses, F32, "grad_losses"), (rows, torch.int64, "rows"))
    _shaped(stat, (n, 2), "stat"), _shaped(grad_losses, (3,), "grad_losses"), _shaped(rows, (2,), "rows")
    _opt(grad_logits, logits.dtype, (n, c), "grad_logits")
    if grad_shift_pred is not None and shift_pred is None:
        raise ValueError("grad_shift_pred: given without shift_pred")
    _opt(grad_shift_pred, None if shift_pred is None else shift_pred.dtype, (n, 3), "grad_shift_pred")
    _call("seg_loss_backward_launcher", logits, n, c, lt, st, ptr(logits), ptr(target), ptr(stat), ptr(shift_pred), ptr(shift), ptr(grad_losses),
          ptr(rows), int(ignore_index), smooth_eps, float(offset_weight), ptr(grad_logits), ptr(grad_shift_pred), opts=opts)


# attention/attention_cuda.cpp
def attention_step1_forward_cuda(N, M, h, C, q, k, index0, index1, attn, *, opts=None):
    _chk((q, F32, "q"), (k, F32, "k"), (index0, I32, "index0"), (index1, I32, "index1"), (attn, F32, "attn"))
    _call("attention_step1_forward_cuda_launcher", q, int(N), int(M), int(h), int(C), ptr(q), ptr(k), ptr(index0), ptr(index1), ptr(attn), opts=opts)


def attention_step1_backward_cuda(N, M, h, C, grad_out, index0, index1, q, k, grad_q, grad_k, *, opts=None):
    _chk((grad_out, F32, "grad_out"), (index0, I32, "index0"), (index1, I32, "index1"), (q, F32, "q"), (k, F32, "k"),
         (grad_q, F32, "grad_q"), (grad_k, F32, "grad_k"))
    _call("attention_step1_backward_cuda_launcher", q, int(N), int(M), int(h), int(C), ptr(grad_out), ptr(index0), ptr(index1),
          ptr(q), ptr(k), ptr(grad_q), ptr(grad_k), opts=opts)


def attention_step2_forward_cuda(N, M, h, C, attn, v, index0, index1, output, *, opts=None):
    _chk((attn, F32, "attn"), (v, F32, "v"), (index0, I32, "index0"), (index1, I32, "index1"), (output, F32, "output"))
    _call("attention_step2_forward_cuda_launcher", v, int(N), int(M), int(h), int(C), ptr(attn), ptr(v), ptr(index0), ptr(index1), ptr(output), opts=opts)


def attention_step2_backward_cuda(N, M, h, C, grad_out, index0, index1, attn, v, grad_attn, grad_v, *, opts=None):
    _chk((grad_out, F32, "grad_out"), (index0, I32, "index0"), (index1, I32, "index1"), (attn, F32, "attn"), (v, F32, "v"),
         (grad_attn, F32, "grad_attn"), (grad_v, F32, "grad_v"))
    _call("attention_step2_backward_cuda_launcher", v, int(N), int(M), int(h), int(C), ptr(grad_out), ptr(index0), ptr(index1),
          ptr(attn), ptr(v), ptr(grad_attn), ptr(grad_v), opts=opts)


# attention_v2/attention_cuda_v2.cpp
def attention_step1_forward_cuda_v2(N, M, h, C, n_max, q, k, index0_offsets, index1, attn, *, opts=None):
    _chk((q, F32, "q"), (k, F32, "k"), (index0_offsets, I32, "index0_offsets"), (index1, I32, "index1"), (attn, F32, "attn"))
    _call("attention_step1_forward_cuda_launcher_v2", q, int(N), int(M), int(h), int(C), int(n_max), ptr(q), ptr(k),
          ptr(index0_offsets), ptr(index1), ptr(attn), opts=opts)


def attention_step1_backward_cuda_v2(N, M, h, C, n_max, grad_out, index0_offsets, index1, q, k, grad_q, grad_k, *, opts=None):
    _chk((grad_out, F32, "grad_out"), (index0_offsets, I32, "index0_offsets"), (index1, I32, "index1"), (q, F32, "q"), (k, F32, "k"),
         (grad_q, F32, "grad_q"), (grad_k, F32, "grad_k"))
    _call("attention_step1_backward_cuda_launcher_v2", q, int(N), int(M), int(h), int(C), int(n_max), ptr(grad_out),
          ptr(index0_offsets), ptr(index1), ptr(q), ptr(k), ptr(grad_q), ptr(grad_k), opts=opts)


def attention_step2_forward_cuda_v2(N, M, h, C, attn, v, index0, index1, output, *, opts=None):
    attention_step2_forward_cuda(N, M, h, C, attn, v, index0, index1, output, opts=opts)


def attention_step2_backward_cuda_v2(N, M, h, C, grad_out, index0, index1, attn, v, grad_attn, grad_v, *, opts=None):
    attention_step2_backward_cuda(N, M, h, C, grad_out, index0, index1, attn, v, grad_attn, grad_v, opts=opts)


# rpe/relative_pos_encoding_cuda.cpp
def dot_prod_with_idx_forward_cuda(N, M, h, hdim, q, index, table, rel_idx, output, *, opts=None):
    _chk((q, F32, "q"), (index, I32, "index"), (table, F32, "table"), (rel_idx, I32, "rel_idx"), (output, F32, "output"))
    _call("dot_prod_with_idx_forward_cuda_launcher", q, int(N), int(M), int(h), int(hdim), ptr(q), ptr(index), ptr(table), ptr(rel_idx), ptr(output), opts=opts)


def dot_prod_with_idx_backward_cuda(N, M, h, hdim, grad_out, q, index, table, rel_idx, grad_q, grad_table, *, opts=None):
    _chk((grad_out, F32, "grad_out"), (q, F32, "q"), (index, I32, "index"), (table, F32, "table"), (rel_idx, I32, "rel_idx"),
         (grad_q, F32, "grad_q"), (grad_table, F32, "grad_table"))
    _call("dot_prod_with_idx_backward_cuda_launcher", q, int(N), int(M), int(h), int(hdim), ptr(grad_out), ptr(q), ptr(index),
          ptr(table), ptr(rel_idx), ptr(grad_q), ptr(grad_table), opts=opts)


def attention_step2_with_rel_pos_value_forward_cuda(N, M, h, hdim, attn, v, index0, index1, table, rel_idx, output, *, opts=None):
    _chk((attn, F32, "attn"), (v, F32, "v"), (index0, I32, "index0"), (index1, I32, "index1"), (table, F32, "table"),
         (rel_idx, I32, "rel_idx"), (output, F32, "output"))
    _call("attention_step2_with_rel_pos_value_forward_cuda_launcher", v, int(N), int(M), int(h), int(hdim), ptr(attn), ptr(v),
          ptr(index0), ptr(index1), ptr(table), ptr(rel_idx), ptr(output), opts=opts)


def attention_step2_with_rel_pos_value_backward_cuda(N, M, h, hdim, grad_out, index0, index1, attn, v, table, rel_idx,
                                                     grad_attn, grad_v, grad_table, *, opts=None):
    _chk((grad_out, F32, "grad_out"), (index0, I32, "index0"), (index1, I32, "index1"), (attn, F32, "attn"), (v, F32, "v"),
         (table, F32, "table"), (rel_idx, I32, "rel_idx"), (grad_attn, F32, "grad_attn"), (grad_v, F32, "grad_v"), (grad_table, F32, "grad_table"))
    _call("attention_step2_with_rel_pos_value_backward_cuda_launcher", v, int(N), int(M), int(h), int(hdim), ptr(grad_out),
          ptr(index0), ptr(index1), ptr(attn), ptr(v), ptr(table), ptr(rel_idx), ptr(grad_attn), ptr(grad_v), ptr(grad_table), opts=opts)


# rpe_v2/relative_pos_encoding_cuda_v2.cpp
def dot_prod_with_idx_forward_cuda_v2(N, M, h, hdim, n_max, T, q, index_q, k, index_k, table_q, table_k, rel_idx,
                                      rel_idx_offsets, sort_indices, output, *, opts=None):
    _chk((q, F32, "q"), (index_q, I32, "index_q"), (k, F32, "k"), (index_k, I32, "index_k"), (table_q, F32, "table_q"),
         (table_k, F32, "table_k"), (rel_idx, I32, "rel_idx"), (output, F32, "output"))
    _call("dot_prod_with_idx_forward_cuda_launcher_v2", q, int(N), int(M), int(h), int(hdim), int(n_max), int(T), ptr(q), ptr(index_q),
          ptr(k), ptr(index_k), ptr(table_q), ptr(table_k), ptr(rel_idx), ptr(rel_idx_offsets), ptr(sort_indices), ptr(output), opts=opts)


def dot_prod_with_idx_backward_cuda_v2(N, M, h, hdim, n_max, T, grad_out, q, index_q, k, index_k, table_q, table_k, rel_idx,
                                       rel_idx_offsets, sort_indices, grad_q, grad_k, grad_table_q, grad_table_k, *, opts=None):
    _chk((grad_out, F32, "grad_out"), (q, F32, "q"), (index_q, I32, "index_q"), (k, F32, "k"), (index_k, I32, "index_k"),
         (table_q, F32, "table_q"), (table_k, F32, "table_k"), (rel_idx, I32, "rel_idx"), (grad_q, F32, "grad_q"),
         (grad_k, F32, "grad_k"), (grad_table_q, F32, "grad_table_q"), (grad_table_k, F32, "grad_table_k"))
    _call("dot_prod_with_idx_backward_cuda_launcher_v2", q, int(N), int(M), int(h), int(hdim), int(n_max), int(T), ptr(grad_out), ptr(q),
          ptr(index_q), ptr(k), ptr(index_k), ptr(table_q), ptr(table_k), ptr(rel_idx), ptr(rel_idx_offsets), ptr(sort_indices),
          ptr(grad_q), ptr(grad_k), ptr(grad_table_q), ptr(grad_table_k), opts=opts)


def dot_prod_with_idx_forward_cuda_v3(N, M, h, hdim, n_max, q, index_q_offsets, k, index_k, table_q, table_k, rel_idx, output, *, opts=None):
    _chk((q, F32, "q"), (index_q_offsets, I32, "index_q_offsets"), (k, F32, "k"), (index_k, I32, "index_k"),
         (table_q, F32, "table_q"), (table_k, F32, "table_k"), (rel_idx, I32, "rel_idx"), (output, F32, "output"))
    opts = _lib.with_table_rows(opts, table_q.shape[0])
    _call("dot_prod_with_idx_forward_cuda_launcher_v3", q, int(N), int(M), int(h), int(hdim), int(n_max), ptr(q), ptr(index_q_offsets),
          ptr(k), ptr(index_k), ptr(table_q), ptr(table_k), ptr(rel_idx), ptr(output), opts=opts)


def dot_prod_with_idx_backward_cuda_v3(N, M, h, hdim, n_max, grad_out, q, index_q_offsets, k, index_k, table_q, table_k, rel_idx,
                                       grad_q, grad_k, grad_table_q, grad_table_k, *, opts=None):
    _chk((grad_out, F32, "grad_out"), (q, F32, "q"), (index_q_offsets, I32, "index_q_offsets"), (k, F32, "k"), (index_k, I32, "index_k"),
         (table_q, F32, "table_q"), (table_k, F32, "table_k"), (rel_idx, I32, "rel_idx"), (grad_q, F32, "grad_q"),
         (grad_k, F32, "grad_k"), (grad_table_q, F32, "grad_table_q"), (grad_table_k, F32, "grad_table_k"))
    opts = _lib.with_table_rows(opts, table_q.shape[0])
    _call("dot_prod_with_idx_backward_cuda_launcher_v3", q, int(N), int(M), int(h), int(hdim), int(n_max), ptr(grad_out), ptr(q),
          ptr(index_q_offsets), ptr(k), ptr(index_k), ptr(table_q), ptr(table_k), ptr(rel_idx), ptr(grad_q), ptr(grad_k),
          ptr(grad_table_q), ptr(grad_table_k), opts=opts)


def attention_step2_with_rel_pos_value_forward_cuda_v2(N, M, h, hdim, n_max, attn, v, index0_offsets, index1, table, rel_idx, output, *, opts=None):
    _chk((attn, F32, "attn"), (v, F32, "v"), (index0_offsets, I32, "index0_offsets"), (index1, I32, "index1"), (table, F32, "table"),
         (rel_idx, I32, "rel_idx"), (output, F32, "output"))
    opts = _lib.with_table_rows(opts, table.shape[0])
    _call("attention_step2_with_rel_pos_value_forward_cuda_launcher_v2", v, int(N), int(M), int(h), int(hdim), int(n_max), ptr(attn), ptr(v),
          ptr(index0_offsets), ptr(index1), ptr(table), ptr(rel_idx), ptr(output), opts=opts)


def attention_step2_with_rel_pos_value_backward_cuda_v2(N, M, h, hdim, n_max, grad_out, index0_offsets, index1, attn, v, table, rel_idx,
                                                        grad_attn, grad_v, grad_table, *, opts=None):
    _chk((grad_out, F32, "grad_out"), (index0_offsets, I32, "index0_offsets"), (index1, I32, "index1"), (attn, F32, "attn"),
         (v, F32, "v"), (table, F32, "table"), (rel_idx, I32, "rel_idx"), (grad_attn, F32, "grad_attn"), (grad_v, F32, "grad_v"),
         (grad_table, F32, "grad_table"))
    opts = _lib.with_table_rows(opts, table.shape[0])
    _call("attention_step2_with_rel_pos_value_backward_cuda_launcher_v2", v, int(N), int(M), int(h), int(hdim), int(n_max), ptr(grad_out),
          ptr(index0_offsets), ptr(index1), ptr(attn), ptr(v), ptr(table), ptr(rel_idx), ptr(grad_attn), ptr(grad_v), ptr(grad_table), opts=opts)


# subtraction/ and aggregation/ (Point-Transformer vector attention) are bound by the reference
# (pointops_api.cpp:23-26) but called by no model in it: not on the hot path.
def _off_path(name):
    def f(*a, **k):
        raise NotImplementedError(f"{name}: Point-Transformer op outside the Stratified hot path (SURVEY.md §8)")
    f.__name__ = name
    return f


subtraction_forward_cuda = _off_path("subtraction_forward_cuda")
subtraction_backward_cuda = _off_path("subtraction_backward_cuda")
aggregation_forward_cuda = _off_path("aggregation_forward_cuda")
aggregation_backward_cuda = _off_path("aggregation_backward_cuda")
