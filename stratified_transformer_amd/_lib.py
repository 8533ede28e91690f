"""ctypes binding of libpointops2_hip.so (C ABI: include/pointops2_hip.h).

The product path has no CPU fallback: if the HIP library is missing, `lib()` raises.  PyTorch is used
only for device memory and streams; every pointer crossing this boundary is a raw device address.
"""
import ctypes
import os
import subprocess

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libpointops2_hip.so")
CSRC = os.path.join(_HERE, "csrc")
_lib = None

I, U, P, Z, F, D = ctypes.c_int, ctypes.c_uint, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_float, ctypes.c_double
Q = ctypes.c_longlong


class LaunchOpts(ctypes.Structure):
    """pointops2_launch_opts (include/pointops2_hip.h): options of the next launch on this thread only; all-zero = the
    reference's arguments alone.  Pointers are raw device addresses of tensors the caller keeps alive over the launch."""
    _fields_ = [("table_rows", I), ("key_rows", I), ("csc_offsets", P), ("csc_pair", P), ("csc_query", P), ("row_order", P),
                ("row_order_rows", I), ("workspace", P), ("workspace_bytes", Z), ("point_count", I), ("batch_count", I),
                ("fps_prev_idx", P), ("fps_prev_new_offset", P), ("fps_unordered", I)]


def with_table_rows(opts, L):
    """`opts` (a new LaunchOpts if None) with table_rows = L, which the rel-pos and window_* fast kernels need"""
    opts = opts if opts is not None else LaunchOpts()
    opts.table_rows = int(L)
    return opts


# name -> argtypes; mirrors include/pointops2_hip.h one to one
SIGNATURES = {
    "pointops2_set_stream": [P],
    "pointops2_diag_set_fps_patience": [ctypes.c_ulonglong],
    "pointops2_set_launch_opts": [ctypes.POINTER(LaunchOpts)],
    "pointops2_csc_build": [I, I, P, P, P, P, P, P, Z],
    "furthestsampling_cuda_launcher": [I, I, P, P, P, P, P],
    "knnquery_cuda_launcher": [I, I, P, P, P, P, P, P],
    "grouping_forward_cuda_launcher": [I, I, I, P, P, P],
    "grouping_backward_cuda_launcher": [I, I, I, P, P, P],
    "interpolation_forward_cuda_launcher": [I, I, I, P, P, P, P],
    "interpolation_backward_cuda_launcher": [I, I, I, P, P, P, P],
    "attention_step1_forward_cuda_launcher": [I, I, I, I, P, P, P, P, P],
    "attention_step1_backward_cuda_launcher": [I, I, I, I, P, P, P, P, P, P, P],
    "attention_step2_forward_cuda_launcher": [I, I, I, I, P, P, P, P, P],
    "attention_step2_backward_cuda_launcher": [I, I, I, I, P, P, P, P, P, P, P],
    "attention_step1_forward_cuda_launcher_v2": [I, I, I, I, U, P, P, P, P, P],
    "attention_step1_backward_cuda_launcher_v2": [I, I, I, I, U, P, P, P, P, P, P, P],
    "attention_step2_forward_cuda_launcher_v2": [I, I, I, I, P, P, P, P, P],
    "attention_step2_backward_cuda_launcher_v2": [I, I, I, I, P, P, P, P, P, P, P],
    "dot_prod_with_idx_forward_cuda_launcher": [I, I, I, I, P, P, P, P, P],
    "dot_prod_with_idx_backward_cuda_launcher": [I, I, I, I, P, P, P, P, P, P, P],
    "attention_step2_with_rel_pos_value_forward_cuda_launcher": [I, I, I, I, P, P, P, P, P, P, P],
    "attention_step2_with_rel_pos_value_backward_cuda_launcher": [I, I, I, I, P, P, P, P, P, P, P, P, P, P],
    "dot_prod_with_idx_forward_cuda_launcher_v2": [I, I, I, I, I, I, P, P, P, P, P, P, P, P, P, P],
    "dot_prod_with_idx_backward_cuda_launcher_v2": [I, I, I, I, I, I, P, P, P, P, P, P, P, P, P, P, P, P, P, P],
    "dot_prod_with_idx_forward_cuda_launcher_v3": [I, I, I, I, I, P, P, P, P, P, P, P, P],
    "dot_prod_with_idx_backward_cuda_launcher_v3": [I, I, I, I, I, P, P, P, P, P, P, P, P, P, P, P, P],
    "attention_step2_with_rel_pos_value_forward_cuda_launcher_v2": [I, I, I, I, I, P, P, P, P, P, P, P],
    "attention_step2_with_rel_pos_value_backward_cuda_launcher_v2": [I, I, I, I, I, P, P, P, P, P, P, P, P, P, P],
    "subtraction_forward_cuda_launcher": [I, I, I, P, P, P, P],
    "subtraction_backward_cuda_launcher": [I, I, I, P, P, P, P],
    "aggregation_forward_cuda_launcher": [I, I, I, I, P, P, P, P, P],
    "aggregation_backward_cuda_launcher": [I, I, I, I, P, P, P, P, P, P, P, P],
    "segment_softmax_forward_launcher": [I, I, I, P, P, P],
    "window_logits_softmax_forward_launcher": [I, I, I, I, P, P, P, P, P, P, P, P],
    "window_attention_backward_launcher": [I, I, I, I] + [P] * 18,
    "segment_softmax_backward_launcher": [I, I, I, P, P, P, P],
    "csr_expand_launcher": [I, I, P, P],
    "pointops2_csr_matches_launcher": [I, I, P, P, I, P],
    "pointops2_bbox_launcher": [I, P, P],
    "pointops2_window_partition_launcher": [I, I, P, P, P, F, F, I, P, P, P, P, P, Z],
    "pointops2_window_partitions4_launcher": [I, I, P, P, P, F, P, P, P, P, P, P, Z],
    "pointops2_row_order_launcher": [I, I, P, P, P, P, Z],
    "pointops2_window_coord_launcher": [I, P, P, F, I, P],
    "pointops2_sampled_buckets_launcher": [I, I, P, P, P, P, P, P, P, P, Z],
    "pointops2_pairs_count_launcher": [I, P, P, P, P, P, P, P, P, Z],
    "pointops2_pairs_fill_launcher": [I, P, F, F, P, P, P, P, P, P, P, P, P, P, P],
    "pointops2_voxel_keys_launcher": [I, I, P, ctypes.c_double, P],
    "pointops2_crop_dist_launcher": [I, I, P, I, P],
    "pointops2_cell_plan_count_launcher": [I, I, P, P, P, P, P, P, P, P, P, P, P, P, P, P, Z],
    "pointops2_cell_plan_prepare_launcher": [I, I, P, P, P, P, P, P, Z],
    "pointops2_cell_plan_sizes_launcher": [I, P, P, P, P, P, P, P, P, P, P, P, P, P, Z],
    "pointops2_cell_plan_fill_launcher": [I, P, F, F, I, P, P, P, P, P, P, P, P, P, P, P, P],
    "pointops2_swin_quant_launcher": [I, P, P, F, F, I, P],
    "pointops2_swin_pairs_rel_launcher": [I, I, P, P, P, I, P],
    "pointops2_swin_cell_fill_launcher": [I, I, I] + [P] * 13,
    "cell_attention_forward_launcher": [P, I, I, I] + [P] * 9,
    "cell_attention_backward_launcher": [P, I, I, I] + [P] * 16,
    "cell_attention_forward_bf16_launcher": [P, I, I, I] + [P] * 9,
    "cell_attention_backward_bf16_launcher": [P, I, I, I] + [P] * 16,
    "cell_attention_qkv_forward_launcher": [P, I, I, I, P, I, F] + [P] * 6,
    "cell_attention_qkv_backward_launcher": [P, I, I, I, P, P, I, F] + [P] * 10,
    "cell_key_grads_reduce_launcher": [I, I, P, P, P, P, I],
    "cell_table_grads_reduce_launcher": [I, I, I, P, P, P, P],
    "cell_attention_det_backward_launcher": [P, I, I, I] + [P] * 16 + [P, P, P, Z, P, Z],
    "cell_attention_det_backward_bf16_launcher": [P, I, I, I] + [P] * 16 + [P, P, P, Z, P, Z],
    "cell_attention_qkv_det_backward_launcher": [P, I, I, I, P, P, I, F] + [P] * 10 + [P, P, P, Z, P, Z],
    "kpconv_aggregate_forward_launcher": [I, I, I, I, I, P, P, P, P, P, F, P],
    "kpconv_aggregate_backward_launcher": [I, I, I, I, I, P, P, P, P, F, P, P],
    "grouped_max_forward_launcher": [I, I, I, I, I, P, P, P, P],
    "grouped_max_backward_launcher": [I, I, I, I, I, P, P, P, P, P],
    "residual_norm_forward_launcher": [I, I, I, I, P, P, P, P, P, F, P, P, P],
    "residual_norm_backward_launcher": [I, I, I, I, P, P, P, P, P, P, P, P, P, I, P, P],
    "batch_norm_act_stats_launcher": [I, I, I, P, P, I, F, F, P, P, P],
    "batch_norm_act_forward_launcher": [I, I, I, I, I, F, P, P, P, I, F, P, P, P, P, P],
    "batch_norm_act_backward_launcher": [I, I, I, I, F, I, P, P, P, P, P, P, I, P, P, P],
    "batch_norm_act_moments_launcher": [I, I, I, P, P, I, P],
    "batch_norm_act_merge_launcher": [I, I, P, F, F, P, P, P, P],
    "batch_norm_act_sync_backward_launcher": [I, I, I, I, F, P, P, P, P, P, I, P, P, P],
    "seg_loss_forward_launcher": [I, I, I, I, P, P, P, P, Q, F, F, P, P, I, P, P, P],
    "seg_loss_backward_launcher": [I, I, I, I, P, P, P, P, P, P, P, Q, F, F, P, P],
    "pointops2_dbscan_keys_launcher": [I, I, P, P, D, D, D, D, I, I, I, P],
    "pointops2_dbscan_prepare_launcher": [I, I, I, I, I, P, P, P, P, P, P],
    "pointops2_dbscan_core_launcher": [I, I, P, P, P, P, P, P, P, P],
    "pointops2_dbscan_round_launcher": [I, I, P, P, P, P, P, P, P],
    "pointops2_dbscan_label_launcher": [I, I, P, P, P, P, P, P, P, P],
    "pointops2_contacts_count_launcher": [I, I, P, P, P, F, P, P],
    "pointops2_contacts_min_launcher": [I, I, P, P],
    "pointops2_label_boxes_launcher": [I, I, P, P, P, P, P],
    "pointops2_reach_rows_launcher": [I, I, P, P, P, F, P],
    "pointops2_supports_keys_launcher": [I, I, P, P, P, D, I, I, I, P],
    "pointops2_supports_means_launcher": [I, I, I, P, P, P, P, P, P, P, P],
    "pointops2_supports_count_launcher": [I, P, P, F, I, P],
    "pointops2_evaltile_seed_dist_launcher": [I, I, P, P, P, P, P, P],
    "pointops2_evaltile_update_launcher": [I, I, I, P, P, P, P, P],
    "pointops2_evaltile_vote_launcher": [I, I, I, I, P, P, P, P, P],
    "pointops2_evaltile_vote_shift_launcher": [I, I, I, I, P, I, P, P, P, P, P, P],
    "pointops2_augment_pass_launcher": [I] * 6 + [P] * 10,
    "pointops2_augment_blur_launcher": [Q, I, I, P, P, P],
    "optim_adamw_step_launcher": [I, I, P, P, Z, P, P, I],
    "optim_step_launcher": [I, I, I, P, P, Z, P, P, I, D, P],
    "residual_norm_stream_forward_launcher": [I, I, I, I, I, P, P, P, P, P, F, P, P, P],
    "residual_norm_stream_backward_launcher": [I, I, I, I, I, P, P, P, P, P, P, P, P, P, I, P, P],
    "linear_grads_partial_launcher": [I, I, I, I, I, P, P, P, I],
    "linear_grads_reduce_launcher": [I, I, I, P, I, P, P],
    "gather_add_forward_launcher": [I, I, I, I, I, I, P, P, P, P, P],
    "gather_add_backward_launcher": [I, I, I, I, I, P, P, P, P, P],
}
# entry points with a non-void result
RESULTS = {
    "pointops2_get_stream": ([], P),
    "pointops2_last_error": ([], ctypes.c_char_p),
    "pointops2_abi_version": ([], I),
    "pointops2_csc_workspace_bytes": ([I, I], Z),
    "pointops2_fps_workspace_bytes": ([I, I], Z),
    "pointops2_knn_workspace_bytes": ([I, I, I], Z),
    "pointops2_index_workspace_bytes": ([I], Z),
    "pointops2_partitions4_workspace_bytes": ([I], Z),
    "pointops2_row_order_workspace_bytes": ([I], Z),
    "pointops2_cell_plan_workspace_bytes": ([I], Z),
    "pointops2_cell_forward_variant": ([P, I, I, I, I], I),
    "pointops2_evaltile_max_parts": ([], I),
    "pointops2_optim_workspace_bytes": ([I, I], Z),
    "pointops2_optim_step_workspace_bytes": ([I, I, Q], Z),
    "pointops2_linear_grads_partial_rows": ([I, I, I], I),
    "pointops2_cell_table_partial_rows": ([P, I], I),
}
# kind of optim_step_launcher (POINTOPS2_OPTIM_*)
OPTIM_KINDS = {"adamw": 0, "sgd": 1}

# codes of pointops2_cell_forward_variant (POINTOPS2_CELL_FWD_* of include/pointops2_hip.h): the forward kernel a cell launch runs
CELL_FWD = {"error": -1, "none": 0, "mfma64": 1, "mfma80": 2, "valu80": 3, "valu160": 4}
# storage type of the rows of a packed qkv (POINTOPS2_ROWS_*): cell_attention_qkv_*_launcher, grouped_max_*_launcher, gather_add_*_launcher
ROW_TYPES = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
# rows of a chunk of linear_grads_partial_launcher (POINTOPS2_LINEAR_GRADS_ROWS): its partials have ceil(n / LINEAR_GRADS_ROWS) blocks
LINEAR_GRADS_ROWS = 512
# activation of batch_norm_act_*_launcher (POINTOPS2_ACT_*)
ACTIVATIONS = {"none": 0, "relu": 1, "leaky_relu": 2, "tanh": 3}


def cell_forward_variant(plan, h, L, bf16=False, hdim=16):
    """Name (a key of CELL_FWD) of the forward kernel cell_attention runs on `plan` (index_build.CellPlan, or a bare
    index_build.CellPlanStruct, or None) for h heads, tables of L rows and fp32 / bf16 storage.  Reads host fields only."""
    arg = None if plan is None else plan.c_arg() if hasattr(plan, "c_arg") else ctypes.byref(plan)
    code = lib().pointops2_cell_forward_variant(arg, int(h), int(hdim), int(L), int(bool(bf16)))
    return {v: k for k, v in CELL_FWD.items()}[code]


def exported_symbols():
    """Every symbol include/pointops2_hip.h declares (used by the no-GPU ABI test)."""
    return sorted(list(SIGNATURES) + list(RESULTS))


def build(verbose=False):
    """Compile the HIP sources for gfx950 (hipcc cross-compiles without a GPU)."""
    cmd = ["make", "-C", CSRC, "-j8"] + ([] if verbose else ["-s"])
    subprocess.check_call(cmd)
    return LIB_PATH


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: the HIP extension has not been built "
                "(run `python -c 'import __graft_entry__ as g; g.build()'` or `make -C stratified_transformer_amd/csrc`). "
                "There is no CPU fallback for the product path.")
        l = ctypes.CDLL(LIB_PATH)
        for name, argtypes in SIGNATURES.items():
            fn = getattr(l, name)
            fn.argtypes = argtypes
            fn.restype = None
        for name, (argtypes, restype) in RESULTS.items():
            fn = getattr(l, name)
            fn.argtypes = argtypes
            fn.restype = restype
        _lib = l
    return _lib


def ptr(t):
    """Raw device address of a tensor (None -> NULL)."""
    if t is None:
        return None
    return t.data_ptr()


def check_tensor(t, dtype, name):
    if not t.is_cuda:
        raise RuntimeError(f"{name}: expected a GPU tensor (the pointops2 HIP path has no CPU fallback), got {t.device}")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise RuntimeError(f"{name}: expected a contiguous tensor")
    return t


def check_tensors(*triples):
    """check_tensor for each (tensor, dtype, name)"""
    for t, dt, name in triples:
        check_tensor(t, dt, name)


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
# the current device's index without torch.cuda.current_device's lazy-init check (a launch has device tensors: torch is initialised)
_current_device = getattr(torch._C, "_cuda_getDevice", None) or torch.cuda.current_device


CALLS = [0]  # library launcher calls so far (bench.py: per pass)


def call(name, *args, device=None, opts=None):
    """Launch `name` on torch's current stream of `device` and surface library errors.  opts: LaunchOpts for this launch
    (None: the reference's arguments alone).

    The library works on the CURRENT HIP device: the side streams and events of ForkJoin (csrc/misc.hip), the
    hipFuncSetAttribute of allow_big_lds, num_cus() and the held-CU events are all state of whichever device was current
    when they were first touched.  So this function, and no caller, makes the operands' device current: `device` None or
    without an index means the current device; an index equal to the current device's builds no guard object (the usual
    case, and these calls are bound by the host); any other index runs the whole sequence - set_stream, set_launch_opts,
    the launcher, last_error - under torch.cuda.device(device)."""
    CALLS[0] += 1
    if device is not None and device.index is not None and device.index != _current_device():
        with torch.cuda.device(device):
            _launch(name, args, device, opts)
    else:
        _launch(name, args, device, opts)


def _launch(name, args, device, opts):
    l = lib()
    if _raw_stream is not None and device is not None and device.index is not None:
        stream = _raw_stream(device.index)  # the raw hipStream_t, without building a torch.cuda.Stream object
    else:
        stream = torch.cuda.current_stream(device).cuda_stream
    l.pointops2_set_stream(stream)
    if opts is not None:
        l.pointops2_set_launch_opts(opts)
    getattr(l, name)(*args)
    err = l.pointops2_last_error()
    if err is not None:
        raise RuntimeError(f"{name}: {err.decode()}")
