"""stratified_transformer_amd — MI355X (gfx950) implementation of the Stratified Transformer's
windowed sparse-attention hot path, behind the reference's own operator API.

    stratified_transformer_amd.pointops        drop-in for lib/pointops2/functions/pointops.py
    stratified_transformer_amd.pointops2_cuda  drop-in for the compiled module `pointops2_cuda`
    stratified_transformer_amd.compat          providers of the third-party names the model imports
                                               (torch_scatter.scatter_softmax, torch_geometric.nn.voxel_grid, ...)
    stratified_transformer_amd.cluster         the steps behind the model: dbscan / instances on csrc/dbscan.hip, contacts / objects on csrc/contacts.hip,
                                               label_boxes / merge_objects on csrc/boxes.hip, clean_supports / box_supports on
                                               csrc/supports.hip, the host-side box_detection and detect_boxes = box_supports + merge_objects
                                               (all ten also exported here)
    stratified_transformer_amd.evaluate        whole-scene evaluation on csrc/evaltile.hip: crop cover, votes with shifts, IoU; the fork's
                                               detection pass in one call (scene_eval, scene_predict, dense_points, detect_scene also exported here)
    stratified_transformer_amd.augment         the train-time transforms of util/transform.py on device tensors (csrc/augment.hip); with
                                               dataprep.data_prepare(transform=, shuffle=) and dataprep.collate: file -> device -> batch
    stratified_transformer_amd.optim           AdamW and GradScaler: scaler.step(optimizer) as one call on csrc/optim.hip, no read-back
    stratified_transformer_amd.layers          installable fast BasicLayer.forward / WindowAttention.forward (same signatures)
    include/pointops2_hip.h                    the C ABI underneath (libpointops2_hip.so)

`install()` registers the drop-in modules in sys.modules so that the reference's
model/stratified_transformer.py imports and runs unmodified under PyTorch-ROCm.
"""
import sys

__all__ = ["install", "build", "dbscan", "instances", "contacts", "objects", "label_boxes", "merge_objects", "box_detection", "scene_eval",
           "clean_supports", "box_supports", "scene_predict", "dense_points", "detect_boxes", "detect_scene", "install_fused_blocks", "install_fast_decoder", "segmentation_loss",
           "fuse_batch_norms", "unfuse_batch_norms", "fuse_sync_batch_norms", "fuse_linear_grads", "unfuse_linear_grads"]


def __getattr__(name):
    # dbscan / instances / contacts / objects / label_boxes / merge_objects / box_detection / clean_supports / box_supports / detect_boxes
    # live in .cluster, which needs torch: bound on first use, as every other submodule is imported on demand
    if name in ("dbscan", "instances", "contacts", "objects", "label_boxes", "merge_objects", "box_detection", "clean_supports", "box_supports",
                "detect_boxes"):
        from . import cluster
        return getattr(cluster, name)
    if name in ("scene_eval", "scene_predict", "dense_points", "detect_scene"):
        from . import evaluate
        return getattr(evaluate, name)
    if name == "install_fused_blocks":  # layers.install_fused_blocks: the blocks' residual / DropPath / LayerNorm glue on csrc/rownorm.hip
        from . import layers
        return layers.install_fused_blocks
    if name == "install_fast_decoder":  # layers.install_fast_decoder: Upsample's interpolation and add on csrc/upsample.hip
        from . import layers
        return layers.install_fast_decoder
    if name in ("fuse_batch_norms", "unfuse_batch_norms", "fuse_sync_batch_norms"):  # layers.*: BatchNorm1d / SyncBatchNorm + activation (+ residual) of the stem and the heads on csrc/batchnorm.hip
        from . import layers
        return getattr(layers, name)
    if name in ("fuse_linear_grads", "unfuse_linear_grads"):  # layers.*: grad_weight / grad_bias of the nn.Linear modules on csrc/linear_grads.hip
        from . import layers
        return getattr(layers, name)
    if name == "segmentation_loss":  # pointops.segmentation_loss: cross-entropy, L1 shift, their sum and the IoU counts on csrc/seg_loss.hip
        from . import pointops
        return pointops.segmentation_loss
    if name == "optim":  # optim.AdamW / optim.GradScaler: the loss scaler's check and the AdamW update in one call on csrc/optim.hip
        import importlib
        return importlib.import_module(".optim", __name__)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def build(verbose=False):
    """Compile libpointops2_hip.so for gfx950 (works without a GPU)."""
    from . import _lib
    return _lib.build(verbose=verbose)


def install(third_party=True, fast_layers=False, pooled_transition=False):
    """Make `import pointops2_cuda`, `from lib.pointops2.functions import pointops` and (optionally) the
    model's third-party imports resolve to this package.

    fast_layers=True: additionally rebind `BasicLayer.forward` / `WindowAttention.forward` of the (unmodified, importable)
    `model.stratified_transformer` to the forms of `stratified_transformer_amd.layers`: the stage's index is built once on
    the device and every attention block runs as one fused function on its cell plan - the path bench.py's headline
    (`single_pass.cell`) measures.  Without it the model runs on the operator API alone (`single_pass.operator_api`).

    pooled_transition: sets `layers.POOLED_TRANSITION`.  True: the installed `TransitionDown.forward` runs its LayerNorm and Linear
    once per source row and pools with `pointops.grouped_max` (csrc/grouped_max.hip) instead of pushing the k gathered copies of
    every sampled row through them; the same maxima up to fp32 rounding.  The default keeps the reference's order of operations."""
    from . import pointops2_cuda
    sys.modules.setdefault("pointops2_cuda", pointops2_cuda)
    if third_party:
        from . import compat
        compat.install()
    from . import layers
    layers.POOLED_TRANSITION = bool(pooled_transition)
    if fast_layers:
        return layers.install_fast_layers()
