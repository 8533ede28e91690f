"""One Swin3D stage (model/swin3d_transformer.py) at the stage-0 shape of the S3DIS config - a 100k-point room, C = 48, h = 3, window 0.16,
quant 0.01 (31-row tables), depth 2 (a plain and a shifted block): the blocks' attention (qkv Linear -> attention -> proj, what
layers.swin_window_attention_forward runs) on the cell plans of index_build.swin_stage_index_hip(..., cell_table_rows=31) beside the
same modules on the pair list (fused.window_attention, rel-pos index by the torch chain of swin_rel_pos_index per call, as the model
file computes it), on the same GPU, same inputs, index build excluded.  Prints ONE JSON line (GPU box only; a missing GPU is an error).

    python tools/bench_swin.py [--points 100000] [--reps 30] [--warmup 5] [--out FILE]

Modes: fp32 and autocast(fp16).  Per mode and side: median over `reps` of the forward and of forward + backward (gradients of the
features and of every parameter) of the two blocks' attention in a row, each bracketed by events on the stream, the two sides
alternating; `ratio_*` = pair list / plan (> 1: the plan is faster).
"""
import argparse

import torch
from torch import nn

import timing  # first: it puts the repository root on sys.path
from stratified_transformer_amd import index_build, layers, scene  # noqa: E402

C, H, W, QUANT, DEPTH = 48, 3, 0.16, 0.01, 2


class Attention(nn.Module):
    """the parameters and attribute names of the model's WindowAttention (swin3d_transformer.py:94-127)"""

    def __init__(self):
        super().__init__()
        self.dim, self.num_heads, self.window_size, self.quant_size = C, H, W, QUANT
        self.scale = (C // H) ** -0.5
        self.rel_query = self.rel_key = self.rel_value = True
        rows = index_build.swin_table_rows(W, QUANT)
        self.relative_pos_query_table = nn.Parameter(torch.randn(rows, H, C // H, 3) * 0.02)
        self.relative_pos_key_table = nn.Parameter(torch.randn(rows, H, C // H, 3) * 0.02)
        self.relative_pos_value_table = nn.Parameter(torch.randn(rows, H, C // H, 3) * 0.02)
        self.qkv, self.proj, self.proj_drop = nn.Linear(C, 3 * C), nn.Linear(C, C), nn.Dropout(0.0)


def stage(attns, feats, xyz, blocks, shifts, on_plan):
    x = feats
    for attn, blk, shift in zip(attns, blocks, shifts):
        attn._sta_block = blk if on_plan else None
        try:
            x = x + layers.swin_window_attention_forward(attn, x, xyz, blk.index_0, blk.offsets, blk.n_max, blk.index_1, shift)
        finally:
            attn._sta_block = None
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    timing.need_gpu("bench_swin")
    xyz = torch.from_numpy(scene.make_room(a.points, 0)).cuda()
    n = xyz.shape[0]
    offset = torch.tensor([n], dtype=torch.int32, device="cuda")
    rows = index_build.swin_table_rows(W, QUANT)
    cap = index_build.cell_query_cap(n, H)
    even, odd, _ = index_build.swin_stage_index_hip(xyz, offset, W, QUANT, cell_table_rows=rows, cell_max_queries=cap)
    blocks = (even, odd)
    shifts = (0.0, 1 / 2 * torch.tensor([W] * 3).type_as(xyz))
    torch.manual_seed(0)
    attns = nn.ModuleList([Attention() for _ in range(DEPTH)]).cuda()
    g = torch.Generator(device="cuda").manual_seed(1)
    feats = torch.randn(n, C, device="cuda", generator=g).requires_grad_(True)
    go = torch.randn(n, C, device="cuda", generator=g)
    sides = {"plan": lambda f: stage(attns, f, xyz, blocks, shifts, True), "pair_list": lambda f: stage(attns, f, xyz, blocks, shifts, False)}
    result = {"tool": "bench_swin", "device": torch.cuda.get_device_name(0), "points": n, "channels": C, "heads": H, "window": W, "quant": QUANT,
              "table_rows": rows, "depth": DEPTH, "cell_max_queries": cap, "reps": a.reps, "warmup": a.warmup,
              "patterns": [{"pairs": int(b.index_1.shape[0]), "cells": b.cells.n_cells, "windows": b.cells.n_parents, "keys_max": b.cells.nk_max}
                           for b in blocks]}

    def clear():
        feats.grad = None
        attns.zero_grad(set_to_none=True)

    for mode, amp in (("fp32", False), ("autocast_f16", True)):
        def forward(fn):
            with torch.autocast("cuda", dtype=torch.float16, enabled=amp):
                return fn(feats)

        times, last = timing.fwd_bwd_windows({s: (lambda fn=fn: forward(fn)) for s, fn in sides.items()}, clear,
                                             lambda out: out.backward(go.to(out.dtype)), a.reps, a.warmup)
        outs = {s: last[s][0].detach().float() for s in sides}
        r = {"max_abs_diff_out": float((outs["plan"] - outs["pair_list"]).abs().max())}
        for s in sides:
            r[s] = timing.fwd_bwd_summary(times, s)
        r["ratio_fwd"] = round(r["pair_list"]["fwd_ms"] / r["plan"]["fwd_ms"], 2)
        r["ratio_fwd_bwd"] = round(r["pair_list"]["fwd_bwd_ms"] / r["plan"]["fwd_bwd_ms"], 2)
        result[mode] = r
    timing.emit(result, a.out)


if __name__ == "__main__":
    main()
