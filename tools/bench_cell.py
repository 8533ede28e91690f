"""Cell attention only (fused.cell_attention forward + backward), per stage and pattern, on the bench scene.
Meant to be run under `rocprofv3 --kernel-trace --stats` for per-kernel times (diagnostic; GPU box only).

    python tools/bench_cell.py [N] [stages e.g. 0,1] [reps] [--deterministic]

--deterministic: the backward without float atomics (fused.cell_attention(..., deterministic=True)) beside the default one, in the same
process, the two modes alternating call by call.  Per stage and pattern the default mode's line as always, then a line with both
backwards (median, and the default's min..max over the repetitions) and the bytes of the two partial buffers; one JSON line at the end.
"""
import json, os, statistics, sys
import torch
import timing  # first: it puts the repository root on sys.path
from stratified_transformer_amd import scene, pipeline, fused


def main():
    argv = [a for a in sys.argv[1:] if a != '--deterministic']
    modes = (False, True) if '--deterministic' in sys.argv[1:] else (False,)
    N = int(argv[0]) if len(argv) > 0 else 100000
    stages = [int(s) for s in argv[1].split(',')] if len(argv) > 1 else [0, 1, 2, 3]
    reps = int(argv[2]) if len(argv) > 2 else 5
    rows = []
    cfg = pipeline.s3dis_config()
    xyz_np = scene.make_room(N, 0)
    if os.environ.get('SORTED'):  # experiment: points in (large) window order - what memory locality of the rows would give
        import numpy as np
        c = np.floor(xyz_np / float(os.environ['SORTED'])).astype(np.int64)
        xyz_np = np.ascontiguousarray(xyz_np[np.argsort((c[:, 2] * 4096 + c[:, 1]) * 4096 + c[:, 0], kind='stable')])
    xyz = torch.from_numpy(xyz_np).cuda()
    off = torch.tensor([N], dtype=torch.int32, device='cuda')
    states, results = pipeline.scene_pass(xyz, off, cfg, cells=True)
    torch.cuda.synchronize()
    for si in stages:
        s, r = states[si], results[si]
        tq, tk, tv = s.tables
        for pat in ('even', 'odd'):
            plan = r[pat].cells
            if os.environ.get('TASKS') == 'natural':  # experiment: cells in their (small window, large window) order instead of by size
                plan = plan.with_tasks(torch.arange(plan.n_cells, dtype=torch.int32, device='cuda'), torch.tensor([plan.n_cells], dtype=torch.int32, device='cuda'))
            for x in (s.q, s.k, s.v, tq, tk, tv):
                x.grad = None
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            tf, tb = {m: [] for m in modes}, {m: [] for m in modes}
            for it in range(reps + 2):
                for det in modes:
                    e[0].record()
                    out = fused.cell_attention(s.q, s.k, s.v, tq, tk, tv, plan, deterministic=det)
                    e[1].record()
                    out.backward(s.grad_out)
                    e[2].record()
                    torch.cuda.synchronize()
                    if it >= 2:
                        tf[det].append(e[0].elapsed_time(e[1])); tb[det].append(e[1].elapsed_time(e[2]))
            print('stage', si, pat, 'cells', plan.n_cells, 'P', plan.n_pairs, 'K', plan.n_keyslots, 'nk_max', plan.nk_max,
                  'fwd us', round(sum(tf[False]) / reps * 1e3), 'bwd us', round(sum(tb[False]) / reps * 1e3), flush=True)
            if True in modes:
                us = lambda ms: round(ms * 1e3)  # noqa: E731
                kp, tp = fused.cell_partial_buffers(plan, s.q.shape[1], tq.shape[0], s.q.device)
                row = dict(stage=si, pattern=pat, heads=s.q.shape[1], K=plan.n_keyslots, bwd_us_default=us(statistics.median(tb[False])),
                           bwd_us_default_min=us(min(tb[False])), bwd_us_default_max=us(max(tb[False])), bwd_us_deterministic=us(statistics.median(tb[True])),
                           bwd_us_deterministic_min=us(min(tb[True])), bwd_us_deterministic_max=us(max(tb[True])),
                           key_partial_bytes=kp.numel() * 4, table_partial_rows=tp.shape[1], table_partial_bytes=tp.numel() * 4)
                del kp, tp
                rows.append(row)
                print('stage', si, pat, 'deterministic bwd us', row['bwd_us_deterministic'], 'default bwd us', row['bwd_us_default'], 'min..max',
                      row['bwd_us_default_min'], row['bwd_us_default_max'], 'key partial bytes', row['key_partial_bytes'], 'table partial bytes',
                      row['table_partial_bytes'], flush=True)
    if rows:
        print(json.dumps(dict(tool='bench_cell', N=N, reps=reps, modes='alternating call by call', rows=rows)), flush=True)


if __name__ == "__main__":
    main()
