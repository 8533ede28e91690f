"""The stand-in layers the block-level benches run: four standin.BasicLayers of depth 2 strung as the model strings them on the room scene
(bench_block's "blocks" legs, bench_linear's).  A workload builder: no clock in it."""
import torch

import timing  # noqa: F401  (first: it puts the repository root on sys.path)
from stratified_transformer_amd import compat, layers, pipeline, pointops as P, scene, standin  # noqa: E402


def stage_rows(points, cfg):
    from stratified_transformer_amd import index_build
    rows, off = [], [points]
    for _ in cfg.stages:
        rows.append(off[-1])
        off = index_build.transition_down_offset(off, cfg.ratio)
    return rows


def stand_in_step(points, amp, drop):
    """-> step(), [(rows, channels) per stage], the net: one forward + backward of four stand-in BasicLayers strung as the model strings them"""
    cfg = pipeline.s3dis_config()
    st = cfg.stages
    xyz = torch.from_numpy(scene.make_room(points, 0)).cuda()
    offset = torch.tensor([points], dtype=torch.int32, device="cuda")
    torch.manual_seed(0)
    net = torch.nn.ModuleList([standin.BasicLayer(cfg.downsample_scale, 2, s.channels, s.num_heads, s.window_size, s.quant_size, ratio=cfg.ratio, k=cfg.k,
                                                  out_channels=st[i + 1].channels if i + 1 < len(st) else None) for i, s in enumerate(st)]).cuda().train()
    with torch.no_grad():
        for name, p in net.named_parameters():
            if "relative_pos" in name:
                p.normal_(0.0, 0.02)
    for layer in net:
        for blk in layer.blocks:
            blk.drop_path = compat.DropPath(drop)
    net.train()
    feats0 = torch.randn(points, st[0].channels, device="cuda")
    sites = [(int(n), s.channels) for n, s in zip(stage_rows(points, cfg), st)]

    def step():
        P.clear_caches()
        layers.forget_clouds()
        net.zero_grad(set_to_none=True)
        f, x, o = feats0.clone().requires_grad_(True), xyz, offset
        loss = None
        with torch.autocast("cuda", dtype=torch.float16, enabled=amp):
            for layer in net:
                f_out, _, _, f, x, o = layer(f, x, o)
                term = f_out.float().square().mean()
                loss = term if loss is None else loss + term
        loss.backward()

    return step, sites, net
