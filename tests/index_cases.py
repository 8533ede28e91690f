"""Clouds for the index build (csrc/index.hip, index_build.py) and the data-side voxel keys (csrc/dataprep.hip): lattices, clouds away
from the origin and degenerate extents - the inputs on which the different ways of taking a floor disagree.  numpy / torch CPU only;
tests/test_index_cases_cpu.py proves the cases are what they claim, tests/test_index_cases_hip.py runs them on the device.

On a cloud with continuous noise (scene.make_room) no coordinate lands on a window face, and `x // w`, `floor(x / w)`,
`floor(x * (1 / w))` and `trunc(x / w)` agree at every point.  On a lattice they do not: the reference's partition (grid_cluster: fp32
divide, truncating cast) and its stratified mask (the fmod-based `//`) can put one point into two different windows, a point is then
a dense AND a stratified key of the same query, and the pair list holds that pair twice.  That is the reference's behaviour; the
oracle (oracle/index_ref.py) reproduces it and `census()` counts it - from the oracle alone, never from code under test.

`python -m tests.index_cases` prints the census as the table of DESIGN.md.
"""
import functools
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "name xyz offset w quant")   # xyz float32 [n, 3], offset int32 [b] (cumulative), window and quantisation size

CELL = 0.04            # the lattice step: the loaders' voxel size
W, QUANT = 0.16, 0.01  # stage 0 of the S3DIS configuration: windows of four cells
FAR_ORIGIN = (-3.217, 12.5, 100.0)
DOWNSAMPLE_SEED = 3


@functools.lru_cache(maxsize=None)
def lattice_cells():
    """the occupied 0.04 m cells of a 2400-point room, one integer triple per cell, in a seeded random order"""
    from stratified_transformer_amd import scene
    room = scene.make_room(2400, 1)
    cells = np.unique(np.floor(room / CELL).astype(np.int64), axis=0)
    return cells[np.random.default_rng(0).permutation(len(cells))]


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _case(name, xyz, sizes, w=W, quant=QUANT):
    xyz = _f32(xyz)
    offset = np.cumsum(sizes).astype(np.int32)
    assert xyz.ndim == 2 and xyz.shape[1] == 3 and offset[-1] == len(xyz)
    return Case(name, xyz, offset, w, quant)


def lattice_origin():
    """cell centres k * 0.04, the cloud's minimum at (or next to) the origin: a quarter of the coordinates sit on a window face"""
    c = lattice_cells()
    return _case("lattice_origin", c * CELL, [len(c)])


def lattice_far_origin():
    """the same lattice in world coordinates: the sums k * 0.04 + origin are rounded to fp32, and the partition's truncated quotient
    and the mask's floor division stop agreeing on the faces"""
    c = lattice_cells()
    return _case("lattice_far_origin", c * CELL + np.array(FAR_ORIGIN), [len(c)])


def lattice_negative():
    """every coordinate below zero"""
    c = lattice_cells()
    return _case("lattice_negative", -(c * CELL) - 0.5, [len(c)])


def mm_rounded_far():
    """a room stored with three decimals (float64) away from the origin, then cast to fp32 - what an S3DIS text file holds"""
    from stratified_transformer_amd import scene
    room = scene.make_room(2400, 1)
    mm = np.round(room.astype(np.float64) + np.array([17.3, -4.2, 0.0]), 3)
    return _case("mm_rounded_far", mm, [len(mm)])


def flat_z():
    """the lattice with one constant z: the extent along z is 0, the voxel multiplier 1, and every window coordinate along z comes
    from the `div == 0` branch of the floor division"""
    xyz = _f32(lattice_cells() * CELL)
    xyz[:, 2] = np.float32(1.28)
    return _case("flat_z", xyz, [len(xyz)])


def batch_mixed_origins():
    """three batch elements: 800 lattice points moved by +5 m in x, one single point, 800 lattice points moved by -7.04 m in y (the
    bounding box and the window coordinate are the whole batch's, the partition is per element)"""
    c = lattice_cells()
    a = c[:800] * CELL + np.array([5.0, 0.0, 0.0])
    b = c[800:1600] * CELL - np.array([0.0, 7.04, 0.0])
    one = np.array([[0.16, 0.32, 0.64]])
    return _case("batch_mixed_origins", np.concatenate([_f32(a), _f32(one), _f32(b)]), [800, 1, 800])


def pow2_lattice():
    """the control: cells of 2^-5 m, windows of 2^-3 m, quantisation 2^-7 m - every product, difference and quotient is exact, so
    every way of taking the floor gives the same window"""
    c = lattice_cells()
    return _case("pow2_lattice", c * 0.03125, [len(c)], w=0.125, quant=0.0078125)


def extent_multiples(case):
    """per axis: (extent / 2w, extent / w) as the partition takes them - fp32 subtract, fp32 divide, truncating cast"""
    lo, hi = case.xyz.min(0), case.xyz.max(0)
    ext = (hi - lo).astype(np.float32)
    w = np.float32(case.w)
    return (ext / (np.float32(2) * w)).astype(np.int64), (ext / w).astype(np.int64)


EXTENT_BOXES = (2, 2, 1)   # windows of 2w (8 cells) per axis of extent_on_face: the lattice spans 22 x 18 x 11 cells


def extent_on_face():
    """a box of the lattice whose extent is 2 x 2 x 1 large windows (16 x 16 x 8 cells) exactly (the two corner cells are added
    where the room has no point there): the maximum point sits ON the last face, alone in the window that the
    `(end - start) / size + 1` multiplier of the voxel id exists for"""
    c = lattice_cells()
    lo = c.min(0)
    hi = lo + 8 * np.array(EXTENT_BOXES)
    box = c[((c >= lo) & (c <= hi)).all(1)]
    box = np.concatenate([box, lo[None], hi[None]])
    _, first = np.unique(box, axis=0, return_index=True)
    box = box[np.sort(first)]
    return _case("extent_on_face", box * CELL, [len(box)])


_BUILDERS = (lattice_origin, lattice_far_origin, lattice_negative, mm_rounded_far, flat_z, batch_mixed_origins, pow2_lattice, extent_on_face)
NAMES = tuple(f.__name__ for f in _BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name):
    return dict(zip(NAMES, _BUILDERS))[name]()


def downsample(c):
    """the stand-in for the stage's FPS subset: n // 4 + b seeded random points, ascending (denser than the model's n // 8, so that
    small clouds still have stratified keys in most windows)"""
    n, b = len(c.xyz), len(c.offset)
    return np.sort(np.random.default_rng(DOWNSAMPLE_SEED).permutation(n)[: n // 4 + b]).astype(np.int32)


def table_rows(c):
    """L of the Stratified tables, as the model computes it (stratified_transformer.py:131)"""
    return 2 * int((2 * c.w + 1e-4) // c.quant)


# ---- the oracle on a case (computed once, shared by every test; nobody writes into the results) ----------------------------------
PARTITIONS = ("small", "small_shift", "large", "large_shift")


@functools.lru_cache(maxsize=None)
def oracle_partitions(name):
    """the four grid_sample calls of a stage (:277,280,297,300): name -> (cluster [n], counts [nW], order [n]) int64 numpy"""
    import torch
    from oracle import index_ref
    c = case(name)
    x = torch.from_numpy(c.xyz)
    batch = index_ref.batch_from_offset(c.offset)
    ws = torch.tensor([c.w] * 3).type_as(x)
    mn = x.min(0)[0]
    args = dict(small=(x, ws, None), small_shift=(x + 1 / 2 * ws, ws, mn), large=(x, 2 * ws, None), large_shift=(x + 1 / 2 * (2 * ws), 2 * ws, mn))
    out = {}
    for part, (pos, size, start) in args.items():
        cluster, p2v, counts = index_ref.grid_sample(pos, batch, size, start)
        p2v, counts = p2v.numpy(), counts.numpy()
        out[part] = (cluster.numpy(), counts, np.concatenate([p2v[w, :k] for w, k in enumerate(counts)]))
    return out


@functools.lru_cache(maxsize=None)
def oracle_block(name, parity):
    """index_ref.build_stage_indices(div_mode="cuda") of one block pattern: index_0, index_1, offsets, rel_idx (raw), n_max"""
    import torch
    from oracle import index_ref
    c = case(name)
    want = index_ref.build_stage_indices(torch.from_numpy(c.xyz), c.offset, c.w, c.quant, torch.from_numpy(downsample(c)), parity, div_mode="cuda")
    return {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in want.items()}


@functools.lru_cache(maxsize=None)
def oracle_swin_block(name, parity):
    import torch
    from oracle import index_ref
    c = case(name)
    want = index_ref.swin_stage_indices(torch.from_numpy(c.xyz), c.offset, c.w, c.quant, parity)
    return {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in want.items()}


def oracle_swin_quant(c, parity):
    """the per-point quantised in-window coordinate of swin3d_transformer.py:151-152, int32 [n, 3] (index_ref.swin_rel_pos_index
    subtracts two rows of it)"""
    import torch
    x = torch.from_numpy(c.xyz)
    shift = 1 / 2 * torch.tensor([c.w] * 3).type_as(x) if parity else 0.0
    return (((x - x.min(0)[0] + shift) % c.w) // c.quant).int().numpy()


def duplicated_pairs(index_0, index_1, n):
    """entries of a pair list that repeat an earlier (query, key)"""
    key = index_0.astype(np.int64) * n + index_1.astype(np.int64)
    return int(key.shape[0] - np.unique(key).shape[0])


@functools.lru_cache(maxsize=None)
def census(name):
    """What a case holds, per block parity (0 even, 1 odd), from oracle/index_ref.py alone:
       on_face       share of the coordinates (xyz [+ w/2] - min) / w that are whole numbers in fp32
       disagree      points whose window coordinate (`//`, the mask's) differs from that of the first point of their partition
                     window (truncated quotient, the partition's): the two roundings put them into different windows
       duplicates    (index_0, index_1) entries that repeat an earlier one
       rel_min, rel_max, rel_outside   range of the raw rel_idx and its entries outside [0, L)
    plus `L` and, per axis, the truncated extent quotients `extent_2w`, `extent_w`."""
    import torch
    from oracle import index_ref
    c = case(name)
    n, L = len(c.xyz), table_rows(c)
    x = torch.from_numpy(c.xyz)
    ws = torch.tensor([c.w] * 3).type_as(x)
    parts = oracle_partitions(name)
    e2, e1 = extent_multiples(c)
    out = dict(n=n, L=L, extent_2w=e2.tolist(), extent_w=e1.tolist())
    for par in (0, 1):
        blk = oracle_block(name, par)
        v = (x + 1 / 2 * ws - x.min(0)[0]) if par else (x - x.min(0)[0])
        on_face = float(((v / ws) == torch.floor(v / ws)).float().mean())
        wc = index_ref.window_coord(x, c.w, par == 1).numpy()
        cluster, _, order = parts["small_shift" if par else "small"]
        first = np.full(int(cluster.max()) + 1, -1, np.int64)
        first[cluster[order][::-1]] = order[::-1]          # the lowest point index of every window
        disagree = int((wc != wc[first[cluster]]).any(1).sum())
        rel = blk["rel_idx"]
        out[par] = dict(on_face=on_face, disagree=disagree, duplicates=duplicated_pairs(blk["index_0"], blk["index_1"], n), pairs=int(rel.shape[0]),
                        rel_min=int(rel.min()), rel_max=int(rel.max()), rel_outside=int(((rel < 0) | (rel >= L)).sum()))
    return out


# ---- the data side: util/voxelize.py on a lattice that does not start at the origin ------------------------------------------------
DATA_VOXEL, DATA_ORIGIN, DATA_STEPS = 0.04, 17.3, 400


def data_axis(dtype):
    """coord = k * 0.04 + 17.3 for k = 0 .. 399 in `dtype`, shifted to minimum 0 as the loaders do (data_util.py:186)"""
    c = (np.arange(DATA_STEPS) * DATA_VOXEL + DATA_ORIGIN).astype(dtype)
    return c - c.min()


def floors_below_nearest(coord, voxel=DATA_VOXEL):
    """values whose np.floor(coord / voxel) - the voxel the reference puts them into - is one below the nearest integer"""
    q = coord / np.asarray(voxel, dtype=coord.dtype)
    return int((np.floor(q) < np.rint(q)).sum())


def data_lattice(dtype, n=20000, seed=4):
    """about 20 000 points of the 3-D lattice of data_axis() (400 x 50 x 10 steps: many voxels hold several points), shifted to
    minimum 0; [n, 3] `dtype`"""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, (DATA_STEPS, 50, 10), (n, 3))
    k[:3] = [[0, 0, 0], [DATA_STEPS - 1, 49, 9], [0, 0, 0]]
    c = (k * DATA_VOXEL + DATA_ORIGIN).astype(dtype)
    return np.ascontiguousarray(c - c.min(0))


def census_table():
    rows = ["| cloud | n | on a face (even / odd) | partition window != window coordinate | duplicated pairs | rel_idx range (even) | outside [0, L) (even / odd) |",
            "|---|---|---|---|---|---|---|"]
    for name in NAMES:
        s = census(name)
        e, o = s[0], s[1]
        rows.append(f"| `{name}` | {s['n']} | {100 * e['on_face']:.1f} % / {100 * o['on_face']:.1f} % | {e['disagree']} / {o['disagree']} | "
                    f"{e['duplicates']} / {o['duplicates']} | [{e['rel_min']}, {e['rel_max']}], L = {s['L']} | {e['rel_outside']} / {o['rel_outside']} |")
    return "\n".join(rows)


if __name__ == "__main__":
    print(census_table())
    for dt in (np.float32, np.float64):
        print(np.dtype(dt).name, "floors below the nearest integer:", floors_below_nearest(data_axis(dt)), "of", DATA_STEPS)
