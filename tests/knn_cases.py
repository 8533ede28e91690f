"""Clouds for the exact kNN (csrc/knn.hip, csrc/knn_grid.hip): one case per kernel path, k boundary and degenerate geometry.
numpy only; the CPU file tests/test_knn_cases_cpu.py proves the cases are what they claim, tests/test_knn_hip.py runs them.

The launcher picks the kernel from k and m*n alone (knnquery_cuda_launcher, knn_grid_launch; the tests always lend a workspace):

    m*n <  2^22                      knn_kernel            the literal heap scan, 64 queries per workgroup, 2048-point tiles
    m*n >= 2^22, k + 1 <= 16         knn_lanes_kernel<16>
                 k + 1 <= 32         knn_lanes_kernel<32>
                 k + 1 <= 64         knn_lanes_kernel<64>
                 k + 1 >  64         knn_grid_kernel       one thread per query, the list in LDS, (k+1)*64*8 bytes
    and, after either grid kernel,   knn_replay_kernel     the heap scan again for the queries with a tie among their k+1 best

Every grid case has n = 4096 candidates and m = 1024 queries (m*n == 2^22, the smallest the grid takes) or a few more.

KERNELS: case family -> {k: kernel}.  `replay` names the families whose queries reach knn_replay_kernel (exact ties).
"""
from collections import namedtuple

import numpy as np

SCAN, LANES16, LANES32, LANES64, GRID, REPLAY = ("knn_kernel", "knn_lanes_kernel<16>", "knn_lanes_kernel<32>", "knn_lanes_kernel<64>",
                                                 "knn_grid_kernel", "knn_replay_kernel")
GRID_THRESHOLD = 1 << 22

_SWEEP = {1: LANES16, 15: LANES16,      # k + 1 == 16: the group's last lane is the (k+1)-th best
          16: LANES32, 31: LANES32,     # the k just after, and k + 1 == 32
          32: LANES64, 63: LANES64,     # the k just after, and k + 1 == 64
          64: GRID, 65: GRID, 100: GRID}
KERNELS = {
    "sweep_random": _SWEEP,                                         # no exact ties: nothing is replayed
    "sweep_mixed": _SWEEP,                                          # + knn_replay_kernel for the lattice half of the queries
    "threshold_below": {16: SCAN},                                  # n = 4095: m*n = 2^22 - 1024
    "threshold_at": {16: LANES32},                                  # n = 4096, the same cloud
    "scan_random": {3: SCAN, 16: SCAN, 64: SCAN, 100: SCAN},        # a workgroup over three batch elements, tiles cut inside elements
    "scan_lattice": {3: SCAN, 16: SCAN, 64: SCAN, 100: SCAN},       # the same with ties (the scan is its own replay)
    "short_km1": {15: LANES16, 16: LANES32, 63: LANES64, 64: GRID},  # first batch element of k - 1 points
    "short_k": {15: LANES16, 16: LANES32, 63: LANES64, 64: GRID},    # ... of k points: the (k+1)-th best stays the filler
    "short_kp1": {15: LANES16, 16: LANES32, 63: LANES64, 64: GRID},  # ... of k + 1 points
    "planar": {16: LANES32, 64: GRID},
    "collinear": {16: LANES32, 64: GRID},
    "coincident": {16: LANES32, 64: GRID},                          # + knn_replay_kernel for every query
    "far_apart": {16: LANES32, 64: GRID},
    "boundary_tie": {15: LANES16, 31: LANES32, 63: LANES64, 64: GRID},   # + knn_replay_kernel: the one tie sits in the last slot
    "translate_0": {16: LANES32, 64: GRID},                         # + knn_replay_kernel: distances are multiples of 2^-16
    "translate_64": {16: LANES32, 64: GRID},
    "translate_1024": {16: LANES32, 64: GRID},
    "translate_16384": {16: LANES32, 64: GRID},
}
REPLAY_FAMILIES = ("sweep_mixed", "coincident", "boundary_tie", "translate_0", "translate_64", "translate_1024", "translate_16384")
TRANSLATIONS = (0, 64, 1024, 16384)

# name: "<family>-k<k>" or "<family>-k<k>-b2" (two batch elements); lattice_queries: the queries that sit on the lattice (or None)
Case = namedtuple("Case", "name family k xyz new_xyz offset new_offset lattice_queries")


def _case(family, k, xyz, new_xyz, offset, new_offset, lattice_queries=None, suffix=""):
    xyz, new_xyz = np.ascontiguousarray(xyz, np.float32), np.ascontiguousarray(new_xyz, np.float32)
    offset, new_offset = np.asarray(offset, np.int32), np.asarray(new_offset, np.int32)
    assert offset[-1] == len(xyz) and new_offset[-1] == len(new_xyz) and len(offset) == len(new_offset)
    return Case(f"{family}-k{k}{suffix}", family, k, xyz, new_xyz, offset, new_offset, lattice_queries)


def _block(nx, ny, nz, origin=(0, 0, 0)):
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1).reshape(-1, 3)
    return (g + np.asarray(origin)).astype(np.float32)


def _half_lattice_queries(rng, count, dims, origin=(0, 0, 0)):
    """points of the half-step lattice inside the block that are NOT block points (at least one coordinate ends in .5): their
    nearest block points come in 2, 4 or 8 at the same distance, so the two best already tie"""
    out = []
    while len(out) < count:
        p = rng.integers(0, 2 * (np.asarray(dims) - 1) + 1, 3)
        if (p % 2).any():
            out.append(p * 0.5 + np.asarray(origin))
    return np.asarray(out, np.float32)


# ---- k sweep on the grid path ------------------------------------------------------------------------------------------------
SWEEP_KS = (1, 15, 16, 31, 32, 63, 64, 65, 100)
SWEEP_SEED = 24   # a draw without a single exact tie among any query's 101 best (tests/test_knn_cases_cpu.py holds it to that)


def sweep_random(k, batched):
    """uniform cloud: no two of a query's k + 1 best distances are equal (checked on the CPU), so nothing is replayed"""
    rng = np.random.default_rng(SWEEP_SEED)
    xyz = rng.random((4096, 3), dtype=np.float32)
    new_xyz = np.concatenate([xyz[rng.permutation(4096)[:512]], rng.random((512, 3), dtype=np.float32)])
    new_xyz = new_xyz[rng.permutation(1024)]
    if batched:
        return _case("sweep_random", k, xyz, new_xyz, [1500, 4096], [400, 1024], suffix="-b2")
    return _case("sweep_random", k, xyz, new_xyz, [4096], [1024])


def sweep_mixed(k, batched):
    """an integer lattice in random index order; half of each element's queries sit on the (half-step) lattice and tie, half are
    uniform draws and do not.  One element: 16^3.  Two elements: 10x10x15 = 1500 and 13x14x14 + a 4x4x3 block far away = 2596.
    A block point's two best are (0, 1): at k = 1 only half-step points tie, so all lattice queries are half-step points there."""
    rng = np.random.default_rng(100 + k)
    if batched:
        blocks = [((10, 10, 15), _block(10, 10, 15)), ((13, 14, 14), np.concatenate([_block(13, 14, 14), _block(4, 4, 3, (53, 0, 0))]))]
        counts = [400, 624]
    else:
        blocks, counts = [((16, 16, 16), _block(16, 16, 16))], [1024]
    xyz, new_xyz, on = [], [], []
    for (dims, pts), m in zip(blocks, counts):
        main = dims[0] * dims[1] * dims[2]
        n_cloud = 0 if k == 1 else m // 4
        q_cloud = pts[rng.permutation(main)[:n_cloud]]
        q_half = _half_lattice_queries(rng, m // 2 - n_cloud, dims)
        q_off = (rng.random((m - m // 2, 3)) * (np.asarray(dims) - 1)).astype(np.float32)
        order = rng.permutation(m)
        new_xyz.append(np.concatenate([q_cloud, q_half, q_off])[order])
        on.append((np.arange(m) < m // 2)[order])
        xyz.append(pts[rng.permutation(len(pts))])
    offset, new_offset = np.cumsum([len(x) for x in xyz]), np.cumsum(counts)
    return _case("sweep_mixed", k, np.concatenate(xyz), np.concatenate(new_xyz), offset, new_offset, np.concatenate(on),
                 suffix="-b2" if batched else "")


# ---- the dispatch line ------------------------------------------------------------------------------------------------------------
def threshold(n):
    """k = 16, m = 1024 and the first n of the same 4096 points: n = 4095 is scanned, n = 4096 goes to the grid"""
    rng = np.random.default_rng(12)
    xyz = rng.random((4096, 3), dtype=np.float32)
    new_xyz = np.concatenate([xyz[:512], rng.random((512, 3), dtype=np.float32)])
    return _case("threshold_below" if n == 4095 else "threshold_at", 16, xyz[:n], new_xyz, [n], [1024])


# ---- full scan, several batch elements per workgroup ------------------------------------------------------------------------------
SCAN_KS = (3, 16, 64, 100)
SCAN_OFFSET, SCAN_NEW_OFFSET = (30, 2300, 5000), (10, 50, 800)   # m*n = 4.0e6 < 2^22


def scan_random(k):
    """the first workgroup's 64 queries cover elements 0, 1 and 2, so its tiles start at point 0: for that workgroup element 1
    [30, 2300) is cut by the tile boundary 2048 and element 2 [2300, 5000) by 4096 (the later workgroups serve element 2 alone and
    start their tiles at 2300); element 0 has fewer points than k = 64 / 100"""
    rng = np.random.default_rng(13)
    xyz = rng.random((5000, 3), dtype=np.float32)
    new_xyz, lo, qlo = [], 0, 0
    for hi, qhi in zip(SCAN_OFFSET, SCAN_NEW_OFFSET):
        m = qhi - qlo
        new_xyz.append(np.concatenate([xyz[lo + rng.permutation(hi - lo)[:m // 2]], rng.random((m - m // 2, 3), dtype=np.float32)]))
        lo, qlo = hi, qhi
    return _case("scan_random", k, xyz, np.concatenate(new_xyz), SCAN_OFFSET, SCAN_NEW_OFFSET)


def scan_lattice(k):
    """the same layout with every element a lattice in random index order (2x3x5; 10x15x15 + a 2x2x5 block far away; 10x15x18);
    every query is a point of its element's main block"""
    rng = np.random.default_rng(14)
    blocks = [(30, _block(2, 3, 5)), (2250, np.concatenate([_block(10, 15, 15), _block(2, 2, 5, (40, 0, 0))])), (2700, _block(10, 15, 18))]
    xyz, new_xyz, qlo = [], [], 0
    for (main, pts), qhi in zip(blocks, SCAN_NEW_OFFSET):
        new_xyz.append(pts[rng.permutation(main)[:qhi - qlo]])
        xyz.append(pts[rng.permutation(len(pts))])
        qlo = qhi
    new_xyz = np.concatenate(new_xyz)
    return _case("scan_lattice", k, np.concatenate(xyz), new_xyz, SCAN_OFFSET, SCAN_NEW_OFFSET, np.ones(len(new_xyz), bool))


# ---- short batch elements on the grid path --------------------------------------------------------------------------------------
SHORT_KS = (15, 16, 63, 64)


def short_element(k, delta):
    """first element: k + delta points (delta -1, 0, +1), all of them queries; second: 4096 uniform points, 1024 queries.  With k
    points or fewer the (k+1)-th best stays the filler (1e10, first index of the element) and the shell walk covers the whole grid."""
    rng = np.random.default_rng(15)
    s = k + delta
    xyz = np.concatenate([rng.random((s, 3), dtype=np.float32), rng.random((4096, 3), dtype=np.float32)])
    new_xyz = np.concatenate([xyz[:s], xyz[s + rng.permutation(4096)[:512]], rng.random((512, 3), dtype=np.float32)])
    return _case({-1: "short_km1", 0: "short_k", 1: "short_kp1"}[delta], k, xyz, new_xyz, [s, s + 4096], [s, s + 1024])


# ---- degenerate geometry on the grid path -------------------------------------------------------------------------------------------
DEGENERATE_KS = (16, 64)


def planar(k):
    """z constant: the plan clamps the zero extent to 1e-6, the cell edge comes out tiny and the cell-cap loop has to grow it"""
    rng = np.random.default_rng(16)
    xyz = rng.random((4096, 3), dtype=np.float32)
    xyz[:, 2] = np.float32(0.375)
    new_xyz = np.concatenate([xyz[:512], rng.random((512, 3), dtype=np.float32)])
    new_xyz[:, 2] = np.float32(0.375)
    return _case("planar", k, xyz, new_xyz, [4096], [1024])


def collinear(k):
    """all points on a line parallel to x (two zero extents): a grid of one row of cells"""
    rng = np.random.default_rng(17)
    xyz = np.zeros((4096, 3), np.float32)
    xyz[:, 0] = rng.random(4096, dtype=np.float32)
    xyz[:, 1], xyz[:, 2] = np.float32(0.25), np.float32(-0.5)
    new_xyz = xyz[rng.permutation(4096)[:1024]].copy()
    new_xyz[512:, 0] = rng.random(512, dtype=np.float32)
    return _case("collinear", k, xyz, new_xyz, [4096], [1024])


def coincident(k):
    """4096 copies of one point (all extents clamped, one or two cells per axis); half the queries are that point, half are
    elsewhere: every distance of a query is the same, every query is replayed"""
    rng = np.random.default_rng(18)
    p = np.array([0.3, -1.2, 2.5], np.float32)
    xyz = np.tile(p, (4096, 1))
    new_xyz = np.concatenate([np.tile(p, (512, 1)), p + rng.random((512, 3), dtype=np.float32)])
    return _case("coincident", k, xyz, new_xyz, [4096], [1024], np.ones(1024, bool))


def far_apart(k):
    """two elements whose boxes are 1000 units apart on x: the shared grid is one long row, each element in one end of it"""
    rng = np.random.default_rng(19)
    xyz = rng.random((4096, 3), dtype=np.float32)
    xyz[2048:, 0] += np.float32(1000.0)
    new_xyz = np.concatenate([xyz[:256], rng.random((256, 3), dtype=np.float32), xyz[2048:2304],
                              rng.random((256, 3), dtype=np.float32) + np.array([1000.0, 0, 0], np.float32)])
    return _case("far_apart", k, xyz, new_xyz, [2048, 4096], [512, 1024])


# ---- a tie in the last slot only ------------------------------------------------------------------------------------------------
BOUNDARY_KS = (15, 31, 63, 64)   # k + 1 == LQ for each lane width, and the first k of knn_grid_kernel


def _sq_dist(q, pts):
    d = q[:, None, :] - pts[None, :, :]
    return (d * d).sum(-1)


def boundary_tie(k):
    """queries whose ONLY exact tie is between their k-th and (k+1)-th best: the kernels see it only by comparing slot k - 1 with
    slot k (the last lane of a full lane group, `ld[k-1] == ld[k]` in knn_grid_kernel), and a kernel that misses it writes the
    lower index where the heap may have kept the higher.  Coordinates are multiples of 2^-12; the first 512 queries each get a
    mirror point b = 2q - a of their k-th nearest point a: q - b == -(q - a) exactly, so both distances have the same bits.  Two
    rounds re-pick a after the other queries' mirrors have moved in.  tests/test_knn_cases_cpu.py counts what the draw yields."""
    rng = np.random.default_rng(40 + k)
    n_tie = 512
    base = rng.integers(0, 4096, (4096 - n_tie, 3)).astype(np.float64) / 4096.0
    q = rng.integers(0, 4096, (1024, 3)).astype(np.float64) / 4096.0
    tq = q[:n_tie]
    mirrors = 2 * tq - base[np.argpartition(_sq_dist(tq, base), k - 1, 1)[:, k - 1]]
    for _ in range(2):
        cloud = np.concatenate([base, mirrors])
        d = _sq_dist(tq, cloud)
        d[np.arange(n_tie), len(base) + np.arange(n_tie)] = np.inf   # without the query's own mirror
        mirrors = 2 * tq - cloud[np.argpartition(d, k - 1, 1)[:, k - 1]]
    xyz = np.concatenate([base, mirrors])[rng.permutation(4096)]
    return _case("boundary_tie", k, xyz, q, [4096], [1024])


# ---- translation ---------------------------------------------------------------------------------------------------------------------
def translated(k, T):
    """coordinates are multiples of 1/256 in [0, 4)^3, moved by T on every axis.  T + 4 <= 16388 < 2^15 with a spacing of 2^-8 needs
    23 bits: every translated coordinate is exact in fp32, every difference is the untranslated one, every d2 (a multiple of 2^-16
    below 48: 22 bits) is exact, so indices and distances must not depend on T.  The grid's face arithmetic does see T."""
    rng = np.random.default_rng(20)
    xyz = rng.integers(0, 1024, (4096, 3)).astype(np.float32) / np.float32(256)
    new_xyz = np.concatenate([xyz[rng.permutation(4096)[:512]], rng.integers(0, 1024, (512, 3)).astype(np.float32) / np.float32(256)])
    return _case(f"translate_{T}", k, xyz + np.float32(T), new_xyz + np.float32(T), [4096], [1024])


def _build_all():
    cases = []
    for k in SWEEP_KS:
        for batched in (False, True):
            cases += [sweep_random(k, batched), sweep_mixed(k, batched)]
    cases += [threshold(4095), threshold(4096)]
    for k in SCAN_KS:
        cases += [scan_random(k), scan_lattice(k)]
    for k in SHORT_KS:
        cases += [short_element(k, d) for d in (-1, 0, 1)]
    for k in DEGENERATE_KS:
        cases += [planar(k), collinear(k), coincident(k), far_apart(k)]
        cases += [translated(k, T) for T in TRANSLATIONS]
    cases += [boundary_tie(k) for k in BOUNDARY_KS]
    out = {c.name: c for c in cases}
    assert len(out) == len(cases)
    return out


CASES = _build_all()


def kernel_of(case):
    return KERNELS[case.family][case.k]
