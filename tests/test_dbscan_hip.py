"""GPU (-m gpu): stratified_transformer_amd.cluster.dbscan / instances on csrc/dbscan.hip against the brute-force fp32 oracle of
tests/dbscan_oracle.py evaluated on the CPU: labels, core and n_clusters bit-identical in every case (integer results of a fixed fp32
arithmetic: there is no tolerance).  The golden clouds additionally pin the device to scikit-learn's recorded labels directly."""
import os

import numpy as np
import pytest
import torch

from tests import dbscan_oracle as O
from tests.util import dev

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"


@pytest.fixture(scope="module")
def C():
    from stratified_transformer_amd import cluster
    return cluster


@pytest.fixture(scope="module")
def sk():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "dbscan_sklearn.npz"), allow_pickle=False))


def _run(C, xyz, eps, min_samples, group=None):
    out = C.dbscan(dev(np.asarray(xyz, np.float32)), eps, min_samples, None if group is None else dev(np.asarray(group)))
    torch.cuda.synchronize()
    labels, core, n_clusters = out
    assert labels.dtype == torch.int32 and core.dtype == torch.bool and n_clusters.dtype == torch.int32
    return labels.cpu().numpy(), core.cpu().numpy(), n_clusters.cpu().numpy()


def _check(C, xyz, eps, min_samples, group=None, n_groups=None, what=""):
    """device against oracle, bit for bit; returns the oracle's result"""
    got = _run(C, xyz, eps, min_samples, group)
    want = O.dbscan(xyz, eps, min_samples, group, n_groups)
    print(f"{what}: n {len(xyz)}, clusters {want[2].tolist()}, core {int(want[1].sum())}, border {int(((want[0] >= 0) & ~want[1]).sum())}, "
          f"noise {int((want[0] < 0).sum())}, rounds {C.LAST['rounds']}, launches {C.LAST['launches']}")
    for name, g, w in zip(("labels", "core", "n_clusters"), got, want):
        assert g.shape == w.shape and np.array_equal(g, w), f"{what}: {name} differs at {np.nonzero(g != w)[0][:10].tolist()}"
    return want


def _blobs(n, seed, n_blobs=6, sigma=0.06, extent=2.0):
    rng = np.random.default_rng(seed)
    centres = rng.uniform(0.3, extent - 0.3, (n_blobs, 3))
    pts = centres[rng.integers(0, n_blobs, n)] + rng.normal(0, sigma, (n, 3))
    noise = rng.random(n) < 0.1
    pts[noise] = rng.uniform(0, extent, (int(noise.sum()), 3))
    return pts.astype(np.float32)


@pytest.mark.parametrize("k", range(5))
def test_golden_clouds_equal_the_oracle_and_scikit_learn(C, sk, k):
    xyz, eps, ms = sk[f"xyz_{k}"], float(sk[f"eps_{k}"]), int(sk[f"min_samples_{k}"])
    labels, core, n_clusters = _check(C, xyz, eps, ms, what=f"golden {k}")
    got = _run(C, xyz, eps, ms)
    assert np.array_equal(got[0], sk[f"labels_{k}"])                       # scikit-learn's labels_, directly
    assert np.array_equal(np.nonzero(got[1])[0], sk[f"core_{k}"])          # core_sample_indices_
    assert got[2].tolist() == [int(sk[f"labels_{k}"].max()) + 1]


def test_chain_of_4096_points_settles_in_few_rounds(C):
    """a line at spacing 0.9 * eps, min_samples 2, shuffled: one cluster.  Neighbour-to-neighbour propagation would need thousands of
    rounds; hooking + pointer jumping at least halves the trees per round, so it stays far below the cap."""
    eps, n = 0.1, 4096
    rng = np.random.default_rng(5)
    xyz = np.zeros((n, 3), np.float32)
    xyz[:, 0] = (np.arange(n) * (0.9 * eps)).astype(np.float32)
    xyz = xyz[rng.permutation(n)]
    labels, core, n_clusters = _check(C, xyz, eps, 2, what="chain")
    assert n_clusters.tolist() == [1] and core.all() and (labels == 0).all()
    print("chain rounds:", C.LAST["rounds"])
    assert C.LAST["rounds"] < C.MAX_ROUNDS


@pytest.mark.parametrize("min_samples", [7, 1])
def test_lattice_at_spacing_exactly_eps(C, min_samples):
    """spacing 0.25 = eps: d2 == eps * eps exactly in fp32, the inclusive comparison decides.  7: interior points are core (six lattice
    neighbours and themselves), points on the faces are not; 1: every point is core"""
    g = np.stack(np.meshgrid(np.arange(6), np.arange(5), np.arange(4), indexing="ij"), -1).reshape(-1, 3)
    xyz = (g * 0.25).astype(np.float32)[np.random.default_rng(1).permutation(len(g))]
    labels, core, n_clusters = _check(C, xyz, 0.25, min_samples, what=f"lattice {min_samples}")
    inner = np.all((xyz > 0) & (xyz < np.array([1.25, 1.0, 0.75], np.float32)), 1)
    assert np.array_equal(core, inner if min_samples == 7 else np.ones(len(g), bool)) and n_clusters.tolist() == [1]
    assert inner.sum() == 4 * 3 * 2


def test_all_points_duplicates_of_one(C):
    labels, core, n_clusters = _check(C, np.full((300, 3), 1.37, np.float32), 0.1, 5, what="duplicates")
    assert core.all() and (labels == 0).all() and n_clusters.tolist() == [1]


def test_all_noise(C):
    rng = np.random.default_rng(2)
    xyz = (np.stack(np.meshgrid(np.arange(6), np.arange(6), np.arange(6), indexing="ij"), -1).reshape(-1, 3) + rng.uniform(0, 0.3, (216, 3))).astype(np.float32)
    labels, core, n_clusters = _check(C, xyz, 0.1, 2, what="noise")
    assert (labels == -1).all() and not core.any() and n_clusters.tolist() == [0]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_wave_and_block_edges(C, n):
    xyz = _blobs(n, n, n_blobs=3)
    _check(C, xyz, 0.15, 3, what=f"n {n}")
    labels, core, _ = _check(C, xyz, 0.15, 1, what=f"n {n}, min_samples 1")
    assert core.all() and (labels >= 0).all()


def test_more_than_1024_cells_and_a_single_cell(C):
    xyz = _blobs(2000, 3, n_blobs=12, sigma=0.05, extent=4.0)
    assert np.prod(np.floor(np.ptp(xyz, 0) / (0.1 * C.CELL_MARGIN)) + 1) > 1024
    _, _, n_clusters = _check(C, xyz, 0.1, 5, what="many cells")
    assert n_clusters[0] >= 5
    one = np.random.default_rng(4).uniform(1.0, 1.09, (40, 3)).astype(np.float32)
    assert np.all(np.floor(np.ptp(one, 0) / (0.1 * C.CELL_MARGIN)) == 0)
    _, core, _ = _check(C, one, 0.1, 39, what="one cell")
    assert core.any() and not core.all()


def test_two_groups_at_identical_positions_do_not_link(C):
    xyz = _blobs(400, 6)
    both, group = np.concatenate([xyz, xyz]), np.repeat([0, 1], 400)
    labels, core, n_clusters = _check(C, both, 0.15, 4, group, what="two groups")
    alone = O.dbscan(xyz, 0.15, 4)
    assert np.array_equal(labels[:400], alone[0]) and np.array_equal(labels[400:], alone[0]) and n_clusters.tolist() == [int(alone[2][0])] * 2
    # one group of all 800 points is another result: every neighbour count doubles
    assert not np.array_equal(O.dbscan(both, 0.15, 4)[1], core)


def test_group_minus_one_is_left_out(C):
    xyz = _blobs(500, 7)
    group = np.random.default_rng(8).integers(-1, 2, 500)
    labels, core, _ = _check(C, xyz, 0.15, 3, group, n_groups=2, what="group -1")
    assert (group == -1).sum() > 100 and (labels[group == -1] == -1).all() and not core[group == -1].any()
    labels, core, n_clusters = _check(C, xyz, [0.15, 0.15, 0.15], 3, np.full(500, -1), n_groups=3, what="only group -1")
    assert (labels == -1).all() and n_clusters.tolist() == [0, 0, 0]


@pytest.mark.parametrize("int_type", [np.int32, np.int64])
def test_settings_per_group_the_larger_eps_sets_the_grid(C, int_type):
    xyz = _blobs(900, 9, sigma=0.08)
    group = np.random.default_rng(10).integers(0, 3, 900).astype(int_type)
    eps, ms = [0.1, 0.3, 0.15], [5, 3, 4]
    labels, _, n_clusters = _check(C, xyz, eps, ms, group, what="per-group settings")
    for g in range(3):                                                      # every group is the single-group problem with its own settings
        alone = O.dbscan(xyz[group == g], eps[g], ms[g])
        assert np.array_equal(labels[group == g], alone[0]) and n_clusters[g] == alone[2][0]
    got = _run(C, xyz, torch.tensor(eps), torch.tensor(ms), group)          # tensors of length G
    assert np.array_equal(got[0], labels)


def test_border_point_between_two_clusters_takes_the_smaller_number(C):
    eps = 0.25
    a = [[0.0, 0, 0], [0.05, 0, 0], [0.1, 0, 0], [0.15, 0, 0]]
    b = [[0.63, 0, 0], [0.68, 0, 0], [0.73, 0, 0], [0.78, 0, 0]]
    xyz = np.array(b + a + [[0.39, 0, 0], [3.0, 3, 3]], np.float32)         # within eps of one core point of each cluster, not core itself
    labels, core, n_clusters = _check(C, xyz, eps, 4, what="border")
    assert labels.tolist() == [0] * 4 + [1] * 4 + [0, -1] and core.tolist() == [True] * 8 + [False] * 2 and n_clusters.tolist() == [2]
    labels, _, _ = _check(C, xyz[[4, 5, 6, 7, 0, 1, 2, 3, 8, 9]], eps, 4, what="border, other order")
    assert labels.tolist() == [0] * 4 + [1] * 4 + [0, -1]


def test_same_input_twice_gives_identical_output(C):
    xyz, group = dev(_blobs(3000, 12, n_blobs=10)), dev(np.random.default_rng(13).integers(0, 2, 3000))
    a = C.dbscan(xyz, 0.12, 4, group)
    b = C.dbscan(xyz, 0.12, 4, group)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and int(a[2].sum()) > 4


def test_rejects_groups_out_of_range_and_non_finite_coordinates(C):
    xyz = dev(_blobs(50, 14))
    with pytest.raises(ValueError, match="group"):
        C.dbscan(xyz, [0.1, 0.1], 3, dev(np.full(50, 2)))
    with pytest.raises(ValueError, match="group"):
        C.dbscan(xyz, 0.1, 3, dev(np.full(50, -2)))
    bad = xyz.clone()
    bad[7, 1] = float("nan")
    with pytest.raises(ValueError, match="finite"):
        C.dbscan(bad, 0.1, 3)


def test_instances_golden_case(C, sk):
    inst, cls, size = C.instances(dev(sk["inst_coord"]), dev(sk["inst_shift"]), dev(sk["inst_pred"]))     # the reference's settings are the defaults
    torch.cuda.synchronize()
    assert inst.dtype == cls.dtype == size.dtype == torch.int32
    assert np.array_equal(inst.cpu().numpy(), sk["inst_instance"])
    assert np.array_equal(cls.cpu().numpy(), sk["inst_class"]) and np.array_equal(size.cpu().numpy(), sk["inst_size"])
    again = C.instances(dev(sk["inst_coord"]), dev(sk["inst_shift"]), dev(sk["inst_pred"].astype(np.int64)), sk["inst_eps"], sk["inst_min_samples"],
                        sk["inst_min_points"])
    assert all(torch.equal(x, y) for x, y in zip(again, (inst, cls, size)))


def test_instances_with_random_shifts_equal_the_oracle(C):
    rng = np.random.default_rng(15)
    coord = _blobs(1500, 16, n_blobs=9, sigma=0.07, extent=3.0)
    shift = rng.normal(0, 0.02, coord.shape).astype(np.float32)
    pred = rng.integers(-1, 8, 1500)
    pred[pred == 2] = 3                                                     # an empty class
    eps, ms, mp = [0.2] * 6 + [0.25] * 2, [5] * 6 + [3] * 2, [12] * 6 + [6] * 2
    want = O.instances(coord, shift, np.where(pred < 0, 99, pred), eps, ms, mp)   # (the oracle leaves out any class it has no settings for)
    got = C.instances(dev(coord), dev(shift), dev(pred), eps, ms, mp)
    torch.cuda.synchronize()
    print("instances:", want[1].tolist(), want[2].tolist())
    assert len(want[1]) >= 4 and (want[0] < 0).sum() > 150
    for g, w in zip(got, want):
        assert np.array_equal(g.cpu().numpy(), w)
    none = C.instances(dev(coord), dev(shift), dev(pred), eps, ms, 10 ** 6)
    assert (none[0] == -1).all() and none[1].numel() == 0 and none[2].numel() == 0
