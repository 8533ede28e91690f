"""GPU (-m gpu): stratified_transformer_amd.cluster.contacts / objects on csrc/contacts.hip against the brute-force fp32 oracle of
tests/contacts_oracle.py evaluated on the CPU: count equal entry for entry, min_d2 equal bit for bit including +inf (integer counts and
minima of a fixed fp32 arithmetic: there is no tolerance).  The golden scenes pin instances() -> objects() to the objects that the
reference's own instantiation_eval recorded (tests/golden/objects_reference.npz)."""
import os

import numpy as np
import pytest
import torch

from tests import contacts_oracle as O
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
def gold():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "objects_reference.npz"), allow_pickle=False))


def _run(C, xyz, label, radius, n_labels=None):
    count, min_d2 = C.contacts(dev(np.asarray(xyz, np.float32)), dev(np.asarray(label)), radius, n_labels)
    torch.cuda.synchronize()
    assert count.dtype == torch.int32 and min_d2.dtype == torch.float32
    return count.cpu().numpy(), min_d2.cpu().numpy()


def _check(C, xyz, label, radius, n_labels=None, what=""):
    """device against oracle, bit for bit; returns the oracle's tables"""
    got = _run(C, xyz, label, radius, n_labels)
    want = O.contacts(xyz, label, radius, n_labels)
    off = want[0][~np.eye(len(want[0]), dtype=bool)]
    print(f"{what}: n {len(xyz)}, labels {len(want[0])}, pairs in contact {int((off > 0).sum())}, finite min_d2 {int(np.isfinite(want[1]).sum())}, "
          f"launches {C.LAST_CONTACTS['launches']}, read-backs {C.LAST_CONTACTS['readbacks']}")
    assert got[0].shape == want[0].shape and np.array_equal(got[0], want[0]), f"{what}: count differs at {np.argwhere(got[0] != want[0])[:10].tolist()}"
    same = got[1].view(np.int32) == want[1].view(np.int32)               # the bit patterns: +inf included
    assert got[1].shape == want[1].shape and same.all(), f"{what}: min_d2 differs at {np.argwhere(~same)[:10].tolist()}"
    assert np.array_equal(got[1], got[1].T)                               # d2(p, q) == d2(q, p)
    return want


def _blobs(n, seed, n_blobs=6, sigma=0.06, extent=2.0):
    rng = np.random.default_rng(seed)
    centres = rng.uniform(0.3, extent - 0.3, (n_blobs, 3))
    which = rng.integers(0, n_blobs, n)
    pts = centres[which] + rng.normal(0, sigma, (n, 3))
    return pts.astype(np.float32), which


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_wave_and_block_edges(C, n):
    xyz, _ = _blobs(n, n, n_blobs=2, sigma=0.1, extent=1.0)
    label = np.random.default_rng(n).integers(0, 3, n)
    count, _ = _check(C, xyz, label, 0.15, 3, what=f"n {n}")
    assert np.array_equal(count.diagonal(), np.bincount(label, minlength=3))


@pytest.mark.parametrize("n_labels", [1, 31, 32, 33, 64, 65, 300])
def test_bitmap_word_edges_and_the_register_boundary(C, n_labels):
    xyz, _ = _blobs(2000, 7, n_blobs=5, sigma=0.08, extent=1.2)
    label = np.random.default_rng(n_labels).integers(0, n_labels, 2000)
    label[:n_labels] = np.arange(n_labels)                                # every label is there, the last one included
    count, _ = _check(C, xyz, label, 0.1, what=f"labels {n_labels}")
    assert count.shape == (n_labels, n_labels) and (count > 0).sum() > n_labels - (n_labels == 1)


def test_lattice_at_spacing_exactly_the_radius(C):
    """spacing 0.25 = radius: d2 == r2 exactly in fp32, so under the strict comparison no lattice neighbours touch; a radius one fp32 step
    up links every neighbour"""
    g = np.stack(np.meshgrid(np.arange(6), np.arange(5), np.arange(4), indexing="ij"), -1).reshape(-1, 3)
    order = np.random.default_rng(1).permutation(len(g))
    xyz, label = (g * 0.25).astype(np.float32)[order], (g.sum(1) % 2)[order]        # a 3-d checkerboard: every neighbour has the other label
    count, min_d2 = _check(C, xyz, label, 0.25, what="lattice, radius 0.25")
    sizes = np.bincount(label)
    assert np.array_equal(count, np.diag(sizes)) and min_d2[0, 1] == np.float32(0.0625)
    count, _ = _check(C, xyz, label, 0.2500001, what="lattice, radius 0.2500001")
    assert np.float32(0.2500001) > np.float32(0.25) and np.array_equal(count, np.array([[sizes[0], sizes[0]], [sizes[1], sizes[1]]]))


def test_all_points_identical(C):
    label = np.array([0] * 120 + [1] * 180)
    count, min_d2 = _check(C, np.full((300, 3), 1.37, np.float32), label, 0.1, what="duplicates")
    assert count.tolist() == [[120, 120], [180, 180]] and not min_d2.any()


def test_more_than_1024_cells_and_a_single_cell(C):
    xyz, label = _blobs(2000, 3, n_blobs=12, sigma=0.05, extent=4.0)
    assert np.prod(np.floor(np.ptp(xyz, 0) / (0.1 * C.CELL_MARGIN)) + 1) > 1024
    _check(C, xyz, label, 0.1, what="many cells")
    xyz = np.random.default_rng(4).uniform(0, 0.05, (500, 3)).astype(np.float32)
    assert np.all(np.floor(np.ptp(xyz, 0) / (0.1 * C.CELL_MARGIN)) == 0)
    count, _ = _check(C, xyz, np.arange(500) % 4, 0.1, what="one cell")
    assert (count == 125).all()


def test_unlabelled_points_never_count(C):
    xyz, which = _blobs(1200, 11, n_blobs=4, sigma=0.08, extent=1.0)
    label = which.copy()
    label[np.random.default_rng(0).random(1200) < 0.4] = -1
    want = _check(C, xyz, label, 0.1, 4, what="40 % unlabelled")
    keep = label >= 0
    got = _run(C, xyz[keep], label[keep], 0.1, 4)                          # the same tables as without those points
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    count, min_d2 = _run(C, xyz, np.full(1200, -1), 0.1, 4)                # nobody takes part
    assert not count.any() and np.isinf(min_d2).all()
    count, min_d2 = _run(C, xyz, np.full(1200, -1), 0.1)
    assert count.shape == (0, 0) and min_d2.shape == (0, 0)


def test_an_empty_label_in_the_middle_of_the_range(C):
    xyz, which = _blobs(900, 13, n_blobs=3, sigma=0.1, extent=1.0)
    label = np.array([0, 2, 4])[which]
    for n_labels in (5, 70):
        count, min_d2 = _check(C, xyz, label, 0.1, n_labels, what=f"empty labels, {n_labels}")
        for empty in (1, 3) + ((n_labels - 1,) if n_labels > 5 else ()):
            assert not count[empty].any() and not count[:, empty].any()
            assert np.isposinf(min_d2[empty]).all() and np.isposinf(min_d2[:, empty]).all()
        assert np.isfinite(min_d2[np.ix_([0, 2, 4], [0, 2, 4])]).all()


def test_count_is_not_symmetric(C):
    """one point of b beside forty of a"""
    rng = np.random.default_rng(17)
    xyz = np.concatenate([rng.uniform(0, 0.03, (40, 3)), [[0.05, 0.05, 0.05]]]).astype(np.float32)
    count, _ = _check(C, xyz, np.array([0] * 40 + [1]), 0.1, what="asymmetric")
    assert count.tolist() == [[40, 40], [1, 1]]


def test_int32_and_int64_labels(C):
    xyz, which = _blobs(700, 19, n_blobs=5, sigma=0.1, extent=1.0)
    a = C.contacts(dev(xyz), dev(which.astype(np.int32)), 0.1)
    b = C.contacts(dev(xyz), dev(which.astype(np.int64)), 0.1)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    want = O.contacts(xyz, which, 0.1)
    assert np.array_equal(a[0].cpu().numpy(), want[0]) and np.array_equal(a[1].cpu().numpy(), want[1])


@pytest.mark.parametrize("n_labels", [40, 100])
def test_the_same_input_twice_gives_identical_tensors(C, n_labels):
    xyz, _ = _blobs(5000, 23, n_blobs=8, sigma=0.1, extent=1.5)
    label = dev(np.random.default_rng(1).integers(-1, n_labels, 5000))
    first = C.contacts(dev(xyz), label, 0.08, n_labels)
    second = C.contacts(dev(xyz), label, 0.08, n_labels)
    assert torch.equal(first[0], second[0]) and torch.equal(first[1].view(torch.int32), second[1].view(torch.int32))


def test_rejections(C):
    from stratified_transformer_amd import _lib
    xyz, label = torch.zeros(10, 3, device="cuda"), torch.zeros(10, dtype=torch.int64, device="cuda")
    calls = _lib.CALLS[0]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        C.contacts(xyz.cpu(), label, 0.1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        C.contacts(xyz, label.cpu(), 0.1)
    with pytest.raises(TypeError, match="float32"):
        C.contacts(xyz.double(), label, 0.1)
    with pytest.raises(TypeError, match="int32"):
        C.contacts(xyz, label.float(), 0.1)
    with pytest.raises(ValueError, match=r"\[N, 3\]"):
        C.contacts(xyz[:, :2], label, 0.1)
    with pytest.raises(ValueError, match="label must be"):
        C.contacts(xyz, label[:9], 0.1)
    for radius in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="radius"):
            C.contacts(xyz, label, radius)
    with pytest.raises(ValueError, match="label values"):
        C.contacts(xyz, label + 3, 0.1, 3)                                 # a label beyond n_labels
    with pytest.raises(ValueError, match="label values"):
        C.contacts(xyz, label - 2, 0.1)                                    # below -1
    bad = xyz.clone()
    bad[3, 1] = float("nan")
    with pytest.raises(ValueError, match="finite"):
        C.contacts(bad, label, 0.1)
    bad[3, 1] = float("inf")
    with pytest.raises(ValueError, match="finite"):
        C.contacts(bad, label, 0.1)
    wide = xyz.clone()
    wide[0, 0] = 1e6
    with pytest.raises(ValueError, match="cells"):
        C.contacts(wide, label, 0.1)                                       # 1e7 cells along x
    big = torch.zeros(300000, 3, device="cuda")
    with pytest.raises(ValueError, match="bitmap"):
        C.contacts(big, torch.zeros(300000, dtype=torch.int32, device="cuda"), 0.1, 32768)   # 300000 * 1024 * 4 bytes > 1 GiB
    with pytest.raises(ValueError, match="labels"):
        C.contacts(xyz, label, 0.1, C.MAX_LABELS + 1)
    with pytest.raises(ValueError, match="instance_class"):
        C.objects(xyz, label, [0])
    with pytest.raises(ValueError, match="instance_size"):
        C.objects(xyz, label, torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(2, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError, match="share"):
        C.objects(xyz, label, torch.zeros(1, dtype=torch.int64, device="cuda"), share=float("nan"))
    assert _lib.CALLS[0] == calls                                          # all of them before any launch


# ---- objects ----
def _objects(C, coord, instance, cls, size=None, **kw):
    obj, object_of, n_objects = C.objects(coord, instance, cls, size, **kw)
    torch.cuda.synchronize()
    assert obj.dtype == torch.int32 and object_of.dtype == torch.int32 and isinstance(n_objects, int)
    return obj.cpu().numpy(), object_of.cpu().numpy(), n_objects


@pytest.mark.parametrize("s", ["a", "b"])
def test_golden_scenes_through_instances_then_objects_equal_the_reference(C, gold, s):
    coord, pred = dev(gold[f"coord_{s}"]), dev(gold[f"pred_{s}"])
    instance, cls, size = C.instances(coord, torch.zeros_like(coord), pred)
    assert np.array_equal(instance.cpu().numpy(), gold[f"instance_{s}"]) and np.array_equal(cls.cpu().numpy(), gold[f"instance_class_{s}"])
    obj, object_of, n_objects = _objects(C, coord, instance, cls, size)
    print(f"scene {s}: {len(gold[f'coord_{s}'])} points, {len(cls)} instances, {n_objects} objects, launches {C.LAST_CONTACTS['launches']}, "
          f"read-backs {C.LAST_CONTACTS['readbacks']}")
    assert n_objects == int(gold[f"n_objects_{s}"]) and np.array_equal(obj, gold[f"object_{s}"])
    want = O.objects(O.contacts(gold[f"coord_{s}"], gold[f"instance_{s}"], 0.08, len(cls))[0], gold[f"instance_size_{s}"], gold[f"instance_class_{s}"])
    assert np.array_equal(object_of, want[0])
    again = _objects(C, coord, instance, cls)                              # instance_size defaults to the bincount
    assert np.array_equal(again[0], obj) and np.array_equal(again[1], object_of) and again[2] == n_objects


@pytest.fixture(scope="module")
def random_scene():
    """1 500 points in 24 overlapping blobs, every blob an instance: ten faces, fourteen edges of classes 6 .. 19 (18 and 19 are ignored
    classes), a tenth of the points in no instance.  The oracle finds 6, 4 and 2 objects under the three settings below."""
    rng = np.random.default_rng(31)
    cls = np.sort(np.concatenate([np.arange(6), rng.integers(0, 6, 4), rng.integers(6, 20, 14)]))
    centres = rng.uniform(0.3, 0.7, (24, 3))
    instance = rng.integers(0, 24, 1500)
    coord = (centres[instance] + rng.normal(0, 0.04, (1500, 3))).astype(np.float32)
    instance[rng.random(1500) < 0.1] = -1
    return coord, instance, cls


@pytest.mark.parametrize("share,radius", [(0.5, 0.08), (0.2, 0.08), (0.5, 0.15)])
def test_random_scene_equals_the_oracle(C, random_scene, share, radius):
    coord, instance, cls = random_scene
    want = O.scene_objects(coord, instance, cls, radius=radius, share=share)
    got = _objects(C, dev(coord), dev(instance), dev(cls), radius=radius, share=share)
    print(f"random scene, share {share}, radius {radius}: {want[2]} objects, {int((want[1] >= 0).sum())} instances in one")
    assert got[2] == want[2] and np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0])
    assert want[2] == {(0.5, 0.08): 6, (0.2, 0.08): 4, (0.5, 0.15): 2}[(share, radius)] and (want[0] >= 0).any()


def test_a_tiny_radius_gives_zero_objects(C, random_scene):
    coord, instance, cls = random_scene
    obj, object_of, n_objects = _objects(C, dev(coord), dev(instance), dev(cls), radius=1e-4)
    assert n_objects == 0 and (obj == -1).all() and (object_of == -1).all() and obj.shape == (1500,) and object_of.shape == (24,)
