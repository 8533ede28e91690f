"""CPU: the oracle of cluster.objects (tests/contacts_oracle.py) against the reference's recorded objects
(tests/golden/objects_reference.npz, written by the reference's own instantiation_eval), the literal merge loop against the connected
components, the host pairing of stratified_transformer_amd.cluster.link_objects on hand-made tables, and the argument checks of
contacts / objects that need no GPU.  No HIP compute runs here."""
import inspect
import os

import numpy as np
import pytest
import torch

import stratified_transformer_amd as sta
from stratified_transformer_amd import _lib, cluster
from tests import contacts_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, L = torch.float32, torch.int64


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "objects_reference.npz"), allow_pickle=False))


@pytest.fixture(scope="module")
def gold_counts(gold):
    """the oracle's contact counts of both golden scenes, computed once"""
    return {s: O.contacts(gold[f"coord_{s}"], gold[f"instance_{s}"], float(gold["radius"]), len(gold[f"instance_class_{s}"]))[0] for s in "ab"}


class _OnGpu:
    """a tensor that claims to be on the GPU: the argument checks run before any launch"""

    def __init__(self, t):
        self._t = t

    is_cuda = True

    def __getattr__(self, name):
        return getattr(self._t, name)


def _tables(cls, links, size=10):
    """count / size / class tables in which edge instance e has `size` points and count[e, k] as given in links {(e, k): count}"""
    cls = np.asarray(cls)
    count = np.zeros((len(cls), len(cls)), np.int32)
    sizes = np.full(len(cls), size, np.int32)
    count[np.arange(len(cls)), np.arange(len(cls))] = sizes
    for (e, k), c in links.items():
        count[e, k] = c
    return count, sizes, cls


def test_fixture_holds_the_scenes_the_issue_asks_for(gold):
    assert float(gold["radius"]) == 0.08 and float(gold["share"]) == 0.5 and gold["lookup_face"].tolist() == O.EDGE_FACES
    assert gold["lookup_face"].tolist() == [list(p) for p in cluster.EDGE_FACES]
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "objects_reference.npz")) < 1 << 20
    for s in "ab":
        coord, pred, obj, inst, cls = (gold[f"{k}_{s}"] for k in ("coord", "pred", "object", "instance", "instance_class"))
        assert coord.dtype == np.float32 and 5000 <= len(coord) <= 12000 and set(np.unique(pred)) == set(range(18))
        assert int(gold[f"n_objects_{s}"]) == obj.max() + 1 and (obj[pred >= 6] == -1).all()           # supports hold face points only
        assert np.array_equal(np.bincount(inst[inst >= 0]), gold[f"instance_size_{s}"]) and np.all(np.diff(cls) >= 0)
    # A: a box without one face, a box with a single edge (an object of two faces), a component of eleven faces that spans two boxes
    cls_a, inst_a, obj_a = gold["instance_class_a"], gold["instance_a"], gold["object_a"]
    assert np.bincount(cls_a[cls_a < 6]).tolist() == [2, 3, 3, 3, 3, 3] and int((cls_a >= 6).sum()) == 25
    faces_per_object = sorted(len(np.unique(inst_a[obj_a == o])) for o in range(obj_a.max() + 1))
    assert faces_per_object == [2, 11]
    assert len(np.unique(inst_a[(obj_a == -1) & (inst_a >= 0) & (gold["pred_a"] < 6)])) == 4                # faces that no edge linked
    # B: no instance of class 5, so the edge classes beside it are discarded; one object of a single face
    cls_b, inst_b, obj_b = gold["instance_class_b"], gold["instance_b"], gold["object_b"]
    assert not (cls_b == 5).any() and all((cls_b == 6 + c).any() for c in (8, 9, 10, 11))
    assert sorted(len(np.unique(inst_b[obj_b == o])) for o in range(obj_b.max() + 1)) == [1, 5, 5]


@pytest.mark.parametrize("s", ["a", "b"])
def test_oracle_objects_equal_the_references(gold, gold_counts, s):
    obj, object_of, n_objects = O.scene_objects(gold[f"coord_{s}"], gold[f"instance_{s}"], gold[f"instance_class_{s}"], gold[f"instance_size_{s}"],
                                                   count=gold_counts[s])
    assert n_objects == int(gold[f"n_objects_{s}"]) and np.array_equal(obj, gold[f"object_{s}"])
    # the host pairing of the package on the oracle's counts: the same tables
    got_of, got_n = cluster.link_objects(gold_counts[s], gold[f"instance_size_{s}"], gold[f"instance_class_{s}"])
    assert got_n == n_objects and got_of.dtype == np.int32 and np.array_equal(got_of, object_of)
    if s == "b":   # rule 2 discarded edges that DO have a face beside them
        cls, count, size = gold["instance_class_b"], gold_counts["b"], gold["instance_size_b"]
        dropped = np.nonzero(cls >= 6 + 8)[0]
        assert len(dropped) and (object_of[dropped] == -1).all()
        assert any((2 * count[e, np.nonzero(cls < 6)[0]] > size[e]).any() for e in dropped)


@pytest.mark.parametrize("s", ["a", "b"])
def test_literal_merge_loop_equals_the_components_on_the_golden_scenes(gold, gold_counts, s):
    cls, size = gold[f"instance_class_{s}"], gold[f"instance_size_{s}"]
    sets, fixed_point = O.objects_literal(gold_counts[s], size, cls)
    assert fixed_point
    object_of, n_objects = O.objects(gold_counts[s], size, cls)
    faces = np.nonzero(cls < 6)[0]
    assert sets == {frozenset(faces[object_of[faces] == o].tolist()) for o in range(n_objects)}


@pytest.mark.parametrize("seed", range(20))
def test_literal_merge_loop_equals_the_components_on_random_link_tables(seed):
    rng = np.random.default_rng(seed)
    n_faces, n_edges = int(rng.integers(6, 30)), int(rng.integers(1, 40))
    cls = np.sort(np.concatenate([np.arange(6), rng.integers(0, 6, n_faces - 6), [6], rng.integers(6, 20, n_edges)]))   # classes 18, 19: ignored
    count, size, cls = _tables(cls, {})
    faces = np.nonzero(cls < 6)[0]
    for e in np.nonzero(cls >= 6)[0]:
        count[e, rng.choice(faces, int(rng.integers(0, 4)), replace=False)] = rng.integers(4, 11)
    if not O.pair_list(count, size, cls)[0]:
        count[np.nonzero(cls == 6)[0][0], :] = 10
    sets, fixed_point = O.objects_literal(count, size, cls)
    assert fixed_point
    object_of, n_objects = O.objects(count, size, cls)
    assert sets == {frozenset(faces[object_of[faces] == o].tolist()) for o in range(n_objects)}
    got_of, got_n = cluster.link_objects(count, size, cls)
    assert got_n == n_objects and np.array_equal(got_of, object_of)


def _link(cls, links, **kw):
    count, size, cls = _tables(cls, links)
    got = cluster.link_objects(count, size, cls, **kw)
    want = O.objects(count, size, cls, **kw)
    assert np.array_equal(got[0], want[0]) and got[1] == want[1]
    return got[0].tolist(), got[1]


def test_rule_2_an_edge_class_without_one_of_its_face_classes_is_skipped():
    # edge class 6 = faces (0, 1); no instance of class 1: the edge is skipped although the class-0 face is right beside it
    assert _link([0, 2, 6], {(2, 0): 10}) == ([-1, -1, -1], 0)
    assert _link([0, 1, 6], {(2, 0): 10}) == ([0, -1, 0], 1)                 # with a class-1 instance anywhere in the scene it links


def test_first_match_the_lower_instance_number_wins():
    # two faces of class 0 both above the share: the first is linked, the second is in no object
    assert _link([0, 0, 1, 6], {(3, 0): 6, (3, 1): 10, (3, 2): 10}) == ([0, -1, 0, 0], 1)


def test_exactly_half_is_not_linked():
    assert _link([0, 1, 6], {(2, 0): 5, (2, 1): 6}) == ([-1, 0, 0], 1)        # 2 * 5 == 10: not more than half
    assert _link([0, 1, 6], {(2, 0): 5, (2, 1): 5}) == ([-1, -1, -1], 0)
    # another share is compared in float64: 3 of 10 is not more than 0.3, 4 of 10 is
    assert _link([0, 1, 6], {(2, 0): 3, (2, 1): 4}, share=0.3) == ([-1, 0, 0], 1)


def test_classes_from_18_are_ignored():
    assert _link([0, 1, 18, 19], {(2, 0): 10, (2, 1): 10, (3, 0): 10}) == ([-1, -1, -1, -1], 0)
    assert _link([0, 1, 17], {(2, 0): 10, (2, 1): 10}) == ([-1, -1, -1], 0)   # class 17 = faces (4, 5): not these
    assert _link([4, 5, 17], {(2, 0): 10, (2, 1): 10}) == ([0, 0, 0], 1)


def test_no_links_zero_objects():
    assert _link([0, 1, 6, 6], {}) == ([-1, -1, -1, -1], 0)
    assert _link([], {}) == ([], 0)
    with pytest.raises(IndexError):                                          # the reference's pair_list[0] (:670)
        O.objects_literal(*_tables([0, 1, 6, 6], {}))


def test_a_chain_of_four_faces_through_three_edges_is_one_object():
    # faces of classes 0, 1, 2, 4; edges of classes 6 = faces (0, 1), 8 = faces (1, 2), 12 = faces (2, 4)
    cls = [0, 1, 2, 4, 6, 8, 12]
    links = {(4, 0): 10, (4, 1): 10, (5, 1): 10, (5, 2): 10, (6, 2): 10, (6, 3): 10}
    assert _link(cls, links) == ([0, 0, 0, 0, 0, 0, 0], 1)


def test_rule_5_numbering_by_ascending_smallest_face():
    # objects {1, 4}, {0, 5} and {2}; face 3 unlinked.  classes: faces 0 0 0 0 1 1, edges 6 6 6
    cls = [0, 0, 0, 0, 1, 1, 6, 6, 6]
    links = {(6, 1): 10, (6, 4): 10, (7, 0): 10, (7, 5): 10, (8, 2): 10}
    object_of, n = _link(cls, links)
    assert n == 3 and object_of == [0, 1, 2, -1, 1, 0, 1, 0, 2]


def test_public_interface():
    assert sta.contacts is cluster.contacts and sta.objects is cluster.objects
    assert {"contacts", "objects"} <= set(sta.__all__)
    assert str(inspect.signature(cluster.contacts)) == "(xyz, label, radius, n_labels=None)"
    assert str(inspect.signature(cluster.objects)) == ("(coord, instance, instance_class, instance_size=None, radius=0.08, share=0.5, "
                                                        "face_classes=6, edge_faces=None)")
    doc = cluster.objects.__doc__
    assert "IndexError" in doc and "fixed point" in doc                      # the two departures from the reference are stated


def test_cpu_tensors_raise_no_cpu_fallback():
    xyz, label = torch.rand(10, 3), torch.zeros(10, dtype=L)
    for a, b in ((xyz, label), (_OnGpu(xyz), label), (xyz, _OnGpu(label))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            cluster.contacts(a, b, 0.1)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            cluster.objects(a, b, torch.zeros(1, dtype=L))


@pytest.mark.parametrize("xyz,label,radius,n_labels,error", [
    (torch.zeros(10, 2), torch.zeros(10, dtype=L), 0.1, None, ValueError),                 # xyz not [N, 3]
    (torch.zeros(30), torch.zeros(10, dtype=L), 0.1, None, ValueError),
    (torch.zeros(10, 3, dtype=torch.float64), torch.zeros(10, dtype=L), 0.1, None, TypeError),
    (torch.zeros(10, 3), torch.zeros(9, dtype=L), 0.1, None, ValueError),                  # label not [N]
    (torch.zeros(10, 3), torch.zeros(10, 1, dtype=L), 0.1, None, ValueError),
    (torch.zeros(10, 3), torch.zeros(10, dtype=F), 0.1, None, TypeError),                  # label dtype
    (torch.zeros(10, 3), torch.zeros(10, dtype=torch.int16), 0.1, None, TypeError),
    (torch.zeros(10, 3), torch.zeros(10, dtype=L), 0.0, None, ValueError),                 # radius
    (torch.zeros(10, 3), torch.zeros(10, dtype=L), -0.1, None, ValueError),
    (torch.zeros(10, 3), torch.zeros(10, dtype=L), float("nan"), None, ValueError),
    (torch.zeros(10, 3), torch.zeros(10, dtype=L), float("inf"), None, ValueError),
    (torch.zeros(10, 3), torch.zeros(10, dtype=L), 1e-30, None, ValueError),               # underflows in fp32
    (torch.zeros(10, 3), torch.zeros(10, dtype=L), "0.1", None, TypeError),
    (torch.zeros(10, 3), torch.zeros(10, dtype=L), 0.1, -1, ValueError),                   # n_labels
    (torch.zeros(10, 3), torch.zeros(10, dtype=L), 0.1, 2.0, TypeError),
])
def test_contacts_rejects_bad_arguments_before_any_launch(xyz, label, radius, n_labels, error):
    calls = _lib.CALLS[0]
    with pytest.raises(error, match="contacts"):
        cluster.contacts(_OnGpu(xyz), _OnGpu(label), radius, n_labels)
    assert _lib.CALLS[0] == calls


def test_link_objects_rejects_bad_tables_and_settings():
    count, size, cls = _tables([0, 1, 6], {})
    with pytest.raises(ValueError, match="count"):
        cluster.link_objects(count[:2], size, cls)
    with pytest.raises(ValueError, match="count"):
        cluster.link_objects(count, size[:2], cls)
    with pytest.raises(ValueError, match="share"):
        cluster.link_objects(count, size, cls, share=float("nan"))
    with pytest.raises(ValueError, match="share"):
        cluster.link_objects(count, size, cls, share=-0.5)
    with pytest.raises(ValueError, match="edge_faces"):
        cluster.link_objects(count, size, cls, edge_faces=[(0, 6)])
    with pytest.raises(ValueError, match="edge_faces"):
        cluster.link_objects(count, size, cls, edge_faces=[(0, 1, 2)])
    # another table: two face classes, one edge class
    assert cluster.link_objects(*_tables([0, 1, 2], {(2, 0): 10, (2, 1): 10}), face_classes=2, edge_faces=[(0, 1)])[0].tolist() == [0, 0, 0]


def test_no_points_returns_the_empty_tables_without_a_launch():
    calls = _lib.CALLS[0]
    count, min_d2 = cluster.contacts(_OnGpu(torch.zeros(0, 3)), _OnGpu(torch.zeros(0, dtype=L)), 0.1, 3)
    assert count.shape == (3, 3) and count.dtype == torch.int32 and not count.any()
    assert min_d2.shape == (3, 3) and min_d2.dtype == torch.float32 and torch.isinf(min_d2).all() and (min_d2 > 0).all()
    count, min_d2 = cluster.contacts(_OnGpu(torch.zeros(0, 3)), _OnGpu(torch.zeros(0, dtype=L)), 0.1)
    assert count.shape == (0, 0) and min_d2.shape == (0, 0)
    assert _lib.CALLS[0] == calls
