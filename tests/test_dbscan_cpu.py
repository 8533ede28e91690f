"""CPU: the oracle of the device DBSCAN (tests/dbscan_oracle.py) against scikit-learn's recorded results
(tests/golden/dbscan_sklearn.npz), the instance numbering of `instantiation_eval`, and the host side of
stratified_transformer_amd.cluster: declarations, argument checks, the missing CPU path, N == 0.  No HIP compute runs here."""
import inspect
import os

import numpy as np
import pytest
import torch

import stratified_transformer_amd as sta
from stratified_transformer_amd import _lib, cluster
from tests import dbscan_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sk():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "dbscan_sklearn.npz"), allow_pickle=False))


class _OnGpu:
    """a tensor that claims to be on the GPU: the argument checks run before any launch"""

    def __init__(self, t):
        self._t = t

    is_cuda = True

    def __getattr__(self, name):
        return getattr(self._t, name)


def test_fixture_holds_the_clouds_the_issue_asks_for(sk):
    assert int(sk["n_clouds"]) == 5
    params = {(round(float(sk[f"eps_{k}"]), 3), int(sk[f"min_samples_{k}"])) for k in range(5)}
    assert params == {(0.1, 5), (0.15, 3), (0.2, 5), (0.12, 4)}
    for k in range(5):
        xyz, labels = sk[f"xyz_{k}"], sk[f"labels_{k}"]
        assert xyz.dtype == np.float32 and 250 <= len(xyz) <= 1200 and xyz.min() >= 0 and xyz.max() < 4
        core = np.zeros(len(xyz), bool)
        core[sk[f"core_{k}"]] = True
        assert labels.max() + 1 >= 8 and ((labels >= 0) & ~core).sum() >= 3 and (labels < 0).sum() >= 30   # clusters, border, noise
        # the condition on the inputs: no pair within 1e-5 of eps (float64 distances)
        x = xyz.astype(np.float64)
        d = np.sqrt(((x[:, None] - x[None]) ** 2).sum(-1))
        assert not (np.abs(d - float(np.float32(sk[f"eps_{k}"]))) < 1e-5).any()
    assert set(np.unique(sk["inst_pred"])) == {0, 1, 2, 4, 5, 7}                                          # two of the classes 0..7 empty


@pytest.mark.parametrize("k", range(5))
def test_oracle_reproduces_scikit_learn_label_for_label(sk, k):
    labels, core, n_clusters = O.dbscan(sk[f"xyz_{k}"], float(sk[f"eps_{k}"]), int(sk[f"min_samples_{k}"]))
    assert np.array_equal(labels, sk[f"labels_{k}"])
    assert np.array_equal(np.nonzero(core)[0], sk[f"core_{k}"])
    assert n_clusters.tolist() == [int(sk[f"labels_{k}"].max()) + 1]


def test_oracle_instance_numbering_is_the_references(sk):
    inst, cls, size = O.instances(sk["inst_coord"], sk["inst_shift"], sk["inst_pred"], sk["inst_eps"], sk["inst_min_samples"], sk["inst_min_points"])
    assert np.array_equal(inst, sk["inst_instance"]) and np.array_equal(cls, sk["inst_class"]) and np.array_equal(size, sk["inst_size"])
    assert np.array_equal(np.bincount(cls, minlength=8), sk["inst_per_class"])
    # class-major, every size above its class's threshold, and some clusters WERE dropped (their points are in no instance)
    assert np.all(np.diff(cls) >= 0) and np.all(size > sk["inst_min_points"][cls])
    labels, _, n_clusters = O.dbscan(sk["inst_coord"] + sk["inst_shift"], sk["inst_eps"], sk["inst_min_samples"], sk["inst_pred"], 8)
    assert int(n_clusters.sum()) > len(cls) and ((labels >= 0) & (inst < 0)).any()
    assert n_clusters[3] == 0 and n_clusters[6] == 0
    assert np.array_equal(np.bincount(inst[inst >= 0]), size)


def test_oracle_rules_on_a_hand_built_case():
    # two quadruples of core points (min_samples 4); a border point within eps of ONE core point of each (three neighbours with itself:
    # not core); one noise point
    eps = 0.25
    a = [[0.0, 0, 0], [0.05, 0, 0], [0.1, 0, 0], [0.15, 0, 0]]
    b = [[0.63, 0, 0], [0.68, 0, 0], [0.73, 0, 0], [0.78, 0, 0]]
    xyz = np.array(b + a + [[0.39, 0, 0], [3.0, 3, 3]], np.float32)        # cluster 0 is b's: it holds the smallest core index
    labels, core, n = O.dbscan(xyz, eps, 4)
    assert labels.tolist() == [0] * 4 + [1] * 4 + [0, -1] and core.tolist() == [True] * 8 + [False] * 2 and n.tolist() == [2]
    labels, _, _ = O.dbscan(xyz[[4, 5, 6, 7, 0, 1, 2, 3, 8, 9]], eps, 4)     # a's first: the border point goes to a's cluster, again 0
    assert labels.tolist() == [0] * 4 + [1] * 4 + [0, -1]
    # groups: numbers restart per group, group -1 is left out
    labels, core, n = O.dbscan(np.concatenate([xyz, xyz]), [eps, eps], [4, 4], np.array([1] * 10 + [0] * 9 + [-1]))
    assert labels.tolist() == ([0] * 4 + [1] * 4 + [0, -1]) * 2 and n.tolist() == [2, 2] and not core[-1]


def test_public_interface():
    assert sta.dbscan is cluster.dbscan and sta.instances is cluster.instances
    assert {"dbscan", "instances"} <= set(sta.__all__)
    assert str(inspect.signature(cluster.dbscan)) == "(xyz, eps, min_samples, group=None)"
    assert str(inspect.signature(cluster.instances)) == "(coord, shift, pred, eps=None, min_samples=None, min_points=None)"
    assert cluster.MAX_ROUNDS >= 32  # the trees halve per round: enough for 2^31 points
    assert "sklearn" not in open(cluster.__file__).read().replace("sklearn.cluster.DBSCAN", "").replace("dbscan_sklearn.npz", "")


def test_cpu_tensors_raise_no_cpu_fallback():
    xyz, group = torch.rand(10, 3), torch.zeros(10, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cluster.dbscan(xyz, 0.1, 5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cluster.dbscan(_OnGpu(xyz), 0.1, 5, group)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cluster.instances(xyz, xyz, group)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cluster.instances(_OnGpu(xyz), xyz, _OnGpu(group))


F, L = torch.float32, torch.int64


@pytest.mark.parametrize("xyz,eps,min_samples,group,error", [
    (torch.zeros(10, 2), 0.1, 5, None, ValueError),                                   # xyz not [N, 3]
    (torch.zeros(30), 0.1, 5, None, ValueError),
    (torch.zeros(10, 3, dtype=torch.float64), 0.1, 5, None, TypeError),               # xyz dtype
    (torch.zeros(10, 3, dtype=torch.float16), 0.1, 5, None, TypeError),
    (torch.zeros(10, 3), 0.1, 5, torch.zeros(9, dtype=L), ValueError),                # group not [N]
    (torch.zeros(10, 3), 0.1, 5, torch.zeros(10, 1, dtype=L), ValueError),
    (torch.zeros(10, 3), 0.1, 5, torch.zeros(10, dtype=F), TypeError),                # group dtype
    (torch.zeros(10, 3), 0.1, 5, torch.zeros(10, dtype=torch.int16), TypeError),
    (torch.zeros(10, 3), 0.0, 5, None, ValueError),                                   # eps <= 0
    (torch.zeros(10, 3), -0.1, 5, None, ValueError),
    (torch.zeros(10, 3), float("nan"), 5, None, ValueError),
    (torch.zeros(10, 3), [0.1, 0.0], [5, 5], torch.zeros(10, dtype=L), ValueError),
    (torch.zeros(10, 3), torch.tensor([0.1, -1.0]), 5, torch.zeros(10, dtype=L), ValueError),
    (torch.zeros(10, 3), 0.1, 0, None, ValueError),                                   # min_samples < 1
    (torch.zeros(10, 3), 0.1, [3, 0], torch.zeros(10, dtype=L), ValueError),
    (torch.zeros(10, 3), 0.1, 2.5, None, ValueError),
    (torch.zeros(10, 3), [0.1, 0.2], [5, 5, 5], torch.zeros(10, dtype=L), ValueError),  # lengths disagree
    (torch.zeros(10, 3), [0.1, 0.2], 5, None, ValueError),                            # two settings for the one group of group=None
    (torch.zeros(10, 3), [[0.1]], 5, None, ValueError),
    (torch.zeros(10, 3), "0.1", 5, None, TypeError),
])
def test_dbscan_rejects_bad_arguments_before_any_launch(xyz, eps, min_samples, group, error):
    calls = _lib.CALLS[0]
    with pytest.raises(error, match="dbscan"):
        cluster.dbscan(_OnGpu(xyz), eps, min_samples, None if group is None else _OnGpu(group))
    assert _lib.CALLS[0] == calls


def test_instances_rejects_bad_arguments():
    xyz, pred = _OnGpu(torch.zeros(10, 3)), _OnGpu(torch.zeros(10, dtype=L))
    with pytest.raises(ValueError, match="shift"):
        cluster.instances(xyz, _OnGpu(torch.zeros(9, 3)), pred)
    with pytest.raises(ValueError, match="shift"):
        cluster.instances(xyz, _OnGpu(torch.zeros(10, 3, dtype=torch.float64)), pred)
    with pytest.raises(ValueError, match="agree"):
        cluster.instances(xyz, xyz, pred, eps=[0.1] * 8, min_samples=[5] * 7)
    with pytest.raises(ValueError, match="eps"):
        cluster.instances(xyz, xyz, pred, eps=[0.1, 0.0], min_samples=[5, 5], min_points=[1, 1])
    with pytest.raises(ValueError, match="min_samples"):
        cluster.instances(xyz, xyz, pred, eps=[0.1, 0.1], min_samples=0, min_points=3)
    with pytest.raises(TypeError, match="group"):
        cluster.instances(xyz, xyz, _OnGpu(torch.zeros(10)))


def test_reference_settings_are_the_defaults():
    want = np.array([[0.1, 5, 50]] * 6 + [[0.15, 3, 20]] * 2)
    for col, (face, edge, dtype) in enumerate(zip(cluster.FACE_SETTINGS, cluster.EDGE_SETTINGS, (np.float32, np.int32, np.int32))):
        got = cluster._class_settings(None, 8, face, edge, dtype, "x")
        assert got.dtype == dtype and np.array_equal(got, want[:, col].astype(dtype))


def test_no_points_returns_empty_tensors_without_a_launch():
    calls = _lib.CALLS[0]
    labels, core, n_clusters = cluster.dbscan(_OnGpu(torch.zeros(0, 3)), 0.1, 5)
    assert labels.shape == (0,) and labels.dtype == torch.int32 and core.shape == (0,) and core.dtype == torch.bool
    assert n_clusters.tolist() == [0] and n_clusters.dtype == torch.int32
    _, _, n_clusters = cluster.dbscan(_OnGpu(torch.zeros(0, 3)), [0.1, 0.2, 0.3], 5, _OnGpu(torch.zeros(0, dtype=L)))
    assert n_clusters.tolist() == [0, 0, 0]
    inst, cls, size = cluster.instances(_OnGpu(torch.zeros(0, 3)), _OnGpu(torch.zeros(0, 3)), _OnGpu(torch.zeros(0, dtype=L)))
    assert inst.shape == cls.shape == size.shape == (0,) and inst.dtype == cls.dtype == size.dtype == torch.int32
    assert _lib.CALLS[0] == calls
