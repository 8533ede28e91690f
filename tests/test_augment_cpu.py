"""CPU: the oracle of the device augmentations (tests/augment_oracle.py) against the fixture the reference's own util/transform.py wrote
(tests/golden/augment_reference.npz), the pass compiler's counts, the draw records, every check that needs no GPU, the declarations
of csrc/augment.hip's launchers, and dataprep.collate against the reference's two collate functions restated here.  No HIP compute runs.

Bounds (float64 inputs; eps = 2^-53):
  * the elementwise classes - scale, shift, jitter, drop colour, flip, the four chromatic classes - are BIT-EQUAL to the reference, NaN
    positions included;
  * the two rotations: numpy's np.dot goes through BLAS (unspecified order and fused operations), the oracle evaluates
    (p0 R0j + p1 R1j) + p2 R2j: |difference| <= 4 eps sum_i |p_i| |R_ij| per element;
  * elastic: the blurred grid is bit-equal to scipy.ndimage's own (stored in the fixture), and the result is held to
    16 eps (|coord| + magnitude max|blurred noise|) - an 8-term sum of 4-factor products;
  * the chains: colours bit-equal; coordinates pass the rotation's error e through a scale s <= 1.2 and at most one jitter |j| <= 0.02,
    each of which rounds both sides once at a magnitude of at most |result| + 0.02: 1.2 e + 4 eps (|result| + 0.02), second-order terms
    covered by the factor 1 + 2^-40.
"""
import os

import numpy as np
import pytest
import torch

from stratified_transformer_amd import _lib, augment as A, dataprep, pointops
from tests import abi_header
from tests import augment_cases as cases
from tests import augment_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -53


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(ROOT, "tests", "golden", "augment_reference.npz"), allow_pickle=False)


def _rotation(name, kw, d):
    if name == "RandomRotate":
        angle = d["u"] * 2 * np.pi if kw.get("rotate_angle") is None else kw["rotate_angle"]
        return O.rotate_matrix(angle, kw.get("along_z", True))
    angles = np.clip(kw.get("angle_sigma", 0.06) * np.asarray(d["randn"]), -kw.get("angle_clip", 0.18), kw.get("angle_clip", 0.18))
    return O.perturbation_matrix(angles)


def _rotation_bound(x, R):
    return 4 * EPS * (np.abs(x) @ np.abs(R))


# ---- every class alone ----
@pytest.mark.parametrize("case", cases.SINGLE, ids=[c[0] for c in cases.SINGLE])
def test_oracle_against_the_reference_single(fixture, case):
    tag, name, kw, which, _ = case
    z = fixture
    coord, feat = z["base.coord"], z[which + ".feat"]
    want_c = z[tag + ".coord"] if tag + ".coord" in z.files else coord
    want_f = z[tag + ".feat"] if tag + ".feat" in z.files else feat
    t = cases.build(O, [(name, kw)])[0]
    d = cases.load_draws(z, tag, 1)[0]
    keep_c, keep_f = coord.copy(), feat.copy()
    got_c, got_f = t(coord, feat, d)
    assert cases.same_bits(coord, keep_c) and cases.same_bits(feat, keep_f)                # the oracle is out of place
    if name in cases.ELEMENTWISE:
        assert cases.same_bits(got_c, want_c) and cases.same_bits(got_f, want_f)
    elif name in cases.ROTATIONS:
        R = _rotation(name, kw, d)
        diff = np.abs(got_c - want_c)
        print(tag, "coord max deviation", diff.max(), "bound min", _rotation_bound(coord, R).min())
        assert np.all(diff <= _rotation_bound(coord, R))
        if kw.get("color_rotate") or kw.get("normals"):
            assert np.all(np.abs(got_f - want_f) <= _rotation_bound(feat, R))
        else:
            assert cases.same_bits(got_f, want_f)
    else:
        assert name == "ElasticDistortion"
        assert cases.same_bits(got_f, want_f)
        if d["gate"] < 0.95:
            assert len(t.blurred) == len(d["blur"]) == 2
            x = coord
            for grid, ref_grid, (_, magnitude) in zip(t.blurred, d["blur"], kw["distortion_params"]):
                assert cases.same_bits(grid, ref_grid)                                         # scipy.ndimage's six filters, bit for bit
            bound = sum(16 * EPS * (np.abs(x).max() + m * np.abs(g).max()) for g, (_, m) in zip(d["blur"], kw["distortion_params"]))
            diff = np.abs(got_c - want_c)
            print(tag, "coord max deviation", diff.max(), "bound", bound)
            assert np.all(diff <= bound)
            assert not cases.same_bits(want_c, coord)
        else:
            assert cases.same_bits(got_c, coord) and tag + ".coord" not in z.files


def test_constant_channel_gives_nan_like_the_reference(fixture):
    want = fixture["contrast_const.feat"]
    assert np.isnan(want[:, 1]).all() and not np.isnan(want[:, [0, 2]]).any()


# ---- the two chains on every scene of the batch ----
@pytest.mark.parametrize("chain_name", list(cases.CHAINS))
def test_oracle_against_the_reference_chains(fixture, chain_name):
    z = fixture
    chain, _ = cases.CHAINS[chain_name]
    ends = [0] + z["batch.offset"].tolist()
    assert tuple(np.diff(ends)) == cases.BATCH_SIZES
    for s in range(3):
        coord, feat = z["batch.coord"][ends[s]:ends[s + 1]], z["batch.feat"][ends[s]:ends[s + 1]]
        p = f"{chain_name}.s{s}"
        want_c = z[p + ".coord"] if p + ".coord" in z.files else coord
        want_f = z[p + ".feat"] if p + ".feat" in z.files else feat
        ds = cases.load_draws(z, p, len(chain))
        c, f, e = coord, feat, None
        for (name, kw), t, d in zip(chain, cases.build(O, chain), ds):
            if name in cases.ROTATIONS:
                e = _rotation_bound(c, _rotation(name, kw, d))
            c, f = t(c, f, d)
        assert cases.same_bits(f, want_f)
        bound = (1.2 * e + 4 * EPS * (np.abs(want_c) + 0.02)) * (1 + 2.0 ** -40)
        diff = np.abs(c - want_c)
        print(p, "coord max deviation", diff.max())
        assert np.all(diff <= bound)


def test_fixture_sees_every_gate_open_and_shut(fixture):
    z = fixture
    for tag in ("drop_off", "elastic_off", "flip_off"):
        assert tag + ".coord" not in z.files and tag + ".feat" not in z.files
    for tag in ("drop_on", "contrast_on", "translate_on", "cjitter_on", "huesat"):
        assert tag + ".feat" in z.files
    assert "contrast_fixed.feat" in z.files and "translate_off.feat" in z.files and "contrast_off.feat" in z.files       # the chromatic classes convert to 0..255 and back even with the gate shut
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "augment_reference.npz")) < 600_000


# ---- the pass compiler ----
def _chain(spec):
    return A.Compose(cases.build(A, spec))


def test_pass_and_readback_counts():
    assert A.plan_counts(_chain(cases.S3DIS_CHAIN)) == {"passes": 1, "readbacks": 0}
    assert A.plan_counts(A.Compose([])) == {"passes": 1, "readbacks": 0}
    # a flip or an auto-contrast: one more pass (the one that reduces the extrema), no read-back
    assert A.plan_counts(_chain(cases.S3DIS_CHAIN + [("RandomHorizontalFlip", {})])) == {"passes": 2, "readbacks": 0}
    assert A.plan_counts(_chain(cases.S3DIS_CHAIN[:3] + [("ChromaticAutoContrast", {})])) == {"passes": 2, "readbacks": 0}
    assert A.plan_counts(A.RandomHorizontalFlip()) == {"passes": 2, "readbacks": 0}
    # colours untouched since the reduction in front of the flip: the auto-contrast joins the flip's pass
    assert A.plan_counts(_chain([("RandomHorizontalFlip", {}), ("RandomScale", {}), ("ChromaticAutoContrast", {})])) == {"passes": 2, "readbacks": 0}
    # ... but not after an op that wrote them
    assert A.plan_counts(_chain([("RandomHorizontalFlip", {}), ("RandomDropColor", {}), ("ChromaticAutoContrast", {})])) == {"passes": 3, "readbacks": 0}
    # elastic: one read-back and one pass per entry; the full chain = reduction, entry 1, entry 2, everything else
    assert A.plan_counts(A.ElasticDistortion(cases.ELASTIC_PARAMS)) == {"passes": 3, "readbacks": 2}
    assert A.plan_counts(A.ElasticDistortion(None)) == {"passes": 1, "readbacks": 0}
    assert A.plan_counts(_chain(cases.FULL_CHAIN)) == {"passes": 4, "readbacks": 2}
    # a tape holds at most 32 ops
    assert A.plan_counts(A.Compose([A.RandomScale()] * 32)) == {"passes": 1, "readbacks": 0}
    assert A.plan_counts(A.Compose([A.RandomScale()] * 33)) == {"passes": 2, "readbacks": 0}


def test_compose_flattens_nested_chains():
    inner = A.Compose([A.RandomScale(), A.RandomShift()])
    leaves = A.Compose([A.RandomRotate(), inner, A.RandomJitter()])._leaves()
    assert [type(x).__name__ for x in leaves] == ["RandomRotate", "RandomScale", "RandomShift", "RandomJitter"]


# ---- draws: record, replay, parameter tables ----
def _host_call(n, b, draws=None, seed=3, feat=True):
    coord = torch.zeros(n, 3, dtype=torch.float64)
    offset = torch.tensor(np.linspace(0, n, b + 1)[1:].astype(np.int32))
    return A._Call(coord, coord.clone() if feat else None, offset, draws, np.random.default_rng(seed), torch.Generator().manual_seed(seed))


def test_draws_record_and_replay_round_trip():
    leaves = _chain(cases.FULL_CHAIN[1:] + cases.S3DIS_CHAIN + [("RandomShift", {}), ("RandomRotatePerturbation", {})])._leaves()
    first = _host_call(40, 3)
    tables = [leaf._params(first, first.record(leaf))[0] for leaf in leaves]
    assert len(first.out.records) == len(leaves)
    assert first.out.records[0]["gate"].shape == (3,) and first.out.records[0]["axes"].shape == (3, 2)
    assert all(t.shape[0] == 3 and t.shape[1] <= A.PARAMS for t in tables)
    again = _host_call(40, 3, draws=first.out, seed=99)                    # another seed: nothing is drawn in a replay
    for leaf, table, rec in zip(leaves, tables, first.out.records):
        assert again.record(leaf) is rec
        assert np.array_equal(leaf._params(again, rec)[0], table)
    other = _host_call(40, 3, seed=4)
    assert not np.array_equal(leaves[2]._params(other, other.record(leaves[2]))[0], tables[2])
    # host draws alone may be replayed: the per-point noise is then drawn by the call
    partial = A.Draws([{"gate": np.array([0.1, 0.99, 0.5])}])
    call = _host_call(40, 3, draws=partial)
    rec = call.record(A.ChromaticJitter())
    A.ChromaticJitter(0.05)._params(call, rec)
    assert rec["noise"].shape == (40, 3) and rec["noise"].dtype == torch.float64


def test_parameter_tables_follow_the_reference_expressions():
    call = _host_call(10, 2)
    rec = {"u": np.array([0.25, 0.7])}
    table = A.RandomRotate(along_z=False)._params(call, rec)[0]
    for s in range(2):
        assert np.array_equal(table[s, 1:10].reshape(3, 3), O.rotate_matrix(rec["u"][s] * 2 * np.pi, False))
    assert table[:, 0].tolist() == [1, 1] and table[:, 10].tolist() == [1, 1] and table[:, 11].tolist() == [0, 0]
    rec = {"randn": np.array([[0.3, -5.0, 1.0], [0.0, 0.1, 9.0]])}
    table = A.RandomRotatePerturbation(0.2, 0.18, normals=True)._params(call, rec)[0]
    for s in range(2):
        assert np.array_equal(table[s, 1:10].reshape(3, 3), O.perturbation_matrix(np.clip(0.2 * rec["randn"][s], -0.18, 0.18)))
    assert table[:, 11].tolist() == [1, 1]
    table = A.RandomDropColor(p=0.8, color_augment=0.5)._params(call, {"u": np.array([0.8, 0.81])})[0]
    assert table.tolist() == [[0, 0.5], [1, 0.5]]                                       # strictly greater than p
    table = A.RandomHorizontalFlip("y")._params(call, {"gate": np.array([0.949, 0.95]), "axes": np.array([[0.4, 0.5], [0.1, 0.1]])})[0]
    assert table.tolist() == [[1, 1, 0, 0], [0, 1, 0, 1]]
    table = A.ChromaticTranslation(0.1)._params(call, {"gate": np.array([0.5, 0.96]), "u": np.array([[0.1, 0.5, 0.9], [0.2, 0.3, 0.4]])})[0]
    assert np.array_equal(table[:, 1:], (np.array([[0.1, 0.5, 0.9], [0.2, 0.3, 0.4]]) - 0.5) * 255 * 2 * 0.1) and table[:, 0].tolist() == [1, 0]
    table = A.HueSaturationTranslation(0.5, 0.2)._params(call, {"hue_u": np.array([0.1, 0.9]), "sat_u": np.array([0.3, 0.6])})[0]
    assert table[0].tolist() == [1, (0.1 - 0.5) * 2 * 0.5, 1 + (0.3 - 0.5) * 2 * 0.2]
    table = A.ChromaticAutoContrast(randomize_blend_factor=False, blend_factor=0.25)._params(call, {"gate": np.array([0.19, 0.2]), "blend": np.array([0.7, 0.7])})[0]
    assert table.tolist() == [[1, 0.25], [0, 0.25]]
    # no colours: the drop draws nothing and is a no-op, as in the reference
    bare = _host_call(10, 2, feat=False)
    assert A.RandomDropColor()._draw(bare) == {} and A.RandomDropColor()._params(bare, {})[0][:, 0].tolist() == [0, 0]


# ---- validation ----
def test_constructor_errors():
    with pytest.raises(ValueError, match="is_temporal"):
        A.RandomHorizontalFlip("z", is_temporal=True)
    with pytest.raises(ValueError, match="upright_axis"):
        A.RandomHorizontalFlip("w")
    with pytest.raises(ValueError, match="clip"):
        A.RandomJitter(0.01, 0.0)
    with pytest.raises(ValueError, match="granularity"):
        A.ElasticDistortion([[0.0, 1.0]])


def test_call_errors_need_no_gpu():
    t = A.RandomScale()
    cpu = torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        t(cpu, cpu)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        t(np.zeros((4, 3)), None)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        A.Compose([t])(cpu.double(), None, torch.tensor([4], dtype=torch.int32))


def test_replayed_draws_are_checked():
    call = _host_call(10, 2, draws=A.Draws([]))
    with pytest.raises(ValueError, match="shorter chain"):
        call.record(A.RandomScale())
    call = _host_call(10, 2)
    with pytest.raises(ValueError, match="shape"):
        A.RandomScale()._params(call, {"scale": np.ones(3)})
    with pytest.raises(ValueError, match="noise"):
        A.RandomJitter()._params(call, {"noise": torch.zeros(9, 3, dtype=torch.float64)})
    with pytest.raises(ValueError, match="needs feat"):
        A.ChromaticTranslation()._emit(_host_call(10, 2, feat=False), A._Tape(None), {})


# ---- the C ABI ----
def test_launchers_are_declared_bound_and_exported():
    I, P, Q = _lib.I, _lib.P, _lib.Q
    assert _lib.SIGNATURES["pointops2_augment_pass_launcher"] == [I] * 6 + [P] * 10
    assert _lib.SIGNATURES["pointops2_augment_blur_launcher"] == [Q, I, I, P, P, P]
    defines = abi_header.codes("POINTOPS2_AUGMENT_")
    assert {k[3:]: v for k, v in defines.items() if k.startswith("op_") and k != "op_nop"} == A.OP
    assert (defines["params"], defines["max_ops"], defines["stat_words"]) == (A.PARAMS, A.MAX_OPS, A.STAT_WORDS)
    assert (defines["has_feat"], defines["store"], defines["stats"]) == (A.HAS_FEAT, A.STORE, A.STATS)
    assert defines["max_scenes"] == 1024
    assert "augment.hip" in open(os.path.join(_lib.CSRC, "Makefile")).read()


# ---- collation: the reference's collate_fn_limit / collate_fn_limit_mix3d restated (util/data_util.py:17-80) ----
def _collate_limit(batch, max_batch_points, mix3d_draw=None, p=None):
    coord, feat, label = list(zip(*batch))
    offset, count, k = [], 0, 0
    for item in coord:
        count += item.shape[0]
        if count > max_batch_points:
            break
        k += 1
        offset.append(count)
    if p is not None and mix3d_draw <= p:
        mixed = []
        for i in range(0, k, 2):
            mixed.append(offset[i] if i == k - 1 else offset[i + 1])
        offset = mixed
    return torch.cat(coord[:k]), torch.cat(feat[:k]), torch.cat(label[:k]), torch.IntTensor(offset)


@pytest.mark.parametrize("limit,kept", [(10 ** 6, 5), (5 + 7 + 3, 3), (5 + 7 + 3 - 1, 2), (5, 1)])
def test_collate_cuts_and_pairs_like_the_reference(limit, kept):
    g = torch.Generator().manual_seed(0)
    sizes = [5, 7, 3, 9, 4]
    batch = [(torch.randn(n, 3, generator=g), torch.randn(n, 3, generator=g), torch.randint(0, 13, (n,), generator=g)) for n in sizes]
    for p, draw in ((None, None), (0.8, 0.8), (0.8, 0.81), (0.8, 0.1)):
        want = _collate_limit(batch, limit, draw, p)
        got = dataprep.collate(batch, limit, mix3d_p=p, draw=draw)
        assert len(got) == 4 and got[3].dtype == torch.int32
        for a, b in zip(got, want):
            assert torch.equal(a, b)
        assert pointops._host_list(got[3]) == want[3].tolist()                              # registered: the sampler reads nothing back
        mixed = p is not None and draw <= p
        assert got[3].shape[0] == ((kept + 1) // 2 if mixed else kept)
    shifted = [s + (torch.randn(s[0].shape[0], 3, generator=g),) for s in batch]
    got = dataprep.collate(shifted, limit)
    assert len(got) == 5 and torch.equal(got[4], torch.cat([s[3] for s in shifted[:kept]]))
    with pytest.raises(ValueError):
        dataprep.collate([batch[0], shifted[1]], limit)
    with pytest.raises(ValueError):
        dataprep.collate([], limit)
