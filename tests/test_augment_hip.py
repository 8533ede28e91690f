"""GPU: the device augmentations (stratified_transformer_amd/augment.py on csrc/augment.hip) against the numpy oracle
(tests/augment_oracle.py) with equal draws - BIT-IDENTICAL for both dtypes: the float64 result is the oracle's, the float32 result is
the oracle's float64 result on the widened input, rounded to float32 once.  The oracle itself is bound to the reference in
tests/test_augment_cpu.py."""
import numpy as np
import pytest
import torch

from stratified_transformer_amd import augment as A, dataprep
from tests import augment_cases as cases
from tests import augment_oracle as O

pytestmark = pytest.mark.gpu
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 1000)
DTYPES = (torch.float64, torch.float32)


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _expect(spec, coord, feat, ends, records):
    """the oracle, scene by scene, on the (widened) rows the device saw"""
    out_c, out_f, lo = [], [], 0
    for s, hi in enumerate(ends):
        c, f = O.Compose(cases.build(O, spec))(coord[lo:hi], None if feat is None else feat[lo:hi], cases.scene_draws(records, s, lo, hi))
        out_c.append(c)
        out_f.append(f)
        lo = hi
    return np.concatenate(out_c), None if feat is None else np.concatenate(out_f)


def _check(spec, coord64, feat64, dtype, ends=None, draws=None, seed=5):
    """run `spec` on the device in `dtype`, compare with the oracle bit for bit; -> the transform (counts, draws)"""
    t = A.Compose(cases.build(A, spec))
    coord, feat = _dev(coord64, dtype), None if feat64 is None else _dev(feat64, dtype)
    keep_c, keep_f = coord.clone(), None if feat is None else feat.clone()
    offset = None if ends is None else _dev(np.asarray(ends, np.int32))
    got_c, got_f = t(coord, feat, offset, draws=draws, rng=np.random.default_rng(seed), generator=_gen(seed))
    assert got_c.dtype == dtype and got_c.shape == coord.shape
    assert torch.equal(coord.view(torch.int64 if dtype == torch.float64 else torch.int32), keep_c.view(torch.int64 if dtype == torch.float64 else torch.int32))
    if feat is not None:
        assert cases.same_bits(feat.cpu().numpy(), keep_f.cpu().numpy())                      # inputs untouched
    seen_c, seen_f = coord.double().cpu().numpy(), None if feat is None else feat.double().cpu().numpy()
    with np.errstate(all="ignore"):
        want_c, want_f = _expect(spec, seen_c, seen_f, [coord.shape[0]] if ends is None else ends, t.last_draws.records)
    np_dtype = np.float64 if dtype == torch.float64 else np.float32
    assert cases.same_bits(got_c.cpu().numpy(), want_c.astype(np_dtype)), spec
    if feat is None:
        assert got_f is None
    else:
        assert got_f.dtype == dtype and cases.same_bits(got_f.cpu().numpy(), want_f.astype(np_dtype)), spec
    return t


def _inputs(which, n, seed=40):
    coord, feat = cases.cloud(n, seed + n)
    if which == "const" and n:
        feat[:, 1] = feat[0, 1]
    return coord, cases.narrow(feat) if which == "narrow" else feat


def _forced(spec, gates, b=1, seed=5):
    """Draws holding host draws only, with the gates of transform k overridden by gates[k] = {name: per-scene values}"""
    records = []
    call = A._Call(torch.zeros(b, 3), torch.zeros(b, 3), torch.arange(1, b + 1, dtype=torch.int32), None, np.random.default_rng(seed), None)
    for k, leaf in enumerate(A.Compose(cases.build(A, spec))._leaves()):
        rec = {key: v for key, v in leaf._draw(call).items() if not isinstance(v, torch.Tensor)}
        for key, v in gates.get(k, {}).items():
            rec[key] = np.broadcast_to(np.asarray(v, np.float64), rec[key].shape).copy()
        records.append(rec)
    return A.Draws(records)


# ---- every class alone, on every size ----
@pytest.mark.parametrize("case", cases.SINGLE, ids=[c[0] for c in cases.SINGLE])
def test_every_class_alone(case):
    tag, name, kw, which, forced = case
    spec = [(name, kw)]
    gates = {}
    if forced:      # the fixture's gate pattern for this case (tests/augment_cases.py)
        keys = {"RandomDropColor": ["u"], "ElasticDistortion": ["gate"], "RandomHorizontalFlip": ["gate", "axes"],
                "ChromaticAutoContrast": ["gate", "blend"], "ChromaticTranslation": ["gate"], "ChromaticJitter": ["gate"],
                "HueSaturationTranslation": ["hue_u", "sat_u"]}[name]
        vals = [forced[0]] + ([forced[1:]] if keys[1:] == ["axes"] else forced[1:])
        gates = {0: {k: v for k, v in zip(keys, vals) if np.size(v)}}
    for n in SIZES:
        coord, feat = _inputs(which, n)
        for dtype in DTYPES:
            _check(spec, coord, feat, dtype, draws=_forced(spec, gates) if gates else None)


def test_no_colours_where_the_reference_allows_it():
    coord, _ = cases.cloud(257, 1)
    spec = cases.S3DIS_CHAIN + [("RandomHorizontalFlip", {}), ("ElasticDistortion", dict(distortion_params=[[0.3, 0.2]])), ("RandomShift", {})]
    for dtype in DTYPES:
        _check(spec, coord, None, dtype)
    with pytest.raises(ValueError, match="needs feat"):
        A.ChromaticJitter()(_dev(coord), None)


# ---- the two chains, single scene and the batch with an empty middle scene ----
ENDS = (257, 257, 857)
FULL_GATES = {0: {"gate": [0.5, 0.5, 0.97]}, 1: {"gate": [0.5, 0.5, 0.3], "axes": [[0.1, 0.2], [0.9, 0.9], [0.8, 0.3]]},
              4: {"gate": [0.1, 0.1, 0.5]}, 5: {"gate": [0.5, 0.5, 0.97]}, 6: {"gate": [0.97, 0.5, 0.5]}}


@pytest.mark.parametrize("dtype", DTYPES)
def test_s3dis_chain(dtype):
    for n in (1, 257, 1000):
        coord, feat = _inputs("base", n)
        t = _check(cases.S3DIS_CHAIN, coord, feat, dtype)
        assert t.last_counts == {"passes": 1, "readbacks": 0}
    coord, feat = _inputs("base", ENDS[-1])
    t = _check(cases.S3DIS_CHAIN, coord, feat, dtype, ends=ENDS, draws=_forced(cases.S3DIS_CHAIN, {3: {"u": [0.9, 0.9, 0.3]}}, b=3))
    assert t.last_counts == {"passes": 1, "readbacks": 0}
    assert t.last_draws.records[1]["scale"].shape == (3,)


@pytest.mark.parametrize("dtype", DTYPES)
def test_full_chain(dtype):
    for n in (1, 65, 1000):
        coord, feat = _inputs("narrow", n)
        t = _check(cases.FULL_CHAIN, coord, feat, dtype, draws=_forced(cases.FULL_CHAIN, {k: {g: np.asarray(v)[:1] for g, v in d.items()} for k, d in FULL_GATES.items()}))
        assert t.last_counts == A.plan_counts(t) == {"passes": 4, "readbacks": 2}     # two elastic entries: two read-backs
    coord, feat = _inputs("narrow", ENDS[-1])
    t = _check(cases.FULL_CHAIN, coord, feat, dtype, ends=ENDS, draws=_forced(cases.FULL_CHAIN, FULL_GATES, b=3))
    assert t.last_counts == {"passes": 4, "readbacks": 2}                              # ... whatever the number of scenes
    noise = t.last_draws.records[0]["noise"]
    assert len(noise) == 2 and noise[0][0] is not None and noise[0][1] is None and noise[0][2] is None   # empty scene, shut gate


def test_replay_is_bitwise():
    coord, feat = _inputs("narrow", ENDS[-1])
    c, f, off = _dev(coord, torch.float32), _dev(feat, torch.float32), _dev(np.asarray(ENDS, np.int32))
    t = A.Compose(cases.build(A, cases.FULL_CHAIN + cases.S3DIS_CHAIN))
    c1, f1 = t(c, f, off, rng=np.random.default_rng(1), generator=_gen(1))
    draws = t.last_draws
    c2, f2 = t(c, f, off, draws=draws, rng=np.random.default_rng(2), generator=_gen(2))
    assert cases.same_bits(c1.cpu().numpy(), c2.cpu().numpy()) and cases.same_bits(f1.cpu().numpy(), f2.cpu().numpy())
    assert t.last_draws.records[0] is draws.records[0]
    c3, _ = t(c, f, off, rng=np.random.default_rng(2), generator=_gen(2))
    assert not torch.equal(c1, c3)
    with pytest.raises(ValueError, match="chain of 12 transforms"):
        A.RandomScale()(c, f, off, draws=draws)


# ---- NaN rows: the reductions propagate NaN as numpy's min / max do ----
@pytest.mark.parametrize("dtype", DTYPES)
def test_nan_rows_reach_the_reductions(dtype):
    coord, feat = _inputs("narrow", 300)
    coord[70, 1] = np.nan
    feat[200, 2] = np.nan
    spec = [("RandomHorizontalFlip", {}), ("RandomScale", {}), ("ChromaticAutoContrast", {}), ("ChromaticTranslation", {}),
            ("HueSaturationTranslation", dict(hue_max=0.5, saturation_max=0.2))]
    gates = {0: {"gate": [0.1, 0.1], "axes": [[0.1, 0.1], [0.1, 0.1]]}, 2: {"gate": [0.1, 0.1]}, 3: {"gate": [0.1, 0.1]}}
    t = A.Compose(cases.build(A, spec))
    _check(spec, coord, feat, dtype, ends=(100, 300), draws=_forced(spec, gates, b=2))
    got_c, got_f = t(_dev(coord, dtype), _dev(feat, dtype), _dev(np.array([100, 300], np.int32)), draws=_forced(spec, gates, b=2))
    assert torch.isnan(got_c[:100, 1]).all() and not torch.isnan(got_c[:100, 0]).any() and not torch.isnan(got_c[100:]).any()
    with pytest.raises(ValueError, match="NaN"):
        A.ElasticDistortion([[0.2, 0.4]])(_dev(coord, dtype), None, draws=A.Draws([{"gate": np.array([0.1])}]))


def test_grey_and_black_points_through_hsv():
    rgb = np.array([[0, 0, 0], [255, 255, 255], [128, 128, 128], [37, 37, 37], [255, 0, 0], [0, 255, 0], [0, 0, 255], [1, 0, 0], [254, 255, 255]], np.float64)
    feat = np.concatenate([rgb / 127.5 - 1, cases.cloud(64, 3)[1]])
    coord = cases.cloud(feat.shape[0], 4)[0]
    spec = [("HueSaturationTranslation", dict(hue_max=0.5, saturation_max=0.2))]
    for hue, sat in ((0.5, 0.5), (0.0, 1.0), (1.0, 0.0), (0.123, 0.9)):
        for dtype in DTYPES:
            _check(spec, coord, feat, dtype, draws=A.Draws([{"hue_u": np.array([hue]), "sat_u": np.array([sat])}]))
    got = A.Compose(cases.build(A, spec))(_dev(coord), _dev(feat), draws=A.Draws([{"hue_u": np.array([0.9]), "sat_u": np.array([0.2])}]))[1]
    assert (got[:4, 0] == got[:4, 1]).all() and (got[:4, 1] == got[:4, 2]).all()              # no saturation: grey stays grey


# ---- elastic: degenerate clouds ----
@pytest.mark.parametrize("dtype", DTYPES)
def test_elastic_on_flat_and_lattice_clouds(dtype):
    spec = [("ElasticDistortion", dict(distortion_params=cases.ELASTIC_PARAMS))]
    on = A.Draws([{"gate": np.array([0.1])}])
    flat, feat = cases.cloud(300, 8)
    flat[:, 2] = 0.75                                                                      # flat on z: three nodes on that axis
    t = _check(spec, flat, feat, dtype, draws=on)
    assert t.last_draws.records[0]["noise"][0][0].shape[2] == 3
    # points on the minimum and the maximum corner and on grid nodes (multiples of both granularities), also a single point
    k = np.stack(np.meshgrid(np.arange(5), np.arange(4), np.arange(3), indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    lattice = k * 0.8 + np.array([-1.6, 0.8, 0.0])
    lattice = np.concatenate([lattice, lattice[:7] + 0.2, lattice[:5] + 0.1])
    _check(spec, lattice, cases.cloud(lattice.shape[0], 9)[1], dtype, draws=A.Draws([{"gate": np.array([0.1])}]))
    _check(spec, lattice[:1], None, dtype, draws=A.Draws([{"gate": np.array([0.1])}]))
    # two equal points: every extent is zero
    _check(spec, lattice[[3, 3]], None, dtype, draws=A.Draws([{"gate": np.array([0.1])}]))


def test_blurred_grid_is_scipys():
    """the device's six box filters against the oracle's, which the CPU test holds bit-equal to scipy.ndimage's"""
    coord, _ = cases.cloud(500, 12)
    t = A.ElasticDistortion([[0.15, 0.4]])
    t(_dev(coord), None, _dev(np.array([200, 500], np.int32)), draws=A.Draws([{"gate": np.array([0.1, 0.2])}]), generator=_gen(3))
    grids, desc = t.last_blurred
    grids = grids.cpu().numpy()
    for s, (start, nx, ny, nz) in enumerate(desc):
        noise = t.last_draws.records[0]["noise"][0][s].cpu().numpy()
        assert noise.shape == (nx, ny, nz, 3)
        assert cases.same_bits(grids[start:start + noise.size].reshape(noise.shape), O.blur(noise))


# ---- limits and errors ----
def test_scene_cap_records_an_error_and_launches_nothing():
    coord = _dev(cases.cloud(64, 2)[0])
    ends = np.minimum(np.arange(1, 1026), 64).astype(np.int32)
    with pytest.raises(RuntimeError, match="1024 scenes"):
        A.RandomScale()(coord, None, _dev(ends))
    scale = A.RandomScale()                                                                    # the cap itself is fine
    got, _ = scale(coord, None, _dev(ends[:1024]), rng=np.random.default_rng(0))
    want = coord.cpu().numpy() * scale.last_draws.records[0]["scale"][:64, None]
    assert cases.same_bits(got.cpu().numpy(), want)


def test_argument_errors_on_device_tensors():
    coord = _dev(cases.cloud(10, 2)[0])
    t = A.RandomScale()
    with pytest.raises(RuntimeError, match="feat"):
        t(coord, coord.float())
    with pytest.raises(RuntimeError, match="offset"):
        t(coord, None, torch.tensor([10], device="cuda"))
    with pytest.raises(ValueError, match="replayed noise"):
        A.ElasticDistortion([[0.2, 0.4]])(coord, None, draws=A.Draws([{"gate": np.array([0.1]), "noise": [[torch.zeros(2, 2, 2, 3, device="cuda")]]}]))


# ---- dataprep: the transform and the shuffle in the loaders' preparation ----
def test_data_prepare_takes_a_transform_and_a_shuffle():
    coord, feat = cases.cloud(3000, 6)
    c, f = _dev(coord), _dev((feat + 1) * 127.5)
    label = torch.arange(3000, device="cuda") % 13
    t = A.Compose(cases.build(A, cases.S3DIS_CHAIN))
    rand = torch.zeros((), dtype=torch.int64, device="cuda")                                  # every voxel keeps its first point
    base = dataprep.data_prepare(c, f, label, split="val", voxel_size=0.04, voxel_max=500, rand=rand)
    assert all(torch.equal(a, b) for a, b in zip(base, dataprep.data_prepare(c, f, label, split="val", voxel_size=0.04, voxel_max=500, rand=rand,
                                                                             transform=None, shuffle=None)))
    tc, tf = t(c, f, rng=np.random.default_rng(3), generator=_gen(3))
    draws = t.last_draws
    want = dataprep.data_prepare(tc, tf, label, split="val", voxel_size=0.04, voxel_max=500, rand=rand)
    perm = torch.randperm(500, generator=torch.Generator().manual_seed(0))
    got = dataprep.data_prepare(c, f, label, split="val", voxel_size=0.04, voxel_max=500, rand=rand,
                                transform=lambda a, b: t(a, b, draws=draws), shuffle=perm)
    # the shuffle comes before the last shift to the minimum, which does not depend on the order
    assert all(torch.equal(g, w[perm.cuda()]) for g, w in zip(got, want))
    drawn = dataprep.data_prepare(c, f, label, split="val", voxel_size=0.04, voxel_max=500, rand=rand, shuffle=True)
    plain = dataprep.data_prepare(c, f, label, split="val", voxel_size=0.04, voxel_max=500, rand=rand)
    assert torch.equal(drawn[2].sort()[0], plain[2].sort()[0]) and drawn[0].shape == plain[0].shape
    with pytest.raises(ValueError, match="permutation"):
        dataprep.data_prepare(c, f, label, split="val", voxel_size=0.04, voxel_max=500, shuffle=perm[:10])
