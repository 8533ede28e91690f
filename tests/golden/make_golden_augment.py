"""Golden vectors of the train-time transforms, produced by EXECUTING THE REFERENCE'S OWN numpy / scipy code (build container
only; nothing of the reference is copied):

  util/transform.py    Compose, RandomRotate, RandomRotatePerturbation, RandomScale, RandomShift, RandomJitter, RandomDropColor,
                       ElasticDistortion, RandomHorizontalFlip, ChromaticAutoContrast, ChromaticTranslation, ChromaticJitter,
                       HueSaturationTranslation - every class alone (tests/augment_cases.py: SINGLE) and in the two chains
                       (CHAINS: the S3DIS training chain and a full chain) on every scene of a three-scene batch.

While the reference runs, its random decisions are RECORDED and stored with the results, so that the oracle and the device can
replay them: `np.random.uniform / randn / rand` and `random.random` are wrapped.  A case may FORCE the leading values of
`random.random()` and of the argument-less `np.random.rand()` - the gates - so that every gate is seen open and shut; a forced
value is a valid draw of the reference.  `scipy.interpolate.RegularGridInterpolator` is wrapped to keep the grid the reference
hands it: the noise after scipy.ndimage's own six box filters (stored as blur<j>).
An output equal to its input bit for bit is not stored (the test then expects the input).

    python tests/golden/make_golden_augment.py   ->  tests/golden/augment_reference.npz
"""
import os
import random
import sys

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))

# tests/augment_cases.py, loaded by path: tests/ must stay off sys.path here, its util.py would hide the reference's util package
import importlib.util  # noqa: E402
_spec = importlib.util.spec_from_file_location("augment_cases", os.path.join(os.path.dirname(HERE), "augment_cases.py"))
cases = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(cases)


class Recorded:
    """recorded (and, for the gates, forced) draws while the reference executes"""

    def __init__(self, forced):
        self.log, self.forced, self.grids = [], list(forced), []

    def __enter__(self):
        import scipy.interpolate
        self._np = {k: getattr(np.random, k) for k in ("uniform", "randn", "rand")}
        self._random, self._rgi = random.random, scipy.interpolate.RegularGridInterpolator

        def wrap(kind, fn, gate):
            def call(*args, **kw):
                r = self.forced.pop(0) if gate(args) and self.forced else fn(*args, **kw)
                self.log.append((kind, np.array(r, copy=True)))
                return r
            return call
        for k, fn in self._np.items():
            setattr(np.random, k, wrap(k, fn, (lambda a: not a) if k == "rand" else (lambda a: False)))
        random.random = wrap("random", self._random, lambda a: True)

        def rgi(points, values, *args, **kw):
            self.grids.append(np.array(values, copy=True))
            return self._rgi(points, values, *args, **kw)
        scipy.interpolate.RegularGridInterpolator = rgi
        return self

    def __exit__(self, *exc):
        import scipy.interpolate
        for k, fn in self._np.items():
            setattr(np.random, k, fn)
        random.random, scipy.interpolate.RegularGridInterpolator = self._random, self._rgi


def draws_of(name, kw, log, grids):
    """this transform's share of the log, under the names tests/augment_oracle.py reads"""
    def take(kind):
        got, v = log.pop(0)
        assert got == kind, (name, got, kind)
        return v
    d = {}
    if name == "RandomRotate":
        if kw.get("rotate_angle") is None:
            d["u"] = take("uniform")
    elif name == "RandomRotatePerturbation":
        d["randn"] = take("randn")
    elif name == "RandomScale":
        d["scale"] = take("uniform")
    elif name == "RandomShift":
        d["shift"] = take("uniform")
    elif name == "RandomJitter":
        d["noise"] = take("randn")
    elif name == "RandomDropColor":
        d["u"] = take("rand")
    elif name == "ElasticDistortion":
        d["gate"] = take("random")
        if d["gate"] < 0.95:
            for j in range(len(kw["distortion_params"])):
                d[f"noise{j}"] = take("randn").astype(np.float32)
                d[f"blur{j}"] = grids.pop(0)
                assert d[f"blur{j}"].dtype == np.float32
    elif name == "RandomHorizontalFlip":
        d["gate"] = take("random")
        d["axes"] = np.array([take("random"), take("random")]) if d["gate"] < 0.95 else np.ones(2)
    elif name == "ChromaticAutoContrast":
        d["gate"] = take("random")
        d["blend"] = take("random") if d["gate"] < 0.2 and kw.get("randomize_blend_factor", True) else np.array(0.0)
    elif name == "ChromaticTranslation":
        d["gate"] = take("random")
        d["u"] = take("rand").reshape(3) if d["gate"] < 0.95 else np.zeros(3)
    elif name == "ChromaticJitter":
        d["gate"] = take("random")
        if d["gate"] < 0.95:
            d["noise"] = take("randn")
    elif name == "HueSaturationTranslation":
        d["hue_u"], d["sat_u"] = take("random"), take("random")
    else:
        raise KeyError(name)
    return d


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def run(T, chain, coord, feat, forced, out, prefix):
    """execute the reference's chain on copies; store the outputs that changed and the draws"""
    ts = []
    for name, kw in chain:
        kw = {k: v for k, v in kw.items() if k != "normals"}
        ts.append(getattr(T, name)(**kw))
    normals = any(kw.get("normals") for _, kw in chain)
    with Recorded(forced) as rec:
        if normals:  # the reference's form of the option: a [N, 6] array whose columns 3:6 are rotated too
            data, _ = T.Compose(ts)(np.concatenate([coord, feat], 1), None)
            c, f = data[:, 0:3], data[:, 3:6]
        else:
            c, f = T.Compose(ts)(coord.copy(), feat.copy())
    assert not rec.forced, (prefix, rec.forced)
    log = list(rec.log)
    for k, (name, kw) in enumerate(chain):
        for key, v in draws_of(name, kw, log, rec.grids).items():
            out[f"{prefix}.d{k}.{key}"] = np.asarray(v)
    assert not log and not rec.grids, prefix
    assert c.dtype == np.float64 and f.dtype == np.float64
    if not same(c, coord):
        out[prefix + ".coord"] = np.ascontiguousarray(c)
    if not same(f, feat):
        out[prefix + ".feat"] = np.ascontiguousarray(f)


def main():
    sys.path.insert(0, REF)
    from util import transform as T  # the reference
    out = {}
    coord, feat = cases.cloud(300, 21)
    const = feat.copy()
    const[:, 1] = const[0, 1]
    inputs = {"base": feat, "const": const, "narrow": cases.narrow(feat)}
    out["base.coord"] = coord
    for k, v in inputs.items():
        out[k + ".feat"] = v
    np.random.seed(17)
    random.seed(18)
    for case, name, kw, which, forced in cases.SINGLE:
        run(T, [(name, kw)], coord, inputs[which], forced, out, case)
    scenes = [cases.cloud(n, 30 + i) for i, n in enumerate(cases.BATCH_SIZES)]
    scenes = [(c, cases.narrow(f)) for c, f in scenes]
    out["batch.coord"] = np.concatenate([s[0] for s in scenes])
    out["batch.feat"] = np.concatenate([s[1] for s in scenes])
    out["batch.offset"] = np.cumsum(cases.BATCH_SIZES).astype(np.int32)
    for chain_name, (chain, forced) in cases.CHAINS.items():
        for s, (c, f) in enumerate(scenes):
            run(T, chain, c, f, forced[s], out, f"{chain_name}.s{s}")
    path = os.path.join(HERE, "augment_reference.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, len(out), "arrays,", round(os.path.getsize(path) / 1e6, 3), "MB")


if __name__ == "__main__":
    main()
