"""Writes tests/golden/dbscan_sklearn.npz: scikit-learn's DBSCAN on a handful of clustered clouds, and one case of the clustering of
`instantiation_eval` (util/train_utils.py:549-566: per predicted class DBSCAN of coord + shift, the clusters with more than a
threshold of points kept).  Run on the CPU where scikit-learn is installed (1.7.2 wrote the committed file):

    python tests/golden/make_golden_dbscan.py

scikit-learn measures distances in float64, csrc/dbscan.hip in fp32.  With coordinates in [0, 4) and eps >= 0.1 the fp32 evaluation
error of a distance is about 1e-6, so every point that belongs to a pair with |dist - eps| < 1e-5 is REMOVED before anything is
recorded, and the script asserts that none is left.  This is a condition on the inputs, not a tolerance on the result.

Per cloud k: xyz_k [n, 3] f32, eps_k, min_samples_k, labels_k (DBSCAN.labels_), core_k (DBSCAN.core_sample_indices_).
The instances case: inst_coord, inst_shift [n, 3] f32, inst_pred [n] (classes 0..7, classes 3 and 6 empty), inst_eps / inst_min_samples
/ inst_min_points [8] (the reference's settings), inst_instance [n] (the position of the point's instance in the reference's
class-major list of lists, -1 = in none), inst_class / inst_size [I], inst_per_class [8] (instances per class)."""
import os

import numpy as np
from sklearn.cluster import DBSCAN

MARGIN = 1e-5
HERE = os.path.dirname(os.path.abspath(__file__))
CLOUDS = [(257, 0.1, 5), (600, 0.15, 3), (900, 0.2, 5), (1200, 0.12, 4), (431, 0.1, 5)]  # points before the removal, eps, min_samples


def near_threshold(x32, eps):
    """indices of the points that belong to a pair with |dist - eps| < MARGIN (float64 distances of the fp32 coordinates)"""
    x = x32.astype(np.float64)
    d = np.sqrt(((x[:, None, :] - x[None, :, :]) ** 2).sum(-1))
    i, j = np.nonzero(np.abs(d - float(eps)) < MARGIN)
    return np.unique(np.concatenate([i, j]))


def blobs(rng, n, n_blobs, sigma, noise_frac=0.1):
    centres = rng.uniform(0.6, 3.4, (n_blobs, 3))
    n_noise = int(n * noise_frac)
    which = rng.integers(0, n_blobs, n - n_noise)
    pts = centres[which] + rng.normal(0, 1, (n - n_noise, 3)) * sigma * rng.uniform(0.6, 1.6, (n_blobs, 1))[which]
    pts = np.concatenate([pts, rng.uniform(0, 4, (n_noise, 3))])
    pts = np.clip(pts, 0, 3.999)[rng.permutation(n)]
    return pts.astype(np.float32)


def main():
    out = {}
    rng = np.random.default_rng(20261018)
    for k, (n, eps, min_samples) in enumerate(CLOUDS):
        xyz = blobs(rng, n + 8, 10, 0.5 * eps)
        xyz = np.delete(xyz, near_threshold(xyz, np.float32(eps)), 0)[:n]
        assert len(near_threshold(xyz, np.float32(eps))) == 0 and 250 <= len(xyz) <= 1200
        assert xyz.min() >= 0 and xyz.max() < 4
        fit = DBSCAN(eps=eps, min_samples=min_samples).fit(xyz.astype(np.float64))
        labels, core = fit.labels_.astype(np.int32), fit.core_sample_indices_.astype(np.int32)
        is_core = np.zeros(len(xyz), bool)
        is_core[core] = True
        print(f"cloud {k}: n {len(xyz)} eps {eps} min_samples {min_samples}: clusters {labels.max() + 1}, "
              f"border {int(((labels >= 0) & ~is_core).sum())}, noise {int((labels < 0).sum())}")
        out.update({f"xyz_{k}": xyz, f"eps_{k}": np.float64(eps), f"min_samples_{k}": np.int32(min_samples), f"labels_{k}": labels,
                    f"core_{k}": core})
    out["n_clouds"] = np.int32(len(CLOUDS))

    # ---- instantiation_eval's clustering: classes 0..7, classes 3 and 6 empty; large and small blobs (the small ones are dropped) ----
    eps_c = np.array([0.1] * 6 + [0.15] * 2)
    ms_c = np.array([5] * 6 + [3] * 2, np.int32)
    thre_c = np.array([50] * 6 + [20] * 2, np.int32)
    coord, pred = [], []
    for c in (0, 1, 2, 4, 5, 7):
        sizes = [130, 35, 90, 64] if c < 6 else [45, 12, 30, 18]
        for s in sizes:
            centre = rng.uniform(0.5, 3.5, 3)
            coord.append(centre + rng.normal(0, 0.045 if c < 6 else 0.06, (s, 3)))
            pred += [c] * s
        coord.append(rng.uniform(0, 4, (15, 3)))  # stray predictions of the class
        pred += [c] * 15
    coord, pred = np.clip(np.concatenate(coord), 0, 3.999).astype(np.float32), np.array(pred, np.int32)
    perm = rng.permutation(len(pred))
    coord, pred = coord[perm], pred[perm]
    shift = rng.normal(0, 0.01, coord.shape).astype(np.float32)
    moved = coord + shift                                             # fp32, as the device adds them
    assert moved.dtype == np.float32
    drop = np.unique(np.concatenate([np.nonzero(pred == c)[0][near_threshold(moved[pred == c], np.float32(eps_c[c]))] for c in range(8)]))
    coord, shift, pred = np.delete(coord, drop, 0), np.delete(shift, drop, 0), np.delete(pred, drop)
    moved = coord + shift
    assert all(len(near_threshold(moved[pred == c], np.float32(eps_c[c]))) == 0 for c in range(8))
    assert moved.min() >= -0.1 and moved.max() < 4.1 and set(np.unique(pred)) == {0, 1, 2, 4, 5, 7}
    # the reference's loop (:553-566) on the same arrays; a class without points has no instances (DBSCAN.fit refuses an empty array)
    instance, inst_class, inst_size, per_class = np.full(len(pred), -1, np.int32), [], [], []
    for c in range(int(pred.max()) + 1):
        rows = np.nonzero(pred == c)[0]
        kept = 0
        if len(rows):
            labels = DBSCAN(eps=eps_c[c], min_samples=int(ms_c[c])).fit(moved[rows].astype(np.float64)).labels_
            for j in range(labels.max() + 1):
                if int((labels == j).sum()) > thre_c[c]:
                    instance[rows[labels == j]] = len(inst_class)
                    inst_class.append(c)
                    inst_size.append(int((labels == j).sum()))
                    kept += 1
            print(f"class {c}: {len(rows)} points, {labels.max() + 1} clusters, {kept} kept")
        per_class.append(kept)
    out.update(inst_coord=coord, inst_shift=shift, inst_pred=pred, inst_eps=eps_c, inst_min_samples=ms_c, inst_min_points=thre_c,
               inst_instance=instance, inst_class=np.array(inst_class, np.int32), inst_size=np.array(inst_size, np.int32),
               inst_per_class=np.array(per_class, np.int32))
    path = os.path.join(HERE, "dbscan_sklearn.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
