"""Oracle of csrc/dbscan.hip: numpy, brute force over all pairs, the kernel's fp32 arithmetic and the four rules.

    1. j is a neighbour of i when both are in the same group and d2(i, j) <= eps2 (i is its own neighbour), with
       d2 = ((dx*dx) + (dy*dy)) + (dz*dz), dx = xi - xj, every operation rounded to fp32, eps2 = fp32(eps) * fp32(eps) rounded once;
    2. i is a core point when it has at least min_samples neighbours;
    3. clusters = connected components of the core points, numbered per group by ascending smallest core index;
    4. a non-core point with a core neighbour takes the smallest cluster number among its core neighbours; every other point gets -1.

scikit-learn is not imported here: tests/golden/dbscan_sklearn.npz holds its results (tests/golden/make_golden_dbscan.py)."""
import numpy as np

ROWS = 512  # rows of the pair matrix evaluated at a time


def adjacency(xyz, eps):
    """bool [n, n]: rule 1 inside one group"""
    x = np.ascontiguousarray(xyz, dtype=np.float32)
    eps = np.float32(eps)
    eps2 = np.float32(eps * eps)
    n = x.shape[0]
    adj = np.zeros((n, n), dtype=bool)
    for r0 in range(0, n, ROWS):
        d = x[r0:r0 + ROWS, None, :] - x[None, :, :]                      # fp32 differences
        sq = d * d                                                        # fp32 products, rounded before they are summed
        d2 = (sq[..., 0] + sq[..., 1]) + sq[..., 2]
        assert d2.dtype == np.float32
        adj[r0:r0 + ROWS] = d2 <= eps2
    return adj


def _find(parent, i):
    root = i
    while parent[root] != root:
        root = parent[root]
    while parent[i] != root:
        parent[i], i = root, parent[i]
    return root


def dbscan_one(xyz, eps, min_samples):
    """one group -> (labels int32 [n], core bool [n], number of clusters)"""
    n = len(xyz)
    labels = np.full(n, -1, dtype=np.int32)
    if n == 0:
        return labels, np.zeros(0, dtype=bool), 0
    adj = adjacency(xyz, eps)
    assert np.array_equal(adj, adj.T) and adj.diagonal().all()           # symmetric by construction, a point is its own neighbour
    core = adj.sum(1) >= int(min_samples)
    parent = np.arange(n)
    ii, jj = np.nonzero(np.triu(adj & core[:, None] & core[None, :], 1))
    for i, j in zip(ii.tolist(), jj.tolist()):
        a, b = _find(parent, i), _find(parent, j)
        if a != b:
            parent[max(a, b)] = min(a, b)                                 # the root is the smallest index of its component
    core_idx = np.nonzero(core)[0]
    root = np.array([_find(parent, i) for i in core_idx.tolist()], dtype=np.int64)
    roots = np.unique(root)                                               # ascending smallest core index
    labels[core_idx] = np.searchsorted(roots, root)
    for i in np.nonzero(~core)[0].tolist():
        near = adj[i] & core
        if near.any():
            labels[i] = labels[near].min()
    return labels, core, len(roots)


def dbscan(xyz, eps, min_samples, group=None, n_groups=None):
    """-> (labels int32 [N], core bool [N], n_clusters int32 [G]), as stratified_transformer_amd.cluster.dbscan defines them"""
    xyz = np.asarray(xyz, dtype=np.float32)
    n = len(xyz)
    group = np.zeros(n, dtype=np.int64) if group is None else np.asarray(group).astype(np.int64)
    if n_groups is None:
        n_groups = max(np.ndim(eps) and len(eps), np.ndim(min_samples) and len(min_samples), int(group.max()) + 1 if n else 1, 1)
    eps = np.broadcast_to(np.asarray(eps, dtype=np.float32), (n_groups,))
    min_samples = np.broadcast_to(np.asarray(min_samples), (n_groups,))
    labels, core, n_clusters = np.full(n, -1, dtype=np.int32), np.zeros(n, dtype=bool), np.zeros(n_groups, dtype=np.int32)
    for g in range(n_groups):
        rows = np.nonzero(group == g)[0]
        labels[rows], core[rows], n_clusters[g] = dbscan_one(xyz[rows], eps[g], min_samples[g])
    return labels, core, n_clusters


def instances(coord, shift, pred, eps, min_samples, min_points):
    """instantiation_eval's clustering (util/train_utils.py:549-566) on the oracle: per class the clusters with MORE than min_points
    points, numbered class-major, then by cluster number -> (instance int32 [N], instance_class int32 [I], instance_size int32 [I])"""
    coord, shift = np.asarray(coord, dtype=np.float32), np.asarray(shift, dtype=np.float32)
    pred = np.asarray(pred).astype(np.int64)
    n_classes = len(eps)
    labels, _, n_clusters = dbscan(coord + shift, eps, min_samples, pred, n_classes)
    instance, classes, sizes = np.full(len(coord), -1, dtype=np.int32), [], []
    for c in range(n_classes):
        for j in range(int(n_clusters[c])):
            rows = (pred == c) & (labels == j)
            if int(rows.sum()) > int(min_points[c]):
                instance[rows] = len(classes)
                classes.append(c)
                sizes.append(int(rows.sum()))
    return instance, np.asarray(classes, dtype=np.int32), np.asarray(sizes, dtype=np.int32)
