// DBSCAN on the device: the clustering step behind the model (util/train_utils.py:549-566 runs sklearn.cluster.DBSCAN per predicted
// class on the host).  A fixed-radius neighbour search on a uniform grid, then connected components over the core points.
//
// Rules (scikit-learn's result, restated so that no thread depends on the order in which others run):
//   1. j is a neighbour of i when both are in the same group and d2(i, j) <= eps2[group]; i is its own neighbour.
//   2. i is a core point when it has at least min_samples[group] neighbours.
//   3. clusters = connected components of the core points under 1, numbered per group in ascending order of their smallest core index.
//   4. a non-core point with a core neighbour takes the smallest cluster number among its core neighbours; all other points get -1.
// Arithmetic, fixed so that tests/dbscan_oracle.py reproduces it bit for bit: fp32, dx = xi - xj, d2 = ((dx*dx) + (dy*dy)) + (dz*dz),
// every operation rounded on its own (the library is built with -ffp-contract=off), compared with eps2 = eps * eps rounded once.
// (xi - xj) and (xj - xi) differ in sign only, so the relation is symmetric.
//
// Grid and walk: radius_grid.h (the cells, the keys, the nine prepared runs per point and the one-thread-per-point walk over them, shared
// with contacts.hip and boxes.hip).  The key and prepare kernels that build the grid are here; the three walks below (count, hook,
// label) are for_each_in_reach<true> with eps2 of the point's group.
//
// Components.  parent[] lives in ORIGINAL index space (parent[i] <= i always, -1 for a non-core point), so a root is the smallest
// core index of its tree and rule 3's numbering needs no second pass.  A round is two kernels:
//   hook: every core point reads parent[] of its core neighbours; where the two labels differ, atomicMin(&parent[larger], smaller).
//         Links only ever point to smaller indices: no cycles, and every kernel ends on its own - no waiting on another thread.
//   jump: every core point follows its chain to the root (strictly descending, so bounded) and stores the root.
// After a jump every label is a root, and every tree with an edge to another tree is merged in the next hook (it hooks, or is
// hooked to), so the number of trees at least halves per round: log2(n) rounds and one that reports no change, where plain
// neighbour-to-neighbour propagation would need as many rounds as the longest chain has points.  The host reads `changed` back once
// per round and caps the rounds (cluster.py).  The final labels are unique minima, so they do not depend on thread order.
#include "radius_grid.h"

namespace p2 {
namespace {

constexpr long long DB_NO_KEY = 0x7fffffffffffffffLL;

struct DbGrid {
    double ox, oy, oz, cell;
    int nx, ny, nz;
};

__device__ __forceinline__ int cell_coord(float x, double origin, double cell, int n) {
    double t = floor(((double)x - origin) / cell);
    t = t >= 0.0 ? t : 0.0;  // (a NaN lands here too; the host rejects non-finite coordinates before any launch)
    t = t <= (double)(n - 1) ? t : (double)(n - 1);
    return (int)t;
}

__global__ __launch_bounds__(RG_BLOCK) void dbscan_keys_kernel(int n, int n_groups, const float *__restrict__ xyz,
                                                               const int *__restrict__ group, DbGrid gr, long long *__restrict__ keys) {
    const int i = blockIdx.x * RG_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int g = group[i];
    long long key = DB_NO_KEY;
    if ((unsigned)g < (unsigned)n_groups) {
        const int cx = cell_coord(xyz[(size_t)i * 3 + 0], gr.ox, gr.cell, gr.nx);
        const int cy = cell_coord(xyz[(size_t)i * 3 + 1], gr.oy, gr.cell, gr.ny);
        const int cz = cell_coord(xyz[(size_t)i * 3 + 2], gr.oz, gr.cell, gr.nz);
        key = (((long long)g * gr.nz + cz) * gr.ny + cy) * gr.nx + cx;
    }
    keys[i] = key;
}

// first position in skeys[0, n) whose key is >= k (upper = false) or > k (upper = true), searched from `lo`
__device__ __forceinline__ int key_bound(const long long *__restrict__ skeys, int lo, int n, long long k, bool upper) {
    int hi = n;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        const long long v = skeys[mid];
        if (upper ? v <= k : v < k) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(RG_BLOCK) void dbscan_prepare_kernel(int n, int n_valid, int nx, int ny, int nz, const float *__restrict__ xyz,
                                                                  const long long *__restrict__ skeys, const long long *__restrict__ order,
                                                                  float4 *__restrict__ pts, int *__restrict__ sgroup,
                                                                  int *__restrict__ ranges) {
    const int p = blockIdx.x * RG_BLOCK + threadIdx.x;
    if (p >= n_valid) return;
    long long i = order[p];
    i = i < 0 ? 0 : i >= n ? n - 1 : i;  // (a permutation of [0, n): never followed outside xyz whatever it holds)
    pts[p] = make_float4(xyz[(size_t)i * 3 + 0], xyz[(size_t)i * 3 + 1], xyz[(size_t)i * 3 + 2], __int_as_float((int)i));
    const long long key = skeys[p];
    const int cx = (int)(key % nx);
    long long t = key / nx;
    const int cy = (int)(t % ny);
    t /= ny;
    const int cz = (int)(t % nz);
    const long long g = t / nz;
    sgroup[p] = (int)g;
    const int x0 = cx > 0 ? cx - 1 : 0, x1 = cx < nx - 1 ? cx + 1 : nx - 1;
#pragma unroll
    for (int r = 0; r < RG_ROWS; r++) {
        const int y = cy + r % 3 - 1, z = cz + r / 3 - 1;
        int lo = 0, hi = 0;
        if (y >= 0 && y < ny && z >= 0 && z < nz) {
            const long long base = ((g * nz + z) * ny + y) * nx;
            lo = key_bound(skeys, 0, n_valid, base + x0, false);
            hi = key_bound(skeys, lo, n_valid, base + x1, true);
        }
        ranges[(size_t)(2 * r) * n_valid + p] = lo;
        ranges[(size_t)(2 * r + 1) * n_valid + p] = hi;
    }
}

__global__ __launch_bounds__(RG_BLOCK) void dbscan_core_kernel(int n, int n_valid, const float4 *__restrict__ pts,
                                                               const int *__restrict__ sgroup, const int *__restrict__ ranges,
                                                               const float *__restrict__ eps2, const int *__restrict__ min_samples,
                                                               unsigned char *__restrict__ core_s, unsigned char *__restrict__ core,
                                                               int *__restrict__ parent) {
    const int p = blockIdx.x * RG_BLOCK + threadIdx.x;
    if (p >= n_valid) return;
    const int g = sgroup[p], i = __float_as_int(pts[p].w);
    int count = 0;
    for_each_in_reach<true>(p, n_valid, pts, ranges, eps2[g], [&](int, int) { count++; });
    const bool is_core = count >= min_samples[g];
    core_s[p] = is_core;
    if ((unsigned)i < (unsigned)n) {
        core[i] = is_core;
        parent[i] = is_core ? i : -1;
    }
}

__global__ __launch_bounds__(RG_BLOCK) void dbscan_hook_kernel(int n, int n_valid, const float4 *__restrict__ pts,
                                                               const int *__restrict__ sgroup, const int *__restrict__ ranges,
                                                               const float *__restrict__ eps2, const unsigned char *__restrict__ core_s,
                                                               int *parent, int *changed) {
    const int p = blockIdx.x * RG_BLOCK + threadIdx.x;
    if (p >= n_valid || !core_s[p]) return;
    const int i = __float_as_int(pts[p].w);
    if ((unsigned)i >= (unsigned)n) return;
    int mine = parent[i];
    bool hooked = false;
    for_each_in_reach<true>(p, n_valid, pts, ranges, eps2[sgroup[p]], [&](int q, int j) {
        if (!core_s[q] || (unsigned)j >= (unsigned)n) return;
        const int theirs = parent[j];
        if (theirs == mine || (unsigned)theirs >= (unsigned)n || (unsigned)mine >= (unsigned)n) return;
        const int lo = min(mine, theirs), hi = max(mine, theirs);
        atomicMin(&parent[hi], lo);
        mine = lo;
        hooked = true;
    });
    if (hooked) *changed = 1;
}

__global__ __launch_bounds__(RG_BLOCK) void dbscan_jump_kernel(int n, int *parent) {
    const int i = blockIdx.x * RG_BLOCK + threadIdx.x;
    if (i >= n) return;
    int x = parent[i];
    if ((unsigned)x >= (unsigned)n) return;  // not a core point
    for (int step = 0; step < n; step++) {   // strictly descending: ends at a root after fewer than n steps
        const int y = parent[x];
        if (y == x || (unsigned)y >= (unsigned)n) break;
        x = y;
    }
    parent[i] = x;
}

__global__ __launch_bounds__(RG_BLOCK) void dbscan_label_kernel(int n, int n_valid, const float4 *__restrict__ pts,
                                                                const int *__restrict__ sgroup, const int *__restrict__ ranges,
                                                                const float *__restrict__ eps2, const unsigned char *__restrict__ core_s,
                                                                const int *__restrict__ parent, const int *__restrict__ cluster_of_root,
                                                                int *__restrict__ labels) {
    const int p = blockIdx.x * RG_BLOCK + threadIdx.x;
    if (p >= n_valid) return;
    const int i = __float_as_int(pts[p].w);
    if ((unsigned)i >= (unsigned)n) return;
    int label = -1;
    if (core_s[p]) {
        const int root = parent[i];
        if ((unsigned)root < (unsigned)n) label = cluster_of_root[root];
    } else {
        int best = 0x7fffffff;
        for_each_in_reach<true>(p, n_valid, pts, ranges, eps2[sgroup[p]], [&](int q, int j) {
            if (!core_s[q] || (unsigned)j >= (unsigned)n) return;
            const int root = parent[j];
            if ((unsigned)root >= (unsigned)n) return;
            const int c = cluster_of_root[root];
            if (c >= 0 && c < best) best = c;
        });
        if (best != 0x7fffffff) label = best;
    }
    labels[i] = label;
}

const char *dbscan_bad_counts(int n, int n_valid) {
    if (n < 0 || n_valid < 0 || n_valid > n) return "dbscan: need 0 <= n_valid <= n";
    return nullptr;
}

}  // namespace
}  // namespace p2

using namespace p2;

extern "C" {

void pointops2_dbscan_keys_launcher(int n, int n_groups, const float *xyz, const int *group, double ox, double oy, double oz, double cell,
                                    int nx, int ny, int nz, long long *keys) {
    const hipStream_t st = begin_launch().stream;
    if (n <= 0) return;
    if (n_groups < 1 || nx < 1 || ny < 1 || nz < 1 || !(cell > 0.0)) { set_error("dbscan_keys: need n_groups, nx, ny, nz >= 1 and cell > 0"); return; }
    if ((double)n_groups * nx * ny * nz >= 4.0e18) { set_error("dbscan_keys: n_groups * nx * ny * nz does not fit the 64-bit cell keys"); return; }
    const DbGrid gr{ox, oy, oz, cell, nx, ny, nz};
    hipLaunchKernelGGL(dbscan_keys_kernel, dim3(div_up(n, RG_BLOCK)), dim3(RG_BLOCK), 0, st, n, n_groups, xyz, group, gr, keys);
    check_launch();
}

void pointops2_dbscan_prepare_launcher(int n, int n_valid, int nx, int ny, int nz, const float *xyz, const long long *sorted_keys,
                                       const long long *order, float *pts, int *sorted_group, int *ranges) {
    const hipStream_t st = begin_launch().stream;
    if (const char *bad = dbscan_bad_counts(n, n_valid)) { set_error(bad); return; }
    if (n_valid == 0) return;
    if (nx < 1 || ny < 1 || nz < 1) { set_error("dbscan_prepare: need nx, ny, nz >= 1"); return; }
    hipLaunchKernelGGL(dbscan_prepare_kernel, dim3(div_up(n_valid, RG_BLOCK)), dim3(RG_BLOCK), 0, st, n, n_valid, nx, ny, nz, xyz, sorted_keys,
                       order, reinterpret_cast<float4 *>(pts), sorted_group, ranges);
    check_launch();
}

void pointops2_dbscan_core_launcher(int n, int n_valid, const float *pts, const int *sorted_group, const int *ranges, const float *eps2,
                                    const int *min_samples, unsigned char *sorted_core, unsigned char *core, int *parent) {
    const hipStream_t st = begin_launch().stream;
    if (const char *bad = dbscan_bad_counts(n, n_valid)) { set_error(bad); return; }
    if (n_valid == 0) return;
    hipLaunchKernelGGL(dbscan_core_kernel, dim3(div_up(n_valid, RG_BLOCK)), dim3(RG_BLOCK), 0, st, n, n_valid,
                       reinterpret_cast<const float4 *>(pts), sorted_group, ranges, eps2, min_samples, sorted_core, core, parent);
    check_launch();
}

void pointops2_dbscan_round_launcher(int n, int n_valid, const float *pts, const int *sorted_group, const int *ranges, const float *eps2,
                                     const unsigned char *sorted_core, int *parent, int *changed) {
    const hipStream_t st = begin_launch().stream;
    if (const char *bad = dbscan_bad_counts(n, n_valid)) { set_error(bad); return; }
    if (hipMemsetAsync(changed, 0, sizeof(int), st) != hipSuccess) { check_launch(); return; }
    if (n_valid == 0) return;
    hipLaunchKernelGGL(dbscan_hook_kernel, dim3(div_up(n_valid, RG_BLOCK)), dim3(RG_BLOCK), 0, st, n, n_valid,
                       reinterpret_cast<const float4 *>(pts), sorted_group, ranges, eps2, sorted_core, parent, changed);
    hipLaunchKernelGGL(dbscan_jump_kernel, dim3(div_up(n, RG_BLOCK)), dim3(RG_BLOCK), 0, st, n, parent);
    check_launch();
}

void pointops2_dbscan_label_launcher(int n, int n_valid, const float *pts, const int *sorted_group, const int *ranges, const float *eps2,
                                     const unsigned char *sorted_core, const int *parent, const int *cluster_of_root, int *labels) {
    const hipStream_t st = begin_launch().stream;
    if (const char *bad = dbscan_bad_counts(n, n_valid)) { set_error(bad); return; }
    if (n_valid == 0) return;
    hipLaunchKernelGGL(dbscan_label_kernel, dim3(div_up(n_valid, RG_BLOCK)), dim3(RG_BLOCK), 0, st, n, n_valid,
                       reinterpret_cast<const float4 *>(pts), sorted_group, ranges, eps2, sorted_core, parent, cluster_of_root, labels);
    check_launch();
}

}  // extern "C"
