// The clean-up of every box support on the device: what `instantiation_eval` does to a support before it returns it
// (util/train_utils.py:716-723: Open3D's voxel_down_sample(0.04), then remove_radius_outlier(nb_points=3, radius=0.1); a support left
// empty is dropped).  stratified_transformer_amd/cluster.py: clean_supports drives the three kernels here and owns every buffer.
//
// Rules, per object o and independent of every other object (tests/supports_oracle.py restates them without keys or grids):
//   1. origin = double(lo[o]) - voxel * 0.5 per axis, lo[o] the object's own componentwise minimum (label_boxes wrote it: boxes.hip);
//      v = floor((double(p) - origin) / voxel) per axis.  float64, a true division, as cell_coord of dbscan.hip.
//   2. every occupied voxel gives one point: the float64 sum of its points in ascending ORIGINAL index, from 0.0, divided by their number
//      as a double, rounded once to fp32.
//   3. a mean is kept when MORE than nb_points means of its object (itself included) lie at d2 < r2 (strict): fp32,
//      d2 = ((dx*dx) + (dy*dy)) + (dz*dz), for_each_in_reach<false> of radius_grid.h.
//
// Shape: a store pass plus a per-destination sum pass - no float atomics, so the means do not depend on the order in which threads run.
//   keys:  one thread per point, key = ((o * nz + vz) * ny + vy) * nx + vx; a point outside every object gets the largest key.  nx, ny,
//          nz are the same for all objects (the host takes them from the scene's box: no object is wider than the scene).
//   sort:  the caller's stable sort (torch) - inside a voxel the points stay in original order, which is rule 2's order of summation.
//   means: one thread per SORTED position; the thread of a voxel's first position (its key differs from its predecessor's) walks the
//          run, sums, divides, rounds and stores into the voxel's slot (slot = number of heads before it, the caller's scan).  A run is a
//          handful of points on real data (at most 4 on the golden scenes).  A run of thousands, from a degenerate cloud, is walked
//          by ONE thread: correct, and slow - there is no second path for it.
//   count: behind dbscan.hip's key and prepare kernels run on the means with group = object: one thread per mean in grid order, no LDS,
//          no early exit (a mean has a few dozen candidates at this density); keep = count > nb_points goes through the original index.
// No kernel waits on another workgroup; ranges are clamped, indices and slots checked, nothing is followed outside its array.
#include "radius_grid.h"

namespace p2 {
namespace {

constexpr long long SP_NO_KEY = 0x7fffffffffffffffLL;

struct SpGrid {
    double voxel;
    int nx, ny, nz;
};

__device__ __forceinline__ int voxel_coord(float x, float lo, double voxel, int n) {
    const double origin = (double)lo - voxel * 0.5;
    double t = floor(((double)x - origin) / voxel);
    t = t >= 0.0 ? t : 0.0;  // (x >= lo, so t >= 0 and t <= n - 1 by the host's choice of n: the clamps only keep the key in range)
    t = t <= (double)(n - 1) ? t : (double)(n - 1);
    return (int)t;
}

__global__ __launch_bounds__(RG_BLOCK) void supports_keys_kernel(int n, int n_objects, const float *__restrict__ xyz,
                                                                 const int *__restrict__ obj, const float *__restrict__ lo, SpGrid gr,
                                                                 long long *__restrict__ keys) {
    const int i = blockIdx.x * RG_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int o = obj[i];
    long long key = SP_NO_KEY;
    if ((unsigned)o < (unsigned)n_objects) {
        const float *l3 = lo + (size_t)o * 3;
        const int vx = voxel_coord(xyz[(size_t)i * 3 + 0], l3[0], gr.voxel, gr.nx);
        const int vy = voxel_coord(xyz[(size_t)i * 3 + 1], l3[1], gr.voxel, gr.ny);
        const int vz = voxel_coord(xyz[(size_t)i * 3 + 2], l3[2], gr.voxel, gr.nz);
        key = (((long long)o * gr.nz + vz) * gr.ny + vy) * gr.nx + vx;
    }
    keys[i] = key;
}

__global__ __launch_bounds__(RG_BLOCK) void supports_means_kernel(int n, int n_valid, int n_voxels, const float *__restrict__ xyz,
                                                                  const int *__restrict__ obj, const long long *__restrict__ skeys,
                                                                  const long long *__restrict__ order, const long long *__restrict__ slot,
                                                                  float *__restrict__ mean, int *__restrict__ mean_object,
                                                                  int *__restrict__ mean_size) {
    const int p = blockIdx.x * RG_BLOCK + threadIdx.x;
    if (p >= n_valid) return;
    const long long key = skeys[p];
    if (p > 0 && skeys[p - 1] == key) return;  // not the head of its run
    const long long s = slot[p];
    if (s < 0 || s >= n_voxels) return;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    int count = 0, o = -1;
    for (int q = p; q < n_valid && skeys[q] == key; q++) {
        long long i = order[q];
        i = i < 0 ? 0 : i >= n ? n - 1 : i;  // (a permutation of [0, n): never followed outside xyz whatever it holds)
        if (q == p) o = obj[i];
        sx += (double)xyz[(size_t)i * 3 + 0];
        sy += (double)xyz[(size_t)i * 3 + 1];
        sz += (double)xyz[(size_t)i * 3 + 2];
        count++;
    }
    const double c = (double)count;
    mean[(size_t)s * 3 + 0] = (float)(sx / c);
    mean[(size_t)s * 3 + 1] = (float)(sy / c);
    mean[(size_t)s * 3 + 2] = (float)(sz / c);
    mean_object[s] = o;
    mean_size[s] = count;
}

__global__ __launch_bounds__(RG_BLOCK) void supports_count_kernel(int n_means, const float4 *__restrict__ pts, const int *__restrict__ ranges,
                                                                  float r2, int nb_points, unsigned char *__restrict__ keep) {
    const int p = blockIdx.x * RG_BLOCK + threadIdx.x;
    if (p >= n_means) return;
    int count = 0;
    for_each_in_reach<false>(p, n_means, pts, ranges, r2, [&](int, int) { count++; });
    const int i = __float_as_int(pts[p].w);
    if ((unsigned)i < (unsigned)n_means) keep[i] = count > nb_points;
}

}  // namespace
}  // namespace p2

using namespace p2;

extern "C" {

void pointops2_supports_keys_launcher(int n, int n_objects, const float *xyz, const int *object, const float *lo, double voxel, int nx, int ny,
                                      int nz, long long *keys) {
    const hipStream_t st = begin_launch().stream;
    if (n < 0) { set_error("supports_keys: need n >= 0"); return; }
    if (n == 0) return;
    if (n_objects < 1 || nx < 1 || ny < 1 || nz < 1 || !(voxel > 0.0)) { set_error("supports_keys: need n_objects, nx, ny, nz >= 1 and voxel > 0"); return; }
    if ((double)n_objects * nx * ny * nz >= 4.0e18) { set_error("supports_keys: n_objects * nx * ny * nz does not fit the 64-bit voxel keys"); return; }
    if (xyz == nullptr || object == nullptr || lo == nullptr || keys == nullptr) { set_error("supports_keys: a NULL array"); return; }
    const SpGrid gr{voxel, nx, ny, nz};
    hipLaunchKernelGGL(supports_keys_kernel, dim3(div_up(n, RG_BLOCK)), dim3(RG_BLOCK), 0, st, n, n_objects, xyz, object, lo, gr, keys);
    check_launch();
}

void pointops2_supports_means_launcher(int n, int n_valid, int n_voxels, const float *xyz, const int *object, const long long *sorted_keys,
                                       const long long *order, const long long *slot, float *mean, int *mean_object, int *mean_size) {
    const hipStream_t st = begin_launch().stream;
    if (n < 0 || n_valid < 0 || n_valid > n || n_voxels < 0 || n_voxels > n_valid) { set_error("supports_means: need 0 <= n_voxels <= n_valid <= n"); return; }
    if (n_valid == 0 || n_voxels == 0) return;
    if (xyz == nullptr || object == nullptr || sorted_keys == nullptr || order == nullptr || slot == nullptr || mean == nullptr ||
        mean_object == nullptr || mean_size == nullptr) { set_error("supports_means: a NULL array"); return; }
    hipLaunchKernelGGL(supports_means_kernel, dim3(div_up(n_valid, RG_BLOCK)), dim3(RG_BLOCK), 0, st, n, n_valid, n_voxels, xyz, object,
                       sorted_keys, order, slot, mean, mean_object, mean_size);
    check_launch();
}

void pointops2_supports_count_launcher(int n_means, const float *pts, const int *ranges, float r2, int nb_points, unsigned char *keep) {
    const hipStream_t st = begin_launch().stream;
    if (n_means < 0 || nb_points < 0) { set_error("supports_count: need n_means, nb_points >= 0"); return; }
    if (n_means == 0) return;
    if (pts == nullptr || ranges == nullptr || keep == nullptr) { set_error("supports_count: a NULL array"); return; }
    hipLaunchKernelGGL(supports_count_kernel, dim3(div_up(n_means, RG_BLOCK)), dim3(RG_BLOCK), 0, st, n_means,
                       reinterpret_cast<const float4 *>(pts), ranges, r2, nb_points, keep);
    check_launch();
}

}  // extern "C"
