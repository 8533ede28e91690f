// Whole-scene evaluation on the device: the crop cover and the vote of the reference's test loop (test_backup.py:238-251, :278-281).
//
// Crop cover of one part (n points, crops of voxel_max): per crop
//   seed  = argmin(priority)                      float64, the LOWEST index among equal values          (:241)
//   dist  = sum((coord - coord[seed])^2)          the coordinates' own type, left to right              (:242)
//   crop  = first voxel_max of the stable ascending sort of dist (the caller's torch sort, as dataprep.crop_nearest) (:243)
//   delta = (1 - dist[crop] / dmax)^2             dmax = dist[crop[-1]]; divide, subtract, multiply - each rounded on its own,
//   priority[crop] += (double)delta               the library is built with -ffp-contract=off             (:245-247)
// and the crop's points are marked covered (:250 keeps np.unique of everything seen so far; only its size is ever used).
// The seed never leaves the device: argmin_partial_kernel leaves one (value, index) pair per workgroup, and every workgroup of
// seed_dist_kernel reduces those pairs again in its prologue (at most ET_MAX_PARTS pairs: four per thread) - the kernel boundary
// between the two is the only ordering needed, no kernel waits on another workgroup.  update_kernel reports through two words
// that the host reads once per crop: the number of covered points so far and a status.
//
// Vote (:278, :281): pred[idx, :] += softmax(logits, -1) is an indexed assignment - when an index repeats inside one call only ONE
// row writes.  Here, as in CPU torch, it is the row at the last position: vote_stamp_kernel takes the maximum row number per
// point (integer atomicMax, order-independent), vote_add_kernel lets row r write when stamp[idx[r]] == r and resets the stamp to
// -1 for the next call.  (A losing row reads either the winner's number or -1: neither is its own.)  A row is spread over LPR
// lanes of one wave, one class per lane: the max and the sum are xor butterflies, so the result does not depend on the launch.
//
// Vote with shifts (the fork's second accumulator, test_iou.py:284-285, :337-338): `pred[idx, :] += softmax(logits)` and
// `pred_shift[idx, :] += shift` are two indexed assignments over the same idx, so one winner per point serves both.  The choice is ONE
// fused kernel, vote_shift_add_kernel, not a second small one: whether row r wins is known only while stamp[idx[r]] still holds r, and
// the winner's reset to -1 is what makes the next call work - a second kernel would either need the reset moved into it (the
// shift-less path, which must stay as it is, resets in vote_add_kernel) or a second stamp pass.  Fused, every lane of the row reads
// the stamp in one wave-wide load that precedes the reset in program order (a row never straddles a wave: LPR divides 64), and the
// row's idx and stamp are read once for both tensors.  The shift components ride on lanes 0..2 of the row: LPR is at least 8, so
// these lanes exist whatever `classes` is - `classes` of 1 or 2 leaves them without a logit (inactive in the softmax, -inf / 0 as any
// lane beyond `classes`), but they are lanes of a writer row all the same.  The softmax is vote_add_kernel's (vote_row, shared); the
// shift is converted to fp32 (exact from f16 / bf16) and added with one fp32 add.  The shift's storage type is a
// run-time argument (a wave-uniform branch around one load), so the kernel is instantiated per lane width and logit type only.
#include "row_types.h"

namespace p2 {
namespace {

constexpr int ET_BLOCK = 256;
constexpr int ET_WAVES = ET_BLOCK / WAVE;
constexpr int ET_MAX_PARTS = 1024;        // workgroups of argmin_partial_kernel = pairs the prologue of seed_dist_kernel reduces
constexpr int ET_POINTS_PER_PART = 1024;  // points per workgroup before the grid stops growing and the threads stride
constexpr int ET_NO_INDEX = 0x7fffffff;

constexpr int ET_STATUS_DMAX_ZERO = 1;    // update: dist[crop[-1]] is not positive - voxel_max points coincide with the seed
constexpr int ET_STATUS_BAD_INDEX = 2;    // update: an entry of crop is outside [0, n); vote: an entry of idx is outside [0, n_points)

inline int argmin_parts(int n) { return min(div_up(n, ET_POINTS_PER_PART), ET_MAX_PARTS); }

// (v, i) orders before (bv, bi): np.argmin's order on non-negative values - smaller value, then smaller index.  A NaN never wins.
__device__ __forceinline__ bool before(double v, int i, double bv, int bi) { return v < bv || (v == bv && i < bi); }

// the best pair of the workgroup, in every thread; `slots` holds one pair per wave
__device__ __forceinline__ void block_best(double &v, int &i, double *slot_v, int *slot_i) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const double ov = __shfl_xor(v, s, WAVE);
        const int oi = __shfl_xor(i, s, WAVE);
        if (before(ov, oi, v, i)) { v = ov; i = oi; }
    }
    if (lane_id() == 0) { slot_v[threadIdx.x / WAVE] = v; slot_i[threadIdx.x / WAVE] = i; }
    __syncthreads();
    v = slot_v[0];
    i = slot_i[0];
#pragma unroll
    for (int w = 1; w < ET_WAVES; w++)
        if (before(slot_v[w], slot_i[w], v, i)) { v = slot_v[w]; i = slot_i[w]; }
}

__global__ __launch_bounds__(ET_BLOCK) void argmin_partial_kernel(int n, const double *__restrict__ priority, double *__restrict__ part_v,
                                                                  int *__restrict__ part_i) {
    __shared__ double slot_v[ET_WAVES];
    __shared__ int slot_i[ET_WAVES];
    double v = INFINITY;
    int i = ET_NO_INDEX;
    for (int p = blockIdx.x * ET_BLOCK + threadIdx.x; p < n; p += gridDim.x * ET_BLOCK) {
        const double pv = priority[p];
        if (before(pv, p, v, i)) { v = pv; i = p; }
    }
    block_best(v, i, slot_v, slot_i);
    if (threadIdx.x == 0) { part_v[blockIdx.x] = v; part_i[blockIdx.x] = i; }
}

template <typename T>
__global__ __launch_bounds__(ET_BLOCK) void seed_dist_kernel(int n, int n_parts, const T *__restrict__ coord, const double *__restrict__ part_v,
                                                             const int *__restrict__ part_i, long long *__restrict__ seed_out,
                                                             T *__restrict__ dist) {
    __shared__ double slot_v[ET_WAVES];
    __shared__ int slot_i[ET_WAVES];
    __shared__ T rows[ET_BLOCK * 3];
    // the workgroup's 3-value rows, read as one contiguous run (a thread reading its own row strides the wave's loads by 12 / 24 bytes)
    const int base = blockIdx.x * ET_BLOCK, count = min(ET_BLOCK, n - base);
    for (int k = threadIdx.x; k < count * 3; k += ET_BLOCK) rows[k] = coord[(size_t)base * 3 + k];

    double v = INFINITY;
    int seed = ET_NO_INDEX;
    for (int p = threadIdx.x; p < n_parts; p += ET_BLOCK)
        if (before(part_v[p], part_i[p], v, seed)) { v = part_v[p]; seed = part_i[p]; }
    block_best(v, seed, slot_v, slot_i);  // (its barrier also publishes rows[])
    if ((unsigned)seed >= (unsigned)n) seed = 0;  // every priority a NaN: np.argmin answers 0
    if (blockIdx.x == 0 && threadIdx.x == 0) seed_out[0] = seed;

    if (threadIdx.x >= count) return;
    T s = 0;
#pragma unroll
    for (int a = 0; a < 3; a++) {  // np.sum(np.power(coord - coord[init_idx], 2), 1): left to right, as crop_dist_kernel
        const T d = rows[threadIdx.x * 3 + a] - coord[(size_t)seed * 3 + a];
        const T sq = d * d;
        s = a == 0 ? sq : s + sq;
    }
    dist[base + threadIdx.x] = s;
}

template <typename T>
__global__ __launch_bounds__(ET_BLOCK) void update_kernel(int n, int voxel_max, const T *__restrict__ dist, const long long *__restrict__ crop,
                                                          double *__restrict__ priority, unsigned char *__restrict__ covered,
                                                          int *__restrict__ report) {
    __shared__ int wave_new[ET_WAVES];
    const int j = blockIdx.x * ET_BLOCK + threadIdx.x;
    const long long last = crop[voxel_max - 1];
    if (last < 0 || last >= n) {  // (the same for every thread of the grid, as the next test: whole workgroups leave)
        if (j == 0) report[1] = ET_STATUS_BAD_INDEX;
        return;
    }
    const T dmax = dist[last];
    if (!(dmax > (T)0)) {
        if (j == 0) report[1] = ET_STATUS_DMAX_ZERO;
        return;
    }
    bool fresh = false;
    if (j < voxel_max) {
        const long long i = crop[j];
        if (i >= 0 && i < n) {
            const T q = dist[i] / dmax;  // np.square(1 - dist / np.max(dist)): three operations in the coordinates' type
            const T t = (T)1 - q;
            const T delta = t * t;
            priority[i] += (double)delta;  // the entries of a crop are distinct: no atomics
            fresh = covered[i] == 0;
            if (fresh) covered[i] = 1;
        } else {
            report[1] = ET_STATUS_BAD_INDEX;
        }
    }
    const int in_wave = __popcll(__ballot(fresh));
    if (lane_id() == 0) wave_new[threadIdx.x / WAVE] = in_wave;
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = 0;
#pragma unroll
        for (int w = 0; w < ET_WAVES; w++) total += wave_new[w];
        if (total > 0) atomicAdd(&report[0], total);
    }
}

__global__ __launch_bounds__(ET_BLOCK) void vote_stamp_kernel(int m, int n_points, const long long *__restrict__ idx, int *stamp,
                                                              int *__restrict__ status) {
    const int r = blockIdx.x * ET_BLOCK + threadIdx.x;
    if (r >= m) return;
    const long long i = idx[r];
    if (i < 0 || i >= n_points) { status[0] = ET_STATUS_BAD_INDEX; return; }
    atomicMax(&stamp[i], r);
}

// f(std::integral_constant<int, LPR>{}) for the lanes a row of `classes` logits takes: the power of two >= classes, at least 8
template <typename F>
void with_row_lanes(int classes, F f) {
    if (classes <= 8) f(std::integral_constant<int, 8>{});
    else if (classes <= 16) f(std::integral_constant<int, 16>{});
    else if (classes <= 32) f(std::integral_constant<int, 32>{});
    else f(std::integral_constant<int, 64>{});
}

// The vote of one row: LPR lanes per row, ET_BLOCK / LPR rows per workgroup; T: the logits' storage type (row_types.h).  Every lane
// of row r learns whether the row is the writer of its point i - before lane 0 resets the stamp, which is the kernel's last step -
// and the active lanes (class slot c < classes) add the row's softmax.
struct VoteLane {
    int r, c;
    long long i;
    bool writer;
};
template <int LPR, typename T>
__device__ __forceinline__ VoteLane vote_row(int m, int classes, int n_points, const T *__restrict__ logits, const long long *__restrict__ idx,
                                             const int *stamp, float *__restrict__ pred) {
    static_assert(LPR >= 3 && WAVE % LPR == 0, "a row holds the three shift lanes and stays inside one wave");
    const int r = blockIdx.x * (ET_BLOCK / LPR) + threadIdx.x / LPR, c = threadIdx.x % LPR;
    long long i = -1;
    if (r < m) i = idx[r];
    const bool writer = i >= 0 && i < n_points && stamp[i] == r;
    const bool active = writer && c < classes;
    float x = active ? ld_elem(&logits[(size_t)r * classes + c]) : -INFINITY;
    float mx = x;
#pragma unroll
    for (int s = 1; s < LPR; s <<= 1) mx = fmaxf(mx, __shfl_xor(mx, s, WAVE));
    const float e = active ? expf(x - mx) : 0.0f;
    float sum = e;
#pragma unroll
    for (int s = 1; s < LPR; s <<= 1) sum += __shfl_xor(sum, s, WAVE);
    if (active) pred[(size_t)i * classes + c] += e / sum;
    return VoteLane{r, c, i, writer};
}

template <int LPR, typename T>
__global__ __launch_bounds__(ET_BLOCK) void vote_add_kernel(int m, int classes, int n_points, const T *__restrict__ logits,
                                                            const long long *__restrict__ idx, int *stamp, float *__restrict__ pred) {
    const VoteLane v = vote_row<LPR>(m, classes, n_points, logits, idx, stamp, pred);
    if (v.writer && v.c == 0) stamp[v.i] = -1;
}

__device__ __forceinline__ float shift_value(const void *p, int type, size_t k) {
    if (type == POINTOPS2_ROWS_F32) return ld_elem(&((const float *)p)[k]);
    if (type == POINTOPS2_ROWS_F16) return ld_elem(&((const f16_t *)p)[k]);
    return ld_elem(&((const bf16_t *)p)[k]);
}

// vote_add_kernel with the second accumulator: the writer row also adds its three shift components, on lanes 0..2 of the row
template <int LPR, typename T>
__global__ __launch_bounds__(ET_BLOCK) void vote_shift_add_kernel(int m, int classes, int n_points, const T *__restrict__ logits, int shift_type,
                                                                  const void *__restrict__ shift, const long long *__restrict__ idx, int *stamp,
                                                                  float *__restrict__ pred, float *__restrict__ pred_shift) {
    const VoteLane v = vote_row<LPR>(m, classes, n_points, logits, idx, stamp, pred);
    if (v.writer && v.c < 3) pred_shift[(size_t)v.i * 3 + v.c] += shift_value(shift, shift_type, (size_t)v.r * 3 + v.c);
    if (v.writer && v.c == 0) stamp[v.i] = -1;
}

}  // namespace
}  // namespace p2

using namespace p2;

extern "C" {

int pointops2_evaltile_max_parts(void) { return ET_MAX_PARTS; }

void pointops2_evaltile_seed_dist_launcher(int n, int is_f64, const void *coord, const double *priority, double *part_value, int *part_index,
                                           long long *seed, void *dist) {
    const hipStream_t st = begin_launch().stream;
    if (n <= 0) { set_error("evaltile_seed_dist: need n >= 1"); return; }
    if (!coord || !priority || !part_value || !part_index || !seed || !dist) { set_error("evaltile_seed_dist: a NULL array"); return; }
    const int parts = argmin_parts(n);
    hipLaunchKernelGGL(argmin_partial_kernel, dim3(parts), dim3(ET_BLOCK), 0, st, n, priority, part_value, part_index);
    if (is_f64)
        hipLaunchKernelGGL(seed_dist_kernel<double>, dim3(div_up(n, ET_BLOCK)), dim3(ET_BLOCK), 0, st, n, parts, (const double *)coord, part_value,
                           part_index, seed, (double *)dist);
    else
        hipLaunchKernelGGL(seed_dist_kernel<float>, dim3(div_up(n, ET_BLOCK)), dim3(ET_BLOCK), 0, st, n, parts, (const float *)coord, part_value,
                           part_index, seed, (float *)dist);
    check_launch();
}

void pointops2_evaltile_update_launcher(int n, int voxel_max, int is_f64, const void *dist, const long long *crop, double *priority,
                                        unsigned char *covered, int *report) {
    const hipStream_t st = begin_launch().stream;
    if (n <= 0 || voxel_max < 1 || voxel_max > n) { set_error("evaltile_update: need 1 <= voxel_max <= n"); return; }
    if (!dist || !crop || !priority || !covered || !report) { set_error("evaltile_update: a NULL array"); return; }
    if (is_f64)
        hipLaunchKernelGGL(update_kernel<double>, dim3(div_up(voxel_max, ET_BLOCK)), dim3(ET_BLOCK), 0, st, n, voxel_max, (const double *)dist, crop,
                           priority, covered, report);
    else
        hipLaunchKernelGGL(update_kernel<float>, dim3(div_up(voxel_max, ET_BLOCK)), dim3(ET_BLOCK), 0, st, n, voxel_max, (const float *)dist, crop,
                           priority, covered, report);
    check_launch();
}

void pointops2_evaltile_vote_launcher(int m, int classes, int n_points, int row_type, const void *logits, const long long *idx, int *stamp,
                                      float *pred, int *status) {
    const hipStream_t st = begin_launch().stream;
    if (m < 0 || n_points < 1 || classes < 1 || classes > 64) { set_error("evaltile_vote: need m >= 0, n_points >= 1 and 1 <= classes <= 64"); return; }
    if (!known_row_type(row_type)) {
        set_error("evaltile_vote: row_type must be POINTOPS2_ROWS_F32, _F16 or _BF16");
        return;
    }
    if (m == 0) return;
    if (!logits || !idx || !stamp || !pred || !status) { set_error("evaltile_vote: a NULL array"); return; }
    hipLaunchKernelGGL(vote_stamp_kernel, dim3(div_up(m, ET_BLOCK)), dim3(ET_BLOCK), 0, st, m, n_points, idx, stamp, status);
    with_row_type(row_type, [&](auto tag) {
        using T = typename decltype(tag)::type;
        with_row_lanes(classes, [&](auto lanes) {
            constexpr int LPR = decltype(lanes)::value;
            hipLaunchKernelGGL((vote_add_kernel<LPR, T>), dim3(div_up(m, ET_BLOCK / LPR)), dim3(ET_BLOCK), 0, st, m, classes, n_points, (const T *)logits,
                               idx, stamp, pred);
        });
    });
    check_launch();
}

void pointops2_evaltile_vote_shift_launcher(int m, int classes, int n_points, int row_type, const void *logits, int shift_row_type, const void *shift,
                                            const long long *idx, int *stamp, float *pred, float *pred_shift, int *status) {
    const hipStream_t st = begin_launch().stream;
    if (m < 0 || n_points < 1 || classes < 1 || classes > 64) { set_error("evaltile_vote_shift: need m >= 0, n_points >= 1 and 1 <= classes <= 64"); return; }
    if (!known_row_type(row_type) || !known_row_type(shift_row_type)) {
        set_error("evaltile_vote_shift: row_type and shift_row_type must be POINTOPS2_ROWS_F32, _F16 or _BF16");
        return;
    }
    if (m == 0) return;
    if (!logits || !shift || !idx || !stamp || !pred || !pred_shift || !status) { set_error("evaltile_vote_shift: a NULL array"); return; }
    hipLaunchKernelGGL(vote_stamp_kernel, dim3(div_up(m, ET_BLOCK)), dim3(ET_BLOCK), 0, st, m, n_points, idx, stamp, status);
    with_row_type(row_type, [&](auto tag) {
        using T = typename decltype(tag)::type;
        with_row_lanes(classes, [&](auto lanes) {
            constexpr int LPR = decltype(lanes)::value;
            hipLaunchKernelGGL((vote_shift_add_kernel<LPR, T>), dim3(div_up(m, ET_BLOCK / LPR)), dim3(ET_BLOCK), 0, st, m, classes, n_points,
                               (const T *)logits, shift_row_type, shift, idx, stamp, pred, pred_shift);
        });
    });
    check_launch();
}

}  // extern "C"
