// Contacts between labelled point sets on the device: the distance primitive behind the second half of `instantiation_eval`
// (util/train_utils.py:595-714 runs one dense scipy cdist per (edge instance, face instance) pair on the host; the same question is
// asked at :251-261 and test.py:311 with other thresholds).  Points carry a label in -1 .. I-1, the results are tables over label pairs.
//
// Tables, over the points whose label is >= 0:
//   count[a, b]  = number of points p of label a for which SOME point q of label b has d2(p, q) < r2 (strict; p counts once per b,
//                  however many q are near; p is its own partner, so count[a, a] is the size of a).  Not symmetric in general.
//   min_d2[a, b] = min of d2(p, q) over p in a, q in b; +inf where either label is empty.  Symmetric.
// Arithmetic, fixed so that tests/contacts_oracle.py reproduces it bit for bit: fp32, dx = xp - xq, d2 = ((dx*dx) + (dy*dy)) + (dz*dz),
// every operation rounded on its own (the library is built with -ffp-contract=off), r2 = r * r rounded once by the caller.
// (xp - xq) and (xq - xp) differ in sign only, so d2(p, q) == d2(q, p) bit for bit.
//
// count: the fixed-radius walk of radius_grid.h on the grid that dbscan.hip's key and prepare kernels build (reused as they are: one
// group, label -1 outside it; cells of edge r * (1 + 2^-7), so every pair the fp32 test accepts is at most one cell apart).  One thread
// per point in sorted order; labels_in_reach sets bit b in the point's OWN row of labels - two registers for up to 64 labels, otherwise
// a row of the caller's zeroed [n_valid, ceil(I / 32)] bitmap that no other thread touches, so the row needs no atomics.  After the walk
// the thread adds its set bits to count with integer atomicAdd: sums of ones, independent of the order in which threads run.
//
// min_d2: the grid cannot answer it - two sets further apart than a cell never meet in a walk, and their distance is asked for all the
// same - so it is a tiled sweep over all pairs of the points sorted BY LABEL.  A thread owns one p, the workgroup stages 256 q at a time
// in LDS; q runs through the labels in order, so the label b of the current q is the same for every lane and a thread carries one
// running minimum, flushed when b changes: reduced over the wave when the wave's points share their label (the common case in label
// order), then atomicMin on the bit pattern of the non-negative fp32, issued only where the value is below a plain load of the entry.
// The entries only ever fall, so a stale read costs a redundant atomic, never a wrong result, and a minimum does not depend on the
// order.  d2 is symmetric, so only q-chunks that reach p's tile or lie behind it are swept and both [a, b] and [b, a] are written.
// No kernel waits on another workgroup; ranges, labels and indices are clamped or skipped, never followed outside their arrays.
#include "radius_grid.h"

namespace p2 {
namespace {

constexpr int CT_CHUNK = 4096;    // q of one workgroup of the all-pairs sweep (a multiple of RG_BLOCK)

template <bool REG>
__global__ __launch_bounds__(RG_BLOCK) void contacts_count_kernel(int n_valid, int n_labels, int words, const float4 *__restrict__ pts,
                                                                  const int *__restrict__ slabel, const int *__restrict__ ranges, float r2,
                                                                  unsigned *__restrict__ bitmap, int *__restrict__ count) {
    const int p = blockIdx.x * RG_BLOCK + threadIdx.x;
    if (p >= n_valid) return;
    const int a = slabel[p];
    if ((unsigned)a >= (unsigned)n_labels) return;
    unsigned bits0 = 0, bits1 = 0;
    unsigned *row = REG ? nullptr : bitmap + (size_t)p * words;
    labels_in_reach<REG>(p, n_valid, n_labels, pts, slabel, ranges, r2, bits0, bits1, row);
    int *mine = count + (size_t)a * n_labels;
    for (int w = 0; w < words; w++) {
        unsigned v = REG ? (w == 0 ? bits0 : bits1) : row[w];
        while (v) {
            const int b = w * 32 + __ffs((int)v) - 1;
            v &= v - 1;
            if (b < n_labels) atomicAdd(&mine[b], 1);
        }
    }
}

__device__ __forceinline__ void lower_entry(int *min_bits, size_t at, float v) {
    if (v < __int_as_float(min_bits[at])) atomicMin(&min_bits[at], __float_as_int(v));  // non-negative fp32: ordered as its bit pattern
}

// the running minimum of a thread against label b goes to min_bits[a, b] and [b, a]
__device__ __forceinline__ void flush_min(int a, int b, float v, int n_labels, int *min_bits) {
    if ((unsigned)b >= (unsigned)n_labels) return;                                   // (uniform: b is the same for every lane)
    const int first = __builtin_amdgcn_readfirstlane(a);
    if (__all(a == first)) {                                                         // one label in the wave: one pair of atomics
#pragma unroll
        for (int s = 1; s < WAVE; s <<= 1) {
            const float t = __shfl_xor(v, s, WAVE);
            v = t < v ? t : v;
        }
        if (lane_id() != 0) return;
    }
    if ((unsigned)a >= (unsigned)n_labels || !(v < __builtin_inff())) return;
    lower_entry(min_bits, (size_t)a * n_labels + b, v);
    if (a != b) lower_entry(min_bits, (size_t)b * n_labels + a, v);
}

// lpts [n_valid] = {x, y, z, label as bits}, ascending label.  grid.x: tiles of RG_BLOCK p, grid.y: chunks of CT_CHUNK q
__global__ __launch_bounds__(RG_BLOCK) void contacts_min_kernel(int n_valid, int n_labels, const float4 *__restrict__ lpts,
                                                                int *__restrict__ min_bits) {
    __shared__ float4 tile[RG_BLOCK];
    const int p0 = blockIdx.x * RG_BLOCK, q0 = blockIdx.y * CT_CHUNK;
    const int q1 = min(q0 + CT_CHUNK, n_valid);
    if (q1 <= p0) return;                                                            // (whole workgroup) the mirrored pairs are swept
    const int p = p0 + threadIdx.x;
    const bool valid = p < n_valid;
    const float4 me = lpts[valid ? p : n_valid - 1];
    const int a = valid ? __float_as_int(me.w) : -1;
    int cur_b = -1;
    float cur = __builtin_inff();
    for (int t0 = q0; t0 < q1; t0 += RG_BLOCK) {
        const int q = t0 + threadIdx.x;
        __syncthreads();
        tile[threadIdx.x] = lpts[q < q1 ? q : q1 - 1];
        __syncthreads();
        const int len = min(RG_BLOCK, q1 - t0);
        for (int j = 0; j < len; j++) {
            const float4 o = tile[j];
            const int b = __float_as_int(o.w);
            if (b != cur_b) {
                flush_min(a, cur_b, cur, n_labels, min_bits);
                cur_b = b;
                cur = __builtin_inff();
            }
            const float dx = me.x - o.x, dy = me.y - o.y, dz = me.z - o.z;
            const float d2 = ((dx * dx) + (dy * dy)) + (dz * dz);
            cur = d2 < cur ? d2 : cur;
        }
    }
    flush_min(a, cur_b, cur, n_labels, min_bits);
}

}  // namespace
}  // namespace p2

using namespace p2;

extern "C" {

void pointops2_contacts_count_launcher(int n_valid, int n_labels, const float *pts, const int *sorted_label, const int *ranges, float r2,
                                       unsigned *bitmap, int *count) {
    const hipStream_t st = begin_launch().stream;
    if (n_valid < 0 || n_labels < 0) { set_error("contacts_count: need n_valid, n_labels >= 0"); return; }
    if (n_valid == 0 || n_labels == 0) return;
    if ((double)n_labels * n_labels >= 2147483648.0) { set_error("contacts_count: n_labels * n_labels does not fit an int"); return; }
    const int words = div_up(n_labels, 32);
    const dim3 grid(div_up(n_valid, RG_BLOCK)), block(RG_BLOCK);
    if (n_labels <= RG_REG_LABELS) {
        hipLaunchKernelGGL(contacts_count_kernel<true>, grid, block, 0, st, n_valid, n_labels, words, reinterpret_cast<const float4 *>(pts),
                           sorted_label, ranges, r2, bitmap, count);
    } else {
        if (bitmap == nullptr) { set_error("contacts_count: more than 64 labels need the bitmap"); return; }
        hipLaunchKernelGGL(contacts_count_kernel<false>, grid, block, 0, st, n_valid, n_labels, words, reinterpret_cast<const float4 *>(pts),
                           sorted_label, ranges, r2, bitmap, count);
    }
    check_launch();
}

void pointops2_contacts_min_launcher(int n_valid, int n_labels, const float *label_pts, float *min_d2) {
    const hipStream_t st = begin_launch().stream;
    if (n_valid < 0 || n_labels < 0) { set_error("contacts_min: need n_valid, n_labels >= 0"); return; }
    if (n_valid == 0 || n_labels == 0) return;
    if ((double)n_labels * n_labels >= 2147483648.0) { set_error("contacts_min: n_labels * n_labels does not fit an int"); return; }
    const int chunks = div_up(n_valid, CT_CHUNK);
    if (chunks > 65535) { set_error("contacts_min: more than 65535 * 4096 points"); return; }
    hipLaunchKernelGGL(contacts_min_kernel, dim3(div_up(n_valid, RG_BLOCK), chunks), dim3(RG_BLOCK), 0, st, n_valid, n_labels,
                       reinterpret_cast<const float4 *>(label_pts), reinterpret_cast<int *>(min_d2));
    check_launch();
}

}  // extern "C"
