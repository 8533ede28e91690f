// Boxes and reach rows of labelled point sets on the device: what the OBB merging behind `instantiation_eval` (test.py:294-326, the same
// loop at test_iou.py:373-406) needs of the points.  That loop builds an axis-aligned box per set with trimesh and runs one dense scipy
// cdist per (current set, target set) pair to count the target's points within 0.2 of the current set; its sets are always unions of
// whole input objects, so per-object boxes and per-point "objects in reach" answer every pair it will ever ask about
// (stratified_transformer_amd/cluster.py: merge_objects / merge_sets run the loop itself on plain host arrays).
//
// label_boxes: lo / hi [I, 3] = componentwise minimum / maximum of the points of every label, size [I] = their number.  One pass over the
// points in any order.  Minimum and maximum run as SIGNED INTEGER atomics on an order-preserving image of the fp32 value: the bit pattern
// for a non-negative value, the pattern with its 31 low bits inverted for a negative one (an involution: the same map takes the image
// back).  -0.0 is made +0.0 first, so the two zeros are one value.  The caller presets lo = +inf, hi = -inf, size = 0 AS FLOATS / INTS;
// the launcher turns lo / hi into images before the pass and back after it (two tiny kernels on the same stream), so an empty label keeps
// its preset and a second call on the same arrays accumulates.  Up to LB_LDS_LABELS labels a workgroup keeps a private table of seven
// words per label in LDS, walks its share of the points and flushes only the entries it touched, one global atomic each; above that the
// atomics go straight to global memory.  Minima, maxima and integer counts do not depend on the order: exact and reproducible.
//
// reach_rows: the fixed-radius walk of radius_grid.h (labels_in_reach, as contacts.hip's count) on the same prepared grid (dbscan.hip's
// key and prepare kernels, one group), the same strict d2 < r2 and the same fp32 expression ((dx*dx) + (dy*dy)) + (dz*dz) (built with
// -ffp-contract=off).  Instead of adding to a count table a thread STORES its point's row of ceil(I / 32) words - bit b = some point of label b within reach - with the point's own bit
// cleared.  Up to 64 labels the row is built in two registers and stored once; above that in the point's own row of the caller's zeroed
// array, which no other thread touches: no atomics, plain vector stores.
// No kernel waits on another workgroup; ranges are clamped, labels outside [0, n_labels) skipped, nothing is followed outside its array.
#include "radius_grid.h"

namespace p2 {
namespace {

constexpr int LB_BLOCK = 256;
constexpr int LB_TILE = 2048;          // points of one workgroup per trip: a table entry is flushed once for many points
constexpr int LB_MAX_GRID = 1024;
constexpr int LB_LDS_LABELS = 1024;    // 7 words per label: 28 KB of LDS
constexpr int LB_WORDS = 7;            // lo[3], hi[3], size

// order-preserving signed image of an fp32 bit pattern, and its own inverse
__device__ __forceinline__ int ordered(int bits) { return bits >= 0 ? bits : bits ^ 0x7fffffff; }

__device__ __forceinline__ int image_of(float v) {
    int bits = __float_as_int(v);
    if ((bits & 0x7fffffff) == 0) bits = 0;                                          // -0.0 -> +0.0
    return ordered(bits);
}

__global__ __launch_bounds__(LB_BLOCK) void boxes_image_kernel(int count, int *__restrict__ lo, int *__restrict__ hi) {
    const int i = blockIdx.x * LB_BLOCK + threadIdx.x;
    if (i >= count) return;
    lo[i] = ordered(lo[i]);
    hi[i] = ordered(hi[i]);
}

template <bool LDS>
__global__ __launch_bounds__(LB_BLOCK) void label_boxes_kernel(int n, int n_labels, const float *__restrict__ xyz, const int *__restrict__ label,
                                                               int *__restrict__ lo, int *__restrict__ hi, int *__restrict__ size) {
    __shared__ int table[LDS ? LB_LDS_LABELS * LB_WORDS : 1];
    if (LDS) {
        for (int l = threadIdx.x; l < n_labels; l += LB_BLOCK) {
            int *e = table + l * LB_WORDS;
            e[0] = e[1] = e[2] = 0x7fffffff;
            e[3] = e[4] = e[5] = (int)0x80000000;
            e[6] = 0;
        }
        __syncthreads();
    }
    for (int64_t t0 = (int64_t)blockIdx.x * LB_TILE; t0 < n; t0 += (int64_t)gridDim.x * LB_TILE) {
        const int64_t t1 = min(t0 + LB_TILE, (int64_t)n);
        for (int64_t p = t0 + threadIdx.x; p < t1; p += LB_BLOCK) {
            const int a = label[p];
            if ((unsigned)a >= (unsigned)n_labels) continue;
            const int x = image_of(xyz[(size_t)p * 3]), y = image_of(xyz[(size_t)p * 3 + 1]), z = image_of(xyz[(size_t)p * 3 + 2]);
            if (LDS) {
                int *e = table + a * LB_WORDS;
                atomicMin(&e[0], x); atomicMin(&e[1], y); atomicMin(&e[2], z);
                atomicMax(&e[3], x); atomicMax(&e[4], y); atomicMax(&e[5], z);
                atomicAdd(&e[6], 1);
            } else {
                int *l3 = lo + (size_t)a * 3, *h3 = hi + (size_t)a * 3;
                atomicMin(&l3[0], x); atomicMin(&l3[1], y); atomicMin(&l3[2], z);
                atomicMax(&h3[0], x); atomicMax(&h3[1], y); atomicMax(&h3[2], z);
                atomicAdd(&size[a], 1);
            }
        }
    }
    if (LDS) {
        __syncthreads();
        for (int l = threadIdx.x; l < n_labels; l += LB_BLOCK) {
            const int *e = table + l * LB_WORDS;
            if (e[6] == 0) continue;                                                 // not touched by this workgroup
            int *l3 = lo + (size_t)l * 3, *h3 = hi + (size_t)l * 3;
            atomicMin(&l3[0], e[0]); atomicMin(&l3[1], e[1]); atomicMin(&l3[2], e[2]);
            atomicMax(&h3[0], e[3]); atomicMax(&h3[1], e[4]); atomicMax(&h3[2], e[5]);
            atomicAdd(&size[l], e[6]);
        }
    }
}

template <bool REG>
__global__ __launch_bounds__(RG_BLOCK) void reach_rows_kernel(int n_valid, int n_labels, int words, const float4 *__restrict__ pts,
                                                              const int *__restrict__ slabel, const int *__restrict__ ranges, float r2,
                                                              unsigned *__restrict__ rows) {
    const int p = blockIdx.x * RG_BLOCK + threadIdx.x;
    if (p >= n_valid) return;
    unsigned *row = rows + (size_t)p * words;
    const int a = slabel[p];
    if ((unsigned)a >= (unsigned)n_labels) {
        if (REG) {                                                                   // the register path writes every row
            row[0] = 0;
            if (words > 1) row[1] = 0;
        }
        return;
    }
    unsigned bits0 = 0, bits1 = 0;
    labels_in_reach<REG>(p, n_valid, n_labels, pts, slabel, ranges, r2, bits0, bits1, row);
    const unsigned own = ~(1u << (a & 31));
    if (REG) {
        if (a < 32) bits0 &= own;
        else bits1 &= own;
        row[0] = bits0;
        if (words > 1) row[1] = bits1;
    } else {
        row[a >> 5] &= own;
    }
}

}  // namespace
}  // namespace p2

using namespace p2;

extern "C" {

void pointops2_label_boxes_launcher(int n, int n_labels, const float *xyz, const int *label, float *lo, float *hi, int *size) {
    const hipStream_t st = begin_launch().stream;
    if (n < 0 || n_labels < 0) { set_error("label_boxes: need n, n_labels >= 0"); return; }
    if (n == 0 || n_labels == 0) return;
    if ((double)n_labels * 3.0 >= 2147483648.0) { set_error("label_boxes: n_labels * 3 does not fit an int"); return; }
    if (xyz == nullptr || label == nullptr || lo == nullptr || hi == nullptr || size == nullptr) { set_error("label_boxes: a NULL array"); return; }
    int *lo_i = reinterpret_cast<int *>(lo), *hi_i = reinterpret_cast<int *>(hi);
    const dim3 image_grid(div_up(n_labels * 3, LB_BLOCK)), block(LB_BLOCK);
    const dim3 grid(min(div_up(n, LB_TILE), LB_MAX_GRID));
    hipLaunchKernelGGL(boxes_image_kernel, image_grid, block, 0, st, n_labels * 3, lo_i, hi_i);
    if (n_labels <= LB_LDS_LABELS)
        hipLaunchKernelGGL(label_boxes_kernel<true>, grid, block, 0, st, n, n_labels, xyz, label, lo_i, hi_i, size);
    else
        hipLaunchKernelGGL(label_boxes_kernel<false>, grid, block, 0, st, n, n_labels, xyz, label, lo_i, hi_i, size);
    hipLaunchKernelGGL(boxes_image_kernel, image_grid, block, 0, st, n_labels * 3, lo_i, hi_i);
    check_launch();
}

void pointops2_reach_rows_launcher(int n_valid, int n_labels, const float *pts, const int *sorted_label, const int *ranges, float r2,
                                   unsigned *rows) {
    const hipStream_t st = begin_launch().stream;
    if (n_valid < 0 || n_labels < 0) { set_error("reach_rows: need n_valid, n_labels >= 0"); return; }
    if (n_valid == 0 || n_labels == 0) return;
    if (pts == nullptr || sorted_label == nullptr || ranges == nullptr || rows == nullptr) { set_error("reach_rows: a NULL array"); return; }
    const int words = div_up(n_labels, 32);
    const dim3 grid(div_up(n_valid, RG_BLOCK)), block(RG_BLOCK);
    if (n_labels <= RG_REG_LABELS)
        hipLaunchKernelGGL(reach_rows_kernel<true>, grid, block, 0, st, n_valid, n_labels, words, reinterpret_cast<const float4 *>(pts),
                           sorted_label, ranges, r2, rows);
    else
        hipLaunchKernelGGL(reach_rows_kernel<false>, grid, block, 0, st, n_valid, n_labels, words, reinterpret_cast<const float4 *>(pts),
                           sorted_label, ranges, r2, rows);
    check_launch();
}

}  // extern "C"
