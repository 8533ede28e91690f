// How the per-row glue kernels (rownorm.hip: LayerNorm over a row; batchnorm.hip: BatchNorm over a column) put rows [n, c] on the lanes,
// and how they add what a workgroup left in `partials` without float atomics.
//
// Lanes: a lane owns one chunk of a row - four channels: 16 bytes of an fp32 row, 8 of a half row (widened and narrowed by row_types.h).  A row of
// `chunks` <= 64 chunks occupies a SEGMENT of seg = the next power of two lanes (12, 24, 48 chunks -> 16, 32, 64 lanes; the lanes
// behind the row's last chunk idle), so 64 / seg rows sit side by side in a wave and a sum over a row is an xor butterfly over the
// aligned segment, a sum over the rows of a wave one over the strides seg .. 32.  Longer rows (up to 256 chunks) take a whole wave,
// each lane ITER = 2 or 4 chunks 64 apart.  Channel counts that are no multiple of four, or operands that are not aligned for the chunk
// accesses, run the same kernels with one channel per lane (VEC = 1: rows of up to 64 channels in segments, longer ones 16 channels a lane).
//
// Column reductions: a workgroup writes one row of `partials` [workgroups][cols]; column_reduce merges those rows - row b in group
// b % 64 in ascending order, then the 64 groups by a fixed halving tree (q takes q + 32, q + 16, ...: a sequential merge of a thousand
// partials would lose three more bits than torch's own reduction does).  The order is a function of the shapes alone.
#pragma once
#include "row_types.h"

namespace p2 {

constexpr int RN_MAX_C = 1024;
constexpr int RN_WAVES = 4;                       // per workgroup
constexpr int RN_THREADS = RN_WAVES * WAVE;
constexpr int RED_COLS = 16, RED_GROUPS = 64;     // column_reduce: a workgroup of RED_COLS * RED_GROUPS threads merges 16 columns of `partials` in 64 groups of rows

// VEC consecutive elements of a row of type rt, from element `e` of `base`, as floats
template <int VEC>
__device__ __forceinline__ void load_chunk(const void *__restrict__ base, size_t e, int rt, float *v) {
    if constexpr (VEC == 4) {
        if (rt == POINTOPS2_ROWS_F32) {
            const float4 w = *reinterpret_cast<const float4 *>(reinterpret_cast<const float *>(base) + e);
            v[0] = w.x, v[1] = w.y, v[2] = w.z, v[3] = w.w;
        } else {
            const uint2 w = *reinterpret_cast<const uint2 *>(reinterpret_cast<const unsigned short *>(base) + e);
            v[0] = widen16(w.x & 0xffffu, rt), v[1] = widen16(w.x >> 16, rt), v[2] = widen16(w.y & 0xffffu, rt), v[3] = widen16(w.y >> 16, rt);
        }
    } else {
        v[0] = rt == POINTOPS2_ROWS_F32 ? reinterpret_cast<const float *>(base)[e]
                                        : widen16(reinterpret_cast<const unsigned short *>(base)[e], rt);
    }
}
template <int VEC>
__device__ __forceinline__ void store_chunk(void *__restrict__ base, size_t e, int rt, const float *v) {
    if constexpr (VEC == 4) {
        if (rt == POINTOPS2_ROWS_F32)
            *reinterpret_cast<float4 *>(reinterpret_cast<float *>(base) + e) = make_float4(v[0], v[1], v[2], v[3]);
        else
            *reinterpret_cast<uint2 *>(reinterpret_cast<unsigned short *>(base) + e) =
                make_uint2(narrow16(v[0], rt) | (narrow16(v[1], rt) << 16), narrow16(v[2], rt) | (narrow16(v[3], rt) << 16));
    } else {
        if (rt == POINTOPS2_ROWS_F32) reinterpret_cast<float *>(base)[e] = v[0];
        else reinterpret_cast<unsigned short *>(base)[e] = (unsigned short)narrow16(v[0], rt);
    }
}

// sum over the aligned segment of `seg` lanes (a power of two <= 64) this lane sits in; every lane of the wave must call it
__device__ __forceinline__ float seg_sum(float v, int seg) {
    for (int st = 1; st < seg; st <<= 1) v += __shfl_xor(v, st, WAVE);
    return v;
}

// rows of a wave: chunks <= 64 -> 64 / seg rows side by side, lane = (row, chunk); else one row, each lane ITER chunks 64 apart
struct SegLanes {
    int per_wave, sub, chunk0;
    __device__ __forceinline__ SegLanes(int seg) {
        const int lane = lane_id();
        per_wave = WAVE / seg;
        sub = lane / seg;
        chunk0 = lane & (seg - 1);
    }
};

__device__ __forceinline__ float lanes_xor(float v, int st) { return __shfl_xor(v, st, WAVE); }  // (overload it for a T of several floats)

// What a workgroup holds per channel, merged: lane = (row slot, chunk) keeps v[it][e] for channel (chunk0 + it * 64) * VEC + e, gathered
// over its rows in ascending order.  The segments of a wave merge by an xor butterfly (a tree), the four waves in order through LDS
// (red: RN_THREADS * ITER * VEC entries), starting from `none`; the thread that takes channel ch calls store(ch, merged).  Every
// thread of the workgroup calls it.
template <int VEC, int ITER, typename T, typename Merge, typename Store>
__device__ __forceinline__ void workgroup_columns(T (&v)[ITER][VEC], int c, int seg, T none, T *red, Merge merge, Store store) {
    const int w = threadIdx.x >> 6, lane = lane_id();
#pragma unroll
    for (int it = 0; it < ITER; it++) {
#pragma unroll
        for (int e = 0; e < VEC; e++) {
            for (int st = seg; st < WAVE; st <<= 1) v[it][e] = merge(v[it][e], lanes_xor(v[it][e], st));
            red[((w * ITER + it) * WAVE + lane) * VEC + e] = v[it][e];
        }
    }
    __syncthreads();
    for (int ch = threadIdx.x; ch < c; ch += RN_THREADS) {
        const int chunk = ch / VEC, e = ch - chunk * VEC, it = chunk >> 6, lane0 = chunk & 63;  // (segment 0 of the wave holds the wave's merge)
        T t = none;
        for (int ww = 0; ww < RN_WAVES; ww++) t = merge(t, red[((ww * ITER + it) * WAVE + lane0) * VEC + e]);
        store(ch, t);
    }
}

// The merge of column `col` of the `rows` rows a launch left in `partials`: load(b) is row b's entry, merge(a, b) joins two of them, `none`
// is what merges to nothing.  Every thread of the RED_COLS * RED_GROUPS workgroup calls it (thread = group * RED_COLS + column;
// have: the thread's column exists); the threads of group 0 return the result.
template <typename T, typename Load, typename Merge>
__device__ __forceinline__ T column_reduce(int rows, bool have, T none, T (*red)[RED_COLS], Load load, Merge merge) {
    const int lc = threadIdx.x % RED_COLS, grp = threadIdx.x / RED_COLS;
    T acc = none;
    if (have)
        for (int b = grp; b < rows; b += RED_GROUPS) acc = merge(acc, load(b));
    red[grp][lc] = acc;
    __syncthreads();
    for (int half = RED_GROUPS / 2; half > 0; half >>= 1) {  // group q takes group q + half: a fixed tree
        if (grp < half) red[grp][lc] = merge(red[grp][lc], red[grp + half][lc]);
        __syncthreads();
    }
    return red[0][lc];
}

// grad_gamma | grad_beta [cols = 2 C] = the column sums of partials [rows][cols], in column_reduce's order: the body of the kernel that
// follows a backward's row pass (a grid of div_up(2 C, RED_COLS) workgroups of RED_COLS * RED_GROUPS threads)
__device__ __forceinline__ void param_sums(int rows, int c, const float *__restrict__ partials, float *__restrict__ grad_gamma,
                                           float *__restrict__ grad_beta) {
    __shared__ float red[RED_GROUPS][RED_COLS];
    const int cols = 2 * c, col = blockIdx.x * RED_COLS + threadIdx.x % RED_COLS;
    const float sum = column_reduce(rows, col < cols, 0.0f, red, [&](int b) { return partials[(size_t)b * cols + col]; },
                                    [](float p, float q) { return p + q; });
    if (threadIdx.x < RED_COLS && col < cols) {
        if (col < c) grad_gamma[col] = sum;
        else grad_beta[col - c] = sum;
    }
}

inline bool aligned_to(const void *p, unsigned bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; }
inline bool rows_aligned(const void *p, int row_type) { return aligned_to(p, row_type == POINTOPS2_ROWS_F32 ? 16 : 8); }  // (NULL is aligned)

struct RowShape {
    int vec, iter, chunks, seg, rows_per_wg;
    RowShape(int c, bool chunked) {
        vec = chunked ? 4 : 1;
        chunks = c / vec;
        if (chunks <= WAVE) {
            iter = 1;
            seg = 1;
            while (seg < chunks) seg <<= 1;
        } else {
            seg = WAVE;
            iter = vec == 1 ? 16 : chunks <= 2 * WAVE ? 2 : 4;
        }
        rows_per_wg = RN_WAVES * (WAVE / seg);
    }
    int grid(int n, int cap) const {
        const int64_t want = div_up64(n, rows_per_wg);
        return (int)(want < cap ? want : cap);
    }
};

// f(kernel tag) for the (VEC, ITER) instance of the shape
template <int V, int I> struct Inst { static constexpr int vec = V, iter = I; };
template <typename F>
void for_shape(const RowShape &sh, F &&f) {
    if (sh.vec == 4) {
        if (sh.iter == 1) f(Inst<4, 1>{});
        else if (sh.iter == 2) f(Inst<4, 2>{});
        else f(Inst<4, 4>{});
    } else {
        if (sh.iter == 1) f(Inst<1, 1>{});
        else f(Inst<1, 16>{});
    }
}

}  // namespace p2
