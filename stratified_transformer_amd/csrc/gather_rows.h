// What the pure row gathers share (grouped_max.hip: max over k gathered rows; upsample.hip: weighted sum of k gathered rows, added to a
// base row): how rows [rows, c] sit on the lanes of a wave in 16-byte chunks, the 16-byte accesses of a typed row, the clamped walk of
// a key-major view (pointops2_csc_build) by source row, and the grids.  No LDS and no cross-lane traffic in any of them.
#pragma once
#include "row_types.h"

namespace p2 {

constexpr int GATHER_WAVES = 4;  // per workgroup

// one 16-byte chunk of a row of storage type RT (row_types.h): VEC elements, widened exactly, compared / summed in fp32
template <typename RT> struct Chunk {
    static constexpr int VEC = 16 / (int)sizeof(RT);
    uint4 bits;
    __device__ __forceinline__ float get(int e) const {
        const unsigned w[4] = {bits.x, bits.y, bits.z, bits.w};
        if constexpr (sizeof(RT) == 4) return __uint_as_float(w[e]);
        else return widen_bits<RT>((e & 1) ? (w[e >> 1] >> 16) : (w[e >> 1] & 0xffffu));
    }
    static __device__ __forceinline__ uint4 pack(const float *v) {
        unsigned w[4];
        if constexpr (sizeof(RT) == 4) {
#pragma unroll
            for (int e = 0; e < 4; e++) w[e] = __float_as_uint(v[e]);
        } else {
#pragma unroll
            for (int e = 0; e < 4; e++) w[e] = narrow_bits<RT>(v[2 * e]) | (narrow_bits<RT>(v[2 * e + 1]) << 16);
        }
        return make_uint4(w[0], w[1], w[2], w[3]);
    }
};
__device__ __forceinline__ uint4 ld16(const void *base, size_t byte_offset) {
    return *reinterpret_cast<const uint4 *>(reinterpret_cast<const char *>(base) + byte_offset);
}
__device__ __forceinline__ void st16(void *base, size_t byte_offset, uint4 v) {
    *reinterpret_cast<uint4 *>(reinterpret_cast<char *>(base) + byte_offset) = v;
}

// rows of a wave: `chunks` < 64 -> 64 / chunks rows side by side, lane = (row, chunk); else one row, the lanes stride over its chunks
struct RowLanes {
    int sub, chunk0, per_wave;
    __device__ __forceinline__ RowLanes(int chunks) {
        const int lane = lane_id();
        per_wave = chunks < WAVE ? WAVE / chunks : 1;
        sub = chunks < WAVE ? lane / chunks : 0;
        chunk0 = lane - sub * chunks;
    }
};

// the pairs [p0, p1) of source row j, clamped into the pair list whatever the offsets hold
__device__ __forceinline__ void pair_range(const int *__restrict__ src_offsets, long long j, int n_pairs, int &p0, int &p1) {
    p0 = min(max(src_offsets[j], 0), n_pairs);
    p1 = min(max(src_offsets[j + 1], p0), n_pairs);
}

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
inline int chunked_grid(int rows, int chunks) {
    const int per_wave = chunks < WAVE ? WAVE / chunks : 1;
    const int want = div_up(div_up(rows, per_wave), GATHER_WAVES), cap = num_cus() * 64;
    return want < cap ? want : cap;
}
inline int scalar_grid(long long total) {
    const long long want = div_up64(total, 256), cap = (long long)num_cus() * 64;
    return (int)(want < cap ? want : cap);
}

}  // namespace p2
