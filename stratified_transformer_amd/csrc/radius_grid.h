// The fixed-radius grid shared by dbscan.hip, contacts.hip and boxes.hip: its constants, the walk over a point's prepared runs and the
// "labels in reach as a bit row" body that the last two build on it.  The key and prepare kernels that build the grid are in dbscan.hip.
//
// Grid.  Cells of edge `cell` (cluster.py: the largest radius, widened by 2^-7 so that a pair the fp32 test accepts is never more than
// one cell apart; cell coordinates are taken in double).  A point's key is ((group * nz + cz) * ny + cy) * nx + cx, so the group is part
// of the cell: points of other groups are never even candidates.  Points outside every group get the largest key and sort behind the
// n_valid points that take part.  The caller sorts the keys (a torch sort, as index.hip and dataprep.hip leave their sorts to it).
// x runs fastest in the key, so the three cells cx-1 .. cx+1 of one (cy, cz) row are ONE run of the sorted points: prepare_kernel
// finds the nine runs of every point with binary searches over the sorted keys (no dense cell table - a sparse cloud costs nothing)
// and stores them once; every walk (dbscan's count, hook and label, the contact counts, the reach rows) reuses them.
//
// Walk.  One thread per point IN SORTED ORDER, no LDS: the lanes of a wave sit in the same cell or in adjacent ones, so they step
// through the same candidate rows at the same time and a candidate's 16-byte record {x, y, z, original index} is one broadcast load
// served by L1 / L2 (100k points are 1.6 MB).  Staging a cell's rows in LDS would save nothing that the cache does not already serve,
// and one wave per cell would leave most lanes idle on the sparse cells of a class's boundary.
// Arithmetic: fp32, dx = xp - xq, d2 = ((dx*dx) + (dy*dy)) + (dz*dz), every operation rounded on its own (the library is built with
// -ffp-contract=off).  Ranges are clamped to [0, n_valid], so a walk never leaves pts whatever `ranges` holds.
#pragma once
#include "common.h"

namespace p2 {

constexpr int RG_BLOCK = 256;      // threads of a workgroup of every kernel on the grid
constexpr int RG_ROWS = 9;         // (dy, dz) rows of three x-adjacent cells each
constexpr int RG_REG_LABELS = 64;  // bit rows of up to this many labels stay in two registers (cluster.py: REG_LABELS)

// f(q, j) for every q in the nine runs of sorted point p (p itself included) with d2(p, q) <= r2 (INCLUSIVE) or d2(p, q) < r2:
// q its sorted position, j its original index (pts[q].w)
template <bool INCLUSIVE, typename F>
__device__ __forceinline__ void for_each_in_reach(int p, int n_valid, const float4 *__restrict__ pts, const int *__restrict__ ranges,
                                                  float r2, F f) {
    const float4 me = pts[p];
#pragma unroll 1
    for (int r = 0; r < RG_ROWS; r++) {
        const int lo = max(ranges[(size_t)(2 * r) * n_valid + p], 0);
        const int hi = min(ranges[(size_t)(2 * r + 1) * n_valid + p], n_valid);
        for (int q = lo; q < hi; q++) {
            const float4 o = pts[q];
            const float dx = me.x - o.x, dy = me.y - o.y, dz = me.z - o.z;
            const float d2 = ((dx * dx) + (dy * dy)) + (dz * dz);
            if (INCLUSIVE ? d2 <= r2 : d2 < r2) f(q, __float_as_int(o.w));
        }
    }
}

// The labels within reach (strict d2 < r2) of sorted point p as a bit row, bit b = some point of label b in [0, n_labels) is in reach:
// in bits0 / bits1 for up to RG_REG_LABELS labels (REG), otherwise in `row`, the point's own zeroed row of ceil(n_labels / 32) words,
// which no other thread touches - no atomics.
template <bool REG>
__device__ __forceinline__ void labels_in_reach(int p, int n_valid, int n_labels, const float4 *__restrict__ pts,
                                                const int *__restrict__ slabel, const int *__restrict__ ranges, float r2,
                                                unsigned &bits0, unsigned &bits1, unsigned *row) {
    for_each_in_reach<false>(p, n_valid, pts, ranges, r2, [&](int q, int) {
        const int b = slabel[q];
        if ((unsigned)b >= (unsigned)n_labels) return;
        const unsigned bit = 1u << (b & 31);
        if (REG) {
            if (b < 32) bits0 |= bit;
            else bits1 |= bit;
        } else {
            const unsigned v = row[b >> 5];
            if (!(v & bit)) row[b >> 5] = v | bit;
        }
    });
}

}  // namespace p2
