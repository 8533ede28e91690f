// Residual add + DropPath row scale + LayerNorm in one pass over the rows: the glue between the GEMMs of a pre-norm transformer block
// (model/stratified_transformer.py:235-248, model/swin3d_transformer.py:204-210: `short_cut + drop_path(attn)` feeds norm2,
// `feats + drop_path(mlp)` feeds the next block's norm1).  All arithmetic in fp32, nothing fused (the project builds with
// -ffp-contract=off and no fmaf is written here):
//
//   forward   z[n,c] = x[n,c] + s[n] * y[n,c]            (s absent: x + y;  y absent: x;  s * y is rounded, then added)
//             mean_n = sum_c z / C     var_n = sum_c (z - mean_n)^2 / C  (two passes over the row held in registers)
//             rstd_n = 1 / sqrt(var_n + eps)     o[n,c] = ((z - mean_n) * rstd_n) * gamma[c] + beta[c]     stat[n] = (mean_n, rstd_n)
//   backward  xhat = (z - mean) * rstd     g = dO * gamma     dz = rstd * ((g - mean_c(g)) - xhat * mean_c(g * xhat)) + dZ
//             dx = dz     dy = s[n] * dz     dgamma[c] = sum_n dO * xhat     dbeta[c] = sum_n dO
//
// x, z, dx, dZ, gamma, beta, s, stat are fp32 (the residual stream is fp32 with and without autocast); y / dy and o / dO each have one
// of the three row types POINTOPS2_ROWS_* (what a Linear yields and wants under autocast), widened exactly and rounded once.
//
// Lanes: a lane owns one chunk of a row - four channels: 16 bytes of an fp32 row, 8 of a half row (widened and narrowed by row_types.h).  A row of
// `chunks` <= 64 chunks occupies a SEGMENT of seg = the next power of two lanes (12, 24, 48 chunks -> 16, 32, 64 lanes; the lanes
// behind the row's last chunk idle and add 0), so 64 / seg rows sit side by side in a wave and the row sums are an xor butterfly
// over the aligned segment: every lane of it ends with the same bits, and no value crosses a segment - a NaN stays in its row.
// Longer rows (up to 256 chunks) take a whole wave, each lane ITER = 2 or 4 chunks 64 apart.  Channel counts that are no multiple
// of four, or operands that are not aligned for the chunk accesses, run the same kernels with one channel per lane
// (VEC = 1: rows of up to 64 channels in segments, longer ones 16 channels a lane): same results.
//
// dgamma / dbeta without float atomics: every lane adds dO * xhat and dO of its channels over its rows in ascending row order; a
// workgroup then adds, per channel, its lanes' sums - the segments of a wave by an xor butterfly, the four waves in order through LDS -
// and writes one row of `partials` [workgroups][2][C]; rownorm_param_kernel adds those rows - row b in group b % 64 in ascending order,
// then the 64 groups by a fixed halving tree (q takes q + 32, q + 16, ...: a sequential sum of a thousand partials would lose three more
// bits than torch's own reduction does).  The backward's grid is capped by the rows of `partials` the caller provides.  The order is
// a function of the shapes alone: the same bits from run to run on one device.
#include "row_types.h"

namespace p2 {
namespace {

constexpr int RN_MAX_C = 1024;
constexpr int RN_WAVES = 4;                       // per workgroup
constexpr int RN_THREADS = RN_WAVES * WAVE;
constexpr int RED_COLS = 16, RED_GROUPS = 64;     // rownorm_param_kernel: a workgroup sums 16 columns of `partials` in 64 groups of rows

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

template <int VEC, int ITER>
__global__ __launch_bounds__(RN_THREADS) void rownorm_fwd_kernel(int n, int c, int chunks, int seg, int y_type, int o_type,
                                                                 const float *__restrict__ x, const void *__restrict__ y,
                                                                 const float *__restrict__ s, const float *__restrict__ gamma,
                                                                 const float *__restrict__ beta, float eps, float *__restrict__ z,
                                                                 void *__restrict__ o, float *__restrict__ stat) {
    const SegLanes sl(seg);
    bool act[ITER];
    float gm[ITER][VEC], bt[ITER][VEC];
#pragma unroll
    for (int it = 0; it < ITER; it++) {
        const int chunk = sl.chunk0 + it * WAVE;
        act[it] = chunk < chunks;
#pragma unroll
        for (int e = 0; e < VEC; e++) gm[it][e] = bt[it][e] = 0.0f;
        if (act[it]) {
            load_chunk<VEC>(gamma, (size_t)chunk * VEC, POINTOPS2_ROWS_F32, gm[it]);
            load_chunk<VEC>(beta, (size_t)chunk * VEC, POINTOPS2_ROWS_F32, bt[it]);
        }
    }
    const float fc = (float)c;
    const long long wave = (long long)blockIdx.x * RN_WAVES + (threadIdx.x >> 6), waves = (long long)gridDim.x * RN_WAVES;
    for (long long first = wave * sl.per_wave; first < n; first += waves * sl.per_wave) {  // (wave-uniform: the shuffles below see all lanes)
        const long long row = first + sl.sub;
        const bool live = row < n;
        const float sc = (live && s != nullptr) ? s[row] : 1.0f;
        float v[ITER][VEC];
        float sum = 0.0f;
#pragma unroll
        for (int it = 0; it < ITER; it++) {
#pragma unroll
            for (int e = 0; e < VEC; e++) v[it][e] = 0.0f;
            if (live && act[it]) {
                const size_t at = (size_t)row * c + (size_t)(sl.chunk0 + it * WAVE) * VEC;
                load_chunk<VEC>(x, at, POINTOPS2_ROWS_F32, v[it]);
                if (y != nullptr) {
                    float yv[VEC];
                    load_chunk<VEC>(y, at, y_type, yv);
#pragma unroll
                    for (int e = 0; e < VEC; e++) {
                        const float t = s != nullptr ? sc * yv[e] : yv[e];
                        v[it][e] = v[it][e] + t;
                    }
                }
                if (z != nullptr) store_chunk<VEC>(z, at, POINTOPS2_ROWS_F32, v[it]);
            }
#pragma unroll
            for (int e = 0; e < VEC; e++) sum += v[it][e];
        }
        const float mean = seg_sum(sum, seg) / fc;
        float sq = 0.0f;
#pragma unroll
        for (int it = 0; it < ITER; it++) {
#pragma unroll
            for (int e = 0; e < VEC; e++) {
                v[it][e] = act[it] ? v[it][e] - mean : 0.0f;
                sq += v[it][e] * v[it][e];
            }
        }
        const float rstd = 1.0f / sqrtf(seg_sum(sq, seg) / fc + eps);
#pragma unroll
        for (int it = 0; it < ITER; it++) {
            if (!(live && act[it])) continue;
            float ov[VEC];
#pragma unroll
            for (int e = 0; e < VEC; e++) ov[e] = (v[it][e] * rstd) * gm[it][e] + bt[it][e];
            store_chunk<VEC>(o, (size_t)row * c + (size_t)(sl.chunk0 + it * WAVE) * VEC, o_type, ov);
        }
        if (live && sl.chunk0 == 0) {
            stat[2 * (size_t)row] = mean;
            stat[2 * (size_t)row + 1] = rstd;
        }
    }
}

template <int VEC, int ITER>
__global__ __launch_bounds__(RN_THREADS) void rownorm_bwd_kernel(int n, int c, int chunks, int seg, int y_type, int o_type,
                                                                 const void *__restrict__ grad_o, const float *__restrict__ grad_z,
                                                                 const float *__restrict__ z, const float *__restrict__ stat,
                                                                 const float *__restrict__ s, const float *__restrict__ gamma,
                                                                 float *__restrict__ grad_x, void *__restrict__ grad_y,
                                                                 float *__restrict__ partials) {
    __shared__ float red[2][RN_THREADS * ITER * VEC];
    const SegLanes sl(seg);
    bool act[ITER];
    float gm[ITER][VEC], ag[ITER][VEC], ab[ITER][VEC];
#pragma unroll
    for (int it = 0; it < ITER; it++) {
        const int chunk = sl.chunk0 + it * WAVE;
        act[it] = chunk < chunks;
#pragma unroll
        for (int e = 0; e < VEC; e++) gm[it][e] = ag[it][e] = ab[it][e] = 0.0f;
        if (act[it] && grad_o != nullptr) load_chunk<VEC>(gamma, (size_t)chunk * VEC, POINTOPS2_ROWS_F32, gm[it]);
    }
    const float fc = (float)c;
    const long long wave = (long long)blockIdx.x * RN_WAVES + (threadIdx.x >> 6), waves = (long long)gridDim.x * RN_WAVES;
    for (long long first = wave * sl.per_wave; first < n; first += waves * sl.per_wave) {
        const long long row = first + sl.sub;
        const bool live = row < n;
        const float sc = (live && s != nullptr) ? s[row] : 1.0f;
        float xh[ITER][VEC], g[ITER][VEC];
        float m1 = 0.0f, m2 = 0.0f, rstd = 0.0f;
        if (grad_o != nullptr) {  // (kernel-uniform)
            const float mean = live ? stat[2 * (size_t)row] : 0.0f;
            rstd = live ? stat[2 * (size_t)row + 1] : 0.0f;
            float p1 = 0.0f, p2 = 0.0f;
#pragma unroll
            for (int it = 0; it < ITER; it++) {
#pragma unroll
                for (int e = 0; e < VEC; e++) xh[it][e] = g[it][e] = 0.0f;
                if (live && act[it]) {
                    const size_t at = (size_t)row * c + (size_t)(sl.chunk0 + it * WAVE) * VEC;
                    float zv[VEC], dov[VEC];
                    load_chunk<VEC>(z, at, POINTOPS2_ROWS_F32, zv);
                    load_chunk<VEC>(grad_o, at, o_type, dov);
#pragma unroll
                    for (int e = 0; e < VEC; e++) {
                        xh[it][e] = (zv[e] - mean) * rstd;
                        g[it][e] = dov[e] * gm[it][e];
                        ag[it][e] += dov[e] * xh[it][e];
                        ab[it][e] += dov[e];
                    }
                }
#pragma unroll
                for (int e = 0; e < VEC; e++) {
                    p1 += g[it][e];
                    p2 += g[it][e] * xh[it][e];
                }
            }
            m1 = seg_sum(p1, seg) / fc;
            m2 = seg_sum(p2, seg) / fc;
        }
#pragma unroll
        for (int it = 0; it < ITER; it++) {
            if (!(live && act[it])) continue;
            const size_t at = (size_t)row * c + (size_t)(sl.chunk0 + it * WAVE) * VEC;
            float dz[VEC];
#pragma unroll
            for (int e = 0; e < VEC; e++) dz[e] = grad_o != nullptr ? rstd * ((g[it][e] - m1) - xh[it][e] * m2) : 0.0f;
            if (grad_z != nullptr) {
                float rz[VEC];
                load_chunk<VEC>(grad_z, at, POINTOPS2_ROWS_F32, rz);
#pragma unroll
                for (int e = 0; e < VEC; e++) dz[e] = dz[e] + rz[e];
            }
            store_chunk<VEC>(grad_x, at, POINTOPS2_ROWS_F32, dz);
            if (grad_y != nullptr) {
                if (s != nullptr) {
#pragma unroll
                    for (int e = 0; e < VEC; e++) dz[e] = sc * dz[e];
                }
                store_chunk<VEC>(grad_y, at, y_type, dz);
            }
        }
    }
    if (partials == nullptr) return;  // (kernel-uniform)
    // the workgroup's sums per channel: the segments of a wave by an xor butterfly (a tree), then the four waves in order through LDS
    const int w = threadIdx.x >> 6, lane = lane_id();
#pragma unroll
    for (int it = 0; it < ITER; it++) {
#pragma unroll
        for (int e = 0; e < VEC; e++) {
            for (int st = seg; st < WAVE; st <<= 1) {
                ag[it][e] += __shfl_xor(ag[it][e], st, WAVE);
                ab[it][e] += __shfl_xor(ab[it][e], st, WAVE);
            }
            const int at = ((w * ITER + it) * WAVE + lane) * VEC + e;
            red[0][at] = ag[it][e];
            red[1][at] = ab[it][e];
        }
    }
    __syncthreads();
    float *out = partials + (size_t)blockIdx.x * 2 * c;
    for (int ch = threadIdx.x; ch < c; ch += RN_THREADS) {
        const int chunk = ch / VEC, e = ch - chunk * VEC, it = chunk >> 6, lane0 = chunk & 63;  // (segment 0 of the wave holds the wave's sum)
        float tg = 0.0f, tb = 0.0f;
        for (int ww = 0; ww < RN_WAVES; ww++) {
            const int at = ((ww * ITER + it) * WAVE + lane0) * VEC + e;
            tg += red[0][at];
            tb += red[1][at];
        }
        out[ch] = tg;
        out[c + ch] = tb;
    }
}

// grad_gamma | grad_beta [cols = 2 C] = the column sums of partials [rows][cols]: row b in group b % 64, ascending; then the groups by halving
__global__ __launch_bounds__(RED_COLS *RED_GROUPS) void rownorm_param_kernel(int rows, int c, const float *__restrict__ partials,
                                                                             float *__restrict__ grad_gamma, float *__restrict__ grad_beta) {
    __shared__ float red[RED_GROUPS][RED_COLS];
    const int cols = 2 * c, lc = threadIdx.x % RED_COLS, grp = threadIdx.x / RED_COLS, col = blockIdx.x * RED_COLS + lc;
    float acc = 0.0f;
    if (col < cols)
        for (int b = grp; b < rows; b += RED_GROUPS) acc += partials[(size_t)b * cols + col];
    red[grp][lc] = acc;
    __syncthreads();
    for (int half = RED_GROUPS / 2; half > 0; half >>= 1) {  // group q takes group q + half: a fixed tree
        if (grp < half) red[grp][lc] += red[grp + half][lc];
        __syncthreads();
    }
    if (grp == 0 && col < cols) {
        if (col < c) grad_gamma[col] = red[0][lc];
        else grad_beta[col - c] = red[0][lc];
    }
}

// nullptr when the arguments are in range
const char *rownorm_bad_args(int n, int c, int y_type, int o_type) {
    if (n < 0) return "residual_norm: negative row count";
    if (c < 1 || c > RN_MAX_C) return "residual_norm: c must be in [1, 1024]";
    if (!known_row_type(y_type) || !known_row_type(o_type)) return "residual_norm: row types must be POINTOPS2_ROWS_F32, _F16 or _BF16";
    return nullptr;  // (n * c: the kernels index with 64-bit offsets)
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

}  // namespace
}  // namespace p2

using namespace p2;

extern "C" {

void residual_norm_forward_launcher(int n, int c, int y_type, int o_type, const float *x, const void *y, const float *s, const float *gamma,
                                    const float *beta, float eps, float *z, void *o, float *stat) {
    const hipStream_t st = begin_launch().stream;
    if (const char *bad = rownorm_bad_args(n, c, y_type, o_type)) { set_error(bad); return; }
    if (n == 0) return;
    if (x == nullptr || gamma == nullptr || beta == nullptr || o == nullptr || stat == nullptr) {
        set_error("residual_norm_forward: x, gamma, beta, o and stat must not be NULL");
        return;
    }
    const bool chunked = c % 4 == 0 && aligned_to(x, 16) && aligned_to(z, 16) && aligned_to(gamma, 16) && aligned_to(beta, 16) &&
                         rows_aligned(y, y_type) && rows_aligned(o, o_type);
    const RowShape sh(c, chunked);
    for_shape(sh, [&](auto tag) {
        hipLaunchKernelGGL((rownorm_fwd_kernel<decltype(tag)::vec, decltype(tag)::iter>), dim3(sh.grid(n, num_cus() * 64)), dim3(RN_THREADS), 0, st,
                           n, c, sh.chunks, sh.seg, y_type, o_type, x, y, s, gamma, beta, eps, z, o, stat);
    });
    check_launch();
}

void residual_norm_backward_launcher(int n, int c, int y_type, int o_type, const void *grad_o, const float *grad_z, const float *z,
                                     const float *stat, const float *s, const float *gamma, float *grad_x, void *grad_y, float *partials,
                                     int partial_rows, float *grad_gamma, float *grad_beta) {
    const hipStream_t st = begin_launch().stream;
    if (const char *bad = rownorm_bad_args(n, c, y_type, o_type)) { set_error(bad); return; }
    if (n == 0) return;
    if (grad_x == nullptr) { set_error("residual_norm_backward: grad_x is NULL"); return; }
    if (grad_o != nullptr && (z == nullptr || stat == nullptr || gamma == nullptr)) {
        set_error("residual_norm_backward: grad_o needs z, stat and gamma");
        return;
    }
    const bool sums = grad_o != nullptr && partials != nullptr;
    if (sums && (partial_rows < 1 || grad_gamma == nullptr || grad_beta == nullptr)) {
        set_error("residual_norm_backward: partials needs partial_rows >= 1, grad_gamma and grad_beta");
        return;
    }
    const bool chunked = c % 4 == 0 && aligned_to(grad_z, 16) && aligned_to(z, 16) && aligned_to(gamma, 16) && aligned_to(grad_x, 16) &&
                         rows_aligned(grad_o, o_type) && rows_aligned(grad_y, y_type);
    const RowShape sh(c, chunked);
    const int grid = sh.grid(n, sums ? partial_rows : num_cus() * 64);
    for_shape(sh, [&](auto tag) {
        hipLaunchKernelGGL((rownorm_bwd_kernel<decltype(tag)::vec, decltype(tag)::iter>), dim3(grid), dim3(RN_THREADS), 0, st, n, c, sh.chunks,
                           sh.seg, y_type, o_type, grad_o, grad_z, z, stat, s, gamma, grad_x, grad_y, sums ? partials : nullptr);
    });
    if (!check_launch()) return;
    if (sums) {
        hipLaunchKernelGGL(rownorm_param_kernel, dim3(div_up(2 * c, RED_COLS)), dim3(RED_COLS * RED_GROUPS), 0, st, grid, c, partials, grad_gamma,
                           grad_beta);
        check_launch();
    }
}

}  // extern "C"
