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
// gamma, beta, s, stat are fp32.  The stream x / z / dx / dZ, y / dy and o / dO each have one of the three row types POINTOPS2_ROWS_*
// (x_type, y_type, o_type), widened exactly and rounded once.  The stream is fp32 without autocast and in the first stage; behind a
// TransitionDown under autocast it is half.  With a half stream z is rounded ONCE to the stream type, and mean, variance, stat and o are
// those of the STORED z widened back - the LayerNorm of the tensor the caller holds, which the backward reads again; dx = round(dz) and
// dy = round(s * dz) both start from the unrounded fp32 dz.  x_type fp32: the rounding is the identity, the bits are those of the fp32 kernels.
//
// Lanes (row_lanes.h): a lane owns a chunk of four channels, a row a power-of-two segment of lanes, 64 / seg rows side by side in a wave;
// the row sums are an xor butterfly over the aligned segment: every lane of it ends with the same bits, and no value crosses a
// segment - a NaN stays in its row.  One channel per lane where c % 4 != 0 or an operand is misaligned: same results.
//
// dgamma / dbeta without float atomics: every lane adds dO * xhat and dO of its channels over its rows in ascending row order; a
// workgroup then adds, per channel, its lanes' sums - the segments of a wave by an xor butterfly, the four waves in order through LDS -
// and writes one row of `partials` [workgroups][2][C]; rownorm_param_kernel adds those rows in the fixed order of column_reduce
// (row_lanes.h).  The backward's grid is capped by the rows of `partials` the caller provides.  The order is
// a function of the shapes alone: the same bits from run to run on one device.
#include "row_lanes.h"

namespace p2 {
namespace {

template <int VEC, int ITER>
__global__ __launch_bounds__(RN_THREADS) void rownorm_fwd_kernel(int n, int c, int chunks, int seg, int x_type, int y_type, int o_type,
                                                                 const void *__restrict__ x, const void *__restrict__ y,
                                                                 const float *__restrict__ s, const float *__restrict__ gamma,
                                                                 const float *__restrict__ beta, float eps, void *__restrict__ z,
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
                load_chunk<VEC>(x, at, x_type, v[it]);
                if (y != nullptr) {
                    float yv[VEC];
                    load_chunk<VEC>(y, at, y_type, yv);
#pragma unroll
                    for (int e = 0; e < VEC; e++) {
                        const float t = s != nullptr ? sc * yv[e] : yv[e];
                        v[it][e] = v[it][e] + t;
                    }
                    if (x_type != POINTOPS2_ROWS_F32) {  // (wave-uniform) the row is what the stored z holds
#pragma unroll
                        for (int e = 0; e < VEC; e++) v[it][e] = widen16(narrow16(v[it][e], x_type), x_type);
                    }
                }
                if (z != nullptr) store_chunk<VEC>(z, at, x_type, v[it]);
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
__global__ __launch_bounds__(RN_THREADS) void rownorm_bwd_kernel(int n, int c, int chunks, int seg, int x_type, int y_type, int o_type,
                                                                 const void *__restrict__ grad_o, const void *__restrict__ grad_z,
                                                                 const void *__restrict__ z, const float *__restrict__ stat,
                                                                 const float *__restrict__ s, const float *__restrict__ gamma,
                                                                 void *__restrict__ grad_x, void *__restrict__ grad_y,
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
                    load_chunk<VEC>(z, at, x_type, zv);
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
                load_chunk<VEC>(grad_z, at, x_type, rz);
#pragma unroll
                for (int e = 0; e < VEC; e++) dz[e] = dz[e] + rz[e];
            }
            store_chunk<VEC>(grad_x, at, x_type, dz);  // (grad_y below starts from the unrounded dz)
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
    // the workgroup's sums per channel
    float *out = partials + (size_t)blockIdx.x * 2 * c;
    const auto add = [](float p, float q) { return p + q; };
    workgroup_columns<VEC, ITER>(ag, c, seg, 0.0f, red[0], add, [&](int ch, float t) { out[ch] = t; });
    workgroup_columns<VEC, ITER>(ab, c, seg, 0.0f, red[1], add, [&](int ch, float t) { out[c + ch] = t; });
}

// grad_gamma | grad_beta [cols = 2 C] = the column sums of partials [rows][cols]: row b in group b % 64, ascending; then the groups by halving
__global__ __launch_bounds__(RED_COLS *RED_GROUPS) void rownorm_param_kernel(int rows, int c, const float *__restrict__ partials,
                                                                             float *__restrict__ grad_gamma, float *__restrict__ grad_beta) {
    param_sums(rows, c, partials, grad_gamma, grad_beta);
}

// nullptr when the arguments are in range
const char *rownorm_bad_args(int n, int c, int x_type, int y_type, int o_type) {
    if (n < 0) return "residual_norm: negative row count";
    if (c < 1 || c > RN_MAX_C) return "residual_norm: c must be in [1, 1024]";
    if (!known_row_type(x_type) || !known_row_type(y_type) || !known_row_type(o_type))
        return "residual_norm: row types must be POINTOPS2_ROWS_F32, _F16 or _BF16";
    return nullptr;  // (n * c: the kernels index with 64-bit offsets)
}

}  // namespace
}  // namespace p2

using namespace p2;

extern "C" {

void residual_norm_stream_forward_launcher(int n, int c, int x_type, int y_type, int o_type, const void *x, const void *y, const float *s,
                                           const float *gamma, const float *beta, float eps, void *z, void *o, float *stat) {
    const hipStream_t st = begin_launch().stream;
    if (const char *bad = rownorm_bad_args(n, c, x_type, y_type, o_type)) { set_error(bad); return; }
    if (n == 0) return;
    if (x == nullptr || gamma == nullptr || beta == nullptr || o == nullptr || stat == nullptr) {
        set_error("residual_norm_forward: x, gamma, beta, o and stat must not be NULL");
        return;
    }
    const bool chunked = c % 4 == 0 && rows_aligned(x, x_type) && rows_aligned(z, x_type) && aligned_to(gamma, 16) && aligned_to(beta, 16) &&
                         rows_aligned(y, y_type) && rows_aligned(o, o_type);
    const RowShape sh(c, chunked);
    for_shape(sh, [&](auto tag) {
        hipLaunchKernelGGL((rownorm_fwd_kernel<decltype(tag)::vec, decltype(tag)::iter>), dim3(sh.grid(n, num_cus() * 64)), dim3(RN_THREADS), 0, st,
                           n, c, sh.chunks, sh.seg, x_type, y_type, o_type, x, y, s, gamma, beta, eps, z, o, stat);
    });
    check_launch();
}

void residual_norm_stream_backward_launcher(int n, int c, int x_type, int y_type, int o_type, const void *grad_o, const void *grad_z,
                                            const void *z, const float *stat, const float *s, const float *gamma, void *grad_x, void *grad_y,
                                            float *partials, int partial_rows, float *grad_gamma, float *grad_beta) {
    const hipStream_t st = begin_launch().stream;
    if (const char *bad = rownorm_bad_args(n, c, x_type, y_type, o_type)) { set_error(bad); return; }
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
    const bool chunked = c % 4 == 0 && rows_aligned(grad_z, x_type) && rows_aligned(z, x_type) && aligned_to(gamma, 16) &&
                         rows_aligned(grad_x, x_type) && rows_aligned(grad_o, o_type) && rows_aligned(grad_y, y_type);
    const RowShape sh(c, chunked);
    const int grid = sh.grid(n, sums ? partial_rows : num_cus() * 64);
    for_shape(sh, [&](auto tag) {
        hipLaunchKernelGGL((rownorm_bwd_kernel<decltype(tag)::vec, decltype(tag)::iter>), dim3(grid), dim3(RN_THREADS), 0, st, n, c, sh.chunks,
                           sh.seg, x_type, y_type, o_type, grad_o, grad_z, z, stat, s, gamma, grad_x, grad_y, sums ? partials : nullptr);
    });
    if (!check_launch()) return;
    if (sums) {
        hipLaunchKernelGGL(rownorm_param_kernel, dim3(div_up(2 * c, RED_COLS)), dim3(RED_COLS * RED_GROUPS), 0, st, grid, c, partials, grad_gamma,
                           grad_beta);
        check_launch();
    }
}

// the fp32 stream: the pair above with x_type = POINTOPS2_ROWS_F32
void residual_norm_forward_launcher(int n, int c, int y_type, int o_type, const float *x, const void *y, const float *s, const float *gamma,
                                    const float *beta, float eps, float *z, void *o, float *stat) {
    residual_norm_stream_forward_launcher(n, c, POINTOPS2_ROWS_F32, y_type, o_type, x, y, s, gamma, beta, eps, z, o, stat);
}

void residual_norm_backward_launcher(int n, int c, int y_type, int o_type, const void *grad_o, const float *grad_z, const float *z,
                                     const float *stat, const float *s, const float *gamma, float *grad_x, void *grad_y, float *partials,
                                     int partial_rows, float *grad_gamma, float *grad_beta) {
    residual_norm_stream_backward_launcher(n, c, POINTOPS2_ROWS_F32, y_type, o_type, grad_o, grad_z, z, stat, s, gamma, grad_x, grad_y, partials,
                                           partial_rows, grad_gamma, grad_beta);
}

}  // extern "C"
