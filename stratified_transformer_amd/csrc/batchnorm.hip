// BatchNorm1d over point rows + activation (+ residual add) in fused passes: the per-row glue of the stem and the heads
// (model/stratified_transformer.py:358 `activation(bn(kpconv))`, :367-368 `Linear, FastBatchNorm1d, LeakyReLU`, :391 `feats += shortcut`,
// :426-443 `Linear, BatchNorm1d, ReLU | Tanh, Linear`).  All arithmetic in fp32, nothing fused (the project builds with
// -ffp-contract=off and no fmaf is written here):
//
//   training  mean_c = sum_n x / N     var_c = sum_n (x - mean_c)^2 / N     rstd_c = 1 / sqrt(var_c + eps)     stat = (mean, rstd) [2, C]
//             running_mean = (1 - m) running_mean + m mean_c     running_var = (1 - m) running_var + m M2_c / (N - 1)   (on the device)
//   eval      mean_c = running_mean     rstd_c = 1 / sqrt(running_var + eps)
//   forward   pre[n,c] = ((x[n,c] - mean_c) * rstd_c) * gamma[c] + beta[c]     o[n,c] = act(pre[n,c]) (+ residual[n,c])
//   backward  xhat and pre recomputed from x and stat     g = dO * act'(pre)     dbeta[c] = sum_n g     dgamma[c] = sum_n g * xhat
//             training: dx = (gamma * rstd) * ((g - dbeta / N) - xhat * (dgamma / N))          eval: dx = (g * gamma) * rstd
//   act       none | relu (pre <= 0 ? 0 : pre) | leaky_relu (pre > 0 ? pre : pre * slope) | tanh (tanhf; its derivative 1 - tanhf(pre)^2 from
//             the forward's own expression); the derivative's branch is the forward's, so a NaN takes torch's side of each
//
// x / o / dO / dx share one of the three row types POINTOPS2_ROWS_*, the residual has one of its own; each is widened exactly and
// rounded once.  gamma, beta, stat, the running statistics and the parameter gradients are fp32.
//
// Variance without E[x^2] - mean^2 (1.125 for 1.0445 on 333 rows of 1e3 + N(0, 1)) and in ONE pass over x: every lane adds, per channel,
// d = x - K and d * d over its rows in ascending order, K being the first value it saw in that channel - a shift inside the column's own
// range, so the sums hold deviations, not magnitudes - and turns them into (count, mean, M2) = (cnt, K + S1 / cnt, S2 - S1 * (S1 / cnt)).
// From there on partial results merge by Chan's formula only (delta = mean_b - mean_a; mean = mean_a + delta * n_b / n; M2 = M2_a + M2_b +
// delta^2 * n_a n_b / n; the one place that leaves fp32: each merge is formed in double and rounded once), in a fixed tree: the segments of a wave by an xor butterfly, the four waves in order through LDS
// (workgroup_columns, row_lanes.h), one row of `partials` [workgroups][3][C] per workgroup, and bn_stat_kernel merges those rows in
// the order of column_reduce.  A constant column gives S1 = S2 = 0 and every delta 0: mean = K and M2 = 0 exactly.  The dgamma / dbeta
// sums travel the same way with `+` as the merge.  No float atomics; every order is a function of the shapes alone: the same bits from
// run to run on one device.  Lanes: row_lanes.h (four channels a lane, rows side by side in a wave; one channel a lane as the fallback).
//
// Several ranks (training under SyncBatchNorm): the statistics are those of all ranks' rows.  Each rank runs the moments pass and merges its
// workgroups' partials into ONE row (count, mean, M2) [3][C] (bn_row_kernel, column_reduce's order); the rows are gathered by the caller
// - a copy, no arithmetic - and bn_merge_kernel Chan-merges them strictly in rank order 0 .. world-1, one thread per channel: the same
// rows give the same (mean, rstd), count and running statistics on every rank.  Backward: each rank's (sum g * xhat, sum g) [2][C] from the
// SUMS pass, gathered likewise; the dx pass adds the rows in rank order in its per-lane channel set-up (world * 2 * C floats per workgroup
// from L2 against a launch and a dependent kernel for a [2][C] buffer: the set-up is once per lane, the row loop is untouched) and
// divides by the global count, which it reads on the device.  Counts are fp32: exact below 2^24 rows.
#include "row_lanes.h"

namespace p2 {
namespace {

constexpr int BN_PARTIAL_ROWS_MAX = 1024;
constexpr int BN_WORLD_MAX = 1024;  // ranks whose rows one merge takes

struct Moments {
    float n, mean, m2;  // of the values merged so far: their number, their mean, the sum of their squared deviations from it
};
__device__ __forceinline__ Moments lanes_xor(Moments m, int st) {
    return Moments{__shfl_xor(m.n, st, WAVE), __shfl_xor(m.mean, st, WAVE), __shfl_xor(m.m2, st, WAVE)};
}
// Chan et al.: the moments of the union of two disjoint sets.  Each result is formed in double and rounded once: in fp32 the mean took three
// roundings the size of delta per level of the tree, and with one row a lane (n <= rows_per_wg) delta is the column's whole spread - 7 rows
// of 8 channels left dx at five times torch's error, outside the tests' bar; rounded once it is at twice.  A merge runs once per lane
// and level after the row loop, never per row.
__device__ __forceinline__ Moments chan_merge(Moments a, Moments b) {
    if (b.n == 0.0f) return a;
    if (a.n == 0.0f) return b;
    const double na = a.n, nb = b.n, n = na + nb, delta = (double)b.mean - (double)a.mean;
    return Moments{(float)n, (float)((double)a.mean + delta * (nb / n)), (float)(((double)a.m2 + (double)b.m2) + (delta * delta) * (na * nb / n))};
}

__device__ __forceinline__ float bn_act(float pre, int act, float slope) {
    if (act == POINTOPS2_ACT_RELU) return pre <= 0.0f ? 0.0f : pre;
    if (act == POINTOPS2_ACT_LEAKY_RELU) return pre > 0.0f ? pre : pre * slope;
    if (act == POINTOPS2_ACT_TANH) return tanhf(pre);
    return pre;
}
// dO * act'(pre)
__device__ __forceinline__ float bn_act_grad(float pre, float go, int act, float slope) {
    if (act == POINTOPS2_ACT_RELU) return pre <= 0.0f ? 0.0f : go;
    if (act == POINTOPS2_ACT_LEAKY_RELU) return pre > 0.0f ? go : go * slope;
    if (act == POINTOPS2_ACT_TANH) {
        const float t = tanhf(pre);
        return go * (1.0f - t * t);
    }
    return go;
}

// what a lane keeps of its channels for the whole launch
template <int VEC, int ITER>
struct Channels {
    bool act[ITER];
    float mean[ITER][VEC], rstd[ITER][VEC], gm[ITER][VEC], bt[ITER][VEC];
    // scale: rstd, or with scale_is_var the variance (eval mode reads the running statistics where they are)
    __device__ __forceinline__ Channels(const SegLanes &sl, int chunks, const float *__restrict__ mean_, const float *__restrict__ scale,
                                        bool scale_is_var, float eps, const float *__restrict__ gamma, const float *__restrict__ beta) {
#pragma unroll
        for (int it = 0; it < ITER; it++) {
            const int chunk = sl.chunk0 + it * WAVE;
            act[it] = chunk < chunks;
#pragma unroll
            for (int e = 0; e < VEC; e++) mean[it][e] = rstd[it][e] = gm[it][e] = bt[it][e] = 0.0f;
            if (!act[it]) continue;
            const size_t at = (size_t)chunk * VEC;
            load_chunk<VEC>(mean_, at, POINTOPS2_ROWS_F32, mean[it]);
            load_chunk<VEC>(scale, at, POINTOPS2_ROWS_F32, rstd[it]);
            load_chunk<VEC>(gamma, at, POINTOPS2_ROWS_F32, gm[it]);
            load_chunk<VEC>(beta, at, POINTOPS2_ROWS_F32, bt[it]);
            if (scale_is_var) {
#pragma unroll
                for (int e = 0; e < VEC; e++) rstd[it][e] = 1.0f / sqrtf(rstd[it][e] + eps);
            }
        }
    }
};

// partials[workgroup] = (count, mean, M2) [3][c] of the workgroup's rows
template <int VEC, int ITER>
__global__ __launch_bounds__(RN_THREADS) void bn_moments_kernel(int n, int c, int chunks, int seg, int x_type, const void *__restrict__ x,
                                                                float *__restrict__ partials) {
    __shared__ Moments red[RN_THREADS * ITER * VEC];
    const SegLanes sl(seg);
    bool act[ITER];
    float k[ITER][VEC], s1[ITER][VEC], s2[ITER][VEC];
#pragma unroll
    for (int it = 0; it < ITER; it++) {
        act[it] = sl.chunk0 + it * WAVE < chunks;
#pragma unroll
        for (int e = 0; e < VEC; e++) k[it][e] = s1[it][e] = s2[it][e] = 0.0f;
    }
    float cnt = 0.0f;
    const long long wave = (long long)blockIdx.x * RN_WAVES + (threadIdx.x >> 6), waves = (long long)gridDim.x * RN_WAVES;
    for (long long first = wave * sl.per_wave; first < n; first += waves * sl.per_wave) {
        const long long row = first + sl.sub;
        if (row >= n) continue;
#pragma unroll
        for (int it = 0; it < ITER; it++) {
            if (!act[it]) continue;
            float xv[VEC];
            load_chunk<VEC>(x, (size_t)row * c + (size_t)(sl.chunk0 + it * WAVE) * VEC, x_type, xv);
#pragma unroll
            for (int e = 0; e < VEC; e++) {
                if (cnt == 0.0f) k[it][e] = xv[e];
                const float d = xv[e] - k[it][e];
                s1[it][e] += d;
                s2[it][e] += d * d;
            }
        }
        cnt += 1.0f;
    }
    Moments m[ITER][VEC];
#pragma unroll
    for (int it = 0; it < ITER; it++) {
#pragma unroll
        for (int e = 0; e < VEC; e++) {
            m[it][e] = Moments{0.0f, 0.0f, 0.0f};
            if (act[it] && cnt > 0.0f) {
                const float off = s1[it][e] / cnt, m2 = s2[it][e] - s1[it][e] * off;
                m[it][e] = Moments{cnt, k[it][e] + off, m2 < 0.0f ? 0.0f : m2};  // (a NaN stays a NaN)
            }
        }
    }
    float *out = partials + (size_t)blockIdx.x * 3 * c;
    workgroup_columns<VEC, ITER>(m, c, seg, Moments{0.0f, 0.0f, 0.0f}, red, [](Moments p, Moments q) { return chan_merge(p, q); }, [&](int ch, Moments t) {
        out[ch] = t.n;
        out[c + ch] = t.mean;
        out[2 * c + ch] = t.m2;
    });
}

// stat = (mean, rstd) [2][c] from the rows of partials, and the running statistics' update where they are given
__global__ __launch_bounds__(RED_COLS *RED_GROUPS) void bn_stat_kernel(int rows, int c, int n, const float *__restrict__ partials, float eps,
                                                                       float momentum, float *__restrict__ running_mean,
                                                                       float *__restrict__ running_var, float *__restrict__ stat) {
    __shared__ Moments red[RED_GROUPS][RED_COLS];
    const int col = blockIdx.x * RED_COLS + threadIdx.x % RED_COLS;
    const Moments m = column_reduce(rows, col < c, Moments{0.0f, 0.0f, 0.0f}, red, [&](int b) {
        const float *p = partials + (size_t)b * 3 * c + col;
        return Moments{p[0], p[c], p[2 * (size_t)c]};
    }, [](Moments p, Moments q) { return chan_merge(p, q); });
    if (threadIdx.x < RED_COLS && col < c) {
        const float fn = (float)n;
        stat[col] = m.mean;
        stat[c + col] = 1.0f / sqrtf(m.m2 / fn + eps);
        if (running_mean != nullptr) running_mean[col] = (1.0f - momentum) * running_mean[col] + momentum * m.mean;
        if (running_var != nullptr) running_var[col] = (1.0f - momentum) * running_var[col] + momentum * (m.m2 / (fn - 1.0f));  // unbiased, as torch
    }
}

// row = (count, mean, M2) [3][c]: the rows of partials merged as bn_stat_kernel merges them (rows == 0: a row of zeros)
__global__ __launch_bounds__(RED_COLS *RED_GROUPS) void bn_row_kernel(int rows, int c, const float *__restrict__ partials, float *__restrict__ row) {
    __shared__ Moments red[RED_GROUPS][RED_COLS];
    const int col = blockIdx.x * RED_COLS + threadIdx.x % RED_COLS;
    const Moments m = column_reduce(rows, col < c, Moments{0.0f, 0.0f, 0.0f}, red, [&](int b) {
        const float *p = partials + (size_t)b * 3 * c + col;
        return Moments{p[0], p[c], p[2 * (size_t)c]};
    }, [](Moments p, Moments q) { return chan_merge(p, q); });
    if (threadIdx.x < RED_COLS && col < c) {
        row[col] = m.n;
        row[c + col] = m.mean;
        row[2 * c + col] = m.m2;
    }
}

// stat = (mean, rstd) [2][c] and total = the summed count from the ranks' rows [world][3][c], merged in rank order (an empty rank's row is
// skipped by chan_merge); the running statistics' update where they are given.  One thread per channel.
__global__ __launch_bounds__(WAVE) void bn_merge_kernel(int world, int c, const float *__restrict__ rows, float eps, float momentum,
                                                        float *__restrict__ running_mean, float *__restrict__ running_var,
                                                        float *__restrict__ stat, float *__restrict__ total) {
    const int col = blockIdx.x * WAVE + threadIdx.x;
    if (col >= c) return;
    Moments m{0.0f, 0.0f, 0.0f};
    for (int r = 0; r < world; r++) {
        const float *p = rows + (size_t)r * 3 * c + col;
        m = chan_merge(m, Moments{p[0], p[c], p[2 * (size_t)c]});
    }
    stat[col] = m.mean;
    stat[c + col] = 1.0f / sqrtf(m.m2 / m.n + eps);
    if (m.n > 0.0f) {
        if (running_mean != nullptr) running_mean[col] = (1.0f - momentum) * running_mean[col] + momentum * m.mean;
        if (running_var != nullptr) running_var[col] = (1.0f - momentum) * running_var[col] + momentum * (m.m2 / (m.n - 1.0f));  // unbiased, as torch
    }
    if (col == 0) total[0] = m.n;  // (every channel holds the same count)
}

template <int VEC, int ITER>
__global__ __launch_bounds__(RN_THREADS) void bn_fwd_kernel(int n, int c, int chunks, int seg, int x_type, int r_type, int act, float slope,
                                                            const void *__restrict__ x, const float *__restrict__ mean,
                                                            const float *__restrict__ scale, int scale_is_var, float eps,
                                                            const float *__restrict__ gamma, const float *__restrict__ beta,
                                                            const void *__restrict__ residual, void *__restrict__ o, float *__restrict__ stat_out) {
    const SegLanes sl(seg);
    const Channels<VEC, ITER> ch(sl, chunks, mean, scale, scale_is_var != 0, eps, gamma, beta);
    const long long wave = (long long)blockIdx.x * RN_WAVES + (threadIdx.x >> 6), waves = (long long)gridDim.x * RN_WAVES;
    if (stat_out != nullptr && wave == 0 && sl.sub == 0) {  // (mean, rstd) as this pass used them, for the backward
#pragma unroll
        for (int it = 0; it < ITER; it++) {
            if (!ch.act[it]) continue;
            const size_t at = (size_t)(sl.chunk0 + it * WAVE) * VEC;
            store_chunk<VEC>(stat_out, at, POINTOPS2_ROWS_F32, ch.mean[it]);
            store_chunk<VEC>(stat_out, (size_t)c + at, POINTOPS2_ROWS_F32, ch.rstd[it]);
        }
    }
    for (long long first = wave * sl.per_wave; first < n; first += waves * sl.per_wave) {
        const long long row = first + sl.sub;
        if (row >= n) continue;
#pragma unroll
        for (int it = 0; it < ITER; it++) {
            if (!ch.act[it]) continue;
            const size_t at = (size_t)row * c + (size_t)(sl.chunk0 + it * WAVE) * VEC;
            float v[VEC];
            load_chunk<VEC>(x, at, x_type, v);
#pragma unroll
            for (int e = 0; e < VEC; e++) v[e] = bn_act(((v[e] - ch.mean[it][e]) * ch.rstd[it][e]) * ch.gm[it][e] + ch.bt[it][e], act, slope);
            if (residual != nullptr) {
                float rv[VEC];
                load_chunk<VEC>(residual, at, r_type, rv);
#pragma unroll
                for (int e = 0; e < VEC; e++) v[e] = v[e] + rv[e];
            }
            store_chunk<VEC>(o, at, x_type, v);
        }
    }
}

// SUMS: partials[workgroup] = (sum g * xhat, sum g) [2][c] of the workgroup's rows.  else: grad_x, from the finished sums.
// SYNC (grad_x only): sum_gx / sum_g are rows 0 / 1 of the first of `world` gathered sum rows [world][2][c], added here in rank order,
// and the row count is total[0], the ranks' summed count
template <int VEC, int ITER, bool SUMS, bool SYNC = false>
__global__ __launch_bounds__(RN_THREADS) void bn_bwd_kernel(int n, int c, int chunks, int seg, int x_type, int act, float slope, int training,
                                                            const void *__restrict__ x, const void *__restrict__ grad_o,
                                                            const float *__restrict__ stat, const float *__restrict__ gamma,
                                                            const float *__restrict__ beta, const float *__restrict__ sum_gx,
                                                            const float *__restrict__ sum_g, float *__restrict__ partials,
                                                            void *__restrict__ grad_x, int world, const float *__restrict__ total) {
    __shared__ float red[SUMS ? 2 : 1][SUMS ? RN_THREADS * ITER * VEC : 1];
    const SegLanes sl(seg);
    const Channels<VEC, ITER> ch(sl, chunks, stat, stat + c, false, 0.0f, gamma, beta);
    float a[ITER][VEC], b[ITER][VEC];  // SUMS: the lane's sums of g * xhat and g;  else: dgamma / N and dbeta / N
    float fn = (float)n;
    if constexpr (SYNC) fn = total[0];
#pragma unroll
    for (int it = 0; it < ITER; it++) {
#pragma unroll
        for (int e = 0; e < VEC; e++) a[it][e] = b[it][e] = 0.0f;
        if (!SUMS && training && ch.act[it]) {
            const size_t at = (size_t)(sl.chunk0 + it * WAVE) * VEC;
            load_chunk<VEC>(sum_gx, at, POINTOPS2_ROWS_F32, a[it]);
            load_chunk<VEC>(sum_g, at, POINTOPS2_ROWS_F32, b[it]);
            if constexpr (SYNC) {
                for (int r = 1; r < world; r++) {  // rank order: the same sums on every rank
                    float ar[VEC], br[VEC];
                    load_chunk<VEC>(sum_gx, (size_t)r * 2 * c + at, POINTOPS2_ROWS_F32, ar);
                    load_chunk<VEC>(sum_g, (size_t)r * 2 * c + at, POINTOPS2_ROWS_F32, br);
#pragma unroll
                    for (int e = 0; e < VEC; e++) a[it][e] += ar[e], b[it][e] += br[e];
                }
            }
#pragma unroll
            for (int e = 0; e < VEC; e++) a[it][e] = a[it][e] / fn, b[it][e] = b[it][e] / fn;
        }
    }
    const long long wave = (long long)blockIdx.x * RN_WAVES + (threadIdx.x >> 6), waves = (long long)gridDim.x * RN_WAVES;
    for (long long first = wave * sl.per_wave; first < n; first += waves * sl.per_wave) {
        const long long row = first + sl.sub;
        if (row >= n) continue;
#pragma unroll
        for (int it = 0; it < ITER; it++) {
            if (!ch.act[it]) continue;
            const size_t at = (size_t)row * c + (size_t)(sl.chunk0 + it * WAVE) * VEC;
            float xv[VEC], gv[VEC];
            load_chunk<VEC>(x, at, x_type, xv);
            load_chunk<VEC>(grad_o, at, x_type, gv);
#pragma unroll
            for (int e = 0; e < VEC; e++) {
                const float xh = (xv[e] - ch.mean[it][e]) * ch.rstd[it][e];
                const float g = bn_act_grad(xh * ch.gm[it][e] + ch.bt[it][e], gv[e], act, slope);
                if constexpr (SUMS) {
                    a[it][e] += g * xh;
                    b[it][e] += g;
                } else {
                    xv[e] = training ? (ch.gm[it][e] * ch.rstd[it][e]) * ((g - b[it][e]) - xh * a[it][e]) : (g * ch.gm[it][e]) * ch.rstd[it][e];
                }
            }
            if constexpr (!SUMS) store_chunk<VEC>(grad_x, at, x_type, xv);
        }
    }
    if constexpr (SUMS) {
        float *out = partials + (size_t)blockIdx.x * 2 * c;
        const auto add = [](float p, float q) { return p + q; };
        workgroup_columns<VEC, ITER>(a, c, seg, 0.0f, red[0], add, [&](int col, float t) { out[col] = t; });
        workgroup_columns<VEC, ITER>(b, c, seg, 0.0f, red[1], add, [&](int col, float t) { out[c + col] = t; });
    }
}

// grad_gamma | grad_beta [cols = 2 C] = the column sums of partials [rows][cols]
__global__ __launch_bounds__(RED_COLS *RED_GROUPS) void bn_param_kernel(int rows, int c, const float *__restrict__ partials,
                                                                        float *__restrict__ grad_gamma, float *__restrict__ grad_beta) {
    param_sums(rows, c, partials, grad_gamma, grad_beta);
}

// nullptr when the arguments are in range
const char *bn_bad_args(int n, int c, int x_type, int r_type, int act) {
    if (n < 0) return "batch_norm_act: negative row count";
    if (c < 1 || c > RN_MAX_C) return "batch_norm_act: c must be in [1, 1024]";
    if (!known_row_type(x_type) || !known_row_type(r_type)) return "batch_norm_act: row types must be POINTOPS2_ROWS_F32, _F16 or _BF16";
    if (act < POINTOPS2_ACT_NONE || act > POINTOPS2_ACT_TANH) return "batch_norm_act: act must be POINTOPS2_ACT_NONE, _RELU, _LEAKY_RELU or _TANH";
    return nullptr;  // (n * c: the kernels index with 64-bit offsets)
}
bool bad_partial_rows(int rows) { return rows < 1 || rows > BN_PARTIAL_ROWS_MAX; }

}  // namespace
}  // namespace p2

using namespace p2;

extern "C" {

void batch_norm_act_stats_launcher(int n, int c, int x_type, const void *x, float *partials, int partial_rows, float eps, float momentum,
                                   float *running_mean, float *running_var, float *stat) {
    const hipStream_t st = begin_launch().stream;
    if (const char *bad = bn_bad_args(n, c, x_type, POINTOPS2_ROWS_F32, POINTOPS2_ACT_NONE)) { set_error(bad); return; }
    if (n == 0) return;
    if (x == nullptr || partials == nullptr || stat == nullptr || bad_partial_rows(partial_rows)) {
        set_error("batch_norm_act_stats: x, partials and stat must not be NULL, partial_rows in [1, 1024]");
        return;
    }
    const RowShape sh(c, c % 4 == 0 && rows_aligned(x, x_type));
    const int grid = sh.grid(n, partial_rows);
    for_shape(sh, [&](auto tag) {
        hipLaunchKernelGGL((bn_moments_kernel<decltype(tag)::vec, decltype(tag)::iter>), dim3(grid), dim3(RN_THREADS), 0, st, n, c, sh.chunks, sh.seg,
                           x_type, x, partials);
    });
    if (!check_launch()) return;
    hipLaunchKernelGGL(bn_stat_kernel, dim3(div_up(c, RED_COLS)), dim3(RED_COLS * RED_GROUPS), 0, st, grid, c, n, partials, eps, momentum,
                       running_mean, running_var, stat);
    check_launch();
}

void batch_norm_act_forward_launcher(int n, int c, int x_type, int r_type, int act, float slope, const void *x, const float *mean,
                                     const float *scale, int scale_is_var, float eps, const float *gamma, const float *beta,
                                     const void *residual, void *o, float *stat_out) {
    const hipStream_t st = begin_launch().stream;
    if (const char *bad = bn_bad_args(n, c, x_type, r_type, act)) { set_error(bad); return; }
    if (n == 0) return;
    if (x == nullptr || mean == nullptr || scale == nullptr || gamma == nullptr || beta == nullptr || o == nullptr) {
        set_error("batch_norm_act_forward: x, mean, scale, gamma, beta and o must not be NULL");
        return;
    }
    const bool chunked = c % 4 == 0 && rows_aligned(x, x_type) && rows_aligned(o, x_type) && rows_aligned(residual, r_type) && aligned_to(mean, 16) &&
                         aligned_to(scale, 16) && aligned_to(gamma, 16) && aligned_to(beta, 16) && aligned_to(stat_out, 16);
    const RowShape sh(c, chunked);
    for_shape(sh, [&](auto tag) {
        hipLaunchKernelGGL((bn_fwd_kernel<decltype(tag)::vec, decltype(tag)::iter>), dim3(sh.grid(n, num_cus() * 64)), dim3(RN_THREADS), 0, st, n, c,
                           sh.chunks, sh.seg, x_type, r_type, act, slope, x, mean, scale, scale_is_var, eps, gamma, beta, residual, o, stat_out);
    });
    check_launch();
}

void batch_norm_act_backward_launcher(int n, int c, int x_type, int act, float slope, int training, const void *x, const void *grad_o,
                                      const float *stat, const float *gamma, const float *beta, float *partials, int partial_rows,
                                      float *grad_gamma, float *grad_beta, void *grad_x) {
    const hipStream_t st = begin_launch().stream;
    if (const char *bad = bn_bad_args(n, c, x_type, POINTOPS2_ROWS_F32, act)) { set_error(bad); return; }
    if (n == 0) return;
    if (x == nullptr || grad_o == nullptr || stat == nullptr || gamma == nullptr || beta == nullptr) {
        set_error("batch_norm_act_backward: x, grad_o, stat, gamma and beta must not be NULL");
        return;
    }
    const bool sums = partials != nullptr;
    if (sums && (bad_partial_rows(partial_rows) || grad_gamma == nullptr || grad_beta == nullptr)) {
        set_error("batch_norm_act_backward: partials needs partial_rows in [1, 1024], grad_gamma and grad_beta");
        return;
    }
    if (grad_x != nullptr && training && (grad_gamma == nullptr || grad_beta == nullptr)) {
        set_error("batch_norm_act_backward: grad_x in training mode needs the sums grad_gamma and grad_beta");
        return;
    }
    const bool chunked = c % 4 == 0 && rows_aligned(x, x_type) && rows_aligned(grad_o, x_type) && rows_aligned(grad_x, x_type) && aligned_to(stat, 16) &&
                         aligned_to(gamma, 16) && aligned_to(beta, 16) && aligned_to(grad_gamma, 16) && aligned_to(grad_beta, 16);
    const RowShape sh(c, chunked);
    if (sums) {
        const int grid = sh.grid(n, partial_rows);
        for_shape(sh, [&](auto tag) {
            hipLaunchKernelGGL((bn_bwd_kernel<decltype(tag)::vec, decltype(tag)::iter, true>), dim3(grid), dim3(RN_THREADS), 0, st, n, c, sh.chunks,
                               sh.seg, x_type, act, slope, training, x, grad_o, stat, gamma, beta, (const float *)nullptr, (const float *)nullptr,
                               partials, (void *)nullptr, 0, (const float *)nullptr);
        });
        if (!check_launch()) return;
        hipLaunchKernelGGL(bn_param_kernel, dim3(div_up(2 * c, RED_COLS)), dim3(RED_COLS * RED_GROUPS), 0, st, grid, c, partials, grad_gamma,
                           grad_beta);
        if (!check_launch()) return;
    }
    if (grad_x != nullptr) {
        for_shape(sh, [&](auto tag) {
            hipLaunchKernelGGL((bn_bwd_kernel<decltype(tag)::vec, decltype(tag)::iter, false>), dim3(sh.grid(n, num_cus() * 64)), dim3(RN_THREADS), 0,
                               st, n, c, sh.chunks, sh.seg, x_type, act, slope, training, x, grad_o, stat, gamma, beta, grad_gamma, grad_beta,
                               (float *)nullptr, grad_x, 0, (const float *)nullptr);
        });
        check_launch();
    }
}

void batch_norm_act_moments_launcher(int n, int c, int x_type, const void *x, float *partials, int partial_rows, float *row) {
    const hipStream_t st = begin_launch().stream;
    if (const char *bad = bn_bad_args(n, c, x_type, POINTOPS2_ROWS_F32, POINTOPS2_ACT_NONE)) { set_error(bad); return; }
    if (row == nullptr || (n > 0 && (x == nullptr || partials == nullptr || bad_partial_rows(partial_rows)))) {
        set_error("batch_norm_act_moments: row - and with n > 0 x and partials - must not be NULL, partial_rows in [1, 1024]");
        return;
    }
    int grid = 0;
    if (n > 0) {
        const RowShape sh(c, c % 4 == 0 && rows_aligned(x, x_type));
        grid = sh.grid(n, partial_rows);
        for_shape(sh, [&](auto tag) {
            hipLaunchKernelGGL((bn_moments_kernel<decltype(tag)::vec, decltype(tag)::iter>), dim3(grid), dim3(RN_THREADS), 0, st, n, c, sh.chunks,
                               sh.seg, x_type, x, partials);
        });
        if (!check_launch()) return;
    }
    hipLaunchKernelGGL(bn_row_kernel, dim3(div_up(c, RED_COLS)), dim3(RED_COLS * RED_GROUPS), 0, st, grid, c, partials, row);
    check_launch();
}

void batch_norm_act_merge_launcher(int world, int c, const float *rows, float eps, float momentum, float *running_mean, float *running_var,
                                   float *stat, float *total) {
    const hipStream_t st = begin_launch().stream;
    if (const char *bad = bn_bad_args(0, c, POINTOPS2_ROWS_F32, POINTOPS2_ROWS_F32, POINTOPS2_ACT_NONE)) { set_error(bad); return; }
    if (world < 1 || world > BN_WORLD_MAX || rows == nullptr || stat == nullptr || total == nullptr ||
        (running_mean == nullptr) != (running_var == nullptr)) {
        set_error("batch_norm_act_merge: world in [1, 1024]; rows, stat and total must not be NULL; running_mean and running_var go together");
        return;
    }
    hipLaunchKernelGGL(bn_merge_kernel, dim3(div_up(c, WAVE)), dim3(WAVE), 0, st, world, c, rows, eps, momentum, running_mean, running_var, stat,
                       total);
    check_launch();
}

void batch_norm_act_sync_backward_launcher(int n, int c, int x_type, int act, float slope, const void *x, const void *grad_o, const float *stat,
                                           const float *gamma, const float *beta, int world, const float *sums, const float *total,
                                           void *grad_x) {
    const hipStream_t st = begin_launch().stream;
    if (const char *bad = bn_bad_args(n, c, x_type, POINTOPS2_ROWS_F32, act)) { set_error(bad); return; }
    if (world < 1 || world > BN_WORLD_MAX) { set_error("batch_norm_act_sync_backward: world must be in [1, 1024]"); return; }
    if (n == 0) return;
    if (x == nullptr || grad_o == nullptr || stat == nullptr || gamma == nullptr || beta == nullptr || sums == nullptr || total == nullptr ||
        grad_x == nullptr) {
        set_error("batch_norm_act_sync_backward: x, grad_o, stat, gamma, beta, sums, total and grad_x must not be NULL");
        return;
    }
    const bool chunked = c % 4 == 0 && rows_aligned(x, x_type) && rows_aligned(grad_o, x_type) && rows_aligned(grad_x, x_type) && aligned_to(stat, 16) &&
                         aligned_to(gamma, 16) && aligned_to(beta, 16) && aligned_to(sums, 16);
    const RowShape sh(c, chunked);
    for_shape(sh, [&](auto tag) {
        hipLaunchKernelGGL((bn_bwd_kernel<decltype(tag)::vec, decltype(tag)::iter, false, true>), dim3(sh.grid(n, num_cus() * 64)), dim3(RN_THREADS), 0,
                           st, n, c, sh.chunks, sh.seg, x_type, act, slope, 1, x, grad_o, stat, gamma, beta, sums, sums + c, (float *)nullptr, grad_x,
                           world, total);
    });
    check_launch();
}

}  // extern "C"
