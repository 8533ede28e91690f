// KPConv neighbourhood aggregation (rigid kernel points, linear influence, sum aggregation): the stem of the model
// (model/stratified_transformer.py:344-392).  Restated from the published behaviour of torch_points3d 1.3.0
// (modules/KPConv/kernels.py, kernel_utils.py: KPConv_ops) - third party, not under the reference: PARITY UNPINNED.
//
//   w[i,k,n]  = max(0, 1 - |(support[j] - query[i]) - K[k]| / extent),  j = neighbors[i,n], 0 for j outside [0, n_s)
//               (max as torch.clamp(min=0): a NaN coordinate gives a NaN influence; an infinitely distant point weighs 0)
//   wf[i,k,:] = sum_n w[i,k,n] * feat[j,:]                              forward  (this file)
//   gf[j,:]  += sum_k w[i,k,n] * grad_wf[i,k,:]                         backward (this file; w recomputed)
// The product of wf [n_q, K*c] with the layer's weight [K*c, out] and its two gradients are matrix products (pointops.py).
//
// One wave per query, everything of the query staged once in the wave's LDS slice:
//   1. lane n reads neighbour n; a ballot compacts the valid ones (order kept), their relative coordinates and ids go to LDS
//      - the padding of a ball query (a third of the row on a surface) costs nothing after this step;
//   2. the valid rows of feat (forward) / the query's grad_wf rows (backward) are copied to LDS, consecutive lanes on
//      consecutive floats;
//   3. every influence w[k,n] is computed once, by one lane, into LDS (row stride odd: lanes on different k hit different banks);
//   4. forward: lane t owns the output float t = k * c + ch of the query's [K, c] block and walks the neighbours in index order
//      - no atomics, a fixed summation order (bitwise reproducible), and stores of consecutive floats;
//      backward: lane t owns (neighbour n, channel ch), sums over k on chip and issues ONE float atomic per (neighbour, channel):
//      consecutive lanes add into consecutive floats of a row of grad_feat.
#include "common.h"

namespace p2 {
namespace {

constexpr int KP_WAVES = 4;  // queries in flight per workgroup
constexpr int KP_MAX_C = 64, KP_MAX_NB = 64, KP_MAX_KP = 32;

// floats of LDS: [K points 3 * n_kp, padded to 4] then per wave [rel 3 * n_nb][ids n_nb][rows max(n_nb, n_kp) * c][w n_kp * ws]
struct KpLayout {
    int ws, kp_floats, rows_off, w_off, wave_floats;
    __host__ __device__ KpLayout(int n_nb, int c, int n_kp) {
        ws = n_nb | 1;
        kp_floats = (3 * n_kp + 3) & ~3;
        rows_off = 4 * n_nb;
        w_off = rows_off + (n_nb > n_kp ? n_nb : n_kp) * c;
        wave_floats = (w_off + n_kp * ws + 3) & ~3;
    }
    __host__ size_t bytes() const { return sizeof(float) * ((size_t)kp_floats + (size_t)KP_WAVES * wave_floats); }
};

__device__ __forceinline__ void lds_fence() {
    __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): this wave's LDS writes have landed
    __builtin_amdgcn_wave_barrier();
}
// t / d for 0 <= t < 4096, 1 <= d <= 64 with inv = 1.0f / d: (t + 0.5) / d is at least 1 / 128 away from an integer
__device__ __forceinline__ int small_div(int t, float inv) { return (int)(((float)t + 0.5f) * inv); }

// steps 1 and 3 for query i; returns the number of valid neighbours (wave-uniform).  rel: x | y | z planes of n_nb floats.
__device__ __forceinline__ int stage_query(int i, int n_s, int n_nb, int n_kp, float extent,
                                           const float *__restrict__ query_xyz, const float *__restrict__ support_xyz,
                                           const int *__restrict__ neighbors, const float *kp, float *rel, int *ids, float *w, int ws) {
    const int lane = lane_id();
    int j = -1;
    if (lane < n_nb) j = neighbors[(size_t)i * n_nb + lane];
    const bool valid = j >= 0 && j < n_s;
    const unsigned long long mask = __ballot(valid);
    const int n_valid = __popcll(mask);
    if (valid) {
        const int pos = __popcll(mask & ((1ull << lane) - 1ull));
        const float qx = query_xyz[(size_t)i * 3], qy = query_xyz[(size_t)i * 3 + 1], qz = query_xyz[(size_t)i * 3 + 2];
        rel[pos] = support_xyz[(size_t)j * 3] - qx;
        rel[n_nb + pos] = support_xyz[(size_t)j * 3 + 1] - qy;
        rel[2 * n_nb + pos] = support_xyz[(size_t)j * 3 + 2] - qz;
        ids[pos] = j;
    }
    lds_fence();
    if (n_valid > 0) {
        const float inv_nv = 1.0f / (float)n_valid;
        for (int t = lane; t < n_kp * n_valid; t += WAVE) {
            const int k = small_div(t, inv_nv), n = t - k * n_valid;
            const float dx = rel[n] - kp[3 * k], dy = rel[n_nb + n] - kp[3 * k + 1], dz = rel[2 * n_nb + n] - kp[3 * k + 2];
            const float d = sqrtf(dx * dx + dy * dy + dz * dz);
            const float v = 1.0f - d / extent;
            w[k * ws + n] = v < 0.0f ? 0.0f : v;  // torch.clamp(min=0): a NaN stays NaN (fmaxf would give 0)
        }
    }
    return n_valid;
}

__global__ __launch_bounds__(KP_WAVES * WAVE) void kpconv_aggregate_fwd_kernel(
    int n_q, int n_s, int n_nb, int c, int n_kp, const float *__restrict__ query_xyz, const float *__restrict__ support_xyz,
    const int *__restrict__ neighbors, const float *__restrict__ feat, const float *__restrict__ k_points, float extent,
    float *__restrict__ wf) {
    extern __shared__ __attribute__((aligned(16))) float kp_lds[];
    const KpLayout lay(n_nb, c, n_kp);
    const int wave = threadIdx.x >> 6, lane = lane_id();
    float *kp = kp_lds, *rel = kp_lds + lay.kp_floats + wave * lay.wave_floats, *rows = rel + lay.rows_off, *w = rel + lay.w_off;
    int *ids = reinterpret_cast<int *>(rel + 3 * n_nb);
    for (int t = threadIdx.x; t < 3 * n_kp; t += KP_WAVES * WAVE) kp[t] = k_points[t];
    __syncthreads();
    const float inv_c = 1.0f / (float)c;
    const int out_floats = n_kp * c;
    for (int i = blockIdx.x * KP_WAVES + wave; i < n_q; i += gridDim.x * KP_WAVES) {
        const int n_valid = stage_query(i, n_s, n_nb, n_kp, extent, query_xyz, support_xyz, neighbors, kp, rel, ids, w, lay.ws);
        for (int t = lane; t < n_valid * c; t += WAVE) {
            const int n = small_div(t, inv_c), ch = t - n * c;
            rows[t] = feat[(size_t)ids[n] * c + ch];
        }
        lds_fence();
        float *out = wf + (size_t)i * out_floats;
        for (int t = lane; t < out_floats; t += WAVE) {
            const int k = small_div(t, inv_c), ch = t - k * c;
            const float *wk = w + k * lay.ws;
            float acc = 0.0f;
            for (int n = 0; n < n_valid; n++) acc = fmaf(wk[n], rows[n * c + ch], acc);
            out[t] = acc;
        }
        __builtin_amdgcn_wave_barrier();  // the next query's staging stays behind these LDS reads
    }
}

__global__ __launch_bounds__(KP_WAVES * WAVE) void kpconv_aggregate_bwd_kernel(
    int n_q, int n_s, int n_nb, int c, int n_kp, const float *__restrict__ query_xyz, const float *__restrict__ support_xyz,
    const int *__restrict__ neighbors, const float *__restrict__ k_points, float extent, const float *__restrict__ grad_wf,
    float *__restrict__ grad_feat) {
    extern __shared__ __attribute__((aligned(16))) float kp_lds[];
    const KpLayout lay(n_nb, c, n_kp);
    const int wave = threadIdx.x >> 6, lane = lane_id();
    float *kp = kp_lds, *rel = kp_lds + lay.kp_floats + wave * lay.wave_floats, *rows = rel + lay.rows_off, *w = rel + lay.w_off;
    int *ids = reinterpret_cast<int *>(rel + 3 * n_nb);
    for (int t = threadIdx.x; t < 3 * n_kp; t += KP_WAVES * WAVE) kp[t] = k_points[t];
    __syncthreads();
    const float inv_c = 1.0f / (float)c;
    const int in_floats = n_kp * c;
    for (int i = blockIdx.x * KP_WAVES + wave; i < n_q; i += gridDim.x * KP_WAVES) {
        const int n_valid = stage_query(i, n_s, n_nb, n_kp, extent, query_xyz, support_xyz, neighbors, kp, rel, ids, w, lay.ws);
        if (n_valid > 0) {
            const float *g = grad_wf + (size_t)i * in_floats;
            for (int t = lane; t < in_floats; t += WAVE) rows[t] = g[t];
        }
        lds_fence();
        for (int t = lane; t < n_valid * c; t += WAVE) {
            const int n = small_div(t, inv_c), ch = t - n * c;
            float acc = 0.0f;
            for (int k = 0; k < n_kp; k++) acc = fmaf(w[k * lay.ws + n], rows[k * c + ch], acc);
            atomicAdd(grad_feat + (size_t)ids[n] * c + ch, acc);  // ids[n] in [0, n_s): checked when it was staged
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// nullptr when the arguments are in range
const char *kpconv_bad_args(int n_q, int n_s, int n_nb, int c, int n_kp, float extent) {
    if (n_q < 0 || n_s < 0) return "kpconv_aggregate: negative point count";
    if (c < 1 || c > KP_MAX_C) return "kpconv_aggregate: c must be in [1, 64]";
    if (n_nb < 1 || n_nb > KP_MAX_NB) return "kpconv_aggregate: n_nb must be in [1, 64]";
    if (n_kp < 1 || n_kp > KP_MAX_KP) return "kpconv_aggregate: n_kp must be in [1, 32]";
    if (!(extent > 0.0f) || !(extent <= 3.0e38f)) return "kpconv_aggregate: extent must be positive and finite";
    return nullptr;
}
inline int kpconv_grid(int n_q) {
    const int want = div_up(n_q, KP_WAVES), cap = num_cus() * 16;
    return want < cap ? want : cap;
}

}  // namespace
}  // namespace p2

using namespace p2;

extern "C" {

void kpconv_aggregate_forward_launcher(int n_q, int n_s, int n_nb, int c, int n_kp, const float *query_xyz, const float *support_xyz,
                                       const int *neighbors, const float *feat, const float *k_points, float extent, float *wf) {
    const hipStream_t st = begin_launch().stream;
    if (const char *bad = kpconv_bad_args(n_q, n_s, n_nb, c, n_kp, extent)) { set_error(bad); return; }
    if (n_q == 0) return;
    const size_t lds = KpLayout(n_nb, c, n_kp).bytes();
    allow_big_lds(kpconv_aggregate_fwd_kernel, lds);
    hipLaunchKernelGGL(kpconv_aggregate_fwd_kernel, dim3(kpconv_grid(n_q)), dim3(KP_WAVES * WAVE), lds, st, n_q, n_s, n_nb, c, n_kp,
                       query_xyz, support_xyz, neighbors, feat, k_points, extent, wf);
    check_launch();
}

void kpconv_aggregate_backward_launcher(int n_q, int n_s, int n_nb, int c, int n_kp, const float *query_xyz, const float *support_xyz,
                                        const int *neighbors, const float *k_points, float extent, const float *grad_wf,
                                        float *grad_feat) {
    const hipStream_t st = begin_launch().stream;
    if (const char *bad = kpconv_bad_args(n_q, n_s, n_nb, c, n_kp, extent)) { set_error(bad); return; }
    if (n_q == 0 || n_s == 0) return;
    const size_t lds = KpLayout(n_nb, c, n_kp).bytes();
    allow_big_lds(kpconv_aggregate_bwd_kernel, lds);
    hipLaunchKernelGGL(kpconv_aggregate_bwd_kernel, dim3(kpconv_grid(n_q)), dim3(KP_WAVES * WAVE), lds, st, n_q, n_s, n_nb, c, n_kp,
                       query_xyz, support_xyz, neighbors, k_points, extent, grad_wf, grad_feat);
    check_launch();
}

}  // extern "C"
