// Gather-add: the arithmetic of the decoder's Upsample (model/stratified_transformer.py:341) behind its kNN search - the weighted sum
// of k source rows (lib/pointops2/functions/pointops.py:767-769) and the add of the support row - in one pass, and its backward by
// source row.
//
//   forward:   t = 0; for i = 0 .. k-1: t = t + (float(feat[idx[n, i], ch]) * weight[n, i]);  out[n, ch] = float(base[n, ch]) + t
//   backward:  grad_feat[j, ch] = sum over the pairs (n, i) with idx[n, i] == j of (grad_out[n, ch] * weight[n, i])
//
// Every product is rounded, then every add (__fmul_rn / __fadd_rn: nothing contracts to an FMA), in the order written: the reference's
// loop and its `+`, operation for operation.  feat and base are rows of f32, f16 or bf16, each of its own type, widened exactly; out
// and grad_out are fp32.  An idx entry outside [0, m) is skipped and its row never read; out and grad_feat are fully written.
//
// Both kernels are pure gathers on the lanes of gather_rows.h: a lane owns one 16-byte chunk of a feat row (4 floats, 8 halves), a row
// of `chunks` < 64 chunks is a group of that many lanes and 64 / chunks rows sit side by side in a wave; wider rows take a whole wave.
//   forward:   the row group loads the row's indices and weights GA_NB at a time (one address per row: a broadcast), then the GA_NB
//              feat chunks that depend on them, then multiplies and adds in index order.  A row of more than 64 chunks keeps up to
//              GA_WIDE chunks per lane in registers under ONE walk of its indices, so a row's k indices and weights are loaded once.
//   backward:  by SOURCE row through the key-major view of idx (pointops2_csc_build: per source row its pair ids n * k + i,
//              ascending): per pair the weight and the grad_out chunk of its fine row; fp32 accumulation from 0 in pair order, one
//              rounding to feat's row type, every row of grad_feat written.  No atomics, no zero-fill, the same bits from run to run.
// Channel counts that are no multiple of the chunk, or operands that are not aligned for the chunk accesses, take one thread per
// element: the same operations in the same order, the same bits.
#include "gather_rows.h"
#include "row_lanes.h"

namespace p2 {
namespace {

constexpr int GA_MAX_K = 64, GA_MAX_C = 1024;
constexpr int GA_NB = 4;    // neighbours / pairs in flight per lane (the decoder's k = 3: one batch)
constexpr int GA_WIDE = 4;  // chunks per lane of a row of more than 64 chunks (1024 fp32 channels = 256 chunks)

// VEC (4 or 8) consecutive elements of a base row of type rt as floats: the 4-element accesses of row_lanes.h
template <int VEC>
__device__ __forceinline__ void load_base(const void *__restrict__ base, size_t e, int rt, float *v) {
#pragma unroll
    for (int q = 0; q < VEC / 4; q++) load_chunk<4>(base, e + 4 * q, rt, v + 4 * q);
}

// ITER chunks per lane, WAVE apart: 1 for rows of up to 64 chunks, GA_WIDE beyond
template <typename FT, int ITER>
__global__ __launch_bounds__(GATHER_WAVES * WAVE) void gather_add_fwd_kernel(int n, int m, int k, int c, int chunks, const void *__restrict__ feat,
                                                                             const int *__restrict__ idx, const float *__restrict__ weight,
                                                                             const void *__restrict__ base, int base_type,
                                                                             float *__restrict__ out) {
    typedef Chunk<FT> C;
    constexpr int VEC = C::VEC;
    const RowLanes rl(chunks);
    const size_t row_bytes = (size_t)c * sizeof(FT);
    const int wave = blockIdx.x * GATHER_WAVES + (threadIdx.x >> 6), waves = gridDim.x * GATHER_WAVES;
    for (long long first = (long long)wave * rl.per_wave; first < n; first += (long long)waves * rl.per_wave) {
        const long long r = first + rl.sub;
        if (rl.sub >= rl.per_wave || r >= n) continue;  // (no cross-lane step below: lanes may leave)
        const int *row_idx = idx + (size_t)r * k;
        const float *row_w = weight + (size_t)r * k;
        float t[ITER][VEC];
#pragma unroll
        for (int it = 0; it < ITER; it++)
#pragma unroll
            for (int e = 0; e < VEC; e++) t[it][e] = 0.0f;
        for (int i0 = 0; i0 < k; i0 += GA_NB) {
            int j[GA_NB];
            float w[GA_NB];
#pragma unroll
            for (int u = 0; u < GA_NB; u++) {
                j[u] = i0 + u < k ? row_idx[i0 + u] : -1;
                w[u] = i0 + u < k ? row_w[i0 + u] : 0.0f;
            }
#pragma unroll
            for (int it = 0; it < ITER; it++) {
                const int ch = rl.chunk0 + it * WAVE;
                if (ch >= chunks) continue;
                C v[GA_NB];
#pragma unroll
                for (int u = 0; u < GA_NB; u++) {  // an entry outside [0, m) loads nothing and adds nothing
                    v[u].bits = make_uint4(0u, 0u, 0u, 0u);
                    if ((unsigned)j[u] < (unsigned)m) v[u].bits = ld16(feat, (size_t)j[u] * row_bytes + (size_t)ch * 16);
                }
#pragma unroll
                for (int u = 0; u < GA_NB; u++) {
                    if ((unsigned)j[u] >= (unsigned)m) continue;
#pragma unroll
                    for (int e = 0; e < VEC; e++) t[it][e] = __fadd_rn(t[it][e], __fmul_rn(v[u].get(e), w[u]));
                }
            }
        }
#pragma unroll
        for (int it = 0; it < ITER; it++) {
            const int ch = rl.chunk0 + it * WAVE;
            if (ch >= chunks) continue;
            const size_t e0 = (size_t)r * c + (size_t)ch * VEC;
            if (base != nullptr) {
                float b[VEC];
                load_base<VEC>(base, e0, base_type, b);
#pragma unroll
                for (int e = 0; e < VEC; e++) t[it][e] = __fadd_rn(b[e], t[it][e]);
            }
#pragma unroll
            for (int q = 0; q < VEC / 4; q++) stg4(out + e0 + 4 * q, make_float4(t[it][4 * q], t[it][4 * q + 1], t[it][4 * q + 2], t[it][4 * q + 3]));
        }
    }
}

// one thread per (fine row, channel): any c, any alignment
template <typename FT>
__global__ __launch_bounds__(256) void gather_add_fwd_scalar_kernel(int n, int m, int k, int c, const void *__restrict__ feat,
                                                                    const int *__restrict__ idx, const float *__restrict__ weight,
                                                                    const void *__restrict__ base, int base_type, float *__restrict__ out) {
    const FT *f = reinterpret_cast<const FT *>(feat);
    const long long total = (long long)n * c;
    for (long long x = (long long)blockIdx.x * blockDim.x + threadIdx.x; x < total; x += (long long)gridDim.x * blockDim.x) {
        const long long r = x / c;
        const int ch = (int)(x - r * c);
        float t = 0.0f;
        for (int i = 0; i < k; i++) {
            const int j = idx[(size_t)r * k + i];
            if ((unsigned)j >= (unsigned)m) continue;
            t = __fadd_rn(t, __fmul_rn(ld_elem(&f[(size_t)j * c + ch]), weight[(size_t)r * k + i]));
        }
        if (base != nullptr) {
            float b;
            load_chunk<1>(base, (size_t)x, base_type, &b);
            t = __fadd_rn(b, t);
        }
        out[x] = t;
    }
}

template <typename FT>
__global__ __launch_bounds__(GATHER_WAVES * WAVE) void gather_add_bwd_kernel(int n, int m, int k, int c, int chunks,
                                                                             const float *__restrict__ grad_out, const float *__restrict__ weight,
                                                                             const int *__restrict__ src_offsets, const int *__restrict__ src_pair,
                                                                             void *__restrict__ grad_feat) {
    typedef Chunk<FT> C;
    constexpr int VEC = C::VEC;
    const RowLanes rl(chunks);
    const int n_pairs = n * k;  // (fits: the launcher checked)
    const int wave = blockIdx.x * GATHER_WAVES + (threadIdx.x >> 6), waves = gridDim.x * GATHER_WAVES;
    for (long long first = (long long)wave * rl.per_wave; first < m; first += (long long)waves * rl.per_wave) {
        const long long j = first + rl.sub;
        if (rl.sub >= rl.per_wave || j >= m) continue;
        int p0, p1;
        pair_range(src_offsets, j, n_pairs, p0, p1);
        for (int ch = rl.chunk0; ch < chunks; ch += WAVE) {
            float acc[VEC];
#pragma unroll
            for (int e = 0; e < VEC; e++) acc[e] = 0.0f;
            for (int p = p0; p < p1; p += GA_NB) {
                int row[GA_NB];  // the pair's fine row, -1: no pair (behind p1, or an id outside the list: skipped, never followed)
                float w[GA_NB];
#pragma unroll
                for (int u = 0; u < GA_NB; u++) {
                    const int q = p + u < p1 ? src_pair[p + u] : -1;
                    const bool ok = (unsigned)q < (unsigned)n_pairs;
                    row[u] = ok ? q / k : -1;
                    w[u] = ok ? weight[q] : 0.0f;  // (weight [n, k] flat: the pair id is its index)
                }
                float4 g[GA_NB][VEC / 4];
#pragma unroll
                for (int u = 0; u < GA_NB; u++)
#pragma unroll
                    for (int q = 0; q < VEC / 4; q++)
                        g[u][q] = row[u] >= 0 ? ldg4(grad_out + (size_t)row[u] * c + (size_t)ch * VEC + 4 * q) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
                for (int u = 0; u < GA_NB; u++) {
                    if (row[u] < 0) continue;
#pragma unroll
                    for (int q = 0; q < VEC / 4; q++) {
                        acc[4 * q + 0] = __fadd_rn(acc[4 * q + 0], __fmul_rn(g[u][q].x, w[u]));
                        acc[4 * q + 1] = __fadd_rn(acc[4 * q + 1], __fmul_rn(g[u][q].y, w[u]));
                        acc[4 * q + 2] = __fadd_rn(acc[4 * q + 2], __fmul_rn(g[u][q].z, w[u]));
                        acc[4 * q + 3] = __fadd_rn(acc[4 * q + 3], __fmul_rn(g[u][q].w, w[u]));
                    }
                }
            }
            st16(grad_feat, ((size_t)j * c + (size_t)ch * VEC) * sizeof(FT), C::pack(acc));
        }
    }
}

template <typename FT>
__global__ __launch_bounds__(256) void gather_add_bwd_scalar_kernel(int n, int m, int k, int c, const float *__restrict__ grad_out,
                                                                    const float *__restrict__ weight, const int *__restrict__ src_offsets,
                                                                    const int *__restrict__ src_pair, void *__restrict__ grad_feat) {
    const int n_pairs = n * k;
    const long long total = (long long)m * c;
    for (long long x = (long long)blockIdx.x * blockDim.x + threadIdx.x; x < total; x += (long long)gridDim.x * blockDim.x) {
        const long long j = x / c;
        const int ch = (int)(x - j * c);
        int p0, p1;
        pair_range(src_offsets, j, n_pairs, p0, p1);
        float acc = 0.0f;
        for (int p = p0; p < p1; p++) {
            const int q = src_pair[p];
            if ((unsigned)q >= (unsigned)n_pairs) continue;
            acc = __fadd_rn(acc, __fmul_rn(grad_out[(size_t)(q / k) * c + ch], weight[q]));
        }
        st_elem(&reinterpret_cast<FT *>(grad_feat)[x], acc);
    }
}

// nullptr when the arguments are in range
const char *gather_add_bad_args(int n, int m, int k, int c, int feat_type) {
    if (n < 0 || m < 0) return "gather_add: negative row count";
    if (k < 1 || k > GA_MAX_K) return "gather_add: k must be in [1, 64]";
    if (c < 1 || c > GA_MAX_C) return "gather_add: c must be in [1, 1024]";
    if (!known_row_type(feat_type)) return "gather_add: feat_type must be POINTOPS2_ROWS_F32, _F16 or _BF16";
    if ((long long)n * k > 0x7fffffffLL) return "gather_add: n * k does not fit the int32 pair ids";
    return nullptr;
}

template <typename FT>
void launch_fwd(hipStream_t st, int n, int m, int k, int c, const void *feat, const int *idx, const float *weight, const void *base,
                int base_type, float *out) {
    constexpr int VEC = Chunk<FT>::VEC;
    const bool chunked = c % VEC == 0 && aligned16(feat) && aligned16(out) && (base == nullptr || rows_aligned(base, base_type));
    const int chunks = c / VEC;
    if (chunked && chunks <= WAVE)
        hipLaunchKernelGGL((gather_add_fwd_kernel<FT, 1>), dim3(chunked_grid(n, chunks)), dim3(GATHER_WAVES * WAVE), 0, st, n, m, k, c, chunks, feat,
                           idx, weight, base, base_type, out);
    else if (chunked)  // (c <= 1024: at most GA_WIDE * 64 chunks)
        hipLaunchKernelGGL((gather_add_fwd_kernel<FT, GA_WIDE>), dim3(chunked_grid(n, chunks)), dim3(GATHER_WAVES * WAVE), 0, st, n, m, k, c, chunks,
                           feat, idx, weight, base, base_type, out);
    else
        hipLaunchKernelGGL(gather_add_fwd_scalar_kernel<FT>, dim3(scalar_grid((long long)n * c)), dim3(256), 0, st, n, m, k, c, feat, idx, weight,
                           base, base_type, out);
}
template <typename FT>
void launch_bwd(hipStream_t st, int n, int m, int k, int c, const float *grad_out, const float *weight, const int *src_offsets,
                const int *src_pair, void *grad_feat) {
    constexpr int VEC = Chunk<FT>::VEC;
    if (c % VEC == 0 && aligned16(grad_out) && aligned16(grad_feat))
        hipLaunchKernelGGL(gather_add_bwd_kernel<FT>, dim3(chunked_grid(m, c / VEC)), dim3(GATHER_WAVES * WAVE), 0, st, n, m, k, c, c / VEC, grad_out,
                           weight, src_offsets, src_pair, grad_feat);
    else
        hipLaunchKernelGGL(gather_add_bwd_scalar_kernel<FT>, dim3(scalar_grid((long long)m * c)), dim3(256), 0, st, n, m, k, c, grad_out, weight,
                           src_offsets, src_pair, grad_feat);
}

}  // namespace
}  // namespace p2

using namespace p2;

extern "C" {

void gather_add_forward_launcher(int n, int m, int k, int c, int feat_type, int base_type, const void *feat, const int *idx,
                                 const float *weight, const void *base, float *out) {
    const hipStream_t st = begin_launch().stream;
    if (const char *bad = gather_add_bad_args(n, m, k, c, feat_type)) { set_error(bad); return; }
    if (base != nullptr && !known_row_type(base_type)) { set_error("gather_add: base_type must be POINTOPS2_ROWS_F32, _F16 or _BF16"); return; }
    if (n == 0) return;
    with_row_type(feat_type, [&](auto tag) {
        launch_fwd<typename decltype(tag)::type>(st, n, m, k, c, feat, idx, weight, base, base_type, out);  // (m = 0: every entry is skipped)
    });
    check_launch();
}

void gather_add_backward_launcher(int n, int m, int k, int c, int feat_type, const float *grad_out, const float *weight,
                                  const int *src_offsets, const int *src_pair, void *grad_feat) {
    const hipStream_t st = begin_launch().stream;
    if (const char *bad = gather_add_bad_args(n, m, k, c, feat_type)) { set_error(bad); return; }
    if (m == 0) return;
    with_row_type(feat_type, [&](auto tag) {
        launch_bwd<typename decltype(tag)::type>(st, n, m, k, c, grad_out, weight, src_offsets, src_pair, grad_feat);  // (n = 0: no pairs, zeros)
    });
    check_launch();
}

}  // extern "C"
