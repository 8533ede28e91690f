// Grouped max pooling: the tail of TransitionDown (model/stratified_transformer.py:106-109).  LayerNorm and the bias-free Linear act
// on one row at a time, so linear(norm(feats[knn])) pooled over the k gathered copies equals, with y = linear(norm(feats)),
//
//   out[i, ch]       = max_n y[idx[i, n], ch]            arg[i, ch] = the smallest n that attains it      forward  (this file)
//   grad_y[j, ch]    = sum over (i, n) with idx[i, n] == j and arg[i, ch] == n of grad_out[i, ch]         backward (this file)
//
// Rules of the forward: nn.MaxPool1d's - the first maximum wins a tie (the kNN returns duplicate rows for a batch element with fewer
// than k points), a NaN among the k values gives NaN (arg: the first NaN); an idx entry outside [0, n_s) is skipped and never read; a
// row without a valid entry gives 0 and arg 255, which no pair matches (no gradient).  The maximum is a selection: exact in every
// row type.
//
// Both kernels are pure gathers.  Lanes over channels in 16-byte chunks (4 floats, 8 halves): a row of 96 floats is 24 lanes, and a
// wave takes 64 / chunks rows at a time; rows of 64 chunks or more take a whole wave, its lanes striding over the chunks.  No LDS,
// no cross-lane traffic.
//   forward:  the lanes of a query load its indices FWD_NB at a time (one address per query: a broadcast), then issue the FWD_NB
//             row loads that depend on them, then compare in index order.  An invalid index loads row 0 and is ignored.
//   backward: by SOURCE row, through the key-major view of idx (pointops2_csc_build: per source row its pair ids i * k + n,
//             ascending): per pair the `arg` chunk, and the grad_out chunk only where a channel of the chunk matches (one pair in k
//             does, per query and channel).  fp32 accumulation in pair order, one rounding to the row type, every row of grad_feat
//             written: no atomics, no zero-fill, the same bits from run to run.
// Channel counts that are no multiple of the chunk (or operands that are not 16-byte aligned) take one thread per element.
#include "gather_rows.h"

namespace p2 {
namespace {

constexpr int GM_MAX_K = 64, GM_MAX_C = 1024;
constexpr int GM_WAVES = GATHER_WAVES;
constexpr int FWD_NB = 16;    // neighbours in flight per lane (the model's k: one batch)
constexpr int BWD_NB = 4;     // pairs in flight per lane (m * k / n_s = 4 at ratio 0.25, k = 16)
constexpr int NO_ARG = 255;

// MaxPool1d's update: the first entry, a larger value, or the first NaN
__device__ __forceinline__ bool takes(float x, float best, int arg) { return arg == NO_ARG || x > best || (x != x && best == best); }

template <typename RT>
__global__ __launch_bounds__(GM_WAVES * WAVE) void grouped_max_fwd_kernel(int m, int n_s, int k, int c, int chunks, const void *__restrict__ feat,
                                                                          const int *__restrict__ idx, void *__restrict__ out,
                                                                          unsigned char *__restrict__ arg) {
    typedef Chunk<RT> C;
    constexpr int VEC = C::VEC;
    const RowLanes rl(chunks);
    const size_t row_bytes = (size_t)c * sizeof(RT);
    const int wave = blockIdx.x * GM_WAVES + (threadIdx.x >> 6), waves = gridDim.x * GM_WAVES;
    for (long long first = (long long)wave * rl.per_wave; first < m; first += (long long)waves * rl.per_wave) {
        const long long i = first + rl.sub;
        if (rl.sub >= rl.per_wave || i >= m) continue;  // (no cross-lane step below: lanes may leave)
        const int *row_idx = idx + (size_t)i * k;
        for (int ch = rl.chunk0; ch < chunks; ch += WAVE) {
            float best[VEC];
            int a[VEC];
#pragma unroll
            for (int e = 0; e < VEC; e++) best[e] = 0.0f, a[e] = NO_ARG;
            for (int n0 = 0; n0 < k; n0 += FWD_NB) {
                int j[FWD_NB];
#pragma unroll
                for (int u = 0; u < FWD_NB; u++) j[u] = n0 + u < k ? row_idx[n0 + u] : -1;
                C v[FWD_NB];
#pragma unroll
                for (int u = 0; u < FWD_NB; u++) {  // an invalid entry reads row 0 (n_s >= 1 here) and is ignored below
                    const int jj = (unsigned)j[u] < (unsigned)n_s ? j[u] : 0;
                    v[u].bits = ld16(feat, (size_t)jj * row_bytes + (size_t)ch * 16);
                }
#pragma unroll
                for (int u = 0; u < FWD_NB; u++) {
                    const bool valid = (unsigned)j[u] < (unsigned)n_s;
#pragma unroll
                    for (int e = 0; e < VEC; e++) {
                        const float x = v[u].get(e);
                        const bool take = valid & takes(x, best[e], a[e]);  // selects, no branch per neighbour
                        best[e] = take ? x : best[e];
                        a[e] = take ? n0 + u : a[e];
                    }
                }
            }
            st16(out, (size_t)i * row_bytes + (size_t)ch * 16, C::pack(best));
            if (arg != nullptr) {
                unsigned w[VEC / 4];
#pragma unroll
                for (int q = 0; q < VEC / 4; q++)
                    w[q] = (unsigned)a[4 * q] | ((unsigned)a[4 * q + 1] << 8) | ((unsigned)a[4 * q + 2] << 16) | ((unsigned)a[4 * q + 3] << 24);
                unsigned *dst = reinterpret_cast<unsigned *>(arg + (size_t)i * c + (size_t)ch * VEC);
#pragma unroll
                for (int q = 0; q < VEC / 4; q++) dst[q] = w[q];
            }
        }
    }
}

// one thread per (query, channel): any c, any alignment
template <typename RT>
__global__ __launch_bounds__(256) void grouped_max_fwd_scalar_kernel(int m, int n_s, int k, int c, const void *__restrict__ feat,
                                                                     const int *__restrict__ idx, void *__restrict__ out,
                                                                     unsigned char *__restrict__ arg) {
    const RT *f = reinterpret_cast<const RT *>(feat);
    const long long total = (long long)m * c;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
        const long long i = t / c;
        const int ch = (int)(t - i * c);
        float best = 0.0f;
        int a = NO_ARG;
        for (int n = 0; n < k; n++) {
            const int j = idx[(size_t)i * k + n];
            if ((unsigned)j >= (unsigned)n_s) continue;
            const float x = ld_elem(&f[(size_t)j * c + ch]);
            if (takes(x, best, a)) best = x, a = n;
        }
        st_elem(&reinterpret_cast<RT *>(out)[t], best);  // (exact: best is an element of feat, or 0)
        if (arg != nullptr) arg[t] = (unsigned char)a;
    }
}

template <typename RT>
__global__ __launch_bounds__(GM_WAVES * WAVE) void grouped_max_bwd_kernel(int m, int n_s, int k, int c, int chunks,
                                                                          const void *__restrict__ grad_out,
                                                                          const unsigned char *__restrict__ arg,
                                                                          const int *__restrict__ src_offsets,
                                                                          const int *__restrict__ src_pair, void *__restrict__ grad_feat) {
    typedef Chunk<RT> C;
    constexpr int VEC = C::VEC;
    const RowLanes rl(chunks);
    const size_t row_bytes = (size_t)c * sizeof(RT);
    const int n_pairs = m * k;  // (fits: the launcher checked)
    const int wave = blockIdx.x * GM_WAVES + (threadIdx.x >> 6), waves = gridDim.x * GM_WAVES;
    for (long long first = (long long)wave * rl.per_wave; first < n_s; first += (long long)waves * rl.per_wave) {
        const long long j = first + rl.sub;
        if (rl.sub >= rl.per_wave || j >= n_s) continue;
        int p0, p1;
        pair_range(src_offsets, j, n_pairs, p0, p1);
        for (int ch = rl.chunk0; ch < chunks; ch += WAVE) {
            float acc[VEC];
#pragma unroll
            for (int e = 0; e < VEC; e++) acc[e] = 0.0f;
            for (int p = p0; p < p1; p += BWD_NB) {
                int i[BWD_NB], n[BWD_NB];
#pragma unroll
                for (int u = 0; u < BWD_NB; u++) {
                    const int q = p + u < p1 ? src_pair[p + u] : -1;
                    const bool ok = (unsigned)q < (unsigned)n_pairs;  // a pair id outside the list is skipped, never followed
                    i[u] = ok ? q / k : 0;
                    n[u] = ok ? q - i[u] * k : NO_ARG + 1;              // matches no arg byte
                }
                unsigned hit[BWD_NB];  // bit e: channel e of the chunk took its maximum from this pair
#pragma unroll
                for (int u = 0; u < BWD_NB; u++) {
                    const unsigned *src = reinterpret_cast<const unsigned *>(arg + (size_t)i[u] * c + (size_t)ch * VEC);
                    hit[u] = 0u;
#pragma unroll
                    for (int q = 0; q < VEC / 4; q++) {
                        const unsigned w = src[q];
#pragma unroll
                        for (int b = 0; b < 4; b++) hit[u] |= (unsigned)(((w >> (8 * b)) & 0xffu) == (unsigned)n[u]) << (4 * q + b);
                    }
                }
                C g[BWD_NB];
#pragma unroll
                for (int u = 0; u < BWD_NB; u++)
                    if (hit[u] != 0u) g[u].bits = ld16(grad_out, (size_t)i[u] * row_bytes + (size_t)ch * 16);
#pragma unroll
                for (int u = 0; u < BWD_NB; u++) {
                    if (hit[u] == 0u) continue;
#pragma unroll
                    for (int e = 0; e < VEC; e++)
                        if ((hit[u] >> e) & 1u) acc[e] += g[u].get(e);
                }
            }
            st16(grad_feat, (size_t)j * row_bytes + (size_t)ch * 16, C::pack(acc));
        }
    }
}

template <typename RT>
__global__ __launch_bounds__(256) void grouped_max_bwd_scalar_kernel(int m, int n_s, int k, int c, const void *__restrict__ grad_out,
                                                                     const unsigned char *__restrict__ arg,
                                                                     const int *__restrict__ src_offsets, const int *__restrict__ src_pair,
                                                                     void *__restrict__ grad_feat) {
    const RT *g = reinterpret_cast<const RT *>(grad_out);
    const int n_pairs = m * k;
    const long long total = (long long)n_s * c;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
        const long long j = t / c;
        const int ch = (int)(t - j * c);
        int p0, p1;
        pair_range(src_offsets, j, n_pairs, p0, p1);
        float acc = 0.0f;
        for (int p = p0; p < p1; p++) {
            const int q = src_pair[p];
            if ((unsigned)q >= (unsigned)n_pairs) continue;
            const int i = q / k, n = q - i * k;
            if ((int)arg[(size_t)i * c + ch] == n) acc += ld_elem(&g[(size_t)i * c + ch]);
        }
        st_elem(&reinterpret_cast<RT *>(grad_feat)[t], acc);
    }
}

// nullptr when the arguments are in range
const char *grouped_max_bad_args(int m, int n_s, int k, int c, int row_type) {
    if (m < 0 || n_s < 0) return "grouped_max: negative row count";
    if (k < 1 || k > GM_MAX_K) return "grouped_max: k must be in [1, 64]";
    if (c < 1 || c > GM_MAX_C) return "grouped_max: c must be in [1, 1024]";
    if (!known_row_type(row_type)) return "grouped_max: row_type must be POINTOPS2_ROWS_F32, _F16 or _BF16";
    if ((long long)m * k > 0x7fffffffLL) return "grouped_max: m * k does not fit the int32 pair ids";
    return nullptr;
}
// 16-byte chunks per row when the chunked kernels apply (whole chunks, aligned operands), else 0
inline int row_chunks(int c, int vec, const void *a, const void *b, const unsigned char *arg) {
    if (c % vec != 0 || !aligned16(a) || !aligned16(b) || (reinterpret_cast<uintptr_t>(arg) & 3u) != 0) return 0;
    return c / vec;
}

template <typename RT>
void launch_fwd(hipStream_t st, int m, int n_s, int k, int c, const void *feat, const int *idx, void *out, unsigned char *arg) {
    const int chunks = row_chunks(c, Chunk<RT>::VEC, feat, out, arg);
    if (chunks > 0)
        hipLaunchKernelGGL(grouped_max_fwd_kernel<RT>, dim3(chunked_grid(m, chunks)), dim3(GM_WAVES * WAVE), 0, st, m, n_s, k, c, chunks, feat, idx,
                           out, arg);
    else
        hipLaunchKernelGGL(grouped_max_fwd_scalar_kernel<RT>, dim3(scalar_grid((long long)m * c)), dim3(256), 0, st, m, n_s, k, c, feat, idx, out,
                           arg);
}
template <typename RT>
void launch_bwd(hipStream_t st, int m, int n_s, int k, int c, const void *grad_out, const unsigned char *arg, const int *src_offsets,
                const int *src_pair, void *grad_feat) {
    const int chunks = row_chunks(c, Chunk<RT>::VEC, grad_out, grad_feat, arg);
    if (chunks > 0)
        hipLaunchKernelGGL(grouped_max_bwd_kernel<RT>, dim3(chunked_grid(n_s, chunks)), dim3(GM_WAVES * WAVE), 0, st, m, n_s, k, c, chunks, grad_out,
                           arg, src_offsets, src_pair, grad_feat);
    else
        hipLaunchKernelGGL(grouped_max_bwd_scalar_kernel<RT>, dim3(scalar_grid((long long)n_s * c)), dim3(256), 0, st, m, n_s, k, c, grad_out, arg,
                           src_offsets, src_pair, grad_feat);
}

}  // namespace
}  // namespace p2

using namespace p2;

extern "C" {

void grouped_max_forward_launcher(int m, int n_s, int k, int c, int row_type, const void *feat, const int *idx, void *out,
                                  unsigned char *arg) {
    const hipStream_t st = begin_launch().stream;
    if (const char *bad = grouped_max_bad_args(m, n_s, k, c, row_type)) { set_error(bad); return; }
    if (m == 0 || n_s == 0) return;
    with_row_type(row_type, [&](auto tag) { launch_fwd<typename decltype(tag)::type>(st, m, n_s, k, c, feat, idx, out, arg); });
    check_launch();
}

void grouped_max_backward_launcher(int m, int n_s, int k, int c, int row_type, const void *grad_out, const unsigned char *arg,
                                   const int *src_offsets, const int *src_pair, void *grad_feat) {
    const hipStream_t st = begin_launch().stream;
    if (const char *bad = grouped_max_bad_args(m, n_s, k, c, row_type)) { set_error(bad); return; }
    if (m == 0 || n_s == 0) return;
    if (arg == nullptr) { set_error("grouped_max_backward: arg is NULL (the forward was run without it)"); return; }
    with_row_type(row_type, [&](auto tag) {
        launch_bwd<typename decltype(tag)::type>(st, m, n_s, k, c, grad_out, arg, src_offsets, src_pair, grad_feat);
    });
    check_launch();
}

}  // extern "C"
