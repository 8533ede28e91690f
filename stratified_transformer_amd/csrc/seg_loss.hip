// The loss tail of a segmentation training step in one pass over the logits (tool/train.py:336-362: CrossEntropyLoss(ignore_index) on the
// [N, C] class logits, L1Loss on the [N, 3] shift head, their weighted sum; train_backup.py:403: intersectionAndUnionGPU of the argmax),
// and its backward in one pass.  All arithmetic in fp32 on exactly widened operands, nothing fused (-ffp-contract=off, no fmaf here); the
// forward's |shift_pred - shift| alone is taken in double, as the sum it goes into, so that l1 is the float64 value rounded once:
//
//   forward   m_n = max_c x[n,c]     ls_n = log(sum_c exp(x[n,c] - m_n))     stat[n] = (m_n, ls_n)     (lse_n = m_n + ls_n)
//             logp[n,c] = (x[n,c] - m_n) - ls_n        row n is VALID when 0 <= target[n] < C and target[n] != ignore_index
//             loss_n = -logp[n,t]                                                    (eps == 0, t = target[n])
//                    = -((1 - eps) * logp[n,t] + eps / (C - 1) * sum_{c != t} logp[n,c])   (eps > 0: util/common_util.py:180-185)
//             ce = sum_valid loss_n / n_valid     l1 = sum |shift_pred - shift| / (3 N) over ALL rows     total = ce + offset_weight * l1
//             pred_n = argmax_c x[n,c] (first maximum; the first NaN if any); over the valid rows counts[0,k] = #(pred == target == k),
//             counts[1,k] = #(pred == k) + #(target == k) - counts[0,k], counts[2,k] = #(target == k); rows = (valid, label out of range)
//   backward  a = g[0] + g[2]     b = g[1] + offset_weight * g[2]        (g = grad_losses, read on the device, as is n_valid = rows[0])
//             grad_x[n,c] = (a / n_valid) * (exp((x[n,c] - m_n) - ls_n) - w[n,c])   valid rows (w: 1 at t, or 1 - eps at t and eps / (C - 1) elsewhere)
//                         = 0                                                      every other row
//             grad_shift_pred[n,j] = (b / (3 N)) * sign(shift_pred - shift)        sign(0) = 0
//
// The maximum and the log of the sum are kept apart: a row of 1e4 + N(0,1) has an lse whose fp32 spacing is 1e-3, and a softmax rebuilt
// from it alone would be wrong in the fourth digit; (x - m) - ls is what torch's log_softmax keeps, too.
//
// Forward layout.  Rows are 26 to 256 bytes, so a thread per row reading global memory would stride.  A workgroup takes a TILE of
// consecutive rows (256 for C <= 32, 128 above), whose bytes are contiguous: it loads them 16 bytes a lane (a 16-byte aligned base;
// otherwise and for the last few elements one element a lane), widens and stores them as fp32 in LDS at a row stride of C | 1 words -
// odd, so the 32 lanes of a ds_read_b32 group, one row each, fall on 32 different banks.  Thread r then walks row r in LDS: maximum
// and argmax, then the sum of exponentials.  Class counts go to an LDS histogram with LDS integer atomics and leave the workgroup as
// one global integer atomic per non-zero bin; the two float sums are kept per thread in double over its tiles, added over the
// workgroup in a fixed order (xor butterfly per wave, the four waves in order) and written to partials[workgroup];
// seg_loss_finish_kernel adds the partials (lane l takes l, l + 64, ... ascending, then a butterfly) and divides.  No float atomics:
// the order is a function of the shapes alone, so two runs on one device give the same bits.
//
// Backward layout: elementwise.  A workgroup takes the same tiles; a lane takes 16 bytes of logits (4 fp32 or 8 half elements), finds
// the row of each element (a 32-bit division inside the tile), reads that row's target and stat (neighbouring lanes share the cache
// lines), and stores 16 bytes of gradient; the 3 N shift elements follow in the same launch, one element a lane.
#include "row_types.h"

namespace p2 {
namespace {

constexpr int SL_MAX_C = 64;
constexpr int SL_THREADS = 256;
constexpr int SL_WAVES = SL_THREADS / WAVE;
constexpr int SL_TILE_WORDS = 256 * 33;  // 256 rows at a stride of up to 33 words, or 128 rows at up to 65
constexpr int SL_BINS = 3 * SL_MAX_C + 2;

inline __host__ __device__ int tile_rows_of(int c) { return c <= 32 ? 256 : 128; }

__device__ __forceinline__ float load_elem(const void *__restrict__ base, size_t e, int rt) {
    return rt == POINTOPS2_ROWS_F32 ? reinterpret_cast<const float *>(base)[e] : widen16(reinterpret_cast<const unsigned short *>(base)[e], rt);
}
__device__ __forceinline__ void store_elem(void *__restrict__ base, size_t e, int rt, float f) {
    if (rt == POINTOPS2_ROWS_F32) reinterpret_cast<float *>(base)[e] = f;
    else reinterpret_cast<unsigned short *>(base)[e] = (unsigned short)narrow16(f, rt);
}
// a 16-byte piece: 4 fp32 or 8 half elements (v[4..7] are untouched for fp32)
__device__ __forceinline__ void unpack_piece(uint4 w, int rt, float *v) {
    if (rt == POINTOPS2_ROWS_F32) {
        v[0] = __uint_as_float(w.x), v[1] = __uint_as_float(w.y), v[2] = __uint_as_float(w.z), v[3] = __uint_as_float(w.w);
    } else {
        v[0] = widen16(w.x & 0xffffu, rt), v[1] = widen16(w.x >> 16, rt), v[2] = widen16(w.y & 0xffffu, rt), v[3] = widen16(w.y >> 16, rt);
        v[4] = widen16(w.z & 0xffffu, rt), v[5] = widen16(w.z >> 16, rt), v[6] = widen16(w.w & 0xffffu, rt), v[7] = widen16(w.w >> 16, rt);
    }
}
__device__ __forceinline__ uint4 pack_piece(const float *v, int rt) {
    if (rt == POINTOPS2_ROWS_F32) return make_uint4(__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3]));
    return make_uint4(narrow16(v[0], rt) | (narrow16(v[1], rt) << 16), narrow16(v[2], rt) | (narrow16(v[3], rt) << 16),
                      narrow16(v[4], rt) | (narrow16(v[5], rt) << 16), narrow16(v[6], rt) | (narrow16(v[7], rt) << 16));
}
__device__ __forceinline__ const uint4 *piece_ptr(const void *base, size_t first_elem, int rt) {
    return reinterpret_cast<const uint4 *>(reinterpret_cast<const char *>(base) + first_elem * row_elem_bytes(rt));
}

// the rows of a launch in tiles of tile_rows: tile t of workgroup b = b, b + gridDim.x, ...
struct Tiles {
    long long n, count;
    int rows_per;
    __device__ __forceinline__ Tiles(long long n_, int c) : n(n_), rows_per(tile_rows_of(c)) { count = (n + rows_per - 1) / rows_per; }
    __device__ __forceinline__ long long first_row(long long t) const { return t * rows_per; }
    __device__ __forceinline__ int rows(long long t) const {
        const long long left = n - t * rows_per;
        return left < rows_per ? (int)left : rows_per;
    }
};

__global__ __launch_bounds__(SL_THREADS) void seg_loss_fwd_kernel(int n, int c, int x_type, int s_type, int vec, const void *__restrict__ x,
                                                                  const long long *__restrict__ target, const void *__restrict__ shift_pred,
                                                                  const float *__restrict__ shift, long long ignore_index, float eps,
                                                                  float *__restrict__ stat, double *__restrict__ partials,
                                                                  unsigned long long *__restrict__ counts, unsigned long long *__restrict__ rows) {
    __shared__ float tile[SL_TILE_WORDS];
    __shared__ int hist[SL_BINS];  // [0, c): pred == target; [c, 2c): pred; [2c, 3c): target; 3c: valid rows; 3c + 1: labels out of range
    __shared__ double red[2][SL_WAVES];
    const int tid = threadIdx.x, stride = c | 1, per = x_type == POINTOPS2_ROWS_F32 ? 4 : 8;
    for (int i = tid; i < 3 * c + 2; i += SL_THREADS) hist[i] = 0;
    __syncthreads();
    const Tiles tiles(n, c);
    double ce = 0.0, l1 = 0.0;
    for (long long t = blockIdx.x; t < tiles.count; t += gridDim.x) {
        const long long row0 = tiles.first_row(t);
        const int tr = tiles.rows(t), elems = tr * c, pieces = vec ? elems / per : 0;
        const size_t e0 = (size_t)row0 * c;
        const uint4 *src = piece_ptr(x, e0, x_type);
        for (int p = tid; p < pieces; p += SL_THREADS) {
            float v[8];
            unpack_piece(src[p], x_type, v);
            int r = (p * per) / c, col = p * per - r * c;
#pragma unroll
            for (int k = 0; k < 8; k++) {
                if (k < per) {
                    tile[r * stride + col] = v[k];
                    if (++col == c) col = 0, ++r;
                }
            }
        }
        for (int le = pieces * per + tid; le < elems; le += SL_THREADS) {
            const int r = le / c;
            tile[r * stride + (le - r * c)] = load_elem(x, e0 + le, x_type);
        }
        __syncthreads();
        if (tid < tr) {
            const long long row = row0 + tid, tg = target[row];
            const float *xr = tile + tid * stride;
            float m = xr[0];
            int arg = 0;
            for (int ch = 1; ch < c; ch++) {  // numpy's argmax: the first maximum, and a NaN once met stays
                const float v = xr[ch];
                if (m == m && (v > m || v != v)) m = v, arg = ch;
            }
            float s = 0.0f, sd = 0.0f;
            for (int ch = 0; ch < c; ch++) {
                const float d = xr[ch] - m;
                s += expf(d);
                sd += d;
            }
            const float ls = logf(s);
            stat[2 * (size_t)row] = m;
            stat[2 * (size_t)row + 1] = ls;
            if (tg >= 0 && tg < c && tg != ignore_index) {
                const int k = (int)tg;
                const float lt = (xr[k] - m) - ls;
                float loss = -lt;
                if (eps > 0.0f) loss = -((1.0f - eps) * lt + (eps / (float)(c - 1)) * ((sd - (float)c * ls) - lt));
                ce += (double)loss;
                if (arg == k) atomicAdd(&hist[k], 1);
                atomicAdd(&hist[c + arg], 1);
                atomicAdd(&hist[2 * c + k], 1);
                atomicAdd(&hist[3 * c], 1);
            } else if (tg != ignore_index) {
                atomicAdd(&hist[3 * c + 1], 1);  // counted, never used as an index
            }
        }
        if (shift_pred != nullptr) {
            const size_t s0 = (size_t)row0 * 3;
            // the difference in double, where the sum is kept: an fp32 difference rounds each term, and a few rows' l1 then ends a whole
            // fp32 step off the float64 value (seen at n = 1: 5.96e-08 on 0.7995); so the one rounding is the finish kernel's
            for (int le = tid; le < tr * 3; le += SL_THREADS) l1 += fabs((double)load_elem(shift_pred, s0 + le, s_type) - (double)shift[s0 + le]);
        }
        __syncthreads();  // the tile and, after the last one, the histogram
    }
    for (int k = tid; k < c; k += SL_THREADS) {
        const int both = hist[k], pred = hist[c + k], tgt = hist[2 * c + k];
        if (both != 0) atomicAdd(&counts[k], (unsigned long long)both);
        if (pred + tgt - both != 0) atomicAdd(&counts[c + k], (unsigned long long)(pred + tgt - both));
        if (tgt != 0) atomicAdd(&counts[2 * c + k], (unsigned long long)tgt);
    }
    if (tid < 2 && hist[3 * c + tid] != 0) atomicAdd(&rows[tid], (unsigned long long)hist[3 * c + tid]);
    for (int st = 1; st < WAVE; st <<= 1) {
        ce += __shfl_xor(ce, st, WAVE);
        l1 += __shfl_xor(l1, st, WAVE);
    }
    if (lane_id() == 0) red[0][tid >> 6] = ce, red[1][tid >> 6] = l1;
    __syncthreads();
    if (tid < 2) {
        double sum = 0.0;
        for (int w = 0; w < SL_WAVES; w++) sum += red[tid][w];
        partials[2 * (size_t)blockIdx.x + tid] = sum;
    }
}

// losses = (ce, l1, total) from `blocks` rows of partials and the valid-row count; one wave
__global__ __launch_bounds__(WAVE) void seg_loss_finish_kernel(int blocks, int n, int has_shift, float offset_weight, const double *__restrict__ partials,
                                                               const unsigned long long *__restrict__ rows, float *__restrict__ losses) {
    double ce = 0.0, l1 = 0.0;
    for (int b = threadIdx.x; b < blocks; b += WAVE) {
        ce += partials[2 * (size_t)b];
        l1 += partials[2 * (size_t)b + 1];
    }
    for (int st = 1; st < WAVE; st <<= 1) {
        ce += __shfl_xor(ce, st, WAVE);
        l1 += __shfl_xor(l1, st, WAVE);
    }
    if (threadIdx.x == 0) {
        const float ce_f = (float)(ce / (double)rows[0]);  // no valid row: 0 / 0 = NaN, as torch
        const float l1_f = has_shift ? (float)(l1 / (3.0 * (double)n)) : 0.0f;
        losses[0] = ce_f;
        losses[1] = l1_f;
        losses[2] = has_shift ? ce_f + offset_weight * l1_f : ce_f;
    }
}

__global__ __launch_bounds__(SL_THREADS) void seg_loss_bwd_kernel(int n, int c, int x_type, int s_type, int vec, const void *__restrict__ x,
                                                                  const long long *__restrict__ target, const float *__restrict__ stat,
                                                                  const void *__restrict__ shift_pred, const float *__restrict__ shift,
                                                                  const float *__restrict__ grad_losses, const unsigned long long *__restrict__ rows,
                                                                  long long ignore_index, float eps, float offset_weight,
                                                                  void *__restrict__ grad_x, void *__restrict__ grad_shift) {
    const int tid = threadIdx.x, per = x_type == POINTOPS2_ROWS_F32 ? 4 : 8;
    const float g0 = grad_losses[0], g1 = grad_losses[1], g2 = grad_losses[2];
    const float sa = (g0 + g2) / (float)rows[0], sb = (g1 + offset_weight * g2) / (float)(3.0 * (double)n);
    const float w_hit = 1.0f - eps, w_miss = eps > 0.0f ? eps / (float)(c - 1) : 0.0f;
    const Tiles tiles(n, c);
    // the state of one row: its label (-1: not valid), maximum and log-sum
    struct RowState {
        int k;
        float m, ls;
    };
    auto row_state = [&](long long row) {
        const long long tg = target[row];
        RowState r;
        r.k = (tg >= 0 && tg < c && tg != ignore_index) ? (int)tg : -1;
        r.m = stat[2 * (size_t)row];
        r.ls = stat[2 * (size_t)row + 1];
        return r;
    };
    auto grad = [&](const RowState &r, int col, float xv) { return r.k < 0 ? 0.0f : sa * (expf((xv - r.m) - r.ls) - (col == r.k ? w_hit : w_miss)); };
    for (long long t = blockIdx.x; t < tiles.count; t += gridDim.x) {
        const long long row0 = tiles.first_row(t);
        const int tr = tiles.rows(t);
        if (grad_x != nullptr) {  // (kernel-uniform)
            const int elems = tr * c, pieces = vec ? elems / per : 0;
            const size_t e0 = (size_t)row0 * c;
            const uint4 *src = piece_ptr(x, e0, x_type);
            uint4 *dst = const_cast<uint4 *>(piece_ptr(grad_x, e0, x_type));
            for (int p = tid; p < pieces; p += SL_THREADS) {
                float v[8];
                unpack_piece(src[p], x_type, v);
                int r = (p * per) / c, col = p * per - r * c;
                RowState rs = row_state(row0 + r);
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    if (k < per) {
                        v[k] = grad(rs, col, v[k]);
                        if (++col == c && k + 1 < per && r + 1 < tr) col = 0, rs = row_state(row0 + ++r);
                    }
                }
                dst[p] = pack_piece(v, x_type);
            }
            for (int le = pieces * per + tid; le < elems; le += SL_THREADS) {
                const int r = le / c;
                store_elem(grad_x, e0 + le, x_type, grad(row_state(row0 + r), le - r * c, load_elem(x, e0 + le, x_type)));
            }
        }
        if (grad_shift != nullptr) {
            const size_t s0 = (size_t)row0 * 3;
            for (int le = tid; le < tr * 3; le += SL_THREADS) {
                const float d = load_elem(shift_pred, s0 + le, s_type) - shift[s0 + le];
                store_elem(grad_shift, s0 + le, s_type, sb * (float)((d > 0.0f) - (d < 0.0f)));
            }
        }
    }
}

// nullptr when the arguments are in range
const char *seg_loss_bad_args(int n, int c, int logits_type, int shift_type, float eps, const void *shift_pred, const float *shift) {
    if (n < 0) return "seg_loss: negative row count";
    if (c < 1 || c > SL_MAX_C) return "seg_loss: c must be in [1, 64]";
    if (!known_row_type(logits_type) || !known_row_type(shift_type)) return "seg_loss: row types must be POINTOPS2_ROWS_F32, _F16 or _BF16";
    if (!(eps >= 0.0f && eps < 1.0f)) return "seg_loss: smooth_eps must be in [0, 1)";
    if (eps > 0.0f && c < 2) return "seg_loss: smooth_eps > 0 needs c >= 2";
    if ((shift_pred == nullptr) != (shift == nullptr)) return "seg_loss: shift_pred and shift are given together or not at all";
    return nullptr;  // (n * c: the kernels index with 64-bit offsets)
}
inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }  // (NULL is aligned)
inline int tile_count(int n, int c) { return (int)div_up64(n, tile_rows_of(c)); }

}  // namespace
}  // namespace p2

using namespace p2;

extern "C" {

void seg_loss_forward_launcher(int n, int c, int logits_type, int shift_type, const void *logits, const long long *target, const void *shift_pred,
                               const float *shift, long long ignore_index, float smooth_eps, float offset_weight, float *stat, double *partials,
                               int partial_rows, long long *counts, long long *rows, float *losses) {
    const hipStream_t st = begin_launch().stream;
    if (const char *bad = seg_loss_bad_args(n, c, logits_type, shift_type, smooth_eps, shift_pred, shift)) { set_error(bad); return; }
    if (counts == nullptr || rows == nullptr || losses == nullptr) { set_error("seg_loss_forward: counts, rows and losses must not be NULL"); return; }
    if (n > 0 && (logits == nullptr || target == nullptr || stat == nullptr || partials == nullptr || partial_rows < 1)) {
        set_error("seg_loss_forward: logits, target, stat and partials (partial_rows >= 1) must not be NULL");
        return;
    }
    const int tiles = tile_count(n, c), grid = tiles < partial_rows ? tiles : partial_rows;
    unsigned long long *ucounts = reinterpret_cast<unsigned long long *>(counts), *urows = reinterpret_cast<unsigned long long *>(rows);
    if (n > 0) {
        hipLaunchKernelGGL(seg_loss_fwd_kernel, dim3(grid), dim3(SL_THREADS), 0, st, n, c, logits_type, shift_type, (int)aligned16(logits), logits,
                           target, shift_pred, shift, ignore_index, smooth_eps, stat, partials, ucounts, urows);
        if (!check_launch()) return;
    }
    hipLaunchKernelGGL(seg_loss_finish_kernel, dim3(1), dim3(WAVE), 0, st, grid, n, (int)(shift_pred != nullptr), offset_weight, partials, urows,
                       losses);
    check_launch();
}

void seg_loss_backward_launcher(int n, int c, int logits_type, int shift_type, const void *logits, const long long *target, const float *stat,
                                const void *shift_pred, const float *shift, const float *grad_losses, const long long *rows,
                                long long ignore_index, float smooth_eps, float offset_weight, void *grad_logits, void *grad_shift_pred) {
    const hipStream_t st = begin_launch().stream;
    if (const char *bad = seg_loss_bad_args(n, c, logits_type, shift_type, smooth_eps, shift_pred, shift)) { set_error(bad); return; }
    if (n == 0 || (grad_logits == nullptr && grad_shift_pred == nullptr)) return;
    if (grad_losses == nullptr || rows == nullptr) { set_error("seg_loss_backward: grad_losses and rows must not be NULL"); return; }
    if (grad_logits != nullptr && (logits == nullptr || target == nullptr || stat == nullptr)) {
        set_error("seg_loss_backward: grad_logits needs logits, target and stat");
        return;
    }
    if (grad_shift_pred != nullptr && shift_pred == nullptr) { set_error("seg_loss_backward: grad_shift_pred needs shift_pred and shift"); return; }
    const int tiles = tile_count(n, c), cap = num_cus() * 8;
    hipLaunchKernelGGL(seg_loss_bwd_kernel, dim3(tiles < cap ? tiles : cap), dim3(SL_THREADS), 0, st, n, c, logits_type, shift_type,
                       (int)(aligned16(logits) && aligned16(grad_logits)), logits, target, stat, shift_pred, shift, grad_losses,
                       reinterpret_cast<const unsigned long long *>(rows), ignore_index, smooth_eps, offset_weight, grad_logits, grad_shift_pred);
    check_launch();
}

}  // extern "C"
