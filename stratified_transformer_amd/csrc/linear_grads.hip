// The two parameter gradients of y = x W^T + b in one pass over the point rows, on the matrix cores:
//
//   dW[o, i] = sum_n g[n, o] * x[n, i]        g = grad_out [N, out],  x [N, in]
//   db[o]    = sum_n g[n, o]
//
// The result is tiny ([out, in] <= a few thousand elements at the model's shapes) and the reduction runs over all N rows: a tiled GEMM
// finds no output tiles to spread over the chip.  Here the ROWS are spread: N is cut into G = ceil(N / LG_ROWS) chunks (a function of N
// alone), a workgroup keeps its share of [out, in] in accumulator registers over the LG_ROWS rows of one chunk and writes one partial
// block, and linear_grads_reduce_kernel adds the G partials in ascending chunk order.  No float atomics: the order of every addition is
// a function of the shapes alone, the same bits from run to run.
//
// MFMA: v_mfma_f32_16x16x4_f32, D[16 x 16] += A[16 x 4] B[4 x 16] with A[l & 15][k = l >> 4] and B[k = l >> 4][l & 15] one fp32 register
// each.  With k running over four consecutive rows n0 .. n0 + 3 this is what row-major g and x hand out: lane l loads
// g[n0 + (l >> 4)][o0 + (l & 15)] as A and x[n0 + (l >> 4)][i0 + (l & 15)] as B - sixteen consecutive elements of a row on sixteen
// lanes, no transpose and no LDS.  D: lane l holds D[o0 + 4 (l >> 4) + r][i0 + (l & 15)] in register r.  Per element the result is a
// chain of fp32 fused multiply-adds in ascending row order.  16-bit rows (f16 / bf16) are widened exactly on load, one element per
// lane (no vector load that an odd width could misalign); the two operands may differ in type.
//
// Tiles: [out, in] is ceil(out / 16) x ceil(in / 16) tiles of 16 x 16.  A wave owns a block of LG_MO x LG_MI = 3 x 3 of them (nine
// independent accumulators: 36 registers; 3 + 3 loads feed 9 MFMAs a step), a workgroup four consecutive blocks (out-major, so its
// waves share their x columns), the grid's second dimension the rest: 48 -> 192 is one workgroup per chunk, 384 -> 1536 is 64.
// Rows behind N and columns behind in / out enter as zeros (0 * 0 adds nothing and makes no NaN), and nothing behind [out, in] is stored.
//
// db: the A operand already holds g; every lane adds the values it loads for the tiles of its out-columns, the four row groups of the
// wave merge by an xor butterfly, and the waves of the first in-block store it as column `in` of the partial block
// (partials [G][out][in + 1]).  g is read once.
#include "row_types.h"

namespace p2 {
namespace {

constexpr int LG_ROWS = POINTOPS2_LINEAR_GRADS_ROWS;  // R: rows of a chunk
constexpr int LG_MAX_DIM = 1536;                      // in, out
constexpr int LG_WAVES = 4;                           // per workgroup
constexpr int LG_MO = 3, LG_MI = 3;                   // tiles of a wave's block: out x in
constexpr int LG_UNROLL = 8;                          // steps (of four rows) whose operands are in flight together: 48 loads a wave, whose 72 MFMAs (2304 cycles) cover a trip to memory
static_assert(LG_ROWS % (4 * LG_UNROLL) == 0, "a chunk is a whole number of unrolled steps");

typedef float f32x4 __attribute__((ext_vector_type(4)));

// the operands of LG_UNROLL steps from row `first`: ga[u][m] = g[first + 4 u + (l >> 4)][o column of tile m], xa likewise; 0 behind `end`
// and behind the last column.  Every lane loads - a masked-off one from the clamped row / column (ocl, icl), always inside the
// operand - and then selects: straight-line loads that travel together, no branch per element.  Needs end >= 1.
template <typename XT, typename GT>
__device__ __forceinline__ void lg_fetch(float (&ga)[LG_UNROLL][LG_MO], float (&xa)[LG_UNROLL][LG_MI], long long first, long long end, int in,
                                         int out, const XT *__restrict__ x, const GT *__restrict__ g, const int (&ocol)[LG_MO],
                                         const int (&icol)[LG_MI]) {
    const int k = lane_id() >> 4;
#pragma unroll
    for (int u = 0; u < LG_UNROLL; u++) {
        const long long row = first + 4 * u + k, at = min(row, end - 1);
        const bool live = row < end;
#pragma unroll
        for (int m = 0; m < LG_MO; m++) {
            const float v = ld_elem(g + (size_t)at * out + min(ocol[m], out - 1));
            ga[u][m] = (live && ocol[m] < out) ? v : 0.0f;
        }
#pragma unroll
        for (int m = 0; m < LG_MI; m++) {
            const float v = ld_elem(x + (size_t)at * in + min(icol[m], in - 1));
            xa[u][m] = (live && icol[m] < in) ? v : 0.0f;
        }
    }
}

// LG_UNROLL steps of a wave's block: acc[mo][mi] += g-tile mo (A) x x-tile mi (B), bsum[mo] += the g values.  FULL: all nine tiles are
// live - nothing to ask inside the steps; else only the first mo_n x mi_n are multiplied.
template <bool FULL>
__device__ __forceinline__ void lg_multiply(f32x4 (&acc)[LG_MO][LG_MI], float (&bsum)[LG_MO], const float (&ga)[LG_UNROLL][LG_MO],
                                            const float (&xa)[LG_UNROLL][LG_MI], int mo_n, int mi_n) {
#pragma unroll
    for (int u = 0; u < LG_UNROLL; u++) {
#pragma unroll
        for (int mo = 0; mo < LG_MO; mo++) {
            if (!FULL && mo >= mo_n) continue;
            bsum[mo] += ga[u][mo];
#pragma unroll
            for (int mi = 0; mi < LG_MI; mi++) {
                if (!FULL && mi >= mi_n) continue;
                acc[mo][mi] = __builtin_amdgcn_mfma_f32_16x16x4f32(ga[u][mo], xa[u][mi], acc[mo][mi], 0, 0, 0);
            }
        }
    }
}

// grid (G, ceil(blocks / LG_WAVES)): chunk blockIdx.x, wave w takes tile block blockIdx.y * LG_WAVES + w.  One body for the nine pairs of
// row types (XT, GT of float / f16_t / bf16_t): only the widening of a loaded element differs.
template <typename XT, typename GT>
__global__ __launch_bounds__(LG_WAVES *WAVE) void linear_grads_partial_kernel(int n, int in, int out, const XT *__restrict__ x,
                                                                              const GT *__restrict__ g, float *__restrict__ partials) {
    const int lane = lane_id(), c = lane & 15, k = lane >> 4;
    const int to = (out + 15) >> 4, ti = (in + 15) >> 4, ob_n = (to + LG_MO - 1) / LG_MO, ib_n = (ti + LG_MI - 1) / LG_MI;
    const int wb = blockIdx.y * LG_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // (in a scalar register: what follows from it branches, not masks)
    if (wb >= ob_n * ib_n) return;  // (wave-uniform; the kernel has no barrier)
    const int ob = wb % ob_n, ib = wb / ob_n;
    const int mo_n = min(LG_MO, to - ob * LG_MO), mi_n = min(LG_MI, ti - ib * LG_MI);  // the block's live tiles (wave-uniform)
    const bool full = mo_n == LG_MO && mi_n == LG_MI;
    int ocol[LG_MO], icol[LG_MI];
#pragma unroll
    for (int m = 0; m < LG_MO; m++) ocol[m] = (ob * LG_MO + m) * 16 + c;
#pragma unroll
    for (int m = 0; m < LG_MI; m++) icol[m] = (ib * LG_MI + m) * 16 + c;

    f32x4 acc[LG_MO][LG_MI];
    float bsum[LG_MO];
#pragma unroll
    for (int mo = 0; mo < LG_MO; mo++) {
        bsum[mo] = 0.0f;
#pragma unroll
        for (int mi = 0; mi < LG_MI; mi++) acc[mo][mi] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    }

    const long long begin = (long long)blockIdx.x * LG_ROWS, end = min((long long)n, begin + LG_ROWS);
    float ga[LG_UNROLL][LG_MO], xa[LG_UNROLL][LG_MI];
    if (begin < end) lg_fetch(ga, xa, begin, end, in, out, x, g, ocol, icol);  // (kernel-uniform: only n == 0 has a chunk without rows)
    for (long long first = begin; first < end; first += 4 * LG_UNROLL) {
        float gn[LG_UNROLL][LG_MO], xn[LG_UNROLL][LG_MI];  // the next steps' operands travel while these multiply
        lg_fetch(gn, xn, first + 4 * LG_UNROLL, end, in, out, x, g, ocol, icol);
        if (full) lg_multiply<true>(acc, bsum, ga, xa, mo_n, mi_n);
        else lg_multiply<false>(acc, bsum, ga, xa, mo_n, mi_n);
#pragma unroll
        for (int u = 0; u < LG_UNROLL; u++) {
#pragma unroll
            for (int m = 0; m < LG_MO; m++) ga[u][m] = gn[u][m];
#pragma unroll
            for (int m = 0; m < LG_MI; m++) xa[u][m] = xn[u][m];
        }
    }

    float *part = partials + (size_t)blockIdx.x * out * (in + 1);
#pragma unroll
    for (int mo = 0; mo < LG_MO; mo++) {
        if (mo >= mo_n) continue;
#pragma unroll
        for (int mi = 0; mi < LG_MI; mi++) {
            if (mi >= mi_n) continue;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int o = (ob * LG_MO + mo) * 16 + 4 * k + r;
                if (o < out && icol[mi] < in) part[(size_t)o * (in + 1) + icol[mi]] = acc[mo][mi][r];
            }
        }
        if (ib == 0) {  // (wave-uniform) the bias column: rows k, k + 4, ... of this lane, then the four row groups
            const float s = xor_sum<16, 64>(bsum[mo]);
            if (k == 0 && ocol[mo] < out) part[(size_t)ocol[mo] * (in + 1) + in] = s;
        }
    }
}

// grad_weight [out, in] and grad_bias [out] = the sum of the G blocks of partials [G][out][in + 1], chunk 0 first: one thread per element
__global__ __launch_bounds__(256) void linear_grads_reduce_kernel(int in, int out, int rows, const float *__restrict__ partials,
                                                                  float *__restrict__ grad_weight, float *__restrict__ grad_bias) {
    const int block = out * (in + 1), e = blockIdx.x * 256 + threadIdx.x;
    if (e >= block) return;
    const int o = e / (in + 1), i = e - o * (in + 1);
    if (i == in && grad_bias == nullptr) return;
    float sum = 0.0f;
    int b = 0;
    for (; b + 16 <= rows; b += 16) {  // sixteen loads in flight, added in order
        float v[16];
#pragma unroll
        for (int j = 0; j < 16; j++) v[j] = partials[(size_t)(b + j) * block + e];
#pragma unroll
        for (int j = 0; j < 16; j++) sum += v[j];
    }
    for (; b < rows; b++) sum += partials[(size_t)b * block + e];
    if (i < in) grad_weight[(size_t)o * in + i] = sum;
    else grad_bias[o] = sum;
}

// nullptr when the shape is in range
const char *linear_grads_bad_shape(int in, int out) {
    if (in < 1 || in > LG_MAX_DIM || out < 1 || out > LG_MAX_DIM) return "linear_grads: in and out must be in [1, 1536]";
    return nullptr;
}

}  // namespace
}  // namespace p2

using namespace p2;

extern "C" {

int pointops2_linear_grads_partial_rows(int n, int in, int out) {
    if (n < 0 || linear_grads_bad_shape(in, out) != nullptr) return 0;
    return n == 0 ? 1 : (int)div_up64(n, LG_ROWS);
}

void linear_grads_partial_launcher(int n, int in, int out, int x_type, int g_type, const void *x, const void *g, float *partials,
                                   int partial_rows) {
    const hipStream_t st = begin_launch().stream;
    if (n < 0) { set_error("linear_grads_partial: negative row count"); return; }
    if (const char *bad = linear_grads_bad_shape(in, out)) { set_error(bad); return; }
    if (!known_row_type(x_type) || !known_row_type(g_type)) {
        set_error("linear_grads_partial: row types must be POINTOPS2_ROWS_F32, _F16 or _BF16");
        return;
    }
    if (partial_rows != pointops2_linear_grads_partial_rows(n, in, out)) {
        set_error("linear_grads_partial: partial_rows must be pointops2_linear_grads_partial_rows(n, in, out)");
        return;
    }
    if (partials == nullptr || (n > 0 && (x == nullptr || g == nullptr))) { set_error("linear_grads_partial: x, g and partials must not be NULL"); return; }
    const int blocks = div_up(div_up(out, 16), LG_MO) * div_up(div_up(in, 16), LG_MI);
    with_row_type(x_type, [&](auto xt) {
        with_row_type(g_type, [&](auto gt) {
            using XT = typename decltype(xt)::type;
            using GT = typename decltype(gt)::type;
            hipLaunchKernelGGL((linear_grads_partial_kernel<XT, GT>), dim3(partial_rows, div_up(blocks, LG_WAVES)), dim3(LG_WAVES * WAVE), 0, st, n,
                               in, out, static_cast<const XT *>(x), static_cast<const GT *>(g), partials);
        });
    });
    check_launch();
}

void linear_grads_reduce_launcher(int in, int out, int has_bias, const float *partials, int partial_rows, float *grad_weight, float *grad_bias) {
    const hipStream_t st = begin_launch().stream;
    if (const char *bad = linear_grads_bad_shape(in, out)) { set_error(bad); return; }
    if (partial_rows < 1) { set_error("linear_grads_reduce: partial_rows must be >= 1"); return; }
    if (partials == nullptr || grad_weight == nullptr || (has_bias && grad_bias == nullptr)) {
        set_error("linear_grads_reduce: partials, grad_weight and (with has_bias) grad_bias must not be NULL");
        return;
    }
    hipLaunchKernelGGL(linear_grads_reduce_kernel, dim3(div_up(out * (in + 1), 256)), dim3(256), 0, st, in, out, partial_rows, partials, grad_weight,
                       has_bias ? grad_bias : nullptr);
    check_launch();
}

}  // extern "C"
