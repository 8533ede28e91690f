// The sum passes of the deterministic cell attention backward, gfx950.
//
// The default backward of cell_attn.hip adds dK, dV and the three table gradients across workgroups with float atomics, whose order is
// the order in which the workgroups happen to arrive.  The deterministic launchers run the same sweeps and table bodies with plain
// stores instead (the DET instances of cell_bwd_kernel and cell_table_grad3_kernel): every key SLOT of every cell receives its own row
// of a partial buffer, every workgroup of a table body its own image of the table.  The two kernels here add those partials per
// destination in an order that the operands alone decide:
//   keys    grad[i] = ((0 + partials[order[a]]) + partials[order[a + 1]]) + ...   over a .. b - 1 = slot_offsets[i] .. slot_offsets[i + 1] - 1
//           (the key-major view of plan->cell_keys: a point's slots, ascending), a point without a slot gets 0
//   tables  grad_table[x] = ((0 + p[0][x]) + p[1][x]) + ...   over the partial rows, ascending
// fp32, every destination written once: no atomics, no zero-fill, no tickets or flags between workgroups - separate launches behind
// the store passes.  The same bits from run to run for one library build on one device model: the number of table partial rows
// follows the device's CU count (pointops2_cell_table_partial_rows), so another device groups the table sums differently.
#include "cell_common.h"

namespace p2 {

// one thread per (point, four floats of its C = h * 16 channels); c4 = C / 4.  blockIdx.y picks the buffer pair (dK / dV).
__global__ __launch_bounds__(256) void cell_key_grads_reduce_kernel(int n, int c4, const int *__restrict__ slot_offsets, const int *__restrict__ slot_order,
                                                                    const float *__restrict__ partials0, float *__restrict__ grad0,
                                                                    const float *__restrict__ partials1, float *__restrict__ grad1, int row_stride) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)n * c4) return;
    const int i = (int)(idx / c4), j = (int)(idx % c4);
    const float *part = (blockIdx.y ? partials1 : partials0) + 4 * j;
    float *grad = blockIdx.y ? grad1 : grad0;
    const size_t C = (size_t)c4 * 4;
    const int b = slot_offsets[i + 1];
    int e = slot_offsets[i];
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    for (; e + 4 <= b; e += 4) {  // four rows in flight, added in slot order
        const int s0 = slot_order[e], s1 = slot_order[e + 1], s2 = slot_order[e + 2], s3 = slot_order[e + 3];
        const float4 r0 = ldg4(part + s0 * C), r1 = ldg4(part + s1 * C), r2 = ldg4(part + s2 * C), r3 = ldg4(part + s3 * C);
        s = add4(add4(add4(add4(s, r0), r1), r2), r3);
    }
    for (; e < b; e++) s = add4(s, ldg4(part + slot_order[e] * C));
    stg4(grad + (size_t)i * row_stride + 4 * j, s);
}

// one thread per element of a table [L, h, 16, 3]; blockIdx.y picks the table (0 = q, 1 = k, 2 = v).  partials of a table:
// [rows][h][L * 48], an image per workgroup of the table body in the order of the table's (row, head) blocks of 48 floats
__global__ __launch_bounds__(256) void cell_table_grads_reduce_kernel(int rows, int h, int L, const float *__restrict__ partials, float *__restrict__ gtq,
                                                                      float *__restrict__ gtk, float *__restrict__ gtv) {
    const int x = blockIdx.x * 256 + threadIdx.x, total = L * h * 48;
    if (x >= total) return;
    const int r = x / (h * 48), head = (x / 48) % h, el = x % 48;
    const size_t image = (size_t)L * 48, row = (size_t)h * image;
    const float *p = partials + blockIdx.y * (size_t)rows * row + head * image + (size_t)r * 48 + el;
    float s = 0.f;
    int w = 0;
    for (; w + 4 <= rows; w += 4) {
        const float a0 = p[w * row], a1 = p[(w + 1) * row], a2 = p[(w + 2) * row], a3 = p[(w + 3) * row];
        s = (((s + a0) + a1) + a2) + a3;
    }
    for (; w < rows; w++) s += p[w * row];
    (blockIdx.y == 0 ? gtq : blockIdx.y == 1 ? gtk : gtv)[x] = s;
}

void cell_key_grads_reduce_launch(hipStream_t st, int n, int h, const int *slot_offsets, const int *slot_order, const float *partials0, float *grad0,
                                  const float *partials1, float *grad1, int row_stride) {
    const int c4 = h * 4;
    hipLaunchKernelGGL(cell_key_grads_reduce_kernel, dim3((unsigned)div_up64((int64_t)n * c4, 256), partials1 != nullptr ? 2 : 1), dim3(256), 0, st, n, c4,
                       slot_offsets, slot_order, partials0, grad0, partials1, grad1, row_stride);
}

void cell_table_grads_reduce_launch(hipStream_t st, int rows, int h, int L, const float *partials, float *gtq, float *gtk, float *gtv) {
    hipLaunchKernelGGL(cell_table_grads_reduce_kernel, dim3(div_up(L * h * 48, 256), 3), dim3(256), 0, st, rows, h, L, partials, gtq, gtk, gtv);
}

}  // namespace p2

using namespace p2;

extern "C" {

void cell_key_grads_reduce_launcher(int n, int h, const int *slot_offsets, const int *slot_order, const float *partials, float *grad, int row_stride) {
    const hipStream_t st = begin_launch().stream;
    if (n <= 0) return;
    if (h < 1 || slot_offsets == nullptr || slot_order == nullptr || partials == nullptr || grad == nullptr) {
        set_error("cell_key_grads_reduce: h >= 1; slot_offsets, slot_order, partials and grad must not be NULL");
        return;
    }
    if (row_stride < h * 16 || row_stride % 4 != 0 || (reinterpret_cast<uintptr_t>(partials) | reinterpret_cast<uintptr_t>(grad)) % 16 != 0) {
        set_error("cell_key_grads_reduce: row_stride must be a multiple of 4 and at least h * 16, partials and grad 16-byte aligned");
        return;
    }
    cell_key_grads_reduce_launch(st, n, h, slot_offsets, slot_order, partials, grad, nullptr, nullptr, row_stride);
    check_launch();
}

void cell_table_grads_reduce_launcher(int partial_rows, int h, int L, const float *table_partials, float *grad_table_q, float *grad_table_k,
                                      float *grad_table_v) {
    const hipStream_t st = begin_launch().stream;
    if (partial_rows < 1 || h < 1 || L < 1 || table_partials == nullptr || grad_table_q == nullptr || grad_table_k == nullptr || grad_table_v == nullptr) {
        set_error("cell_table_grads_reduce: partial_rows, h, L >= 1; table_partials and the three gradients must not be NULL");
        return;
    }
    cell_table_grads_reduce_launch(st, partial_rows, h, L, table_partials, grad_table_q, grad_table_k, grad_table_v);
    check_launch();
}

}  // extern "C"
