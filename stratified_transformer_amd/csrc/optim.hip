// The tail of a training step in one call: the loss scaler's finite check and the AdamW update of every parameter tensor
// (tool/train.py:350-352: scaler.step(optimizer) on torch.optim.AdamW, amsgrad = False, maximize = False), over a descriptor table.
//
// The table (pointops2_optim_tensor [T], then pointops2_optim_group [G]) is built by the caller in host memory, completed here
// (first_chunk: the prefix sum of the tensors' chunk counts) and copied into the caller's device workspace on the stream; the kernels
// read the copy.  Four passes, each one launch, whatever T is:
//
//   check     (only with run_check; the flag is cleared on the stream in front of it)  every gradient element once; a workgroup that
//             meets an element with all exponent bits set stores 1.0f to *found_inf - a plain store, any number of lanes, one value.
//   prologue  one thread per tensor, the only code that touches a step count:
//               t = *step + 1 (fp32, exact below 2^24), stored back when *found_inf == 0
//               pow1 = beta1^t, pow2 = beta2^t: binary exponentiation in float64, multiplications only
//                   r = 1, b = beta, n = t;  while n: { if (n & 1) r = r * b;  n >>= 1;  if (n) b = b * b; }
//               rec = { float(lr / (1 - pow1)), float(sqrt(1 - pow2)), float(beta1), float(1 - beta1), float(beta2), float(1 - beta2),
//                       float(eps), float(1 - lr * weight_decay), inv_scale }      every entry computed in float64 and rounded once;
//               inv_scale = float(1.0 / double(*scale)), or 1 without a scale
//   update    a 256-thread workgroup owns one chunk (POINTOPS2_OPTIM_CHUNK elements) of one tensor; per element, in fp32, nothing fused:
//               g  = grad * inv_scale
//               p1 = p * decay
//               m  = (m * beta1) + (g * omb1)
//               v  = (v * beta2) + ((g * g) * omb2)
//               denom = (sqrtf(v) / sqrt_bias2) + eps
//               p  = p1 - (step_size * (m / denom))
//             division and sqrtf are the correctly rounded ones.  A workgroup returns at once when *found_inf != 0.
//
// The update reads the prologue's records, never a step count, so no workgroup reads what another workgroup of its launch writes.
// A workgroup finds its (tensor, chunk) by a binary search of first_chunk with blockIdx.x: the same for every lane, so the compiler
// keeps it in scalar registers and scalar loads.  A full chunk of a tensor whose four pointers are 16-byte aligned moves as 16-byte
// loads and stores, four per array and thread; a tensor's last partial chunk and every chunk of a tensor with a misaligned pointer
// (a Parameter may be a view at any element offset) go one element a lane through the same arithmetic.
#include "common.h"

namespace p2 {
namespace {

constexpr int OPT_THREADS = 256;
constexpr int OPT_CHUNK = POINTOPS2_OPTIM_CHUNK;
constexpr int OPT_VEC_STEPS = OPT_CHUNK / (4 * OPT_THREADS);
static_assert(OPT_CHUNK % (4 * OPT_THREADS) == 0, "a full chunk is a whole number of 16-byte pieces per thread");
constexpr int OPT_REC = 12;  // floats per prologue record (9 used)

static_assert(sizeof(pointops2_optim_tensor) == 56 && sizeof(pointops2_optim_group) == 40, "the table is packed by the callers");

inline size_t table_bytes(int t, int g) { return ((size_t)t * sizeof(pointops2_optim_tensor) + (size_t)g * sizeof(pointops2_optim_group) + 63) / 64 * 64; }

// the tensor whose chunks include workgroup `wg`: the last t with first_chunk <= wg (tensors without chunks share their successor's)
__device__ __forceinline__ int tensor_of(const pointops2_optim_tensor *__restrict__ tab, int n_tensors, int wg) {
    int lo = 0, hi = n_tensors;  // the answer is in [lo, hi)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tab[mid].first_chunk <= wg) lo = mid;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ bool misaligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }
__device__ __forceinline__ bool non_finite(float f) { return (__float_as_uint(f) & 0x7f800000u) == 0x7f800000u; }

__global__ __launch_bounds__(OPT_THREADS) void optim_check_kernel(int n_tensors, const pointops2_optim_tensor *__restrict__ tab,
                                                                  float *__restrict__ found_inf) {
    const int wg = blockIdx.x, tid = threadIdx.x;
    const int t = tensor_of(tab, n_tensors, wg);
    const long long base = (long long)(wg - tab[t].first_chunk) * OPT_CHUNK, left = tab[t].numel - base;
    const int n = left < OPT_CHUNK ? (int)left : OPT_CHUNK;
    const float *g = tab[t].grad + base;
    bool bad = false;
    if (n == OPT_CHUNK && !misaligned16(g)) {
#pragma unroll
        for (int s = 0; s < OPT_VEC_STEPS; s++) {
            const float4 x = ldg4(g + 4 * (s * OPT_THREADS + tid));
            bad = bad || non_finite(x.x) || non_finite(x.y) || non_finite(x.z) || non_finite(x.w);
        }
    } else {
        for (int i = tid; i < n; i += OPT_THREADS) bad |= non_finite(g[i]);
    }
    if (bad) *found_inf = 1.0f;
}

__device__ __forceinline__ double pow_by_squaring(double beta, unsigned long long n) {
    double r = 1.0, b = beta;
    while (n != 0) {
        if (n & 1) r = r * b;
        n >>= 1;
        if (n != 0) b = b * b;
    }
    return r;
}

__global__ __launch_bounds__(OPT_THREADS) void optim_prologue_kernel(int n_tensors, const pointops2_optim_tensor *__restrict__ tab,
                                                                     const pointops2_optim_group *__restrict__ groups,
                                                                     const float *__restrict__ scale, const float *__restrict__ found_inf,
                                                                     float *__restrict__ recs) {
    const int t = blockIdx.x * OPT_THREADS + threadIdx.x;
    if (t >= n_tensors) return;
    const pointops2_optim_group gr = groups[tab[t].group];
    float *step = tab[t].step;
    const float t_new = *step + 1.0f;
    if (*found_inf == 0.0f) *step = t_new;
    const unsigned long long n = t_new >= 1.0f ? (unsigned long long)t_new : 0ull;  // (a NaN or negative count: beta^0, and 1 / 0 below)
    const double bias1 = 1.0 - pow_by_squaring(gr.beta1, n), bias2 = 1.0 - pow_by_squaring(gr.beta2, n);
    float *rec = recs + (size_t)t * OPT_REC;
    rec[0] = (float)(gr.lr / bias1);
    rec[1] = (float)sqrt(bias2);
    rec[2] = (float)gr.beta1;
    rec[3] = (float)(1.0 - gr.beta1);
    rec[4] = (float)gr.beta2;
    rec[5] = (float)(1.0 - gr.beta2);
    rec[6] = (float)gr.eps;
    rec[7] = (float)(1.0 - gr.lr * gr.weight_decay);
    rec[8] = scale != nullptr ? (float)(1.0 / (double)*scale) : 1.0f;
}

struct Rec {
    float step_size, sqrt_bias2, beta1, omb1, beta2, omb2, eps, decay, inv_scale;
};

// one element; the order of the file's header
__device__ __forceinline__ void adamw_elem(const Rec &r, float &p, float grad, float &m, float &v) {
    const float g = grad * r.inv_scale;
    const float p1 = p * r.decay;
    m = (m * r.beta1) + (g * r.omb1);
    v = (v * r.beta2) + ((g * g) * r.omb2);
    const float denom = (sqrtf(v) / r.sqrt_bias2) + r.eps;
    p = p1 - (r.step_size * (m / denom));
}

__global__ __launch_bounds__(OPT_THREADS) void optim_adamw_kernel(int n_tensors, const pointops2_optim_tensor *__restrict__ tab,
                                                                  const float *__restrict__ recs, const float *__restrict__ found_inf) {
    if (*found_inf != 0.0f) return;
    const int wg = blockIdx.x, tid = threadIdx.x;
    const int t = tensor_of(tab, n_tensors, wg);
    const long long base = (long long)(wg - tab[t].first_chunk) * OPT_CHUNK, left = tab[t].numel - base;
    const int n = left < OPT_CHUNK ? (int)left : OPT_CHUNK;
    float *__restrict__ p = tab[t].param + base;
    const float *__restrict__ g = tab[t].grad + base;
    float *__restrict__ m = tab[t].exp_avg + base;
    float *__restrict__ v = tab[t].exp_avg_sq + base;
    const float *rp = recs + (size_t)t * OPT_REC;
    const Rec r{rp[0], rp[1], rp[2], rp[3], rp[4], rp[5], rp[6], rp[7], rp[8]};
    if (n == OPT_CHUNK && !(misaligned16(p) || misaligned16(g) || misaligned16(m) || misaligned16(v))) {
        float4 pv[OPT_VEC_STEPS], gv[OPT_VEC_STEPS], mv[OPT_VEC_STEPS], vv[OPT_VEC_STEPS];
#pragma unroll
        for (int s = 0; s < OPT_VEC_STEPS; s++) {
            const int e = 4 * (s * OPT_THREADS + tid);
            pv[s] = ldg4(p + e), gv[s] = ldg4(g + e), mv[s] = ldg4(m + e), vv[s] = ldg4(v + e);
        }
#pragma unroll
        for (int s = 0; s < OPT_VEC_STEPS; s++) {
            const int e = 4 * (s * OPT_THREADS + tid);
            adamw_elem(r, pv[s].x, gv[s].x, mv[s].x, vv[s].x);
            adamw_elem(r, pv[s].y, gv[s].y, mv[s].y, vv[s].y);
            adamw_elem(r, pv[s].z, gv[s].z, mv[s].z, vv[s].z);
            adamw_elem(r, pv[s].w, gv[s].w, mv[s].w, vv[s].w);
            stg4(p + e, pv[s]), stg4(m + e, mv[s]), stg4(v + e, vv[s]);
        }
    } else {
        for (int i = tid; i < n; i += OPT_THREADS) {
            float pe = p[i], me = m[i], ve = v[i];
            adamw_elem(r, pe, g[i], me, ve);
            p[i] = pe, m[i] = me, v[i] = ve;
        }
    }
}

}  // namespace
}  // namespace p2

using namespace p2;

extern "C" {

size_t pointops2_optim_workspace_bytes(int n_tensors, int n_groups) {
    if (n_tensors < 0 || n_groups < 0) return 0;
    return table_bytes(n_tensors, n_groups) + (size_t)n_tensors * OPT_REC * sizeof(float);
}

void optim_adamw_step_launcher(int n_tensors, int n_groups, void *host_table, void *workspace, size_t workspace_bytes, const float *scale,
                               float *found_inf, int run_check) {
    const hipStream_t st = begin_launch().stream;
    if (n_tensors < 0) { set_error("optim_adamw_step: negative tensor count"); return; }
    if (n_groups < 0) { set_error("optim_adamw_step: negative group count"); return; }
    if (found_inf == nullptr) { set_error("optim_adamw_step: found_inf must not be NULL"); return; }
    if (n_tensors > 0 && (host_table == nullptr || workspace == nullptr)) { set_error("optim_adamw_step: host_table and workspace must not be NULL"); return; }
    if (workspace_bytes < pointops2_optim_workspace_bytes(n_tensors, n_groups)) {
        set_error("optim_adamw_step: workspace smaller than pointops2_optim_workspace_bytes(n_tensors, n_groups)");
        return;
    }
    pointops2_optim_tensor *tensors = static_cast<pointops2_optim_tensor *>(host_table);
    long long chunks = 0;
    for (int t = 0; t < n_tensors; t++) {
        if (tensors[t].numel < 0 || tensors[t].numel >= (1ll << 31)) { set_error("optim_adamw_step: numel must be in [0, 2^31)"); return; }
        if (tensors[t].group < 0 || tensors[t].group >= n_groups) { set_error("optim_adamw_step: group index out of range"); return; }
        if (tensors[t].step == nullptr || (tensors[t].numel > 0 && (tensors[t].param == nullptr || tensors[t].grad == nullptr ||
                                                                    tensors[t].exp_avg == nullptr || tensors[t].exp_avg_sq == nullptr))) {
            set_error("optim_adamw_step: a tensor's param, grad, exp_avg, exp_avg_sq and step must not be NULL");
            return;
        }
        chunks += div_up64(tensors[t].numel, OPT_CHUNK);
    }
    if (chunks > 0x7fffffffll) { set_error("optim_adamw_step: more than 2^31 - 1 chunks"); return; }
    if (run_check) {
        if (hipMemsetAsync(found_inf, 0, sizeof(float), st) != hipSuccess) { check_launch(); return; }
    }
    if (n_tensors == 0) return;
    int first = 0;
    for (int t = 0; t < n_tensors; t++) {
        tensors[t].first_chunk = first;
        first += (int)div_up64(tensors[t].numel, OPT_CHUNK);
    }
    const size_t tab_bytes = (size_t)n_tensors * sizeof(pointops2_optim_tensor) + (size_t)n_groups * sizeof(pointops2_optim_group);
    if (hipMemcpyAsync(workspace, host_table, tab_bytes, hipMemcpyHostToDevice, st) != hipSuccess) { check_launch(); return; }
    const pointops2_optim_tensor *tab = static_cast<const pointops2_optim_tensor *>(workspace);
    const pointops2_optim_group *groups = reinterpret_cast<const pointops2_optim_group *>(tab + n_tensors);
    float *recs = reinterpret_cast<float *>(static_cast<char *>(workspace) + table_bytes(n_tensors, n_groups));
    if (run_check && chunks > 0) {
        hipLaunchKernelGGL(optim_check_kernel, dim3((unsigned)chunks), dim3(OPT_THREADS), 0, st, n_tensors, tab, found_inf);
        if (!check_launch()) return;
    }
    hipLaunchKernelGGL(optim_prologue_kernel, dim3(div_up(n_tensors, OPT_THREADS)), dim3(OPT_THREADS), 0, st, n_tensors, tab, groups, scale,
                       (const float *)found_inf, recs);
    if (!check_launch()) return;
    if (chunks > 0) {
        hipLaunchKernelGGL(optim_adamw_kernel, dim3((unsigned)chunks), dim3(OPT_THREADS), 0, st, n_tensors, tab, (const float *)recs,
                           (const float *)found_inf);
        check_launch();
    }
}

}  // extern "C"
