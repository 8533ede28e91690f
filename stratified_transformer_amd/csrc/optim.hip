// The tail of a training step in one call: the loss scaler's finite check, an optional clip of the gradients' global 2-norm and the
// update of every parameter tensor - torch.optim.AdamW (amsgrad = False, maximize = False; tool/train.py:137-146, :350-352:
// scaler.step(optimizer)) or torch.optim.SGD (dampening = 0, maximize = False; tool/train.py:127-128) - over a descriptor table.
//
// The table (pointops2_optim_tensor [T], then pointops2_optim_group [G]) is built by the caller in host memory, completed here
// (first_chunk: the prefix sum of the tensors' chunk counts) and copied into the caller's device workspace on the stream; the kernels
// read the copy.  Four passes (five with clipping), each one launch, whatever T is:
//
//   check     (only with run_check; the flag is cleared on the stream in front of it)  every gradient element once; a workgroup that
//             meets an element with all exponent bits set stores 1.0f to *found_inf - a plain store, any number of lanes, one value.
//   norm      (only with clipping; the same kernel and the same read as the check)  the chunk's sum of squares in float64, in an order
//             that no alignment changes: element i of the chunk belongs to thread (i / 4) % 256, which visits its elements in ascending i:
//               x = grad[i] * inv_scale (fp32);  acc = acc + double(x) * double(x)
//             then the 256 sums are folded by a halving tree, stride = 128, 64, ..., 1: a[j] = a[j] + a[j + stride] for j < stride
//             (LDS down to one wave, an xor butterfly inside it: the same bits in lane 0), and a[0] is stored to partial[chunk].
//   reduce    (only with clipping)  one workgroup: thread j adds partial[j], partial[j + 256], ... in ascending order, the same tree gives
//             S;  norm = sqrt(S) (float64);  *grad_norm = float(norm);  coef = float(min(1.0, max_norm / (norm + 1e-6))), which is
//             torch.nn.utils.clip_grad_norm_'s factor, rounded to fp32 once.  No float atomics anywhere.
//   prologue  one thread per tensor, the only code that touches a step count:
//               t = *step + 1 (fp32, exact below 2^24), stored back when *found_inf == 0
//               pow1 = beta1^t, pow2 = beta2^t: binary exponentiation in float64, multiplications only
//                   r = 1, b = beta, n = t;  while n: { if (n & 1) r = r * b;  n >>= 1;  if (n) b = b * b; }
//               rec = { float(lr / (1 - pow1)), float(sqrt(1 - pow2)), float(beta1), float(1 - beta1), float(beta2), float(1 - beta2),
//                       float(eps), float(1 - lr * weight_decay), inv_scale, coef }   every entry computed in float64 and rounded once;
//               inv_scale = float(1.0 / double(*scale)), or 1 without a scale;  coef: the reduce pass's, or 1 without clipping
//             SGD has no step count:  rec = { float(lr), float(momentum), float(weight_decay), inv_scale, coef, nesterov ? 1 : 0 }
//   update    a 256-thread workgroup owns one chunk (POINTOPS2_OPTIM_CHUNK elements) of one tensor; per element, in fp32, nothing fused:
//               g  = (grad * inv_scale) * coef
//               p1 = p * decay
//               m  = (m * beta1) + (g * omb1)
//               v  = (v * beta2) + ((g * g) * omb2)
//               denom = (sqrtf(v) / sqrt_bias2) + eps
//               p  = p1 - (step_size * (m / denom))
//             division and sqrtf are the correctly rounded ones.  SGD (the buffer starts as zeros, so the first step gives buf = g):
//               g = (grad * inv_scale) * coef
//               if (weight_decay != 0)  g = g + (p * weight_decay)
//               if (momentum != 0)    { buf = (buf * momentum) + g;  g = nesterov ? g + (buf * momentum) : buf }
//               p = p - (g * lr)
//             A workgroup returns at once when *found_inf != 0.
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
constexpr int OPT_REC = 12;  // floats per prologue record (AdamW uses 10, SGD 6)

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

// the halving tree over the 256 per-thread sums: a[j] = a[j] + a[j + stride], stride = 128 ... 1; the result is thread 0's
__device__ __forceinline__ double tree_sum(double acc, double *red) {
    const int tid = threadIdx.x;
    red[tid] = acc;
    __syncthreads();
    if (tid < 128) red[tid] = red[tid] + red[tid + 128];
    __syncthreads();
    double a = 0.0;
    if (tid < 64) {
        a = red[tid] + red[tid + 64];
#pragma unroll
        for (int stride = 32; stride >= 1; stride >>= 1) a = a + __shfl_xor(a, stride);
    }
    return a;
}

__device__ __forceinline__ void add_square(double &acc, float grad, float inv_scale) {
    const float x = grad * inv_scale;
    acc = acc + (double)x * (double)x;
}

template <bool CHECK, bool NORM>
__global__ __launch_bounds__(OPT_THREADS) void optim_check_kernel(int n_tensors, const pointops2_optim_tensor *__restrict__ tab,
                                                                  const float *__restrict__ scale, float *__restrict__ found_inf,
                                                                  double *__restrict__ partial) {
    const int wg = blockIdx.x, tid = threadIdx.x;
    const int t = tensor_of(tab, n_tensors, wg);
    const long long base = (long long)(wg - tab[t].first_chunk) * OPT_CHUNK, left = tab[t].numel - base;
    const int n = left < OPT_CHUNK ? (int)left : OPT_CHUNK;
    const float *g = tab[t].grad + base;
    bool bad = false;
    if constexpr (!NORM) {
        if (n == OPT_CHUNK && !misaligned16(g)) {
#pragma unroll
            for (int s = 0; s < OPT_VEC_STEPS; s++) {
                const float4 x = ldg4(g + 4 * (s * OPT_THREADS + tid));
                bad = bad || non_finite(x.x) || non_finite(x.y) || non_finite(x.z) || non_finite(x.w);
            }
        } else {
            for (int i = tid; i < n; i += OPT_THREADS) bad |= non_finite(g[i]);
        }
    } else {
        __shared__ double red[OPT_THREADS];
        const float inv_scale = scale != nullptr ? (float)(1.0 / (double)*scale) : 1.0f;
        double acc = 0.0;
        if (n == OPT_CHUNK && !misaligned16(g)) {
#pragma unroll
            for (int s = 0; s < OPT_VEC_STEPS; s++) {
                const float4 x = ldg4(g + 4 * (s * OPT_THREADS + tid));
                if (CHECK) bad = bad || non_finite(x.x) || non_finite(x.y) || non_finite(x.z) || non_finite(x.w);
                add_square(acc, x.x, inv_scale), add_square(acc, x.y, inv_scale), add_square(acc, x.z, inv_scale), add_square(acc, x.w, inv_scale);
            }
        } else {  // the same ownership, one element at a time
            for (int s = 0; s < OPT_VEC_STEPS; s++) {
                for (int c = 0; c < 4; c++) {
                    const int i = 4 * (s * OPT_THREADS + tid) + c;
                    if (i < n) {
                        const float x = g[i];
                        if (CHECK) bad |= non_finite(x);
                        add_square(acc, x, inv_scale);
                    }
                }
            }
        }
        const double sum = tree_sum(acc, red);
        if (tid == 0) partial[wg] = sum;
    }
    if (CHECK && bad) *found_inf = 1.0f;
}

__global__ __launch_bounds__(OPT_THREADS) void optim_norm_reduce_kernel(long long n_chunks, const double *__restrict__ partial, double max_norm,
                                                                        float *__restrict__ grad_norm, float *__restrict__ coef) {
    __shared__ double red[OPT_THREADS];
    double acc = 0.0;
    for (long long j = threadIdx.x; j < n_chunks; j += OPT_THREADS) acc = acc + partial[j];
    const double sum = tree_sum(acc, red);
    if (threadIdx.x == 0) {
        const double norm = sqrt(sum), r = max_norm / (norm + 1e-6);
        *grad_norm = (float)norm;
        *coef = (float)(r < 1.0 ? r : 1.0);
    }
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
                                                                     const float *__restrict__ coef, int kind, float *__restrict__ recs) {
    const int t = blockIdx.x * OPT_THREADS + threadIdx.x;
    if (t >= n_tensors) return;
    const pointops2_optim_group gr = groups[tab[t].group];
    float *rec = recs + (size_t)t * OPT_REC;
    const float inv_scale = scale != nullptr ? (float)(1.0 / (double)*scale) : 1.0f, clip = coef != nullptr ? *coef : 1.0f;
    if (kind == POINTOPS2_OPTIM_SGD) {
        rec[0] = (float)gr.lr;
        rec[1] = (float)gr.beta1;
        rec[2] = (float)gr.weight_decay;
        rec[3] = inv_scale;
        rec[4] = clip;
        rec[5] = gr.beta2 != 0.0 ? 1.0f : 0.0f;
        return;
    }
    float *step = tab[t].step;
    const float t_new = *step + 1.0f;
    if (*found_inf == 0.0f) *step = t_new;
    const unsigned long long n = t_new >= 1.0f ? (unsigned long long)t_new : 0ull;  // (a NaN or negative count: beta^0, and 1 / 0 below)
    const double bias1 = 1.0 - pow_by_squaring(gr.beta1, n), bias2 = 1.0 - pow_by_squaring(gr.beta2, n);
    rec[0] = (float)(gr.lr / bias1);
    rec[1] = (float)sqrt(bias2);
    rec[2] = (float)gr.beta1;
    rec[3] = (float)(1.0 - gr.beta1);
    rec[4] = (float)gr.beta2;
    rec[5] = (float)(1.0 - gr.beta2);
    rec[6] = (float)gr.eps;
    rec[7] = (float)(1.0 - gr.lr * gr.weight_decay);
    rec[8] = inv_scale;
    rec[9] = clip;
}

struct Rec {
    float step_size, sqrt_bias2, beta1, omb1, beta2, omb2, eps, decay, inv_scale, coef;
};

// one element; the order of the file's header
__device__ __forceinline__ void adamw_elem(const Rec &r, float &p, float grad, float &m, float &v) {
    const float g = (grad * r.inv_scale) * r.coef;
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
    const Rec r{rp[0], rp[1], rp[2], rp[3], rp[4], rp[5], rp[6], rp[7], rp[8], rp[9]};
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

struct SgdRec {
    float lr, momentum, weight_decay, inv_scale, coef;
    bool nesterov;
};

// one element; the order of the file's header (MOMENTUM = false leaves buf alone)
template <bool MOMENTUM>
__device__ __forceinline__ void sgd_elem(const SgdRec &r, float &p, float grad, float &buf) {
    float g = (grad * r.inv_scale) * r.coef;
    if (r.weight_decay != 0.0f) g = g + (p * r.weight_decay);
    if (MOMENTUM) {
        buf = (buf * r.momentum) + g;
        g = r.nesterov ? g + (buf * r.momentum) : buf;
    }
    p = p - (g * r.lr);
}

template <bool MOMENTUM>
__device__ __forceinline__ void sgd_chunk(const SgdRec &r, int n, float *__restrict__ p, const float *__restrict__ g, float *__restrict__ b) {
    const int tid = threadIdx.x;
    if (n == OPT_CHUNK && !(misaligned16(p) || misaligned16(g) || (MOMENTUM && misaligned16(b)))) {
        float4 pv[OPT_VEC_STEPS], gv[OPT_VEC_STEPS], bv[OPT_VEC_STEPS];
#pragma unroll
        for (int s = 0; s < OPT_VEC_STEPS; s++) {
            const int e = 4 * (s * OPT_THREADS + tid);
            pv[s] = ldg4(p + e), gv[s] = ldg4(g + e);
            bv[s] = MOMENTUM ? ldg4(b + e) : float4{0.0f, 0.0f, 0.0f, 0.0f};
        }
#pragma unroll
        for (int s = 0; s < OPT_VEC_STEPS; s++) {
            const int e = 4 * (s * OPT_THREADS + tid);
            sgd_elem<MOMENTUM>(r, pv[s].x, gv[s].x, bv[s].x);
            sgd_elem<MOMENTUM>(r, pv[s].y, gv[s].y, bv[s].y);
            sgd_elem<MOMENTUM>(r, pv[s].z, gv[s].z, bv[s].z);
            sgd_elem<MOMENTUM>(r, pv[s].w, gv[s].w, bv[s].w);
            stg4(p + e, pv[s]);
            if (MOMENTUM) stg4(b + e, bv[s]);
        }
    } else {
        for (int i = tid; i < n; i += OPT_THREADS) {
            float pe = p[i], be = MOMENTUM ? b[i] : 0.0f;
            sgd_elem<MOMENTUM>(r, pe, g[i], be);
            p[i] = pe;
            if (MOMENTUM) b[i] = be;
        }
    }
}

__global__ __launch_bounds__(OPT_THREADS) void optim_sgd_kernel(int n_tensors, const pointops2_optim_tensor *__restrict__ tab,
                                                                const float *__restrict__ recs, const float *__restrict__ found_inf) {
    if (*found_inf != 0.0f) return;
    const int wg = blockIdx.x;
    const int t = tensor_of(tab, n_tensors, wg);
    const long long base = (long long)(wg - tab[t].first_chunk) * OPT_CHUNK, left = tab[t].numel - base;
    const int n = left < OPT_CHUNK ? (int)left : OPT_CHUNK;
    const float *rp = recs + (size_t)t * OPT_REC;
    const SgdRec r{rp[0], rp[1], rp[2], rp[3], rp[4], rp[5] != 0.0f};
    if (r.momentum != 0.0f) sgd_chunk<true>(r, n, tab[t].param + base, tab[t].grad + base, tab[t].exp_avg + base);
    else sgd_chunk<false>(r, n, tab[t].param + base, tab[t].grad + base, nullptr);
}

}  // namespace
}  // namespace p2

using namespace p2;

namespace {

// the workspace behind the table and the records: one float64 partial per chunk, then the clip coefficient
inline size_t clip_bytes(long long n_chunks) { return (size_t)n_chunks * sizeof(double) + 16; }

// `legacy`: called as optim_adamw_step_launcher, whose messages name it
#define OPTIM_REFUSE(text)                                                        \
    do {                                                                          \
        set_error(legacy ? "optim_adamw_step: " text : "optim_step: " text);      \
        return;                                                                   \
    } while (0)

void optim_step(bool legacy, int kind, int n_tensors, int n_groups, void *host_table, void *workspace, size_t workspace_bytes, const float *scale,
                float *found_inf, int run_check, double max_norm, float *grad_norm) {
    const hipStream_t st = begin_launch().stream;
    if (kind != POINTOPS2_OPTIM_ADAMW && kind != POINTOPS2_OPTIM_SGD) OPTIM_REFUSE("unknown kind");
    if (n_tensors < 0) OPTIM_REFUSE("negative tensor count");
    if (n_groups < 0) OPTIM_REFUSE("negative group count");
    if (found_inf == nullptr) OPTIM_REFUSE("found_inf must not be NULL");
    if (max_norm != max_norm) OPTIM_REFUSE("max_norm must not be a NaN");
    if (n_tensors > 0 && (host_table == nullptr || workspace == nullptr)) OPTIM_REFUSE("host_table and workspace must not be NULL");
    const size_t base_bytes = pointops2_optim_workspace_bytes(n_tensors, n_groups);
    if (workspace_bytes < base_bytes) OPTIM_REFUSE("workspace smaller than pointops2_optim_workspace_bytes(n_tensors, n_groups)");
    const bool clip = max_norm > 0.0 && grad_norm != nullptr;
    pointops2_optim_tensor *tensors = static_cast<pointops2_optim_tensor *>(host_table);
    const pointops2_optim_group *host_groups = reinterpret_cast<const pointops2_optim_group *>(tensors + n_tensors);
    long long chunks = 0;
    for (int t = 0; t < n_tensors; t++) {
        const pointops2_optim_tensor &x = tensors[t];
        if (x.numel < 0 || x.numel >= (1ll << 31)) OPTIM_REFUSE("numel must be in [0, 2^31)");
        if (x.group < 0 || x.group >= n_groups) OPTIM_REFUSE("group index out of range");
        if (kind == POINTOPS2_OPTIM_ADAMW) {
            if (x.step == nullptr || (x.numel > 0 && (x.param == nullptr || x.grad == nullptr || x.exp_avg == nullptr || x.exp_avg_sq == nullptr)))
                OPTIM_REFUSE("a tensor's param, grad, exp_avg, exp_avg_sq and step must not be NULL");
        } else if (x.numel > 0 && (x.param == nullptr || x.grad == nullptr || (x.exp_avg == nullptr && host_groups[x.group].beta1 != 0.0))) {
            OPTIM_REFUSE("SGD: a tensor's param and grad, and with a momentum its buffer (exp_avg), must not be NULL");
        }
        chunks += div_up64(x.numel, OPT_CHUNK);
    }
    if (chunks > 0x7fffffffll) OPTIM_REFUSE("more than 2^31 - 1 chunks");
    if (clip && workspace_bytes < base_bytes + clip_bytes(chunks))
        OPTIM_REFUSE("workspace smaller than pointops2_optim_step_workspace_bytes(n_tensors, n_groups, n_chunks)");
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
    double *partial = reinterpret_cast<double *>(static_cast<char *>(workspace) + base_bytes);
    float *coef = clip ? reinterpret_cast<float *>(partial + chunks) : nullptr;
    if ((run_check || clip) && chunks > 0) {
        const dim3 grid((unsigned)chunks), block(OPT_THREADS);
        if (!clip) hipLaunchKernelGGL((optim_check_kernel<true, false>), grid, block, 0, st, n_tensors, tab, scale, found_inf, (double *)nullptr);
        else if (run_check) hipLaunchKernelGGL((optim_check_kernel<true, true>), grid, block, 0, st, n_tensors, tab, scale, found_inf, partial);
        else hipLaunchKernelGGL((optim_check_kernel<false, true>), grid, block, 0, st, n_tensors, tab, scale, found_inf, partial);
        if (!check_launch()) return;
    }
    if (clip) {
        hipLaunchKernelGGL(optim_norm_reduce_kernel, dim3(1), dim3(OPT_THREADS), 0, st, chunks, (const double *)partial, max_norm, grad_norm, coef);
        if (!check_launch()) return;
    }
    hipLaunchKernelGGL(optim_prologue_kernel, dim3(div_up(n_tensors, OPT_THREADS)), dim3(OPT_THREADS), 0, st, n_tensors, tab, groups, scale,
                       (const float *)found_inf, (const float *)coef, kind, recs);
    if (!check_launch()) return;
    if (chunks > 0) {
        if (kind == POINTOPS2_OPTIM_ADAMW)
            hipLaunchKernelGGL(optim_adamw_kernel, dim3((unsigned)chunks), dim3(OPT_THREADS), 0, st, n_tensors, tab, (const float *)recs,
                               (const float *)found_inf);
        else
            hipLaunchKernelGGL(optim_sgd_kernel, dim3((unsigned)chunks), dim3(OPT_THREADS), 0, st, n_tensors, tab, (const float *)recs,
                               (const float *)found_inf);
        check_launch();
    }
}

#undef OPTIM_REFUSE

}  // namespace

extern "C" {

size_t pointops2_optim_workspace_bytes(int n_tensors, int n_groups) {
    if (n_tensors < 0 || n_groups < 0) return 0;
    return table_bytes(n_tensors, n_groups) + (size_t)n_tensors * OPT_REC * sizeof(float);
}

size_t pointops2_optim_step_workspace_bytes(int n_tensors, int n_groups, long long n_chunks) {
    if (n_tensors < 0 || n_groups < 0 || n_chunks < 0) return 0;
    return pointops2_optim_workspace_bytes(n_tensors, n_groups) + clip_bytes(n_chunks);
}

void optim_adamw_step_launcher(int n_tensors, int n_groups, void *host_table, void *workspace, size_t workspace_bytes, const float *scale,
                               float *found_inf, int run_check) {
    optim_step(true, POINTOPS2_OPTIM_ADAMW, n_tensors, n_groups, host_table, workspace, workspace_bytes, scale, found_inf, run_check, 0.0, nullptr);
}

void optim_step_launcher(int kind, int n_tensors, int n_groups, void *host_table, void *workspace, size_t workspace_bytes, const float *scale,
                         float *found_inf, int run_check, double max_norm, float *grad_norm) {
    optim_step(false, kind, n_tensors, n_groups, host_table, workspace, workspace_bytes, scale, found_inf, run_check, max_norm, grad_norm);
}

}  // extern "C"
