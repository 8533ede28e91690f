/*
 * TEST INFRASTRUCTURE — NOT PRODUCT CODE.
 *
 * CPU restatement ("oracle") of the arithmetic of the reference's pointops2 CUDA
 * kernels, written from the kernel sources under /root/reference/lib/pointops2/src
 * (each function cites the file:line it follows).  Only tests/, __graft_entry__.smoke()
 * and bench.py's cpu_baseline leg may load this library; the product path
 * (stratified_transformer_amd/) never does and fails loudly without its HIP library.
 *
 * Pinning: the attention ops (A1/A2/A4 + v1 forms) are pinned against golden vectors
 * produced by executing the reference's own model code on CPU (tests/golden/
 * make_golden.py).  furthestsampling and knnquery have no Python form and no test in
 * the reference => "parity unpinned" beyond this line-by-line restatement; they are
 * cross-checked against independent numpy formulations in tests/test_oracle.py.
 *
 * Arithmetic notes
 *  - nvcc contracts a*b+c into fma by default; the restatement writes the fmaf chain
 *    explicitly and is compiled with -ffp-contract=off so nothing else is fused.
 *    Squared distance: d = fma(dz,dz, fma(dx,dx, dy*dy)) (the contraction LLVM/NVVM
 *    picks for (dx*dx + dy*dy) + dz*dz).
 *  - CUDA atomicAdd sums have no defined order; the oracle accumulates those sums
 *    sequentially in pair order (fp32), which is one of the orders the reference can
 *    produce.
 *
 * OpenMP: every entry point is parallel over its natural outer loop so the same code
 * doubles as the timed CPU baseline ("port") in bench.py.  Scatter targets that several
 * queries hit (grad_k, grad_v, table grads) use per-thread private tables or atomics.
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#ifdef _OPENMP
#include <omp.h>
#else
static int omp_get_max_threads(void) { return 1; }
static int omp_get_thread_num(void) { return 0; }
#endif

int oracle_num_threads(void) { return omp_get_max_threads(); }
void oracle_set_num_threads(int n) {
#ifdef _OPENMP
    if (n > 0) omp_set_num_threads(n);
#else
    (void)n;
#endif
}

/* cuda_utils.h:10-13 */
static int opt_n_threads(int work_size) {
    if (work_size < 1) return 1;
    int pow_2 = (int)(log((double)work_size) / log(2.0));
    int v = 1 << pow_2;
    if (v > 1024) v = 1024;
    if (v < 1) v = 1;
    return v;
}
int oracle_opt_n_threads(int work_size) { return opt_n_threads(work_size); }

static inline float sqdist(float x1, float y1, float z1, float x2, float y2, float z2) {
    float dx = x2 - x1, dy = y2 - y1, dz = z2 - z1;
    return fmaf(dz, dz, fmaf(dx, dx, dy * dy));
}

/* ------------------------------------------------------------------------------------------
 * furthestsampling: sampling_cuda_kernel.cu:14-129 (kernel), :131-171 (launcher: block size
 * = opt_n_threads(n)).  One "block" per batch element; thread tid owns points start+tid,
 * start+tid+B, ...; strict '>' keeps the first maximum per thread (:57-58); the LDS tree
 * (:64-123) keeps the lower thread on ties (__update :5-10).
 * tmp[n] must be pre-filled with 1e10 and idx[m] zeroed by the caller (pointops.py:25-26).
 * ---------------------------------------------------------------------------------------- */
void oracle_furthestsampling(int b, int n, const float *xyz, const int *offset,
                             const int *new_offset, float *tmp, int *idx) {
    int B = opt_n_threads(n);
    /* default: of the launcher's switch can only be hit for n_threads not a power of two <=1024,
       which opt_n_threads never returns. */
    float *dists = (float *)malloc(sizeof(float) * B);
    int *dists_i = (int *)malloc(sizeof(int) * B);
    for (int bid = 0; bid < b; bid++) {
        int start_n = bid == 0 ? 0 : offset[bid - 1];
        int end_n = offset[bid];
        int start_m = bid == 0 ? 0 : new_offset[bid - 1];
        int end_m = new_offset[bid];
        int old = start_n;
        idx[start_m] = start_n;
        /* One thread team for all iterations.  "CUDA thread" tid owns points start+tid, start+tid+B, ...
           (:49); the loops below walk them chunk-major so memory is swept linearly, which visits every
           thread's points in the same ascending order as the kernel does. */
#pragma omp parallel
        for (int j = start_m + 1; j < end_m; j++) {
            float x1 = xyz[old * 3 + 0], y1 = xyz[old * 3 + 1], z1 = xyz[old * 3 + 2];
#pragma omp for schedule(static)
            for (int tid = 0; tid < B; tid++) { dists[tid] = -1; dists_i[tid] = start_n; }
            int nt = omp_get_num_threads(), me = omp_get_thread_num();
            int t0 = (int)((long long)B * me / nt), t1 = (int)((long long)B * (me + 1) / nt);
            for (int base = start_n; base < end_n; base += B) {
                int hi = t1 < end_n - base ? t1 : end_n - base;
                for (int tid = t0; tid < hi; tid++) {
                    int k = base + tid;
                    float d = sqdist(x1, y1, z1, xyz[k * 3 + 0], xyz[k * 3 + 1], xyz[k * 3 + 2]);
                    float d2 = fminf(d, tmp[k]);
                    tmp[k] = d2;
                    float best = dists[tid];
                    dists_i[tid] = d2 > best ? k : dists_i[tid];
                    dists[tid] = d2 > best ? d2 : best;
                }
            }
#pragma omp barrier
#pragma omp single
            {
                for (int s = B / 2; s >= 1; s >>= 1) {
                    for (int tid = 0; tid < s; tid++) {
                        float v1 = dists[tid], v2 = dists[tid + s];
                        int i1 = dists_i[tid], i2 = dists_i[tid + s];
                        dists[tid] = v1 > v2 ? v1 : v2; /* max(v1, v2) */
                        dists_i[tid] = v2 > v1 ? i2 : i1;
                    }
                }
                old = dists_i[0];
                idx[j] = old;
            } /* implicit barrier: every thread sees the new `old` */
        }
    }
    free(dists);
    free(dists_i);
}

/* ------------------------------------------------------------------------------------------
 * knnquery: knnquery_cuda_kernel.cu:21-108.  Max-heap of size nsample (<=100 in the reference;
 * <=101 here, so that a test can look at the (k+1)-th best of k = 100), candidates visited in
 * index order with strict '<' against the heap top (:96), reheap (:21-37),
 * heap_sort ascending (:40-49).  dist2 holds SQUARED distances (sqrt is applied by the
 * Python wrapper, pointops.py:47).
 * ---------------------------------------------------------------------------------------- */
static void reheap(float *dist, int *idx, int k) {
    int root = 0, child = 1;
    while (child < k) {
        if (child + 1 < k && dist[child + 1] > dist[child]) child++;
        if (dist[root] > dist[child]) return;
        float tf = dist[root]; dist[root] = dist[child]; dist[child] = tf;
        int ti = idx[root]; idx[root] = idx[child]; idx[child] = ti;
        root = child;
        child = root * 2 + 1;
    }
}
static void heap_sort(float *dist, int *idx, int k) {
    for (int i = k - 1; i > 0; i--) {
        float tf = dist[0]; dist[0] = dist[i]; dist[i] = tf;
        int ti = idx[0]; idx[0] = idx[i]; idx[i] = ti;
        reheap(dist, idx, i);
    }
}
void oracle_knnquery(int m, int nsample, const float *xyz, const float *new_xyz,
                     const int *offset, const int *new_offset, int *idx, float *dist2) {
#pragma omp parallel for schedule(dynamic, 64)
    for (int pt = 0; pt < m; pt++) {
        int bt = 0;
        while (!(pt < new_offset[bt])) bt++; /* get_bt_idx :52-63 */
        int start = bt == 0 ? 0 : offset[bt - 1];
        int end = offset[bt];
        float nx = new_xyz[pt * 3 + 0], ny = new_xyz[pt * 3 + 1], nz = new_xyz[pt * 3 + 2];
        float best_dist[101]; /* the reference holds 100; one more lets a test look at the (k+1)-th best of k = 100 */
        int best_idx[101];
        for (int i = 0; i < nsample; i++) { best_dist[i] = 1e10f; best_idx[i] = start; }
        for (int i = start; i < end; i++) {
            float x = xyz[i * 3 + 0], y = xyz[i * 3 + 1], z = xyz[i * 3 + 2];
            /* (new_x - x)*(new_x - x) + ... : same contraction shape as sqdist with d = new - x */
            float dx = nx - x, dy = ny - y, dz = nz - z;
            float d2 = fmaf(dz, dz, fmaf(dx, dx, dy * dy));
            if (d2 < best_dist[0]) {
                best_dist[0] = d2;
                best_idx[0] = i;
                reheap(best_dist, best_idx, nsample);
            }
        }
        heap_sort(best_dist, best_idx, nsample);
        for (int i = 0; i < nsample; i++) {
            idx[pt * nsample + i] = best_idx[i];
            dist2[pt * nsample + i] = best_dist[i];
        }
    }
}

/* ------------------------------------------------------------------------------------------
 * A1  attention_step1 v2: attention_cuda_kernel_v2.cu:7-50 (fwd), :52-91 (bwd).
 * attn[m,h] = sum_i q[q_idx,h,i] * k[index1[m],h,i], i ascending, fma chain (:40-44).
 * ---------------------------------------------------------------------------------------- */
void oracle_attention_step1_forward_v2(int N, int M, int h, int C, const float *q, const float *k,
                                       const int *index0_offsets, const int *index1, float *attn) {
    int d = C / h;
    (void)M;
#pragma omp parallel for schedule(dynamic, 256)
    for (int qi = 0; qi < N; qi++) {
        int s = index0_offsets[qi], e = index0_offsets[qi + 1];
        for (int hh = 0; hh < h; hh++) {
            const float *qv = q + (size_t)qi * C + hh * d;
            for (int m = s; m < e; m++) {
                const float *kv = k + (size_t)index1[m] * C + hh * d;
                float sum = 0;
                for (int i = 0; i < d; i++) sum = fmaf(qv[i], kv[i], sum);
                attn[(size_t)m * h + hh] = sum;
            }
        }
    }
}

static inline void atomic_addf(float *p, float v) {
#pragma omp atomic
    *p += v;
}

void oracle_attention_step1_backward_v2(int N, int M, int h, int C, const float *grad_out,
                                        const int *index0_offsets, const int *index1,
                                        const float *q, const float *k, float *grad_q, float *grad_k) {
    int d = C / h;
    (void)M;
#pragma omp parallel for schedule(dynamic, 256)
    for (int qi = 0; qi < N; qi++) {
        int s = index0_offsets[qi], e = index0_offsets[qi + 1];
        for (int hh = 0; hh < h; hh++) {
            const float *qv = q + (size_t)qi * C + hh * d;
            float gq[64];
            for (int i = 0; i < d; i++) gq[i] = 0;
            for (int m = s; m < e; m++) {
                float g = grad_out[(size_t)m * h + hh];
                size_t kb = (size_t)index1[m] * C + hh * d;
                for (int i = 0; i < d; i++) {
                    gq[i] += g * k[kb + i];                 /* :83 LDS atomicAdd */
                    atomic_addf(grad_k + kb + i, g * qv[i]); /* :84 global atomicAdd */
                }
            }
            for (int i = 0; i < d; i++) grad_q[(size_t)qi * C + hh * d + i] = gq[i];
        }
    }
}

/* v1 (pair-indexed) form: attention_cuda_kernel.cu:7-56.  Same sums via atomics. */
void oracle_attention_step1_forward(int N, int M, int h, int C, const float *q, const float *k,
                                    const int *index0, const int *index1, float *attn) {
    int d = C / h;
    (void)N;
#pragma omp parallel for schedule(static)
    for (int m = 0; m < M; m++)
        for (int hh = 0; hh < h; hh++) {
            const float *qv = q + (size_t)index0[m] * C + hh * d;
            const float *kv = k + (size_t)index1[m] * C + hh * d;
            float sum = attn[(size_t)m * h + hh];
            for (int i = 0; i < d; i++) sum += qv[i] * kv[i];
            attn[(size_t)m * h + hh] = sum;
        }
}
void oracle_attention_step1_backward(int N, int M, int h, int C, const float *grad_out,
                                     const int *index0, const int *index1, const float *q,
                                     const float *k, float *grad_q, float *grad_k) {
    int d = C / h;
    (void)N;
    for (int m = 0; m < M; m++)
        for (int hh = 0; hh < h; hh++) {
            float g = grad_out[(size_t)m * h + hh];
            size_t qb = (size_t)index0[m] * C + hh * d, kb = (size_t)index1[m] * C + hh * d;
            for (int i = 0; i < d; i++) {
                grad_q[qb + i] += g * k[kb + i];
                grad_k[kb + i] += g * q[qb + i];
            }
        }
}

/* A4' attention_step2 (no rel-pos value): attention_cuda_kernel.cu:58-87 */
void oracle_attention_step2_forward(int N, int M, int h, int C, const float *attn, const float *v,
                                    const int *index0, const int *index1, float *output) {
    int d = C / h;
    (void)N;
    for (int m = 0; m < M; m++)
        for (int hh = 0; hh < h; hh++) {
            float a = attn[(size_t)m * h + hh];
            size_t ob = (size_t)index0[m] * C + hh * d, vb = (size_t)index1[m] * C + hh * d;
            for (int i = 0; i < d; i++) output[ob + i] += a * v[vb + i];
        }
}
void oracle_attention_step2_backward(int N, int M, int h, int C, const float *grad_out,
                                     const int *index0, const int *index1, const float *attn,
                                     const float *v, float *grad_attn, float *grad_v) {
    int d = C / h;
    (void)N;
    for (int m = 0; m < M; m++)
        for (int hh = 0; hh < h; hh++) {
            float a = attn[(size_t)m * h + hh];
            size_t ob = (size_t)index0[m] * C + hh * d, vb = (size_t)index1[m] * C + hh * d;
            float ga = grad_attn[(size_t)m * h + hh];
            for (int i = 0; i < d; i++) {
                ga += grad_out[ob + i] * v[vb + i];
                grad_v[vb + i] += grad_out[ob + i] * a;
            }
            grad_attn[(size_t)m * h + hh] = ga;
        }
}

/* ------------------------------------------------------------------------------------------
 * A2  dot_prod_with_idx v3: relative_pos_encoding_cuda_kernel_v2.cu:247-283 (fwd), :287-340 (bwd)
 * T(m,h,i) = table[r0,h,i,0] + table[r1,h,i,1] + table[r2,h,i,2]   (left-to-right, :276,:278)
 * sum = fma(q_i, Tq, sum); sum = fma(k_i, Tk, sum)                 (:277,:279)
 * ---------------------------------------------------------------------------------------- */
#define TBL(t, r, hh, i, ax) (t)[(size_t)(r) * C * 3 + (hh) * d * 3 + (i) * 3 + (ax)]

void oracle_dot_prod_with_idx_forward_v3(int N, int M, int h, int d, const float *q,
                                         const int *index_q_offsets, const float *k,
                                         const int *index_k, const float *table_q,
                                         const float *table_k, const int *rel_idx, float *output) {
    int C = h * d;
    (void)M;
#pragma omp parallel for schedule(dynamic, 256)
    for (int qi = 0; qi < N; qi++) {
        int s = index_q_offsets[qi], e = index_q_offsets[qi + 1];
        for (int hh = 0; hh < h; hh++) {
            const float *qv = q + (size_t)qi * C + hh * d;
            for (int m = s; m < e; m++) {
                const float *kv = k + (size_t)index_k[m] * C + hh * d;
                int r0 = rel_idx[m * 3], r1 = rel_idx[m * 3 + 1], r2 = rel_idx[m * 3 + 2];
                float sum = 0;
                for (int i = 0; i < d; i++) {
                    float tq = TBL(table_q, r0, hh, i, 0) + TBL(table_q, r1, hh, i, 1) + TBL(table_q, r2, hh, i, 2);
                    sum = fmaf(qv[i], tq, sum);
                    float tk = TBL(table_k, r0, hh, i, 0) + TBL(table_k, r1, hh, i, 1) + TBL(table_k, r2, hh, i, 2);
                    sum = fmaf(kv[i], tk, sum);
                }
                output[(size_t)m * h + hh] = sum;
            }
        }
    }
}

void oracle_dot_prod_with_idx_backward_v3(int N, int M, int h, int d, int L, const float *grad_out,
                                          const float *q, const int *index_q_offsets, const float *k,
                                          const int *index_k, const float *table_q, const float *table_k,
                                          const int *rel_idx, float *grad_q, float *grad_k,
                                          float *grad_table_q, float *grad_table_k) {
    int C = h * d;
    (void)M;
    size_t tsz = (size_t)L * C * 3;
    int nt = omp_get_max_threads();
    float *priv = (float *)calloc((size_t)nt * 2 * tsz, sizeof(float));
#pragma omp parallel
    {
        float *gtq = priv + (size_t)omp_get_thread_num() * 2 * tsz;
        float *gtk = gtq + tsz;
#pragma omp for schedule(dynamic, 256)
        for (int qi = 0; qi < N; qi++) {
            int s = index_q_offsets[qi], e = index_q_offsets[qi + 1];
            for (int hh = 0; hh < h; hh++) {
                const float *qv = q + (size_t)qi * C + hh * d;
                float gq[64];
                for (int i = 0; i < d; i++) gq[i] = 0;
                for (int m = s; m < e; m++) {
                    size_t kb = (size_t)index_k[m] * C + hh * d;
                    int r0 = rel_idx[m * 3], r1 = rel_idx[m * 3 + 1], r2 = rel_idx[m * 3 + 2];
                    float g = grad_out[(size_t)m * h + hh];
                    for (int i = 0; i < d; i++) {
                        float tq = TBL(table_q, r0, hh, i, 0) + TBL(table_q, r1, hh, i, 1) + TBL(table_q, r2, hh, i, 2);
                        float tk = TBL(table_k, r0, hh, i, 0) + TBL(table_k, r1, hh, i, 1) + TBL(table_k, r2, hh, i, 2);
                        float qs = qv[i], ks = k[kb + i];
                        gq[i] += tq * g;
                        atomic_addf(grad_k + kb + i, tk * g);
                        TBL(gtq, r0, hh, i, 0) += qs * g;
                        TBL(gtq, r1, hh, i, 1) += qs * g;
                        TBL(gtq, r2, hh, i, 2) += qs * g;
                        TBL(gtk, r0, hh, i, 0) += ks * g;
                        TBL(gtk, r1, hh, i, 1) += ks * g;
                        TBL(gtk, r2, hh, i, 2) += ks * g;
                    }
                }
                for (int i = 0; i < d; i++) grad_q[(size_t)qi * C + hh * d + i] = gq[i];
            }
        }
    }
    for (int t = 0; t < nt; t++) {
        const float *gtq = priv + (size_t)t * 2 * tsz, *gtk = gtq + tsz;
        for (size_t i = 0; i < tsz; i++) { grad_table_q[i] += gtq[i]; grad_table_k[i] += gtk[i]; }
    }
    free(priv);
}

/* v1 single-table form: relative_pos_encoding_cuda_kernel.cu:7-51 */
void oracle_dot_prod_with_idx_forward(int N, int M, int h, int d, const float *q, const int *index,
                                      const float *table, const int *rel_idx, float *output) {
    int C = h * d;
    (void)N;
#pragma omp parallel for schedule(static)
    for (int m = 0; m < M; m++)
        for (int hh = 0; hh < h; hh++) {
            const float *qv = q + (size_t)index[m] * C + hh * d;
            float sum = output[(size_t)m * h + hh];
            for (int i = 0; i < d; i++)
                for (int ax = 0; ax < 3; ax++) sum += qv[i] * TBL(table, rel_idx[m * 3 + ax], hh, i, ax);
            output[(size_t)m * h + hh] = sum;
        }
}
void oracle_dot_prod_with_idx_backward(int N, int M, int h, int d, const float *grad_out, const float *q,
                                       const int *index, const float *table, const int *rel_idx,
                                       float *grad_q, float *grad_table) {
    int C = h * d;
    (void)N;
    for (int m = 0; m < M; m++)
        for (int hh = 0; hh < h; hh++) {
            float g = grad_out[(size_t)m * h + hh];
            size_t qb = (size_t)index[m] * C + hh * d;
            for (int i = 0; i < d; i++)
                for (int ax = 0; ax < 3; ax++) {
                    int r = rel_idx[m * 3 + ax];
                    grad_q[qb + i] += g * TBL(table, r, hh, i, ax);
                    TBL(grad_table, r, hh, i, ax) += g * q[qb + i];
                }
        }
}

/* ------------------------------------------------------------------------------------------
 * A4  attention_step2_with_rel_pos_value v2: ..._kernel_v2.cu:397-438 (fwd), :441-484 (bwd)
 * out[q,h,i] = sum_m (T(m,h,i) + v[idx1,h,i]) * attn[m,h]           (:428-430)
 * ---------------------------------------------------------------------------------------- */
void oracle_attention_step2_with_rel_pos_value_forward_v2(int N, int M, int h, int d, const float *attn,
                                                          const float *v, const int *index0_offsets,
                                                          const int *index1, const float *table,
                                                          const int *rel_idx, float *output) {
    int C = h * d;
    (void)M;
#pragma omp parallel for schedule(dynamic, 256)
    for (int qi = 0; qi < N; qi++) {
        int s = index0_offsets[qi], e = index0_offsets[qi + 1];
        for (int hh = 0; hh < h; hh++) {
            float res[64];
            for (int i = 0; i < d; i++) res[i] = 0;
            for (int m = s; m < e; m++) {
                float a = attn[(size_t)m * h + hh];
                int r0 = rel_idx[m * 3], r1 = rel_idx[m * 3 + 1], r2 = rel_idx[m * 3 + 2];
                const float *vv = v + (size_t)index1[m] * C + hh * d;
                for (int i = 0; i < d; i++) {
                    float t = TBL(table, r0, hh, i, 0) + TBL(table, r1, hh, i, 1) + TBL(table, r2, hh, i, 2);
                    res[i] += (t + vv[i]) * a;
                }
            }
            for (int i = 0; i < d; i++) output[(size_t)qi * C + hh * d + i] = res[i];
        }
    }
}

void oracle_attention_step2_with_rel_pos_value_backward_v2(int N, int M, int h, int d, int L,
                                                           const float *grad_out, const int *index0_offsets,
                                                           const int *index1, const float *attn, const float *v,
                                                           const float *table, const int *rel_idx,
                                                           float *grad_attn, float *grad_v, float *grad_table) {
    int C = h * d;
    (void)M;
    size_t tsz = (size_t)L * C * 3;
    int nt = omp_get_max_threads();
    float *priv = (float *)calloc((size_t)nt * tsz, sizeof(float));
#pragma omp parallel
    {
        float *gt = priv + (size_t)omp_get_thread_num() * tsz;
#pragma omp for schedule(dynamic, 256)
        for (int qi = 0; qi < N; qi++) {
            int s = index0_offsets[qi], e = index0_offsets[qi + 1];
            for (int hh = 0; hh < h; hh++) {
                const float *go = grad_out + (size_t)qi * C + hh * d;
                for (int m = s; m < e; m++) {
                    size_t vb = (size_t)index1[m] * C + hh * d;
                    int r0 = rel_idx[m * 3], r1 = rel_idx[m * 3 + 1], r2 = rel_idx[m * 3 + 2];
                    float a = attn[(size_t)m * h + hh];
                    float gsum = 0;
                    for (int i = 0; i < d; i++) {
                        float t = TBL(table, r0, hh, i, 0) + TBL(table, r1, hh, i, 1) + TBL(table, r2, hh, i, 2);
                        gsum = fmaf(t + v[vb + i], go[i], gsum); /* :475 */
                        float ag = a * go[i];
                        atomic_addf(grad_v + vb + i, ag);
                        TBL(gt, r0, hh, i, 0) += ag;
                        TBL(gt, r1, hh, i, 1) += ag;
                        TBL(gt, r2, hh, i, 2) += ag;
                    }
                    grad_attn[(size_t)m * h + hh] = gsum;
                }
            }
        }
    }
    for (int t = 0; t < nt; t++) {
        const float *gt = priv + (size_t)t * tsz;
        for (size_t i = 0; i < tsz; i++) grad_table[i] += gt[i];
    }
    free(priv);
}

/* v1 form: relative_pos_encoding_cuda_kernel.cu:69-118.  Three threads per pair, each adds
 * attn * (v/3.0 + table[dim]) with the v/3.0 term evaluated in double (:87, :112-114). */
void oracle_attention_step2_with_rel_pos_value_forward(int N, int M, int h, int d, const float *attn,
                                                       const float *v, const int *index0, const int *index1,
                                                       const float *table, const int *rel_idx, float *output) {
    int C = h * d;
    (void)N;
    for (int m = 0; m < M; m++)
        for (int hh = 0; hh < h; hh++) {
            float a = attn[(size_t)m * h + hh];
            size_t ob = (size_t)index0[m] * C + hh * d, vb = (size_t)index1[m] * C + hh * d;
            for (int i = 0; i < d; i++)
                for (int ax = 0; ax < 3; ax++) {
                    float tv = TBL(table, rel_idx[m * 3 + ax], hh, i, ax);
                    float val = (float)((double)a * ((double)v[vb + i] / 3.0 + (double)tv));
                    output[ob + i] += val;
                }
        }
}
void oracle_attention_step2_with_rel_pos_value_backward(int N, int M, int h, int d, const float *grad_out,
                                                        const int *index0, const int *index1, const float *attn,
                                                        const float *v, const float *table, const int *rel_idx,
                                                        float *grad_attn, float *grad_v, float *grad_table) {
    int C = h * d;
    (void)N;
    for (int m = 0; m < M; m++)
        for (int hh = 0; hh < h; hh++) {
            float a = attn[(size_t)m * h + hh];
            size_t ob = (size_t)index0[m] * C + hh * d, vb = (size_t)index1[m] * C + hh * d;
            for (int i = 0; i < d; i++)
                for (int ax = 0; ax < 3; ax++) {
                    int r = rel_idx[m * 3 + ax];
                    float g = grad_out[ob + i];
                    float tv = TBL(table, r, hh, i, ax);
                    grad_attn[(size_t)m * h + hh] += g * (v[vb + i] / 3 + tv);
                    grad_v[vb + i] += g * a / 3;
                    TBL(grad_table, r, hh, i, ax) += g * a;
                }
        }
}

/* grouping: grouping_cuda_kernel.cu:5-25 */
void oracle_grouping_forward(int m, int nsample, int c, const float *input, const int *idx, float *output) {
#pragma omp parallel for schedule(static)
    for (int i = 0; i < m * nsample; i++)
        memcpy(output + (size_t)i * c, input + (size_t)idx[i] * c, sizeof(float) * c);
}
void oracle_grouping_backward(int m, int nsample, int c, const float *grad_output, const int *idx, float *grad_input) {
    for (int i = 0; i < m * nsample; i++)
        for (int j = 0; j < c; j++) grad_input[(size_t)idx[i] * c + j] += grad_output[(size_t)i * c + j];
}

/* interpolation: interpolation_cuda_kernel.cu:5-33 */
void oracle_interpolation_forward(int n, int c, int k, const float *input, const int *idx, const float *weight, float *output) {
#pragma omp parallel for schedule(static)
    for (int p = 0; p < n; p++)
        for (int j = 0; j < c; j++) {
            float o = output[(size_t)p * c + j];
            for (int i = 0; i < k; i++) o += input[(size_t)idx[p * k + i] * c + j] * weight[p * k + i];
            output[(size_t)p * c + j] = o;
        }
}
void oracle_interpolation_backward(int n, int c, int k, const float *grad_output, const int *idx, const float *weight, float *grad_input) {
    for (int p = 0; p < n; p++)
        for (int j = 0; j < c; j++)
            for (int i = 0; i < k; i++)
                grad_input[(size_t)idx[p * k + i] * c + j] += grad_output[(size_t)p * c + j] * weight[p * k + i];
}

/* A3 scatter_softmax over CSR segments (torch_scatter 2.0.6 composite/softmax.py: max, exp(x-max),
 * sum, divide; sorted index => segments).  Third-party, absent from /root/reference: parity unpinned. */
void oracle_segment_softmax_forward(int N, int h, const float *src, const int *offsets, float *out) {
#pragma omp parallel for schedule(dynamic, 256)
    for (int qi = 0; qi < N; qi++) {
        int s = offsets[qi], e = offsets[qi + 1];
        for (int hh = 0; hh < h; hh++) {
            float mx = -INFINITY;
            for (int m = s; m < e; m++) mx = fmaxf(mx, src[(size_t)m * h + hh]);
            float sum = 0;
            for (int m = s; m < e; m++) { float ex = expf(src[(size_t)m * h + hh] - mx); out[(size_t)m * h + hh] = ex; sum += ex; }
            for (int m = s; m < e; m++) out[(size_t)m * h + hh] /= sum;
        }
    }
}
void oracle_segment_softmax_backward(int N, int h, const float *y, const float *grad_y, const int *offsets, float *grad_x) {
#pragma omp parallel for schedule(dynamic, 256)
    for (int qi = 0; qi < N; qi++) {
        int s = offsets[qi], e = offsets[qi + 1];
        for (int hh = 0; hh < h; hh++) {
            float dot = 0;
            for (int m = s; m < e; m++) dot += y[(size_t)m * h + hh] * grad_y[(size_t)m * h + hh];
            for (int m = s; m < e; m++) grad_x[(size_t)m * h + hh] = y[(size_t)m * h + hh] * (grad_y[(size_t)m * h + hh] - dot);
        }
    }
}
