// Window-centric ("cell") attention, forward and backward, gfx950.
//
// The reference's three operators and every pair walker of rpe.hip / attention.hip gather a key row once per
// (query, key) pair although ~70 % of a pair list are dense window x window blocks
// (model/stratified_transformer.py:15-18) and the rest are shared by all queries of a (small window, large
// window) intersection (:20-38).  index.hip's cell plan states that structure: a CELL is a set of n_q queries
// that share one list of n_k candidate keys, i.e. a dense n_q x n_k tile of pairs, with a packed rel-pos index
// and a "not a key of this query" flag per tile entry.
//
// One wave per (cell, head).  Lane (p, c) = key slot p (16 per pass) x quarter c of the 16 floats of a head row,
// as in the pair walkers - but here a lane OWNS its keys for the whole cell: the key / value rows of up to
// 16 * CA_NP keys are loaded ONCE into registers (float4 per key slot) and reused by all n_q queries, and in the
// backward the key-side gradients dK / dV are register accumulators that leave the wave once per cell.  What
// remains per pair is what cannot be shared: the 9 table rows T(rel) from the LDS image of the head's three
// tables, the packed rel-pos word and the softmax weight.
//
// forward   sweep 1 (K in registers): logits -> softmax per query -> p stored to the cell-ordered buffer pbuf
//           sweep 2 (V in registers): out = sum p (v + Tv)
// backward  sweep A (V, dV in registers): grad_attn, softmax backward -> gs stored; dV
//           sweep B (K, dK in registers): dQ, dK
//           cell_table_grad_kernel: the three table gradients from p / gs (fixed-point LDS histograms per row,
//           outer products on the matrix cores: the scheme of rpe_bwd_mfma.hip on cell rows - a query's row of
//           the tile is contiguous, a key's column is strided by n_k - no pair map, no CSC)
// Cells with more than 16 * CA_NP keys are taken in chunks (a running max / sum per query in `ml`, logits parked
// in pbuf); the shipped configs never need more than one chunk.
#include "cell_common.h"

namespace p2 {


// image of one head's table: [axis][row][16] elements of T (global layout [L, h, 16, 3])
template <typename T>
__device__ __forceinline__ void stage_table_t(T *lds, const T *__restrict__ tab, int L, int h, int head) {
    const int total = 3 * L * 16;
    for (int x = threadIdx.x; x < total; x += blockDim.x) {
        const int i = x % 16, r = (x / 16) % L, ax = x / (16 * L);
        lds[x] = tab[(((size_t)r * h + head) * 16 + i) * 3 + ax];
    }
}
// the three tables of a head, TS elements apart, ready for every wave of the workgroup
template <int TS, typename T>
__device__ __forceinline__ void stage_tables(T *lds, const T *__restrict__ table_q, const T *__restrict__ table_k, const T *__restrict__ table_v, int L,
                                             int h, int head) {
    stage_table_t<T>(lds, table_q, L, h, head);
    stage_table_t<T>(lds + TS, table_k, L, h, head);
    stage_table_t<T>(lds + 2 * TS, table_v, L, h, head);
    __syncthreads();
}

// ---- LDS image of a head's three tables: table TB at float offset TB * TS (TS a compile-time constant, so that the
// three tables of one (axis, row) differ by an immediate offset), inside a table [axis][row][16] ----
template <int LCAP>
struct TabGeo {
    static constexpr int TS = 3 * LCAP * 16;  // elements per table image
    static constexpr size_t bytes(size_t elem) { return (size_t)3 * TS * elem; }
};
struct RowOff {
    int o0, o1, o2;
};
__device__ __forceinline__ RowOff row_off(unsigned w, int L, int c) {
    RowOff r;
    r.o0 = (int)(w & 255u) * 16 + 4 * c;
    r.o1 = (int)(L + ((w >> 8) & 255u)) * 16 + 4 * c;
    r.o2 = (int)(2 * L + ((w >> 16) & 255u)) * 16 + 4 * c;
    return r;
}
// T(m)[4c..4c+3] = tab[r0,.,.,0] + tab[r1,.,.,1] + tab[r2,.,.,2]   (left to right, as the reference)
template <int OFF>
__device__ __forceinline__ float4 tsum_at(const float *lds, RowOff r) {
    return add4(add4(*reinterpret_cast<const float4 *>(lds + OFF + r.o0), *reinterpret_cast<const float4 *>(lds + OFF + r.o1)),
                *reinterpret_cast<const float4 *>(lds + OFF + r.o2));
}

// the three rows (one per axis) of one table for one pair, requested together
struct Rows3 {
    float4 a, b, c;
};
template <int OFF, typename T>
__device__ __forceinline__ Rows3 rows_at(const T *lds, RowOff r) {
    Rows3 x;
    x.a = ld_row4(lds + OFF + r.o0);
    x.b = ld_row4(lds + OFF + r.o1);
    x.c = ld_row4(lds + OFF + r.o2);
    return x;
}
// T(m)[4c..4c+3] = tab[r0,.,.,0] + tab[r1,.,.,1] + tab[r2,.,.,2]   (left to right, as the reference), as packed
// two-float adds (v_pk_add_f32: two lanes' worth of fp32 adds per instruction slot)
typedef float f32x2c __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float4 padd4(float4 a, float4 b) {
    const f32x2c lo = f32x2c{a.x, a.y} + f32x2c{b.x, b.y}, hi = f32x2c{a.z, a.w} + f32x2c{b.z, b.w};
    return make_float4(lo.x, lo.y, hi.x, hi.y);
}
__device__ __forceinline__ float4 pfma4(float s, float4 a, float4 acc) {
    const f32x2c ss = f32x2c{s, s};
    const f32x2c lo = __builtin_elementwise_fma(ss, f32x2c{a.x, a.y}, f32x2c{acc.x, acc.y});
    const f32x2c hi = __builtin_elementwise_fma(ss, f32x2c{a.z, a.w}, f32x2c{acc.z, acc.w});
    return make_float4(lo.x, lo.y, hi.x, hi.y);
}
__device__ __forceinline__ float4 rsum(Rows3 r) { return padd4(padd4(r.a, r.b), r.c); }
// <a, b> over this lane's four floats with packed multiply-adds (the two halves are summed at the end)
__device__ __forceinline__ f32x2c pdot_acc(float4 a, float4 b, f32x2c acc) {
    acc = __builtin_elementwise_fma(f32x2c{a.x, a.y}, f32x2c{b.x, b.y}, acc);
    return __builtin_elementwise_fma(f32x2c{a.z, a.w}, f32x2c{b.z, b.w}, acc);
}
__device__ __forceinline__ float pdot4(float4 a, float4 b) {
    const f32x2c r = pdot_acc(a, b, f32x2c{0.f, 0.f});
    return r.x + r.y;
}

// A chunk of a cell has np = 1..NP passes of 16 keys (wave-uniform).  The sweeps are straight-line code for a fixed
// number of passes - the table rows of pass t+1 are requested before pass t is consumed, which a per-pass branch
// would forbid (each pass a basic block of its own, every LDS round trip exposed) - instantiated for 2, 3, 4, 6 and 8
// passes; a chunk runs the smallest instance that holds it (slots past its end are masked anyway).
template <int NPMAX, typename F>
__device__ __forceinline__ void dispatch_passes(int np, F f) {
    if (np <= 2) f(std::integral_constant<int, 2>{});
    else if (np == 3) f(std::integral_constant<int, 3>{});
    else if (np == 4 || NPMAX <= 4) f(std::integral_constant<int, 4>{});
    else if constexpr (NPMAX > 4) {
        if (np <= 6) f(std::integral_constant<int, 6>{});
        else f(std::integral_constant<int, 8>{});
    }
}

// TT: storage type of the tables.  PK: the rows are those of a packed projection - rs (elements from one point's q / k / v row to the
// next, gradients laid out alike) and qscale (q is scaled as it is loaded, round_rows) come from the launch.  Otherwise the rows are
// [N, h, 16] tensors: rs = C, q is taken as it stands, and the instances are the ones the unpacked launchers always ran.
template <typename TT, bool PK>
struct LaneCtx {
    const TT *lds;
    int L, lane, p, c, head, h, C, hoff, rs_packed;
    float qscale;
    __device__ __forceinline__ int rs() const { return PK ? rs_packed : C; }
    template <typename RT>
    __device__ __forceinline__ float4 q_row4(const RT *q, int i) const {
        if constexpr (PK) return scaled_row4<RT>(q + (size_t)i * rs_packed + hoff, qscale);
        else return ld_row4(q + (size_t)i * C + hoff);
    }
};
// this thread's context in a workgroup that serves head blockIdx.y
template <typename TT, bool PK>
__device__ __forceinline__ LaneCtx<TT, PK> make_lane_ctx(const TT *lds, int h, int L, int rs, float qscale) {
    LaneCtx<TT, PK> x;
    x.lds = lds;
    x.L = L;
    x.h = h;
    x.head = blockIdx.y;
    x.C = h * 16;
    x.rs_packed = rs;
    x.qscale = qscale;
    x.lane = threadIdx.x & 63;
    x.p = x.lane >> 2;
    x.c = x.lane & 3;
    x.hoff = x.head * 16 + 4 * x.c;
    return x;
}

// ------------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------------
// Key slots: lane (p, c) of an NPA-pass instance owns the NPA CONSECUTIVE keys j0 + p * NPA + t, t < NPA, of the chunk, so
// that its rel-pos words, softmax weights and logit gradients of one query are NPA consecutive dwords = one wide load.
// Query ids: 64 at a time, one per lane; a query's id is then a v_readlane away (a scalar: the q row address is uniform).
// A slot past the chunk's end reads key 0 from the bounds-checked list: its row is replaced by zeros, not left to a weight of 0 to
// cancel (0 * inf = NaN: a non-finite row 0 would reach every cell with a partial last pass).
//
// Store order of the query loops: loads, stores and atomics share one counter (vmcnt) that retires in issue order, and
// the number of stores a wave issues depends on its lanes' paths (c == 0 / p == 0, nvalid), so a wait for a prefetched operand also
// covers every store issued before that wait.  A query's results are therefore held for one iteration and stored at the top of the
// next one, BEHIND the requests for the query after it: the one drain per iteration then covers loads and a store that were issued a
// whole iteration earlier.  The last query's results leave after the loop.  That drain is written out at the top of the body
// (wait_vmem: the wait this query's operands need anyway), so that no path into the loop's head - the prologue, a peeled first
// iteration - leaves a pending load that the compiler would have to wait for inside the body, by a count that includes this
// iteration's own requests.
// (the empty asm keeps the requests issued before the wait before it: the builtin alone does not order loads, and the compiler sinks them)
__device__ __forceinline__ void wait_vmem() {
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_waitcnt(0x0F70);  // s_waitcnt vmcnt(0)
}
// the next 64 query ids, waited for where they are requested (once per 64 queries) and not at the loop's head
__device__ __forceinline__ int next_query_ids(rsrc_t qid, int off) {
    const int ids = (int)bload_u32(qid, off);
    wait_vmem();
    return ids;
}

template <int NPA, typename RT, typename T, bool PK>
__device__ __forceinline__ void load_key_rows(const LaneCtx<T, PK> &x, const CellBufs &cb, const RT *__restrict__ rows, int j0, int nvalid,
                                              float4 (&r4)[NPA]) {
    unsigned keys[NPA];
    bload_words<NPA>(cb.key, (j0 + x.p * NPA) * 4, keys);  // (past the end: key 0)
#pragma unroll
    for (int t = 0; t < NPA; t++) {
        const float4 r = ld_row4(rows + (size_t)keys[t] * x.rs() + x.hoff);
        r4[t] = t < nvalid ? r : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

template <int NPA, int TS, typename RT, typename T, bool PK>
__device__ __forceinline__ void fwd_sweep_logits(const LaneCtx<T, PK> &x, const CellTask &ct, const CellBufs &cb, rsrc_t rs_p,
                                                 const RT *__restrict__ q, const RT *__restrict__ k, float *__restrict__ ml,
                                                 int ch, bool single, int j0, int nkc) {
    const int p = x.p, c = x.c;
    const int nvalid = min(max(nkc - p * NPA, 0), NPA);  // this lane's slots inside the chunk
    float4 k4[NPA];
    load_key_rows<NPA, RT, T, PK>(x, cb, k, j0, nvalid, k4);
    // the inputs of query il+1 are requested while query il is worked on
    int ids = (int)bload_u32(cb.qid, x.lane * 4);
    int i_nx = __builtin_amdgcn_readlane(ids, 0);
    float4 q4_nx = x.q_row4(q, i_nx);
    unsigned w_nx[NPA];
    bload_words<NPA>(cb.rel, (j0 + p * NPA) * 4, w_nx);
    float lg_pv[NPA];  // single: the weights of query il-1
#pragma unroll
    for (int t = 0; t < NPA; t++) lg_pv[t] = 0.f;
#pragma unroll 1  // (and no peeling of query 0)
    for (int il = 0; il < ct.nq; il++) {
        wait_vmem();  // this query's operands
        const int i = i_nx;
        const float4 q4 = q4_nx;
        unsigned w[NPA];
#pragma unroll
        for (int t = 0; t < NPA; t++) w[t] = w_nx[t];
        const int roff = (il * ct.nk + j0 + p * NPA) * 4;
        if (((il + 1) & 63) == 0) ids = next_query_ids(cb.qid, (il + 1 + x.lane) * 4);
        i_nx = __builtin_amdgcn_readlane(ids, (il + 1) & 63);  // (past the end: query 0, never used)
        q4_nx = x.q_row4(q, i_nx);
        bload_words<NPA>(cb.rel, roff + ct.nk * 4, w_nx);
        if (single && il && c == 0) bstore_floats<NPA>(rs_p, roff - ct.nk * 4, lg_pv, nvalid);
        float lg[NPA];
        float mx = -INFINITY;
        RowOff ro = row_off(w[0], x.L, c);
        Rows3 rq = rows_at<0, T>(x.lds, ro), rk = rows_at<TS, T>(x.lds, ro);
#pragma unroll
        for (int t = 0; t < NPA; t++) {
            Rows3 rq1 = rq, rk1 = rk;
            if (t + 1 < NPA) {
                ro = row_off(w[t + 1], x.L, c);
                rq1 = rows_at<0, T>(x.lds, ro);
                rk1 = rows_at<TS, T>(x.lds, ro);
            }
            const f32x2c d2 = pdot_acc(k4[t], rsum(rk), pdot_acc(q4, rsum(rq), pdot_acc(q4, k4[t], f32x2c{0.f, 0.f})));
            const float s = quad_sum(d2.x + d2.y);
            lg[t] = (t < nvalid && !(w[t] >> 31)) ? s : -INFINITY;
            mx = fmaxf(mx, lg[t]);
            rq = rq1;
            rk = rk1;
            __builtin_amdgcn_sched_barrier(0);  // at most two passes' table rows in flight (register budget)
        }
        mx = slots_max16(mx);
        if (single) {
            float sum = 0.f;
#pragma unroll
            for (int t = 0; t < NPA; t++) {
                lg[t] = __expf(lg[t] - mx);  // exp(-inf) = 0: flagged entries and slots past the end
                sum += lg[t];
            }
            const float inv = 1.0f / slots_sum16(sum);
#pragma unroll
            for (int t = 0; t < NPA; t++) lg_pv[t] = lg[t] * inv;
        } else {
            float *st = ml + ((size_t)i * x.h + x.head) * 2;
            const float m_old = ch ? st[0] : -INFINITY, l_old = ch ? st[1] : 0.f;
            const float m_new = fmaxf(m_old, mx);
            float sum = 0.f;
#pragma unroll
            for (int t = 0; t < NPA; t++) sum += __expf(lg[t] - m_new);
            if (c == 0) bstore_floats<NPA>(rs_p, roff, lg, nvalid);  // logits; the second sweep makes them weights
            sum = slots_sum16(sum);
            if (x.lane == 0) {
                st[0] = m_new;
                st[1] = (m_old == -INFINITY ? 0.f : l_old * __expf(m_old - m_new)) + sum;
            }
        }
    }
    if (single && ct.nq > 0 && c == 0) bstore_floats<NPA>(rs_p, ((ct.nq - 1) * ct.nk + j0 + p * NPA) * 4, lg_pv, nvalid);
}

template <int NPA, int TS, typename RT, typename T, bool PK>
__device__ __forceinline__ void fwd_sweep_values(const LaneCtx<T, PK> &x, const CellTask &ct, const CellBufs &cb, rsrc_t rs_p,
                                                 const RT *__restrict__ v, const float *__restrict__ ml, float *__restrict__ out,
                                                 int ch, bool single, int j0, int nkc) {
    const int p = x.p, c = x.c;
    const int nvalid = min(max(nkc - p * NPA, 0), NPA);
    float4 v4[NPA];
    load_key_rows<NPA, RT, T, PK>(x, cb, v, j0, nvalid, v4);
    unsigned w_nx[NPA];
    float a_nx[NPA];
    bload_words<NPA>(cb.rel, (j0 + p * NPA) * 4, w_nx);
    bload_floats<NPA>(rs_p, (j0 + p * NPA) * 4, a_nx);
    int ids = (int)bload_u32(cb.qid, x.lane * 4);
    float4 tot_pv = make_float4(0.f, 0.f, 0.f, 0.f);  // the sums of query i_pv = il-1
    int i_pv = 0;
    auto store_out = [&](int i, float4 tot) {
        float *o = out + (size_t)i * x.C + x.hoff;
        stg4(o, ch ? add4(tot, ldg4(o)) : tot);
    };
#pragma unroll 1  // (and no peeling of query 0)
    for (int il = 0; il < ct.nq; il++) {
        wait_vmem();  // this query's operands
        if (il && (il & 63) == 0) ids = next_query_ids(cb.qid, (il + x.lane) * 4);
        const int i = __builtin_amdgcn_readlane(ids, il & 63);
        const int roff = (il * ct.nk + j0 + p * NPA) * 4;
        unsigned w[NPA];
        float a[NPA];
#pragma unroll
        for (int t = 0; t < NPA; t++) {
            w[t] = w_nx[t];
            a[t] = a_nx[t];
        }
        bload_words<NPA>(cb.rel, roff + ct.nk * 4, w_nx);
        bload_floats<NPA>(rs_p, roff + ct.nk * 4, a_nx);
        if (il && p == 0) store_out(i_pv, tot_pv);
        if (!single) {
            const float *st = ml + ((size_t)i * x.h + x.head) * 2;
            const float m = st[0], inv = 1.0f / st[1];
#pragma unroll
            for (int t = 0; t < NPA; t++) a[t] = __expf(a[t] - m) * inv;
            if (c == 0) bstore_floats<NPA>(rs_p, roff, a, nvalid);
        }
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        Rows3 rv = rows_at<2 * TS, T>(x.lds, row_off(w[0], x.L, c));
#pragma unroll
        for (int t = 0; t < NPA; t++) {
            Rows3 rv1 = rv;
            if (t + 1 < NPA) rv1 = rows_at<2 * TS, T>(x.lds, row_off(w[t + 1], x.L, c));
            const float at = t < nvalid ? a[t] : 0.f;  // (a flagged entry's weight is stored as 0)
            acc = pfma4(at, padd4(rsum(rv), v4[t]), acc);
            rv = rv1;
            __builtin_amdgcn_sched_barrier(0);
        }
        tot_pv = slots_sum16_4(acc);
        i_pv = i;
    }
    if (ct.nq > 0 && p == 0) store_out(i_pv, tot_pv);
}

template <int NP, int LCAP, typename RT, typename T, bool PK>
__global__ __launch_bounds__(CA_WAVES * 64) void cell_fwd_kernel(pointops2_cell_plan pl, int h, int L, const RT *__restrict__ q,
                                                                 const RT *__restrict__ k, const RT *__restrict__ v, int rs, float qscale,
                                                                 const T *__restrict__ table_q, const T *__restrict__ table_k,
                                                                 const T *__restrict__ table_v, float *__restrict__ out,
                                                                 float *__restrict__ ml, float *__restrict__ pbuf, size_t plane) {
    constexpr int TS = TabGeo<LCAP>::TS;
    extern __shared__ float lds_raw[];
    T *lds = reinterpret_cast<T *>(lds_raw);
    const LaneCtx<T, PK> x = make_lane_ctx<T, PK>(lds, h, L, rs, qscale);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    stage_tables<TS, T>(lds, table_q, table_k, table_v, L, h, x.head);
    const int nC = share_count(pl, pl.counts[0]);
    float *pb = pbuf + (size_t)x.head * plane;
    const int slots = gridDim.x * CA_WAVES, slot = blockIdx.x * CA_WAVES + wave;
    for (int round = 0; round * slots < nC; round++) {
        const int task = snake_task(round, slot, slots);
        if (task >= nC) continue;
        const CellTask ct = cell_task(pl, share_task(pl, task));
        const int nch = (ct.nk + 16 * NP - 1) / (16 * NP);
        const CellBufs cb = make_cell_bufs(pl, ct);
        const rsrc_t rs_p = tile_rsrc(pb, ct);
        for (int ch = 0; ch < nch; ch++) {  // sweep 1: logits and softmax
            const int j0 = ch * 16 * NP, nkc = min(16 * NP, ct.nk - j0);
            dispatch_passes<NP>((nkc + 15) >> 4, [&](auto tag) {
                fwd_sweep_logits<decltype(tag)::value, TS, RT, T, PK>(x, ct, cb, rs_p, q, k, ml, ch, nch == 1, j0, nkc);
            });
        }
        for (int ch = 0; ch < nch; ch++) {  // sweep 2: out = sum p (v + Tv)
            const int j0 = ch * 16 * NP, nkc = min(16 * NP, ct.nk - j0);
            dispatch_passes<NP>((nkc + 15) >> 4, [&](auto tag) {
                fwd_sweep_values<decltype(tag)::value, TS, RT, T, PK>(x, ct, cb, rs_p, v, ml, out, ch, nch == 1, j0, nkc);
            });
        }
    }
}

// ------------------------------------------------------------------------------------------------
// backward, sweeps A and B
// ------------------------------------------------------------------------------------------------
// adds the key-side accumulators of a chunk (lane (p, c): floats 4c..4c+3 of the keys j0 + p * NPA + t, t < NPA) to grad[key, head, :],
// pass by pass through a wave-private LDS tile, so that one atomic instruction covers four whole 64-byte head rows.  The key ids of all
// 4 * NPA atomics (slot s = (lane >> 4) + 4 kk of pass t: key j0 + s * NPA + t - the NPA keys of a slot are consecutive dwords) are
// requested together before the first pass: an id loaded where it is used costs a memory round trip per atomic, and from the second
// one on that wait also covers the atomic before it.
// DET (the deterministic launchers, cell_det.hip): no atomics and no key ids.  `grad` is a partial buffer [K, h, 16] and a lane stores
// its own four floats of key slot kb + j0 + p * NPA + t (kb: the cell's first key slot): the four lanes of a slot write one 64-byte
// row.  Every slot of every cell is written exactly once; cell_key_grads_reduce sums a point's slots in a fixed order.
template <int NPA, typename T, bool PK, bool DET>
__device__ __forceinline__ void flush_key_grads(float *scr, const float4 (&acc)[NPA], rsrc_t rs_key, int kb, int j0, int nkc, float *__restrict__ grad,
                                                const LaneCtx<T, PK> &x) {
    if constexpr (DET) {
        float *row = grad + (size_t)(kb + j0 + x.p * NPA) * x.C + x.hoff;
#pragma unroll
        for (int t = 0; t < NPA; t++)
            if (x.p * NPA + t < nkc) stg4(row + (size_t)t * x.C, acc[t]);
        return;
    }
    unsigned keys[4][NPA];
#pragma unroll
    for (int kk = 0; kk < 4; kk++) bload_words<NPA>(rs_key, (j0 + ((x.lane >> 4) + 4 * kk) * NPA) * 4, keys[kk]);  // (past the end: key 0, unused)
    wait_vmem();  // once, here: a wait placed by the compiler behind the first (conditional) atomic would count that atomic too
#pragma unroll
    for (int t = 0; t < NPA; t++) {
        *reinterpret_cast<float4 *>(scr + x.p * 16 + 4 * x.c) = acc[t];
        __builtin_amdgcn_s_waitcnt(0xC07F);
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int kk = 0; kk < 4; kk++) {
            const int s = (x.lane >> 4) + 4 * kk;
            if (s * NPA + t < nkc) unsafeAtomicAdd(grad + (size_t)keys[kk][t] * x.rs() + x.head * 16 + (x.lane & 15), scr[s * 16 + (x.lane & 15)]);
        }
        __builtin_amdgcn_s_waitcnt(0xC07F);
        __builtin_amdgcn_wave_barrier();
    }
}

// sweep A: grad_attn = <go, v + Tv>, gs = p (grad_attn - <go, out>) stored, dV += p go
template <int NPA, int TS, typename RT, typename T, bool PK, bool DET>
__device__ __forceinline__ void bwd_sweep_values(const LaneCtx<T, PK> &x, const CellTask &ct, const CellBufs &cb, rsrc_t rs_p, rsrc_t rs_g,
                                                 float *scr, const float *__restrict__ go, const float *__restrict__ out,
                                                 const RT *__restrict__ v, float *__restrict__ grad_v, int j0, int nkc) {
    const int p = x.p, c = x.c;
    const int nvalid = min(max(nkc - p * NPA, 0), NPA);
    float4 v4[NPA], dv4[NPA];
    load_key_rows<NPA, RT, T, PK>(x, cb, v, j0, nvalid, v4);
#pragma unroll
    for (int t = 0; t < NPA; t++) dv4[t] = make_float4(0.f, 0.f, 0.f, 0.f);
    unsigned w_nx[NPA];
    float a_nx[NPA];
    bload_words<NPA>(cb.rel, (j0 + p * NPA) * 4, w_nx);
    bload_floats<NPA>(rs_p, (j0 + p * NPA) * 4, a_nx);
    int ids = (int)bload_u32(cb.qid, x.lane * 4);
    int i_nx = __builtin_amdgcn_readlane(ids, 0);
    float4 go_nx = ldg4(go + (size_t)i_nx * x.C + x.hoff), o_nx = ldg4(out + (size_t)i_nx * x.C + x.hoff);
    float gs_pv[NPA];  // the logit gradients of query il-1
#pragma unroll
    for (int t = 0; t < NPA; t++) gs_pv[t] = 0.f;
#pragma unroll 1  // (and no peeling of query 0)
    for (int il = 0; il < ct.nq; il++) {
        wait_vmem();  // this query's operands
        const int roff = (il * ct.nk + j0 + p * NPA) * 4;
        const float4 go4 = go_nx, o4 = o_nx;
        unsigned w[NPA];
        float a[NPA];
#pragma unroll
        for (int t = 0; t < NPA; t++) {
            w[t] = w_nx[t];
            a[t] = t < nvalid ? a_nx[t] : 0.f;
        }
        if (((il + 1) & 63) == 0) ids = next_query_ids(cb.qid, (il + 1 + x.lane) * 4);
        i_nx = __builtin_amdgcn_readlane(ids, (il + 1) & 63);
        go_nx = ldg4(go + (size_t)i_nx * x.C + x.hoff);
        o_nx = ldg4(out + (size_t)i_nx * x.C + x.hoff);
        bload_words<NPA>(cb.rel, roff + ct.nk * 4, w_nx);
        bload_floats<NPA>(rs_p, roff + ct.nk * 4, a_nx);
        if (il && c == 0) bstore_floats<NPA>(rs_g, roff - ct.nk * 4, gs_pv, nvalid);
        const float delta = quad_sum(pdot4(go4, o4));  // = sum over the row of p * grad_attn
        Rows3 rv = rows_at<2 * TS, T>(x.lds, row_off(w[0], x.L, c));
#pragma unroll
        for (int t = 0; t < NPA; t++) {
            Rows3 rv1 = rv;
            if (t + 1 < NPA) rv1 = rows_at<2 * TS, T>(x.lds, row_off(w[t + 1], x.L, c));
            const float ga = quad_sum(pdot4(go4, padd4(rsum(rv), v4[t])));
            gs_pv[t] = a[t] * (ga - delta);
            dv4[t] = pfma4(a[t], go4, dv4[t]);
            rv = rv1;
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    if (ct.nq > 0 && c == 0) bstore_floats<NPA>(rs_g, ((ct.nq - 1) * ct.nk + j0 + p * NPA) * 4, gs_pv, nvalid);
    flush_key_grads<NPA, T, PK, DET>(scr, dv4, cb.key, ct.kb, j0, nkc, grad_v, x);
}

// sweep B: dQ = sum gs (k + Tq), dK += gs (q + Tk)
template <int NPA, int TS, typename RT, typename T, bool PK, bool DET>
__device__ __forceinline__ void bwd_sweep_keys(const LaneCtx<T, PK> &x, const CellTask &ct, const CellBufs &cb, rsrc_t rs_g, float *scr,
                                               const RT *__restrict__ q, const RT *__restrict__ k, float *__restrict__ grad_q,
                                               float *__restrict__ grad_k, int ch, int j0, int nkc) {
    const int p = x.p, c = x.c;
    const int nvalid = min(max(nkc - p * NPA, 0), NPA);
    float4 k4[NPA], dk4[NPA];
    load_key_rows<NPA, RT, T, PK>(x, cb, k, j0, nvalid, k4);
#pragma unroll
    for (int t = 0; t < NPA; t++) dk4[t] = make_float4(0.f, 0.f, 0.f, 0.f);
    unsigned w_nx[NPA];
    float g_nx[NPA];
    bload_words<NPA>(cb.rel, (j0 + p * NPA) * 4, w_nx);
    bload_floats<NPA>(rs_g, (j0 + p * NPA) * 4, g_nx);
    int ids = (int)bload_u32(cb.qid, x.lane * 4);
    int i_nx = __builtin_amdgcn_readlane(ids, 0);
    float4 q_nx = x.q_row4(q, i_nx);
    float4 tot_pv = make_float4(0.f, 0.f, 0.f, 0.f);  // dQ of query i_pv = il-1
    int i_pv = 0;
    auto store_dq = [&](int i, float4 tot) {
        float *o = grad_q + (size_t)i * x.rs() + x.hoff;
        stg4(o, ch ? add4(tot, ldg4(o)) : tot);
    };
#pragma unroll 1  // (and no peeling of query 0)
    for (int il = 0; il < ct.nq; il++) {
        wait_vmem();  // this query's operands
        const int i = i_nx;
        const int roff = (il * ct.nk + j0 + p * NPA) * 4;
        const float4 q4 = q_nx;
        unsigned w[NPA];
        float g[NPA];
#pragma unroll
        for (int t = 0; t < NPA; t++) {
            w[t] = w_nx[t];
            g[t] = t < nvalid ? g_nx[t] : 0.f;
        }
        if (((il + 1) & 63) == 0) ids = next_query_ids(cb.qid, (il + 1 + x.lane) * 4);
        i_nx = __builtin_amdgcn_readlane(ids, (il + 1) & 63);
        q_nx = x.q_row4(q, i_nx);
        bload_words<NPA>(cb.rel, roff + ct.nk * 4, w_nx);
        bload_floats<NPA>(rs_g, roff + ct.nk * 4, g_nx);
        if (il && p == 0) store_dq(i_pv, tot_pv);
        float4 dq = make_float4(0.f, 0.f, 0.f, 0.f);
        RowOff ro = row_off(w[0], x.L, c);
        Rows3 rq = rows_at<0, T>(x.lds, ro), rk = rows_at<TS, T>(x.lds, ro);
#pragma unroll
        for (int t = 0; t < NPA; t++) {
            Rows3 rq1 = rq, rk1 = rk;
            if (t + 1 < NPA) {
                ro = row_off(w[t + 1], x.L, c);
                rq1 = rows_at<0, T>(x.lds, ro);
                rk1 = rows_at<TS, T>(x.lds, ro);
            }
            dq = pfma4(g[t], padd4(rsum(rq), k4[t]), dq);
            dk4[t] = pfma4(g[t], padd4(rsum(rk), q4), dk4[t]);
            rq = rq1;
            rk = rk1;
            __builtin_amdgcn_sched_barrier(0);
        }
        float4 tot = slots_sum16_4(dq);
        if constexpr (PK) tot = make_float4(tot.x * x.qscale, tot.y * x.qscale, tot.z * x.qscale, tot.w * x.qscale);  // dL/dq = scale * dL/dq'
        tot_pv = tot;
        i_pv = i;
    }
    if (ct.nq > 0 && p == 0) store_dq(i_pv, tot_pv);
    flush_key_grads<NPA, T, PK, DET>(scr, dk4, cb.key, ct.kb, j0, nkc, grad_k, x);
}

// DET: grad_k / grad_v are the partial buffers [K, h, 16] of flush_key_grads (plain stores), not the gradients
template <int NP, int LCAP, typename RT, typename T, bool PK, bool DET = false>
__global__ __launch_bounds__(CA_WAVES_BWD * 64) void cell_bwd_kernel(pointops2_cell_plan pl, int h, int L, const float *__restrict__ go,
                                                                 const RT *__restrict__ q, const RT *__restrict__ k,
                                                                 const RT *__restrict__ v, int rs, float qscale, const float *__restrict__ out,
                                                                 const T *__restrict__ table_q, const T *__restrict__ table_k,
                                                                 const T *__restrict__ table_v, const float *__restrict__ pbuf,
                                                                 float *__restrict__ gsbuf, size_t plane, float *__restrict__ grad_q,
                                                                 float *__restrict__ grad_k, float *__restrict__ grad_v) {
    constexpr int TS = TabGeo<LCAP>::TS;
    extern __shared__ float lds_raw[];
    T *lds = reinterpret_cast<T *>(lds_raw);
    const LaneCtx<T, PK> x = make_lane_ctx<T, PK>(lds, h, L, rs, qscale);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float *scr = reinterpret_cast<float *>(lds + 3 * TS) + wave * 256;
    stage_tables<TS, T>(lds, table_q, table_k, table_v, L, h, x.head);
    const int nC = share_count(pl, pl.counts[0]);
    const float *pb = pbuf + (size_t)x.head * plane;
    float *gb = gsbuf + (size_t)x.head * plane;
    const int slots = gridDim.x * CA_WAVES_BWD, slot = blockIdx.x * CA_WAVES_BWD + wave;
    for (int round = 0; round * slots < nC; round++) {
        const int task = snake_task(round, slot, slots);
        if (task >= nC) continue;
        const CellTask ct = cell_task(pl, share_task(pl, task));
        const int nch = (ct.nk + 16 * NP - 1) / (16 * NP);
        const CellBufs cb = make_cell_bufs(pl, ct);
        const rsrc_t rs_p = tile_rsrc(pb, ct), rs_g = tile_rsrc(gb, ct);
        for (int ch = 0; ch < nch; ch++) {
            const int j0 = ch * 16 * NP, nkc = min(16 * NP, ct.nk - j0);
            dispatch_passes<NP>((nkc + 15) >> 4, [&](auto tag) {
                bwd_sweep_values<decltype(tag)::value, TS, RT, T, PK, DET>(x, ct, cb, rs_p, rs_g, scr, go, out, v, grad_v, j0, nkc);
            });
        }
        for (int ch = 0; ch < nch; ch++) {
            const int j0 = ch * 16 * NP, nkc = min(16 * NP, ct.nk - j0);
            dispatch_passes<NP>((nkc + 15) >> 4, [&](auto tag) {
                bwd_sweep_keys<decltype(tag)::value, TS, RT, T, PK, DET>(x, ct, cb, rs_g, scr, q, k, grad_q, grad_k, ch, j0, nkc);
            });
        }
    }
}

// ------------------------------------------------------------------------------------------------
// table gradients on cell tiles.  grad_table[r, head, i, ax] += sum over tile entries with rel[ax] == r of w * X[row point, head, i]
//   BYKEY = false: a row = a query (its row of the tile), X = q (w = logit gradients) or grad_out (w = softmax weights)
//   BYKEY = true:  a row = a key   (its column of the tile), X = k (w = logit gradients)
// The sum is factored per row as in rpe_bwd_mfma.hip: a 3 x L histogram of the row's weights by rel index (32-bit fixed
// point: LDS integer atomics run at LDS write speed, float ones at ~1 lane per 3 cycles), times the row's X vector - an
// outer product, taken on the matrix cores four rows at a time: D[bin, i] += A[bin, row] * B[row, i] is one
// v_mfma_f32_16x16x4_f32 per 16-bin tile and axis.  Here a wave works alone: it takes FOUR ADJACENT ROWS of a cell at
// once (lane (p, c): entry p of a pass, row c of the four - for keys the four columns are 16 contiguous bytes per query),
// keeps the whole table slice of its head in accumulators (TA x 3 tiles) and meets the other waves of its workgroup only
// at the end, when the accumulators are summed through LDS and leave as contiguous atomics.  No row claims, no
// barriers, no descriptor chains in the loop: a cell's rows share one set of scalars.
// ------------------------------------------------------------------------------------------------
struct CFixScale {
    float mul, inv;
};
__device__ __forceinline__ CFixScale c_row_scale(unsigned maxbits, int n) {
    CFixScale sc;
    if (maxbits >= 0x7f800000u) {  // Inf / NaN among the weights
        sc.mul = 0.f;
        sc.inv = __uint_as_float(0x7fc00000u);
        return sc;
    }
    const int E = (int)(maxbits >> 23) - 126;  // max|w| < 2^E
    const int bits_n = 32 - __clz(max(n, 1));  // n < 2^bits_n
    const int S = max(-126, min(126, 30 - bits_n - E));
    sc.mul = __uint_as_float((unsigned)(S + 127) << 23);
    sc.inv = __uint_as_float((unsigned)(127 - S) << 23);
    return sc;
}

constexpr int CT_WAVES = 8;  // (12 in round 2; with the grid below 8 measured 5 % less backward time per step: tools/bench_cell.py, round 3)

template <int TA>
struct CellTableGeo {
    static constexpr int LP = TA * 16;       // padded bins per axis
    static constexpr int ROW = 3 * LP + 16;  // ints per histogram row (+16: the four rows of one read on different banks)
    static constexpr size_t walk_bytes() { return (size_t)CT_WAVES * 4 * ROW * 4; }
    static constexpr size_t sum_bytes() { return (size_t)LP * 48 * 4; }
    static constexpr size_t lds_bytes() { return walk_bytes() > sum_bytes() ? walk_bytes() : sum_bytes(); }
};

// X: rows of XT, xs elements apart; SC: taken times xscale as the forward took q (round_rows)
// DET (the deterministic launchers): grad_table is this body's partial buffer [gridDim.x, h, L * 48]; the workgroup stores its whole sum
// image there, zeros included (a workgroup without work stores zeros), and cell_table_grads_reduce adds the rows in ascending order.
template <int TA, bool BYKEY, bool SC, typename XT, bool DET = false>
__device__ __forceinline__ void cell_table_grad_body(const pointops2_cell_plan &pl, int h, int L, const float *__restrict__ wbuf, size_t plane,
                                                     const XT *__restrict__ X, int xs, float xscale, float *__restrict__ grad_table) {
    constexpr int D = 16;
    constexpr int MAXP = BYKEY ? 4 : 8;  // passes of 16 entries per row a segment holds in registers (a key's column is short)
    using G = CellTableGeo<TA>;
    extern __shared__ float lds[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int head = blockIdx.y;
    const int p = lane >> 2, c = lane & 3;     // entry of a pass, row of the four
    const int kq = lane >> 4, col = lane & 15;  // MFMA operand coordinates: row of the four, bin / feature
    int *hist = reinterpret_cast<int *>(lds) + wave * 4 * G::ROW;  // [4][ROW], private to the wave
    const float *wb = wbuf + (size_t)head * plane;

    f32x4c acc[TA][3];
#pragma unroll
    for (int bt = 0; bt < TA; bt++)
#pragma unroll
        for (int ax = 0; ax < 3; ax++) acc[bt][ax] = f32x4c{0.f, 0.f, 0.f, 0.f};
    for (int x = lane; x < 4 * G::ROW; x += 64) hist[x] = 0;

    // rows = queries: a task is a cell (piece), largest first; rows = keys: a task is a parent (all pieces of an uncut cell:
    // one [sum n_q, n_k] tile), so that a key's column is as long as the cut allows
    // (a share of the cells - one scene over several ranks - applies to the query side; the key side walks every parent, and the
    //  caller zero-fills the weight planes so that the pieces of other ranks contribute nothing)
    const int nC = BYKEY ? pl.counts[4] : share_count(pl, pl.counts[0]);
    const int slots = gridDim.x * CT_WAVES, slot = blockIdx.x * CT_WAVES + wave;
    for (int round = 0; round * slots < nC; round++) {
        const int task = snake_task(round, slot, slots);
        if (task >= nC) continue;
        CellTask ct;
        if (BYKEY) {
            const int c0 = __builtin_amdgcn_readfirstlane(pl.parent_first[task]), c1 = __builtin_amdgcn_readfirstlane(pl.parent_first[task + 1]);
            ct.qs = __builtin_amdgcn_readfirstlane(pl.cell_qstart[c0]);
            ct.nq = __builtin_amdgcn_readfirstlane(pl.cell_qstart[c1]) - ct.qs;
            ct.kb = __builtin_amdgcn_readfirstlane(pl.cell_kbase[c0]);
            ct.nk = __builtin_amdgcn_readfirstlane(pl.cell_kbase[c0 + 1]) - ct.kb;
            ct.pbase = __builtin_amdgcn_readfirstlane(pl.cell_pbase[c0]);
        } else {
            ct = cell_task(pl, share_task(pl, task));
        }
        const CellBufs cb = make_cell_bufs(pl, ct);
        const rsrc_t rs_rel = cb.rel, rs_w = tile_rsrc(wb, ct), rs_row = BYKEY ? cb.key : cb.qid;
        const int nrows = BYKEY ? ct.nk : ct.nq, nent = BYKEY ? ct.nq : ct.nk;
        // entry e of row r0 + c: rows = keys: tile[e][r0 + c];  rows = queries: tile[r0 + c][e]
        auto entry_off = [&](int r0, int ent) -> int { return (BYKEY ? ent * ct.nk + r0 + c : (r0 + c) * ct.nk + ent) * 4; };
        // one segment (<= 16 * MAXP entries per row) of the four rows r0..r0+3: histograms, then the outer products
        auto consume = [&](int r0, int e0, float xv, unsigned (&wr)[MAXP], float (&wt)[MAXP]) {
            const int ne = min(nent - e0, 16 * MAXP);
            const bool row_ok = r0 + c < nrows;
            unsigned mxb = 0u;
#pragma unroll
            for (int t = 0; t < MAXP; t++) {
                const bool live = row_ok && e0 + 16 * t + p < nent && !(wr[t] >> 31);
                wt[t] = live ? wt[t] : 0.f;
                mxb = max(mxb, __float_as_uint(fabsf(wt[t])));
            }
            const CFixScale sc = c_row_scale(wave_max_u32(mxb), ne);
            int *myh = hist + c * G::ROW;
#pragma unroll
            for (int t = 0; t < MAXP; t++) {
                if (16 * t < ne && wt[t] != 0.f) {
                    const int v = __float2int_rn(wt[t] * sc.mul);
                    atomicAdd(&myh[wr[t] & 255u], v);
                    atomicAdd(&myh[G::LP + ((wr[t] >> 8) & 255u)], v);
                    atomicAdd(&myh[2 * G::LP + ((wr[t] >> 16) & 255u)], v);
                }
            }
            __builtin_amdgcn_s_waitcnt(0xC07F);
            __builtin_amdgcn_wave_barrier();
            const float b = xv * sc.inv;
#pragma unroll
            for (int bt = 0; bt < TA; bt++)
#pragma unroll
                for (int ax = 0; ax < 3; ax++) {
                    // read the bin and clear it for the next segment in one LDS operation
                    const float a = (float)__hip_atomic_exchange(&hist[kq * G::ROW + ax * G::LP + bt * 16 + col], 0, __ATOMIC_RELAXED,
                                                                 __HIP_MEMORY_SCOPE_WORKGROUP);
                    acc[bt][ax] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[bt][ax], 0, 0, 0);
                }
            __builtin_amdgcn_s_waitcnt(0xC07F);
            __builtin_amdgcn_wave_barrier();
        };
        // Software pipeline over the cell's row quads: while quad q is consumed, the first segment and the X rows of quad
        // q+1 and the row ids of quad q+2 are in flight (an id, the X row it addresses and the tile entries would otherwise
        // be two dependent memory round trips per quad).  Reads past the end of a buffer return 0 and are never used.
        unsigned wr_n[MAXP];
        float wt_n[MAXP];
#pragma unroll
        for (int t = 0; t < MAXP; t++) {
            wr_n[t] = 0x80000000u;
            wt_n[t] = 0.f;
            if (16 * t < nent) {  // wave-uniform
                wr_n[t] = bload_u32(rs_rel, entry_off(0, 16 * t + p));
                wt_n[t] = bload_f32(rs_w, entry_off(0, 16 * t + p));
            }
        }
        int pt_n = (int)bload_u32(rs_row, kq * 4);
        float xv_n = SC ? scaled_elem<XT>(X + (size_t)pt_n * xs + head * D + col, xscale) : ld_elem(X + (size_t)pt_n * xs + head * D + col);  // B operand: X[point of row r0 + kq, head, col]
        pt_n = (int)bload_u32(rs_row, (4 + kq) * 4);
        for (int r0 = 0; r0 < nrows; r0 += 4) {
            unsigned wr[MAXP];
            float wt[MAXP];
#pragma unroll
            for (int t = 0; t < MAXP; t++) {
                wr[t] = wr_n[t];
                wt[t] = wt_n[t];
            }
            const float xv = r0 + kq < nrows ? xv_n : 0.f;
            xv_n = SC ? scaled_elem<XT>(X + (size_t)pt_n * xs + head * D + col, xscale) : ld_elem(X + (size_t)pt_n * xs + head * D + col);
            pt_n = (int)bload_u32(rs_row, (r0 + 8 + kq) * 4);
#pragma unroll
            for (int t = 0; t < MAXP; t++)
                if (16 * t < nent) {
                    wr_n[t] = bload_u32(rs_rel, entry_off(r0 + 4, 16 * t + p));
                    wt_n[t] = bload_f32(rs_w, entry_off(r0 + 4, 16 * t + p));
                }
            consume(r0, 0, xv, wr, wt);
            for (int e0 = 16 * MAXP; e0 < nent; e0 += 16 * MAXP) {  // rows longer than one segment (rare)
#pragma unroll
                for (int t = 0; t < MAXP; t++) {
                    wr[t] = bload_u32(rs_rel, entry_off(r0, e0 + 16 * t + p));
                    wt[t] = bload_f32(rs_w, entry_off(r0, e0 + 16 * t + p));
                }
                consume(r0, e0, xv, wr, wt);
            }
        }
    }
    // Sum over the workgroup's waves through one LDS image in table order ([bin][16][3]: the 48 floats of a (bin, head) are
    // contiguous in the [L, h, 16, 3] table), then contiguous atomics.  C/D layout of 16x16x4: lane holds
    // D[row = (lane >> 4) * 4 + reg][col = lane & 15]  (row = bin, col = feature).
    __syncthreads();  // every wave is done with its histograms
    float *sum = lds;
    for (int w = 0; w < CT_WAVES; w++) {
        if (wave == w) {
#pragma unroll
            for (int bt = 0; bt < TA; bt++)
#pragma unroll
                for (int ax = 0; ax < 3; ax++)
#pragma unroll
                    for (int reg = 0; reg < 4; reg++) {
                        float *d = &sum[((bt * 16 + kq * 4 + reg) * 16 + col) * 3 + ax];
                        *d = w ? *d + acc[bt][ax][reg] : acc[bt][ax][reg];
                    }
        }
        __syncthreads();
    }
    if constexpr (DET) {
        float *dst = grad_table + ((size_t)blockIdx.x * h + head) * (size_t)(L * 48);
        for (int x = threadIdx.x; x < L * 48; x += CT_WAVES * 64) dst[x] = sum[x];
    } else {
        for (int x = threadIdx.x; x < L * 48; x += CT_WAVES * 64) {
            const float val = sum[x];
            if (val != 0.f) unsafeAtomicAdd(grad_table + ((size_t)(x / 48) * h + head) * 48 + x % 48, val);
        }
    }
}

// the three table gradients of a block as ONE grid (blockIdx.z: 0 = key side, the longest, first in dispatch order; 1 = query side;
// 2 = value side): each of them alone is short of independent work on the small stages, together they overlap
template <int TA, typename T, bool PK, bool DET = false>
__global__ __launch_bounds__(CT_WAVES * 64) void cell_table_grad3_kernel(pointops2_cell_plan pl, int h, int L, const float *__restrict__ gsbuf,
                                                                         const float *__restrict__ pbuf, size_t plane,
                                                                         const T *__restrict__ q, const T *__restrict__ k,
                                                                         const float *__restrict__ grad_out, float *__restrict__ gtq,
                                                                         float *__restrict__ gtk, float *__restrict__ gtv, int rs, float qscale) {
    const int xs = PK ? rs : h * 16;
    if (blockIdx.z == 0) cell_table_grad_body<TA, true, false, T, DET>(pl, h, L, gsbuf, plane, k, xs, 1.0f, gtk);
    else if (blockIdx.z == 1) cell_table_grad_body<TA, false, PK, T, DET>(pl, h, L, gsbuf, plane, q, xs, qscale, gtq);
    else cell_table_grad_body<TA, false, false, float, DET>(pl, h, L, pbuf, plane, grad_out, h * 16, 1.0f, gtv);
}

// What a launch refuses before anything else (nullptr: nothing), forward and backward in one place.  The texts are literals because
// the library keeps the pointer (set_error); the backward names itself in them and states its range of L first.
static const char *cell_refusal(const pointops2_cell_plan *plan, int hdim, int L, bool backward) {
    if (hdim != 16) return "cell_attention: d != 16";
    if (backward && (L < 1 || L > 80)) return "cell_attention backward: table rows L must be in 1..80";
    if (L < 1) return "cell_attention: no table rows";
    // relp's indices were clamped to [0, plan->table_rows) and L is the axis stride of the LDS table image
    if (L != plan->table_rows)
        return backward ? "cell_attention backward: the tables' row count differs from the plan's table_rows"
                        : "cell_attention: the tables' row count differs from the plan's table_rows";
    if (L > 160) return "cell_attention: more than 160 table rows (use the operators)";
    return nullptr;
}

// The forward kernel a launch runs (codes of pointops2_cell_forward_variant): launch_cell_fwd takes its decision from here alone,
// so the table the tests pin is the one that runs.  *why = the error a refusal records (NULL otherwise).
static int cell_fwd_variant(const pointops2_cell_plan *plan, int h, int hdim, int L, bool bf16, const char **why) {
    *why = nullptr;
    if (plan == nullptr || plan->n_points <= 0) return POINTOPS2_CELL_FWD_NONE;
    if ((*why = cell_refusal(plan, hdim, L, false)) != nullptr) return POINTOPS2_CELL_FWD_ERROR;
    if (L > 80) return POINTOPS2_CELL_FWD_VALU160;
    if (!bf16) {
        // The matrix-core forward (cell_attn_mfma.hip) where it was measured faster than the VALU walkers (tools/bench_cell.py, MI355X,
        // the four stages of the S3DIS scene, even / odd pattern, us MFMA : VALU): 292:321 / 372:300, 163:193 / 190:180,
        // 114:152 / 117:120, 103:150 / 92:96.  The matrix-core tiles are 16 queries wide: the shifted pattern of the two large stages
        // cuts the cloud into many cells of ~9 queries (n_pairs / n_keyslots), whose tiles stay half empty.
        const double avg_queries = (double)plan->n_pairs / (double)(plan->n_keyslots > 0 ? plan->n_keyslots : 1);
        if (!((long long)plan->n_points * h >= 96000 && avg_queries < 15.0)) return L <= 64 ? POINTOPS2_CELL_FWD_MFMA64 : POINTOPS2_CELL_FWD_MFMA80;
    }
    return POINTOPS2_CELL_FWD_VALU80;
}

// the VALU forward with a table image of LCAP rows per axis
template <int LCAP, typename RT, typename TT, bool PK>
static void launch_valu_fwd(hipStream_t st, const pointops2_cell_plan *plan, int h, int L, const CellRows<RT> &r, const CellTables<TT> &t, float *out, float *ml,
                            float *pbuf) {
    const size_t lds = TabGeo<LCAP>::bytes(sizeof(TT));
    allow_big_lds(cell_fwd_kernel<CA_NP, LCAP, RT, TT, PK>, lds);
    const dim3 grid(cell_grid_x(1, plan->n_cells, h, CA_WAVES), h);
    hipLaunchKernelGGL((cell_fwd_kernel<CA_NP, LCAP, RT, TT, PK>), grid, dim3(CA_WAVES * 64), lds, st, *plan, h, L, r.q, r.k, r.v, r.rs, r.scale, t.q, t.k, t.v, out,
                       ml, pbuf, (size_t)plan->n_pairs);
}

// RT / TT: storage types of the rows and of the tables.  PK: the packed entry points (CellRows, cell_common.h)
template <typename RT, typename TT, bool PK>
static void launch_cell_fwd(hipStream_t st, const pointops2_cell_plan *plan, int h, int hdim, int L, const CellRows<RT> &r, const CellTables<TT> &t, float *out,
                            float *ml, float *pbuf) {
    const char *why;
    const int variant = cell_fwd_variant(plan, h, hdim, L, !std::is_same<TT, float>::value, &why);
    if (why != nullptr) { set_error(why); return; }
    if (variant == POINTOPS2_CELL_FWD_NONE) return;
    if constexpr (std::is_same<TT, float>::value) {
        if (variant == POINTOPS2_CELL_FWD_MFMA64 || variant == POINTOPS2_CELL_FWD_MFMA80) {
            cell_fwd_mfma_launch(st, variant, plan, h, L, RowTag<RT>::code, PK, CellRows<void>{r.q, r.k, r.v, r.rs, r.scale}, t, out, pbuf);
            check_launch();
            return;
        }
    }
    if (variant == POINTOPS2_CELL_FWD_VALU80) launch_valu_fwd<80, RT, TT, PK>(st, plan, h, L, r, t, out, ml, pbuf);
    else launch_valu_fwd<160, RT, TT, PK>(st, plan, h, L, r, t, out, ml, pbuf);  // POINTOPS2_CELL_FWD_VALU160
    check_launch();
}

// Rows of the table partials of a deterministic backward = grid.x of its table-gradient launch: one workgroup per CU of the device and
// body, over all heads.  NOT usable_cus(): that follows the sampler launches still pending when the backward is enqueued, a matter of
// host timing, and the grouping of the sums must not depend on it.
static int cell_table_partial_rows(const pointops2_cell_plan *plan, int h) {
    return max(1, min(max(1, num_cus() / max(h, 1)), div_up(plan->n_cells, CT_WAVES)));
}

// what a deterministic backward refuses on top of cell_refusal
static const char *cell_det_refusal(const pointops2_cell_plan *plan, int h, int L, const CellDet &det) {
    if (plan->task_step > 1 || plan->task_list != nullptr)
        return "cell_attention deterministic backward: the plan is a share of the cells (task_step > 1 or a task_list)";
    if (det.slot_offsets == nullptr || det.slot_order == nullptr || det.key_partials == nullptr || det.table_partials == nullptr)
        return "cell_attention deterministic backward: slot_offsets, slot_order, key_partials and table_partials must not be NULL";
    if (det.key_partial_floats < (size_t)2 * plan->n_keyslots * h * 16) return "cell_attention deterministic backward: key_partials holds fewer than 2 * K * h * 16 floats";
    if (det.table_partial_floats < (size_t)3 * cell_table_partial_rows(plan, h) * h * L * 48)
        return "cell_attention deterministic backward: table_partials holds fewer than 3 * pointops2_cell_table_partial_rows * h * L * 48 floats";
    return nullptr;
}

// The deterministic launchers: the DET instances of the sweeps and the table bodies store partial sums (det.key_partials: dK [K, h, 16] then dV;
// det.table_partials: [3 = q, k, v][rows][h][L * 48]) and two more launches (cell_det.hip) add them in a fixed order into g.k, g.v
// and gt, which are fully written.
template <typename RT, typename TT, bool PK>
static void launch_cell_bwd_det(hipStream_t st, const pointops2_cell_plan *plan, int h, int hdim, int L, const float *grad_out, const CellRows<RT> &r,
                                const float *out, const CellTables<TT> &t, const float *pbuf, float *gsbuf, const CellGrads &g, const CellGrads &gt,
                                const CellDet &det) {
    if (plan == nullptr || plan->n_points <= 0) return;
    if (const char *why = cell_refusal(plan, hdim, L, true)) { set_error(why); return; }
    if (const char *why = cell_det_refusal(plan, h, L, det)) { set_error(why); return; }
    const size_t lds = TabGeo<80>::bytes(sizeof(TT)) + (size_t)CA_WAVES_BWD * 256 * sizeof(float);
    allow_big_lds(cell_bwd_kernel<CA_NP_BWD, 80, RT, TT, PK, true>, lds);
    const size_t plane = (size_t)plan->n_pairs, kplane = (size_t)plan->n_keyslots * h * 16;
    float *dk = det.key_partials, *dv = det.key_partials + kplane;
    hipLaunchKernelGGL((cell_bwd_kernel<CA_NP_BWD, 80, RT, TT, PK, true>), dim3(cell_grid_x(1, plan->n_cells, h, CA_WAVES_BWD), h), dim3(CA_WAVES_BWD * 64), lds,
                       st, *plan, h, L, grad_out, r.q, r.k, r.v, r.rs, r.scale, out, t.q, t.k, t.v, pbuf, gsbuf, plane, g.q, dk, dv);
    const int rows = cell_table_partial_rows(plan, h);
    const size_t tplane = (size_t)rows * h * L * 48;
    float *tq = det.table_partials, *tk = tq + tplane, *tv = tk + tplane;
    const dim3 grid3(rows, h, 3), tblock(CT_WAVES * 64);
    if (L <= 64) hipLaunchKernelGGL((cell_table_grad3_kernel<4, RT, PK, true>), grid3, tblock, CellTableGeo<4>::lds_bytes(), st, *plan, h, L, gsbuf, pbuf, plane, r.q,
                                    r.k, grad_out, tq, tk, tv, r.rs, r.scale);
    else hipLaunchKernelGGL((cell_table_grad3_kernel<5, RT, PK, true>), grid3, tblock, CellTableGeo<5>::lds_bytes(), st, *plan, h, L, gsbuf, pbuf, plane, r.q, r.k,
                            grad_out, tq, tk, tv, r.rs, r.scale);
    cell_key_grads_reduce_launch(st, plan->n_points, h, det.slot_offsets, det.slot_order, dk, g.k, dv, g.v, PK ? r.rs : h * 16);
    cell_table_grads_reduce_launch(st, rows, h, L, det.table_partials, gt.q, gt.k, gt.v);
    check_launch();
}

template <typename RT, typename TT, bool PK>
static void launch_cell_bwd(hipStream_t st, const pointops2_cell_plan *plan, int h, int hdim, int L, const float *grad_out, const CellRows<RT> &r, const float *out,
                            const CellTables<TT> &t, const float *pbuf, float *gsbuf, const CellGrads &g, const CellGrads &gt) {
    if (plan == nullptr || plan->n_points <= 0) return;
    if (const char *why = cell_refusal(plan, hdim, L, true)) { set_error(why); return; }
    const size_t lds = TabGeo<80>::bytes(sizeof(TT)) + (size_t)CA_WAVES_BWD * 256 * sizeof(float);
    allow_big_lds(cell_bwd_kernel<CA_NP_BWD, 80, RT, TT, PK>, lds);
    const size_t plane = (size_t)plan->n_pairs;
    hipLaunchKernelGGL((cell_bwd_kernel<CA_NP_BWD, 80, RT, TT, PK>), dim3(cell_grid_x(1, plan->n_cells, h, CA_WAVES_BWD), h),
                       dim3(CA_WAVES_BWD * 64), lds, st, *plan, h, L, grad_out, r.q, r.k, r.v, r.rs, r.scale, out, t.q, t.k, t.v, pbuf, gsbuf, plane, g.q, g.k, g.v);
    // the three table gradients read p / gs only
    // Grid of the table-gradient bodies: ONE workgroup of 8 waves per free CU and body (round 2: two of 12).
    // Measured (tools/bench_cell.py, backward of a block, us, two -> one -> half): stage 0 784 -> 717 -> 725 / 905 -> 831 -> 833 (plain / shifted
    // pattern), stage 1 512 -> 448 -> 433 / 505 -> 452 -> 423, stage 2 381 -> 345 -> 304 / 361 -> 302 -> 292, stage 3 317 -> 301 -> 303 /
    // 265 -> 223 -> 212: every workgroup pays a fixed zero-fill, a 12-round reduction through LDS and a 3 072-float atomic flush per body, and
    // the bodies are latency-bound - more resident workgroups only add to both.  (Halving the grids of cell_fwd / cell_bwd the same way
    // costs 40-70 %: those are bound by resident waves.  With 12 waves per workgroup, halving the grid on the smaller stages paid; with 8
    // it does not.)  The three as ONE grid rather than three launches in a row: backward of a block 10-120 us shorter, most on the small
    // stages.
    const dim3 grid3(cell_grid_x(1, plan->n_cells, h, CT_WAVES), h, 3), tblock(CT_WAVES * 64);
    if (L <= 64) hipLaunchKernelGGL((cell_table_grad3_kernel<4, RT, PK>), grid3, tblock, CellTableGeo<4>::lds_bytes(), st, *plan, h, L, gsbuf, pbuf, plane, r.q, r.k,
                                    grad_out, gt.q, gt.k, gt.v, r.rs, r.scale);
    else hipLaunchKernelGGL((cell_table_grad3_kernel<5, RT, PK>), grid3, tblock, CellTableGeo<5>::lds_bytes(), st, *plan, h, L, gsbuf, pbuf, plane, r.q, r.k, grad_out,
                            gt.q, gt.k, gt.v, r.rs, r.scale);
    check_launch();
}

// the rows of a packed projection qkv [N, 3, h, 16] (gradients alike) where they lie
template <typename RT>
static CellRows<RT> packed_rows(const void *qkv, int h, float scale) {
    const RT *r = static_cast<const RT *>(qkv);
    return {r, r + h * 16, r + 2 * h * 16, 3 * h * 16, scale};
}

}  // namespace p2

using namespace p2;

extern "C" {

int pointops2_cell_forward_variant(const pointops2_cell_plan *plan, int h, int hdim, int L, int bf16) {
    const char *why;
    return cell_fwd_variant(plan, h, hdim, L, bf16 != 0, &why);
}

void cell_attention_forward_launcher(const pointops2_cell_plan *plan, int h, int hdim, int L, const float *q, const float *k,
                                     const float *v, const float *table_q, const float *table_k, const float *table_v, float *out,
                                     float *ml, float *pbuf) {
    launch_cell_fwd<float, float, false>(begin_launch().stream, plan, h, hdim, L, {q, k, v, h * 16, 1.0f}, {table_q, table_k, table_v}, out, ml, pbuf);
}
void cell_attention_backward_launcher(const pointops2_cell_plan *plan, int h, int hdim, int L, const float *grad_out, const float *q,
                                      const float *k, const float *v, const float *out, const float *table_q, const float *table_k,
                                      const float *table_v, const float *pbuf, float *gsbuf, float *grad_q, float *grad_k,
                                      float *grad_v, float *grad_table_q, float *grad_table_k, float *grad_table_v) {
    launch_cell_bwd<float, float, false>(begin_launch().stream, plan, h, hdim, L, grad_out, {q, k, v, h * 16, 1.0f}, out, {table_q, table_k, table_v}, pbuf, gsbuf,
                                         {grad_q, grad_k, grad_v}, {grad_table_q, grad_table_k, grad_table_v});
}
// bf16 storage of q / k / v / tables (raw 16-bit patterns), fp32 arithmetic, fp32 outputs and gradients
void cell_attention_forward_bf16_launcher(const pointops2_cell_plan *plan, int h, int hdim, int L, const uint16_t *q, const uint16_t *k,
                                          const uint16_t *v, const uint16_t *table_q, const uint16_t *table_k, const uint16_t *table_v,
                                          float *out, float *ml, float *pbuf) {
    launch_cell_fwd<bf16_t, bf16_t, false>(begin_launch().stream, plan, h, hdim, L, {q, k, v, h * 16, 1.0f}, {table_q, table_k, table_v}, out, ml, pbuf);
}
void cell_attention_backward_bf16_launcher(const pointops2_cell_plan *plan, int h, int hdim, int L, const float *grad_out, const uint16_t *q,
                                           const uint16_t *k, const uint16_t *v, const float *out, const uint16_t *table_q,
                                           const uint16_t *table_k, const uint16_t *table_v, const float *pbuf, float *gsbuf, float *grad_q,
                                           float *grad_k, float *grad_v, float *grad_table_q, float *grad_table_k, float *grad_table_v) {
    launch_cell_bwd<bf16_t, bf16_t, false>(begin_launch().stream, plan, h, hdim, L, grad_out, {q, k, v, h * 16, 1.0f}, out, {table_q, table_k, table_v}, pbuf, gsbuf,
                                           {grad_q, grad_k, grad_v}, {grad_table_q, grad_table_k, grad_table_v});
}

// The rows of the packed projection qkv [N, 3, h, 16] read in place (fp32, half or bf16: what the model's qkv Linear returns, under
// autocast too); fp32 tables, arithmetic, outputs and gradients.  q is scaled as it is loaded; grad_qkv receives scale * dL/dq'.
void cell_attention_qkv_forward_launcher(const pointops2_cell_plan *plan, int h, int hdim, int L, const void *qkv, int row_type, float scale,
                                         const float *table_q, const float *table_k, const float *table_v, float *out, float *ml, float *pbuf) {
    const hipStream_t st = begin_launch().stream;
    if (!with_row_type(row_type, [&](auto tag) {
        using RT = typename decltype(tag)::type;
        launch_cell_fwd<RT, float, true>(st, plan, h, hdim, L, packed_rows<RT>(qkv, h, scale), {table_q, table_k, table_v}, out, ml, pbuf);
    })) set_error("cell_attention_qkv: unknown row_type");
}
void cell_attention_qkv_backward_launcher(const pointops2_cell_plan *plan, int h, int hdim, int L, const float *grad_out, const void *qkv, int row_type,
                                          float scale, const float *out, const float *table_q, const float *table_k, const float *table_v,
                                          const float *pbuf, float *gsbuf, float *grad_qkv, float *grad_table_q, float *grad_table_k,
                                          float *grad_table_v) {
    const hipStream_t st = begin_launch().stream;
    if (!with_row_type(row_type, [&](auto tag) {
        using RT = typename decltype(tag)::type;
        launch_cell_bwd<RT, float, true>(st, plan, h, hdim, L, grad_out, packed_rows<RT>(qkv, h, scale), out, {table_q, table_k, table_v}, pbuf, gsbuf,
                                         {grad_qkv, grad_qkv + h * 16, grad_qkv + 2 * h * 16}, {grad_table_q, grad_table_k, grad_table_v});
    })) set_error("cell_attention_qkv backward: unknown row_type");
}

// The three backward launchers without float atomics (include/pointops2_hip.h, "deterministic backward")
int pointops2_cell_table_partial_rows(const pointops2_cell_plan *plan, int h) { return plan == nullptr ? 1 : cell_table_partial_rows(plan, h); }
void cell_attention_det_backward_launcher(const pointops2_cell_plan *plan, int h, int hdim, int L, const float *grad_out, const float *q, const float *k,
                                          const float *v, const float *out, const float *table_q, const float *table_k, const float *table_v,
                                          const float *pbuf, float *gsbuf, float *grad_q, float *grad_k, float *grad_v, float *grad_table_q,
                                          float *grad_table_k, float *grad_table_v, const int *slot_offsets, const int *slot_order, float *key_partials,
                                          size_t key_partial_floats, float *table_partials, size_t table_partial_floats) {
    launch_cell_bwd_det<float, float, false>(begin_launch().stream, plan, h, hdim, L, grad_out, {q, k, v, h * 16, 1.0f}, out, {table_q, table_k, table_v}, pbuf, gsbuf,
                                             {grad_q, grad_k, grad_v}, {grad_table_q, grad_table_k, grad_table_v},
                                             {slot_offsets, slot_order, key_partials, key_partial_floats, table_partials, table_partial_floats});
}
void cell_attention_det_backward_bf16_launcher(const pointops2_cell_plan *plan, int h, int hdim, int L, const float *grad_out, const uint16_t *q,
                                               const uint16_t *k, const uint16_t *v, const float *out, const uint16_t *table_q, const uint16_t *table_k,
                                               const uint16_t *table_v, const float *pbuf, float *gsbuf, float *grad_q, float *grad_k, float *grad_v,
                                               float *grad_table_q, float *grad_table_k, float *grad_table_v, const int *slot_offsets,
                                               const int *slot_order, float *key_partials, size_t key_partial_floats, float *table_partials,
                                               size_t table_partial_floats) {
    launch_cell_bwd_det<bf16_t, bf16_t, false>(begin_launch().stream, plan, h, hdim, L, grad_out, {q, k, v, h * 16, 1.0f}, out, {table_q, table_k, table_v}, pbuf,
                                               gsbuf, {grad_q, grad_k, grad_v}, {grad_table_q, grad_table_k, grad_table_v},
                                               {slot_offsets, slot_order, key_partials, key_partial_floats, table_partials, table_partial_floats});
}
void cell_attention_qkv_det_backward_launcher(const pointops2_cell_plan *plan, int h, int hdim, int L, const float *grad_out, const void *qkv, int row_type,
                                              float scale, const float *out, const float *table_q, const float *table_k, const float *table_v,
                                              const float *pbuf, float *gsbuf, float *grad_qkv, float *grad_table_q, float *grad_table_k,
                                              float *grad_table_v, const int *slot_offsets, const int *slot_order, float *key_partials,
                                              size_t key_partial_floats, float *table_partials, size_t table_partial_floats) {
    const hipStream_t st = begin_launch().stream;
    if (!with_row_type(row_type, [&](auto tag) {
        using RT = typename decltype(tag)::type;
        launch_cell_bwd_det<RT, float, true>(st, plan, h, hdim, L, grad_out, packed_rows<RT>(qkv, h, scale), out, {table_q, table_k, table_v}, pbuf, gsbuf,
                                             {grad_qkv, grad_qkv + h * 16, grad_qkv + 2 * h * 16}, {grad_table_q, grad_table_k, grad_table_v},
                                             {slot_offsets, slot_order, key_partials, key_partial_floats, table_partials, table_partial_floats});
    })) set_error("cell_attention_qkv deterministic backward: unknown row_type");
}

}  // extern "C"
