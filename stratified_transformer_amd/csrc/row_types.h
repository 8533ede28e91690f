// The three storage types of a row (POINTOPS2_ROWS_* of include/pointops2_hip.h): fp32, IEEE half and bf16.  The only place that knows
// how a 16-bit element becomes a float and back: every operator widens its operands exactly, computes in fp32 and rounds once, to
// nearest even.  Two vocabularies over the same primitives: the storage types float / f16_t / bf16_t for kernels instantiated per row
// type (cell attention, grouped max, the vote), and the POINTOPS2_ROWS_* code as a run-time argument for kernels that branch on it
// (rownorm, seg_loss, the vote's shift).
#pragma once
#include "common.h"

namespace p2 {

typedef unsigned short bf16_t;  // raw bits
struct f16_t {                  // IEEE half, raw bits (a type of its own: bf16_t is the other 16-bit pattern)
    unsigned short bits;
};
typedef _Float16 f16x2c __attribute__((ext_vector_type(2)));

// ---- 16 bits <-> fp32.  Half: the compiler's _Float16 casts.  bf16: widening is a shift, rounding is written out here ----
// the bits of an fp32 value -> its bf16 bits: nearest even, a NaN stays a NaN (quiet, its low 16 payload bits dropped)
constexpr unsigned bf16_round_bits(unsigned u) {
    return (u & 0x7fffffffu) > 0x7f800000u ? (u >> 16) | 0x40u : (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}
static_assert(bf16_round_bits(0x7f800001u) == 0x7fc0u, "a NaN stays a NaN");
static_assert(bf16_round_bits(0x3f808000u) == 0x3f80u && bf16_round_bits(0x3f818000u) == 0x3f82u, "ties go to even");
static_assert(bf16_round_bits(0x7f7f8000u) == 0x7f80u, "the largest finite value rounds to inf");
static_assert(bf16_round_bits(0x80000000u) == 0x8000u, "-0 stays -0");

template <typename RT>
__device__ __forceinline__ float widen_bits(unsigned v);  // v: the 16 bits of an element
template <>
__device__ __forceinline__ float widen_bits<f16_t>(unsigned v) { return (float)__builtin_bit_cast(_Float16, (unsigned short)v); }
template <>
__device__ __forceinline__ float widen_bits<bf16_t>(unsigned v) { return __uint_as_float(v << 16); }
template <typename RT>
__device__ __forceinline__ unsigned narrow_bits(float f);
template <>
__device__ __forceinline__ unsigned narrow_bits<f16_t>(float f) { return (unsigned)__builtin_bit_cast(unsigned short, (_Float16)f); }
template <>
__device__ __forceinline__ unsigned narrow_bits<bf16_t>(float f) { return bf16_round_bits(__float_as_uint(f)); }

// ---- by storage type ----
__device__ __forceinline__ float4 ld_row4(const float *p) { return *reinterpret_cast<const float4 *>(p); }
__device__ __forceinline__ float4 ld_row4(const bf16_t *p) {
    const uint2 u = *reinterpret_cast<const uint2 *>(p);  // four bf16: widening to fp32 is a shift
    return make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16), __uint_as_float(u.y & 0xffff0000u));
}
__device__ __forceinline__ float4 ld_row4(const f16_t *p) {
    const uint2 u = *reinterpret_cast<const uint2 *>(p);  // four halves, two per dword: v_cvt_f32_f16 of each half
    const f16x2c lo = __builtin_bit_cast(f16x2c, u.x), hi = __builtin_bit_cast(f16x2c, u.y);
    return make_float4((float)lo.x, (float)lo.y, (float)hi.x, (float)hi.y);
}
__device__ __forceinline__ float ld_elem(const float *p) { return *p; }
__device__ __forceinline__ float ld_elem(const bf16_t *p) { return widen_bits<bf16_t>(*p); }
__device__ __forceinline__ float ld_elem(const f16_t *p) { return widen_bits<f16_t>(p->bits); }
__device__ __forceinline__ void st_elem(float *p, float f) { *p = f; }
__device__ __forceinline__ void st_elem(bf16_t *p, float f) { *p = (bf16_t)narrow_bits<bf16_t>(f); }
__device__ __forceinline__ void st_elem(f16_t *p, float f) { p->bits = (unsigned short)narrow_bits<f16_t>(f); }
// f rounded to RT, as the float that a tensor of that type holds after f was stored into it
template <typename RT>
__device__ __forceinline__ float round_rows(float f) {
    if constexpr (std::is_same<RT, float>::value) return f;
    else return widen_bits<RT>(narrow_bits<RT>(f));
}
// (bf16: a NaN passes through with its low 16 payload bits, which no bf16 element could hold and nothing reads: the quiet bit is
// set in place, one instruction less than rounding the NaN, and the cell kernels' code is what it was before this header)
template <>
__device__ __forceinline__ float round_rows<bf16_t>(float f) {
    const unsigned u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return __uint_as_float(u | 0x00400000u);
    return __uint_as_float(bf16_round_bits(u) << 16);
}

template <typename RT>
struct RowTag {
    using type = RT;
    static constexpr int code = std::is_same<RT, float>::value ? POINTOPS2_ROWS_F32 : std::is_same<RT, f16_t>::value ? POINTOPS2_ROWS_F16 : POINTOPS2_ROWS_BF16;
};
// f(RowTag<RT>{}) for the storage type that `row_type` (POINTOPS2_ROWS_*) names; false: no such code, f was not called
template <typename F>
static bool with_row_type(int row_type, F f) {
    if (row_type == POINTOPS2_ROWS_F32) f(RowTag<float>{});
    else if (row_type == POINTOPS2_ROWS_F16) f(RowTag<f16_t>{});
    else if (row_type == POINTOPS2_ROWS_BF16) f(RowTag<bf16_t>{});
    else return false;
    return true;
}

// ---- by code, for the 16-bit types (fp32 is the caller's own branch: it has no bits to convert) ----
inline bool known_row_type(int code) { return code == POINTOPS2_ROWS_F32 || code == POINTOPS2_ROWS_F16 || code == POINTOPS2_ROWS_BF16; }
inline __host__ __device__ int row_elem_bytes(int rt) { return rt == POINTOPS2_ROWS_F32 ? 4 : 2; }
__device__ __forceinline__ float widen16(unsigned v, int rt) { return rt == POINTOPS2_ROWS_F16 ? widen_bits<f16_t>(v) : widen_bits<bf16_t>(v); }
__device__ __forceinline__ unsigned narrow16(float f, int rt) { return rt == POINTOPS2_ROWS_F16 ? narrow_bits<f16_t>(f) : narrow_bits<bf16_t>(f); }

}  // namespace p2
