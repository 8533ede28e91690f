// Train-time augmentations on the device: the reference's util/transform.py chain (rotate, scale, shift, jitter, drop colour, flip,
// elastic distortion, the chromatic family) as an OP TAPE that one thread runs over its point (stratified_transformer_amd/augment.py
// compiles a Compose into tapes, owns every buffer and every random draw; there is no random number generator here).
//
// pass: one thread per point.  The thread loads its coord row and its feat row whole (12 bytes for float rows, 24 for double ones),
// widens them to double, finds its scene by a binary search of `offset` staged in LDS, runs the n_ops ops of the tape with its scene's
// slice of the parameter table params[scene][op][AUG_P] (doubles), and stores the rows - rounded to the storage type once, here - or
// keeps them as doubles in the caller's workspace when another pass follows.  The offsets and the opcodes are staged in LDS; the
// parameter table is not (1024 scenes x 32 ops x 16 doubles would be 4 MB): the lanes of a wave read their scene's slice at one address,
// a broadcast load that the caches serve.  Every step is float64 in the reference's expression
// order; the library is built with -ffp-contract=off, so nothing is fused.  cos / sin, the elastic grid's axes and every per-scene
// scalar are computed by the host and arrive as parameters: no transcendental runs here.
//
// Three ops need per-scene statistics of the values as they stand in front of them (FLIP: the maximum of a coordinate; AUTOCONTRAST: the
// colour minimum and maximum; ELASTIC: the coordinate minimum and maximum).  The pass in front of such an op accumulates them
// (AUG_STATS): per scene and column the minimum and the maximum as signed 64-bit integer atomics on an order-preserving image of the
// double (the bit pattern, its 63 low bits inverted for a negative value; -0.0 is taken as +0.0), reduced over the wave first when the
// whole wave lies in one scene - one atomicMin and one atomicMax per wave and column - and a "saw a NaN" bit per column (NaNs are left
// out of the minimum and the maximum; the consumer turns a set bit into NaN, as numpy's min / max propagate it).  Minima, maxima and
// bit-ors do not depend on the order: exact and reproducible.  No float atomics anywhere.
// stats: [n_scenes][AUG_STAT_WORDS] long long = six minima (coord xyz, feat rgb), six maxima, the NaN bits; the caller presets
// LLONG_MAX / LLONG_MIN / 0.
//
// blur: one 3-tap box filter of scipy.ndimage.convolve(mode='constant', cval=0) along one axis of every scene's [nx, ny, nz, 3] float
// noise grid: out = float((a[i-1] * w + a[i] * w) + a[i+1] * w) in double with w = double(float(1) / float(3)), zero outside the grid.
// One thread per grid value of the concatenated grids; desc [n_scenes][4] = first value, nx, ny, nz.
// No kernel waits on another workgroup; every index (scene, grid node, axis interval) is clamped into its array.
#include "common.h"

namespace p2 {
namespace {

constexpr int AUG_BLOCK = 256;
constexpr int AUG_P = POINTOPS2_AUGMENT_PARAMS;
constexpr int AUG_MAX_SCENES = POINTOPS2_AUGMENT_MAX_SCENES;
constexpr int AUG_MAX_OPS = POINTOPS2_AUGMENT_MAX_OPS;
constexpr int AUG_STAT_WORDS = POINTOPS2_AUGMENT_STAT_WORDS;

constexpr int AUG_HAS_FEAT = POINTOPS2_AUGMENT_HAS_FEAT, AUG_STORE = POINTOPS2_AUGMENT_STORE, AUG_STATS = POINTOPS2_AUGMENT_STATS;
enum : int { OP_ROTATE = POINTOPS2_AUGMENT_OP_ROTATE, OP_SCALE = POINTOPS2_AUGMENT_OP_SCALE, OP_SHIFT = POINTOPS2_AUGMENT_OP_SHIFT,
             OP_JITTER = POINTOPS2_AUGMENT_OP_JITTER, OP_FEAT_MUL = POINTOPS2_AUGMENT_OP_FEAT_MUL, OP_FLIP = POINTOPS2_AUGMENT_OP_FLIP,
             OP_AUTOCONTRAST = POINTOPS2_AUGMENT_OP_AUTOCONTRAST, OP_CHROMA_TRANSLATE = POINTOPS2_AUGMENT_OP_CHROMA_TRANSLATE,
             OP_CHROMA_JITTER = POINTOPS2_AUGMENT_OP_CHROMA_JITTER, OP_HUE_SATURATION = POINTOPS2_AUGMENT_OP_HUE_SATURATION,
             OP_ELASTIC = POINTOPS2_AUGMENT_OP_ELASTIC };

template <typename T> struct Row3 { T x, y, z; };

template <typename T>
__device__ __forceinline__ void load_row(const void *base, int64_t i, double v[3]) {
    const Row3<T> r = reinterpret_cast<const Row3<T> *>(base)[i];
    v[0] = (double)r.x; v[1] = (double)r.y; v[2] = (double)r.z;
}
template <typename T>
__device__ __forceinline__ void store_row(void *base, int64_t i, const double v[3]) {
    Row3<T> r;
    r.x = (T)v[0]; r.y = (T)v[1]; r.z = (T)v[2];
    reinterpret_cast<Row3<T> *>(base)[i] = r;
}

__device__ __forceinline__ double nan64() { return __longlong_as_double(0x7ff8000000000000LL); }
__device__ __forceinline__ bool is_nan(double v) { return v != v; }
// order-preserving signed image of a double and its inverse (the same map)
__device__ __forceinline__ long long ordered64(long long bits) { return bits >= 0 ? bits : bits ^ 0x7fffffffffffffffLL; }
__device__ __forceinline__ long long image_of(double v) {
    long long bits = __double_as_longlong(v);
    if ((bits & 0x7fffffffffffffffLL) == 0) bits = 0;                                // -0.0 -> +0.0
    return ordered64(bits);
}
__device__ __forceinline__ double value_of(long long key) { return __longlong_as_double(ordered64(key)); }

// np.clip, np.maximum, np.minimum: a NaN operand gives NaN
__device__ __forceinline__ double clip(double v, double lo, double hi) {
    if (is_nan(v)) return v;
    v = v < lo ? lo : v;
    return v > hi ? hi : v;
}
__device__ __forceinline__ double max_nan(double a, double b) { return (is_nan(a) || is_nan(b)) ? nan64() : (a > b ? a : b); }
__device__ __forceinline__ double min_nan(double a, double b) { return (is_nan(a) || is_nan(b)) ? nan64() : (a < b ? a : b); }
// numpy's remainder(v, 1.0): fmod (exact: v - trunc(v)), then a negative result moves up by one; a zero result is +0.0
__device__ __forceinline__ double mod_one(double v) {
    double m = v - trunc(v);                                                         // inf - inf = NaN, as fmod(inf, 1)
    if (m < 0.0) m += 1.0;
    return m;
}
// astype('uint8') for values in [0, 256); NaN and values outside give 0 (the C cast is undefined there)
__device__ __forceinline__ double u8(double v) { return (v >= 0.0 && v < 256.0) ? trunc(v) : 0.0; }
__device__ __forceinline__ void to_255(double f[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) f[k] = (f[k] + 1.0) * 127.5;
}
__device__ __forceinline__ void from_255(double f[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) f[k] = f[k] / 127.5 - 1.0;
}

__device__ __forceinline__ void rotate3(double v[3], const double *R) {
    const double x = v[0], y = v[1], z = v[2];
#pragma unroll
    for (int j = 0; j < 3; ++j) v[j] = (x * R[j] + y * R[3 + j]) + z * R[6 + j];
}

// minimum (which = 0) or maximum (1) of column col of the scene in front of this pass, NaN when the column held one
__device__ __forceinline__ double stat(const long long *st, int which, int col) {
    if ((st[12] >> col) & 1) return nan64();
    return value_of(st[which * 6 + col]);
}

__device__ __forceinline__ void hue_saturation(double f[3], double hue_val, double sat_ratio) {
    to_255(f);
    const double r = f[0], g = f[1], b = f[2];
    const double maxc = max_nan(max_nan(r, g), b), minc = min_nan(min_nan(r, g), b);
    const bool mask = maxc != minc;
    double s = 0.0, rc = 0.0, gc = 0.0, bc = 0.0;
    if (mask) {
        s = (maxc - minc) / maxc;
        rc = (maxc - r) / (maxc - minc);
        gc = (maxc - g) / (maxc - minc);
        bc = (maxc - b) / (maxc - minc);
    }
    double h = r == maxc ? bc - gc : g == maxc ? (2.0 + rc) - bc : (4.0 + gc) - rc;
    h = mod_one(h / 6.0);
    h = mod_one((hue_val + h) + 1.0);
    s = clip(sat_ratio * s, 0.0, 1.0);
    const double v = maxc;
    const double id = u8(h * 6.0);
    const double fr = (h * 6.0) - id;
    const double p = v * (1.0 - s);
    const double q = v * (1.0 - s * fr);
    const double t = v * (1.0 - s * (1.0 - fr));
    const int i = (int)id % 6;
    double R, G, B;
    if (s == 0.0) { R = v; G = v; B = v; }
    else if (i == 1) { R = q; G = v; B = p; }
    else if (i == 2) { R = p; G = v; B = t; }
    else if (i == 3) { R = p; G = q; B = v; }
    else if (i == 4) { R = t; G = p; B = v; }
    else if (i == 5) { R = v; G = p; B = q; }
    else { R = v; G = t; B = p; }
    f[0] = u8(R); f[1] = u8(G); f[2] = u8(B);                                        // (the reference's clip to [0, 255] changes nothing)
    from_255(f);
}

// scipy's RegularGridInterpolator (linear, bounds_error = 0, fill_value = 0) on the scene's blurred grid, times magnitude, added
__device__ __forceinline__ void elastic(double c[3], const double *p, const float *grids, const double *axes) {
    const double magnitude = p[1];
    const int dim[3] = {(int)p[3], (int)p[4], (int)p[5]};
    if (dim[0] < 2 || dim[1] < 2 || dim[2] < 2) return;
    const float *grid = grids + (long long)p[2];
    const double *ax = axes + (long long)p[6];
    int lo[3];
    double y[3];
    bool outside = false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int n = dim[k];
        const double x = c[k];
        outside = outside || x < ax[0] || x > ax[n - 1];
        int a = 0, b = n - 1;                                                        // the last node with ax[a] <= x, clamped to [0, n - 2]
        while (b - a > 1) {
            const int m = (a + b) >> 1;
            if (ax[m] <= x) a = m; else b = m;
        }
        lo[k] = a;
        y[k] = (x - ax[a]) / (ax[a + 1] - ax[a]);
        ax += n;
    }
    double value[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int corner = 0; corner < 8; ++corner) {
        const int bx = corner >> 2, by = (corner >> 1) & 1, bz = corner & 1;
        double w = 1.0;
        w = w * (bx ? y[0] : 1.0 - y[0]);
        w = w * (by ? y[1] : 1.0 - y[1]);
        w = w * (bz ? y[2] : 1.0 - y[2]);
        const float *node = grid + ((((long long)(lo[0] + bx) * dim[1]) + (lo[1] + by)) * dim[2] + (lo[2] + bz)) * 3;
#pragma unroll
        for (int k = 0; k < 3; ++k) value[k] = value[k] + (double)node[k] * w;
    }
    const bool nan = is_nan(c[0]) || is_nan(c[1]) || is_nan(c[2]);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double v = nan ? nan64() : outside ? 0.0 : value[k];
        c[k] = c[k] + v * magnitude;
    }
}

__device__ __forceinline__ long long wave_min64(long long v) {
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) { const long long o = __shfl_xor(v, s, 64); v = o < v ? o : v; }
    return v;
}
__device__ __forceinline__ long long wave_max64(long long v) {
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) { const long long o = __shfl_xor(v, s, 64); v = o > v ? o : v; }
    return v;
}

template <typename TI, typename TO>
__global__ __launch_bounds__(AUG_BLOCK) void augment_pass_kernel(int n, int n_scenes, int n_ops, int flags, const void *coord_in,
                                                                 const void *feat_in, void *coord_out, void *feat_out,   // a workspace pass runs in place
                                                                 const int *__restrict__ offset,
                                                                 const int *__restrict__ opcodes, const long long *__restrict__ op_ptrs,
                                                                 const double *__restrict__ params, const long long *__restrict__ stats_in,
                                                                 long long *__restrict__ stats_out) {
    __shared__ int ends[AUG_MAX_SCENES];
    __shared__ int codes[AUG_MAX_OPS];
    for (int s = threadIdx.x; s < n_scenes; s += AUG_BLOCK) ends[s] = offset[s];
    for (int o = threadIdx.x; o < n_ops; o += AUG_BLOCK) codes[o] = opcodes[o];
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * AUG_BLOCK + threadIdx.x;
    const bool valid = i < n;
    const bool has_feat = flags & AUG_HAS_FEAT;
    int scene = 0;
    double c[3] = {0.0, 0.0, 0.0}, f[3] = {0.0, 0.0, 0.0};
    if (valid) {
        int a = 0, b = n_scenes - 1;                                                 // the first scene whose end lies above i (the last one if none)
        while (a < b) {
            const int m = (a + b) >> 1;
            if (ends[m] > i) b = m; else a = m + 1;
        }
        scene = a;
        load_row<TI>(coord_in, i, c);
        if (has_feat) load_row<TI>(feat_in, i, f);
        const long long *st = stats_in != nullptr ? stats_in + (size_t)scene * AUG_STAT_WORDS : nullptr;
        for (int o = 0; o < n_ops; ++o) {
            const double *p = params + ((size_t)scene * n_ops + o) * AUG_P;
            const bool on = p[0] != 0.0;
            const long long ptr0 = op_ptrs[2 * o], ptr1 = op_ptrs[2 * o + 1];
            switch (codes[o]) {
            case OP_ROTATE:
                if (on) {
                    if (p[10] != 0.0) rotate3(c, p + 1);
                    if (p[11] != 0.0 && has_feat) rotate3(f, p + 1);
                }
                break;
            case OP_SCALE:
                if (on) { c[0] *= p[1]; c[1] *= p[1]; c[2] *= p[1]; }
                break;
            case OP_SHIFT:
                if (on) { c[0] += p[1]; c[1] += p[2]; c[2] += p[3]; }
                break;
            case OP_JITTER:
                if (on && ptr0 != 0) {
                    double z[3];
                    load_row<double>(reinterpret_cast<const void *>(ptr0), i, z);
#pragma unroll
                    for (int k = 0; k < 3; ++k) c[k] += clip(p[1] * z[k], -1.0 * p[2], p[2]);
                }
                break;
            case OP_FEAT_MUL:
                if (on && has_feat) { f[0] *= p[1]; f[1] *= p[1]; f[2] *= p[1]; }
                break;
            case OP_FLIP:
                if (on && st != nullptr) {
#pragma unroll
                    for (int k = 0; k < 3; ++k)
                        if (p[1 + k] != 0.0) c[k] = stat(st, 1, k) - c[k];
                }
                break;
            case OP_AUTOCONTRAST:
                if (has_feat) {
                    to_255(f);
                    if (on && st != nullptr) {
#pragma unroll
                        for (int k = 0; k < 3; ++k) {                                // x -> (x + 1) * 127.5 is monotone: the extrema map to the extrema
                            const double lo = (stat(st, 0, 3 + k) + 1.0) * 127.5, hi = (stat(st, 1, 3 + k) + 1.0) * 127.5;
                            const double scale = 255.0 / (hi - lo);
                            const double contrast = (f[k] - lo) * scale;
                            f[k] = (1.0 - p[1]) * f[k] + p[1] * contrast;
                        }
                    }
                    from_255(f);
                }
                break;
            case OP_CHROMA_TRANSLATE:
                if (has_feat) {
                    to_255(f);
                    if (on) {
#pragma unroll
                        for (int k = 0; k < 3; ++k) f[k] = clip(p[1 + k] + f[k], 0.0, 255.0);
                    }
                    from_255(f);
                }
                break;
            case OP_CHROMA_JITTER:
                if (has_feat) {
                    to_255(f);
                    if (on && ptr0 != 0) {
                        double z[3];
                        load_row<double>(reinterpret_cast<const void *>(ptr0), i, z);
#pragma unroll
                        for (int k = 0; k < 3; ++k) f[k] = clip(z[k] * p[1] + f[k], 0.0, 255.0);
                    }
                    from_255(f);
                }
                break;
            case OP_HUE_SATURATION:
                if (on && has_feat) hue_saturation(f, p[1], p[2]);
                break;
            case OP_ELASTIC:
                if (on && ptr0 != 0 && ptr1 != 0) elastic(c, p, reinterpret_cast<const float *>(ptr0), reinterpret_cast<const double *>(ptr1));
                break;
            default:
                break;
            }
        }
        if (flags & AUG_STORE) {
            store_row<TO>(coord_out, i, c);
            if (has_feat) store_row<TO>(feat_out, i, f);
        }
    }
    if (flags & AUG_STATS) {
        // lane 0 of a wave holds the wave's first point, so it is valid whenever any lane is
        const int first = __shfl(scene, 0, 64);
        const bool whole = __all(!valid || scene == first);
        const int cols = has_feat ? 6 : 3;
        unsigned long long nan_bits = 0;
        for (int col = 0; col < cols; ++col) {
            const double v = col < 3 ? c[col] : f[col - 3];
            const bool use = valid && !is_nan(v);
            if (valid && is_nan(v)) nan_bits |= 1ull << col;
            long long lo = use ? image_of(v) : 0x7fffffffffffffffLL, hi = use ? image_of(v) : (long long)0x8000000000000000LL;
            if (whole) {
                lo = wave_min64(lo);
                hi = wave_max64(hi);
                if (lane_id() == 0 && valid) {
                    long long *st = stats_out + (size_t)first * AUG_STAT_WORDS;
                    if (lo != 0x7fffffffffffffffLL) atomicMin(&st[col], lo);
                    if (hi != (long long)0x8000000000000000LL) atomicMax(&st[6 + col], hi);
                }
            } else if (use) {
                long long *st = stats_out + (size_t)scene * AUG_STAT_WORDS;
                atomicMin(&st[col], lo);
                atomicMax(&st[6 + col], hi);
            }
        }
        if (nan_bits != 0) atomicOr(reinterpret_cast<unsigned long long *>(stats_out + (size_t)scene * AUG_STAT_WORDS + 12), nan_bits);
    }
}

__global__ __launch_bounds__(AUG_BLOCK) void augment_blur_kernel(long long total, int n_scenes, int axis, const long long *__restrict__ desc,
                                                                 const float *__restrict__ in, float *__restrict__ out) {
    const long long e = (long long)blockIdx.x * AUG_BLOCK + threadIdx.x;
    if (e >= total) return;
    int a = 0, b = n_scenes - 1;                                                     // the last scene whose first value is <= e
    while (a < b) {
        const int m = (a + b + 1) >> 1;
        if (desc[4 * m] <= e) a = m; else b = m - 1;
    }
    const long long start = desc[4 * a], nx = desc[4 * a + 1], ny = desc[4 * a + 2], nz = desc[4 * a + 3];
    const long long local = e - start;
    if (local < 0 || local >= nx * ny * nz * 3) { out[e] = in[e]; return; }         // a gap between grids: nothing to filter
    const long long node = local / 3;
    const long long iz = node % nz, iy = (node / nz) % ny, ix = node / (nz * ny);
    const long long pos = axis == 0 ? ix : axis == 1 ? iy : iz, len = axis == 0 ? nx : axis == 1 ? ny : nz;
    const long long stride = (axis == 0 ? ny * nz : axis == 1 ? nz : 1) * 3;
    const double w = (double)(1.0f / 3.0f);
    const double prev = pos > 0 ? (double)in[e - stride] : 0.0, next = pos + 1 < len ? (double)in[e + stride] : 0.0;
    out[e] = (float)((prev * w + (double)in[e] * w) + next * w);
}

}  // namespace
}  // namespace p2

using namespace p2;

extern "C" {

void pointops2_augment_pass_launcher(int n, int n_scenes, int n_ops, int in_f64, int out_f64, int flags, const void *coord_in,
                                     const void *feat_in, void *coord_out, void *feat_out, const int *offset, const int *opcodes,
                                     const long long *op_ptrs, const double *params, const long long *stats_in, long long *stats_out) {
    const hipStream_t st = begin_launch().stream;
    if (n < 0 || n_scenes < 1 || n_ops < 0) { set_error("augment_pass: need n >= 0, n_scenes >= 1, n_ops >= 0"); return; }
    if (n_scenes > AUG_MAX_SCENES) { set_error("augment_pass: more than 1024 scenes in one launch"); return; }
    if (n_ops > AUG_MAX_OPS) { set_error("augment_pass: more than 32 ops in one launch"); return; }
    if (n == 0) return;
    const bool has_feat = flags & AUG_HAS_FEAT, store = flags & AUG_STORE, stats = flags & AUG_STATS;
    if (coord_in == nullptr || offset == nullptr || (has_feat && feat_in == nullptr)) { set_error("augment_pass: a NULL input"); return; }
    if (store && (coord_out == nullptr || (has_feat && feat_out == nullptr))) { set_error("augment_pass: a NULL output"); return; }
    if (stats && stats_out == nullptr) { set_error("augment_pass: no table for the statistics"); return; }
    if (n_ops > 0 && (opcodes == nullptr || op_ptrs == nullptr || params == nullptr)) { set_error("augment_pass: a NULL tape"); return; }
    const dim3 grid(div_up(n, AUG_BLOCK)), block(AUG_BLOCK);
#define AUG_LAUNCH(TI, TO)                                                                                                              \
    hipLaunchKernelGGL((augment_pass_kernel<TI, TO>), grid, block, 0, st, n, n_scenes, n_ops, flags, coord_in, feat_in, coord_out,      \
                       feat_out, offset, opcodes, op_ptrs, params, stats_in, stats_out)
    if (in_f64 && out_f64) AUG_LAUNCH(double, double);
    else if (in_f64) AUG_LAUNCH(double, float);
    else if (out_f64) AUG_LAUNCH(float, double);
    else AUG_LAUNCH(float, float);
#undef AUG_LAUNCH
    check_launch();
}

void pointops2_augment_blur_launcher(long long total, int n_scenes, int axis, const long long *desc, const float *in, float *out) {
    const hipStream_t st = begin_launch().stream;
    if (total < 0 || n_scenes < 1 || axis < 0 || axis > 2) { set_error("augment_blur: need total >= 0, n_scenes >= 1, axis in 0..2"); return; }
    if (total >= 2147483648LL * AUG_BLOCK) { set_error("augment_blur: too many grid values for one launch"); return; }
    if (total == 0) return;
    if (desc == nullptr || in == nullptr || out == nullptr || in == out) { set_error("augment_blur: a NULL array, or in == out"); return; }
    hipLaunchKernelGGL(augment_blur_kernel, dim3((unsigned)div_up64(total, AUG_BLOCK)), dim3(AUG_BLOCK), 0, st, total, n_scenes, axis, desc, in, out);
    check_launch();
}

}  // extern "C"
