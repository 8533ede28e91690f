"""numpy restatement of the reference's train-time transforms (util/transform.py), in float64 and in the reference's expression
order, with every random decision passed in: `t(coord, feat, d)` where `d` holds this transform's draws for this scene (the keys
are listed per class).  Out of place; float32 inputs are widened first and the caller rounds the result once (the device's
semantics, stratified_transformer_amd/augment.py).  Nothing of the reference is imported.

Three things are restated rather than called, so that the device can be compared bit for bit:
  * the rotations' `np.dot(points, R)` (BLAS: unspecified order / fused operations) is (p0*R0j + p1*R1j) + p2*R2j, unfused;
  * scipy.ndimage's 3-tap correlate is ((a[i-1]*w + a[i]*w) + a[i+1]*w) in float64, w = float64(float32(1)/3), one float32 store;
  * scipy's RegularGridInterpolator (linear, fill_value 0) is the 8-term sum in the order of its hypercube walk.
The flips' per-axis maximum is taken as `max + 0.0`: a maximum of -0.0 counts as +0.0 (the device reduces on an order-preserving
integer image in which the two zeros are one value); results differ from numpy's in the sign of a zero only.
`u8` is numpy's astype('uint8') for values in [0, 256); NaN and values outside (unpinned in the reference: the C cast is undefined
there) give 0.
"""
import itertools

import numpy as np


def _f64(a):
    return None if a is None else np.array(a, dtype=np.float64)


def dot3(x, R):
    return np.stack([(x[:, 0] * R[0, j] + x[:, 1] * R[1, j]) + x[:, 2] * R[2, j] for j in range(3)], 1)


def u8(x):
    x = np.asarray(x, dtype=np.float64)
    ok = (x >= 0.0) & (x < 256.0)
    return np.where(ok, np.trunc(np.where(ok, x, 0.0)), 0.0)


def rotate_matrix(angle, along_z=True):
    c, s = np.cos(angle), np.sin(angle)
    if along_z:
        return np.array([[c, s, 0], [-s, c, 0], [0, 0, 1]])
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


def perturbation_matrix(angles):
    Rx = np.array([[1, 0, 0], [0, np.cos(angles[0]), -np.sin(angles[0])], [0, np.sin(angles[0]), np.cos(angles[0])]])
    Ry = np.array([[np.cos(angles[1]), 0, np.sin(angles[1])], [0, 1, 0], [-np.sin(angles[1]), 0, np.cos(angles[1])]])
    Rz = np.array([[np.cos(angles[2]), -np.sin(angles[2]), 0], [np.sin(angles[2]), np.cos(angles[2]), 0], [0, 0, 1]])
    return np.dot(Rz, np.dot(Ry, Rx))


class Compose:
    """d: one dict per transform, in order"""

    def __init__(self, transforms):
        self.transforms = transforms

    def __call__(self, coord, feat, d):
        coord, feat = _f64(coord), _f64(feat)
        for t, dt in zip(self.transforms, d):
            coord, feat = t(coord, feat, dt)
        return coord, feat


class RandomRotate:
    """d: u (angle = u * 2 * pi) unless rotate_angle is given"""

    def __init__(self, rotate_angle=None, along_z=True, color_rotate=False):
        self.rotate_angle, self.along_z, self.color_rotate = rotate_angle, along_z, color_rotate

    def __call__(self, coord, feat, d):
        coord, feat = _f64(coord), _f64(feat)
        angle = d["u"] * 2 * np.pi if self.rotate_angle is None else self.rotate_angle
        R = rotate_matrix(angle, self.along_z)
        coord = dot3(coord, R)
        if self.color_rotate:
            feat = dot3(feat, R)
        return coord, feat


class RandomRotatePerturbation:
    """d: randn [3]"""

    def __init__(self, angle_sigma=0.06, angle_clip=0.18, normals=False):
        self.angle_sigma, self.angle_clip, self.normals = angle_sigma, angle_clip, normals

    def __call__(self, coord, feat, d):
        coord, feat = _f64(coord), _f64(feat)
        angles = np.clip(self.angle_sigma * np.asarray(d["randn"], np.float64), -self.angle_clip, self.angle_clip)
        R = perturbation_matrix(angles)
        coord = dot3(coord, R)
        if self.normals:
            feat = dot3(feat, R)
        return coord, feat


class RandomScale:
    """d: scale"""

    def __init__(self, scale_low=0.8, scale_high=1.2):
        self.scale_low, self.scale_high = scale_low, scale_high

    def __call__(self, coord, feat, d):
        return _f64(coord) * d["scale"], _f64(feat)


class RandomShift:
    """d: shift [3]"""

    def __init__(self, shift_range=0.1):
        self.shift_range = shift_range

    def __call__(self, coord, feat, d):
        return _f64(coord) + np.asarray(d["shift"], np.float64), _f64(feat)


class RandomJitter:
    """d: noise [N, 3]"""

    def __init__(self, sigma=0.01, clip=0.05):
        self.sigma, self.clip = sigma, clip

    def __call__(self, coord, feat, d):
        jitter = np.clip(self.sigma * np.asarray(d["noise"], np.float64), -1 * self.clip, self.clip)
        return _f64(coord) + jitter, _f64(feat)


class RandomDropColor:
    """d: u (the colour is scaled when u > p)"""

    def __init__(self, p=0.8, color_augment=0.0):
        self.p, self.color_augment = p, color_augment

    def __call__(self, coord, feat, d):
        coord, feat = _f64(coord), _f64(feat)
        if feat is not None and d["u"] > self.p:
            feat = feat * self.color_augment
        return coord, feat


BLUR_W = np.float64(np.float32(1) / np.float32(3))


def blur_axis(g, axis):
    """one 3-tap box filter of scipy.ndimage.convolve(mode='constant', cval=0) along `axis` of a float32 grid"""
    x = np.moveaxis(g.astype(np.float64), axis, 0)
    z = np.zeros((1,) + x.shape[1:])
    p = np.concatenate([z, x, z], 0)
    out = (p[:-2] * BLUR_W + p[1:-1] * BLUR_W) + p[2:] * BLUR_W
    return np.ascontiguousarray(np.moveaxis(out.astype(np.float32), 0, axis))


def blur(noise):
    for _ in range(2):
        for axis in range(3):
            noise = blur_axis(noise, axis)
    return noise


def noise_dim(coord, granularity):
    lo = coord.min(0)
    return (np.floor_divide((coord - lo).max(0), granularity)).astype(int) + 3


def elastic_axes(lo, granularity, dim):
    return [np.linspace(a, b, n) for a, b, n in zip(lo - granularity, lo + granularity * (dim - 2), dim)]


def interp(ax, values, x):
    """RegularGridInterpolator(ax, values, bounds_error=0, fill_value=0)(x) for a [nx, ny, nz, 3] float32 grid"""
    idx, w = [], []
    oob = np.zeros(x.shape[0], bool)
    for k in range(3):
        a = ax[k]
        i = np.clip(np.searchsorted(a, x[:, k], side="right") - 1, 0, a.shape[0] - 2)
        y = (x[:, k] - a[i]) / (a[i + 1] - a[i])
        idx.append((i, i + 1))
        w.append((1 - y, y))
        oob |= (x[:, k] < a[0]) | (x[:, k] > a[-1])
    value = np.zeros((x.shape[0], 3))
    for corner in itertools.product((0, 1), repeat=3):
        weight = np.ones(x.shape[0])
        for k in range(3):
            weight = weight * w[k][corner[k]]
        term = values[idx[0][corner[0]], idx[1][corner[1]], idx[2][corner[2]]] * weight[:, None]
        value = value + term
    value[oob] = 0.0
    return value


class ElasticDistortion:
    """d: gate (applied when gate < 0.95), noise: per (granularity, magnitude) entry the float32 [nx, ny, nz, 3] grid"""

    def __init__(self, distortion_params):
        self.distortion_params = distortion_params

    def __call__(self, coord, feat, d):
        coord, feat = _f64(coord), _f64(feat)
        self.blurred = []
        if self.distortion_params is not None and d["gate"] < 0.95 and coord.shape[0] > 0:
            for (granularity, magnitude), noise in zip(self.distortion_params, d["noise"]):
                lo = coord.min(0)
                dim = noise_dim(coord, granularity)
                noise = np.asarray(noise, np.float32)
                assert noise.shape == tuple(dim) + (3,), (noise.shape, dim)
                grid = blur(noise)
                self.blurred.append(grid)
                coord = coord + interp(elastic_axes(lo, granularity, dim), grid, coord) * magnitude
        return coord, feat


class RandomHorizontalFlip:
    """d: gate (< 0.95), axes: one u per horizontal axis in ascending order (flipped when u < 0.5)"""

    def __init__(self, upright_axis="z", is_temporal=False):
        if is_temporal:
            raise ValueError("is_temporal flips are not supported")
        self.upright_axis = {"x": 0, "y": 1, "z": 2}[upright_axis.lower()]
        self.horz_axes = sorted(set(range(3)) - {self.upright_axis})

    def __call__(self, coord, feat, d):
        coord, feat = _f64(coord), _f64(feat)
        if d["gate"] < 0.95 and coord.shape[0] > 0:
            for ax, u in zip(self.horz_axes, d["axes"]):
                if u < 0.5:
                    coord[:, ax] = (np.max(coord[:, ax]) + 0.0) - coord[:, ax]
        return coord, feat


class ChromaticAutoContrast:
    """d: gate (< 0.2), blend (used when randomize_blend_factor)"""

    def __init__(self, randomize_blend_factor=True, blend_factor=0.5):
        self.randomize_blend_factor, self.blend_factor = randomize_blend_factor, blend_factor

    def __call__(self, coord, feat, d):
        coord, feat = _f64(coord), _f64(feat)
        feat = (feat + 1.0) * 127.5
        if d["gate"] < 0.2 and feat.shape[0] > 0:
            with np.errstate(all="ignore"):
                lo = np.min(feat, 0, keepdims=True)
                hi = np.max(feat, 0, keepdims=True)
                scale = 255 / (hi - lo)
                contrast = (feat - lo) * scale
                b = d["blend"] if self.randomize_blend_factor else self.blend_factor
                feat = (1 - b) * feat + b * contrast
        feat = feat / 127.5 - 1
        return coord, feat


class ChromaticTranslation:
    """d: gate (< 0.95), u [3]"""

    def __init__(self, trans_range_ratio=1e-1):
        self.trans_range_ratio = trans_range_ratio

    def __call__(self, coord, feat, d):
        coord, feat = _f64(coord), _f64(feat)
        feat = (feat + 1.0) * 127.5
        if d["gate"] < 0.95:
            tr = (np.asarray(d["u"], np.float64).reshape(1, 3) - 0.5) * 255 * 2 * self.trans_range_ratio
            feat = np.clip(tr + feat, 0, 255)
        feat = feat / 127.5 - 1
        return coord, feat


class ChromaticJitter:
    """d: gate (< 0.95), noise [N, 3]"""

    def __init__(self, std=0.01):
        self.std = std

    def __call__(self, coord, feat, d):
        coord, feat = _f64(coord), _f64(feat)
        feat = (feat + 1.0) * 127.5
        if d["gate"] < 0.95:
            noise = np.array(d["noise"], np.float64)
            noise *= self.std * 255
            feat = np.clip(noise + feat, 0, 255)
        feat = feat / 127.5 - 1
        return coord, feat


def rgb_to_hsv(rgb):
    r, g, b = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    with np.errstate(all="ignore"):
        maxc = np.maximum(np.maximum(r, g), b)
        minc = np.minimum(np.minimum(r, g), b)
        mask = maxc != minc
        zero = np.zeros_like(r)
        s = np.where(mask, (maxc - minc) / maxc, zero)
        rc = np.where(mask, (maxc - r) / (maxc - minc), zero)
        gc = np.where(mask, (maxc - g) / (maxc - minc), zero)
        bc = np.where(mask, (maxc - b) / (maxc - minc), zero)
        h = np.select([r == maxc, g == maxc], [bc - gc, 2.0 + rc - bc], default=4.0 + gc - rc)
        h = (h / 6.0) % 1.0
    return h, s, maxc


def hsv_to_rgb(h, s, v):
    i = u8(h * 6.0)
    f = (h * 6.0) - i
    p = v * (1.0 - s)
    q = v * (1.0 - s * f)
    t = v * (1.0 - s * (1.0 - f))
    i = i % 6
    conditions = [s == 0.0, i == 1, i == 2, i == 3, i == 4, i == 5]
    r = np.select(conditions, [v, q, p, p, t, v], default=v)
    g = np.select(conditions, [v, v, v, q, p, p], default=t)
    b = np.select(conditions, [v, p, t, v, v, q], default=p)
    return np.stack([u8(r), u8(g), u8(b)], 1)


class HueSaturationTranslation:
    """d: hue_u, sat_u"""

    def __init__(self, hue_max, saturation_max):
        self.hue_max, self.saturation_max = hue_max, saturation_max

    def __call__(self, coord, feat, d):
        coord, feat = _f64(coord), _f64(feat)
        feat = (feat + 1.0) * 127.5
        h, s, v = rgb_to_hsv(feat)
        hue_val = (d["hue_u"] - 0.5) * 2 * self.hue_max
        sat_ratio = 1 + (d["sat_u"] - 0.5) * 2 * self.saturation_max
        with np.errstate(all="ignore"):
            h = np.remainder(hue_val + h + 1, 1)
            s = np.clip(sat_ratio * s, 0, 1)
            feat = np.clip(hsv_to_rgb(h, s, v), 0, 255)
        feat = feat / 127.5 - 1
        return coord, feat
