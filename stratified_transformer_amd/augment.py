"""The reference's train-time transforms (util/transform.py) on device tensors: rotate, scale, shift, jitter, drop colour, elastic
distortion, flip and the chromatic family, under the reference's class names and constructor arguments, composable, for one scene or
a whole batch with `offset` - a scene that is already on the GPU is augmented there (csrc/augment.hip).

    t = Compose([RandomRotate(along_z=True), RandomScale(0.8, 1.2), RandomJitter(0.005, 0.02), RandomDropColor(color_augment=0.0)])
    coord, feat = t(coord, feat, offset)          # out of place; the outputs have the inputs' dtype

Call: t(coord, feat, offset=None, draws=None, rng=None, generator=None) -> (coord, feat).  coord / feat [N, 3] float32 or float64 GPU
tensors (feat may be None where the reference allows it: every class but the chromatic ones), offset the cumulative int32 ends of
the scenes (omitted: one scene).

Randomness.  Every random decision of the reference is a DRAW: per-scene draws (angles, scales, shifts, gates, blend factors, colour
translations, hue / saturation values) are made on the host from `rng` (a numpy.random.Generator), one set per scene of the batch;
per-point noise (the two jitters) and the elastic noise grids are drawn on the device with torch.randn(..., generator=generator).
The call leaves a `Draws` object in `t.last_draws`; passed back as `draws=` it replays the call exactly (bitwise).  The reference's own
Mersenne-Twister stream (np.random.* / random.random in call order) is NOT reproduced: equal seeds give different augmentations
than the reference, equal draws give the reference's result.

Arithmetic.  Both dtypes take one path: a row is widened to float64 on load, every step runs in float64 in the reference's expression
order (no fused multiply-add), values that cross a pass boundary stay float64 in a workspace, and the result is rounded to the storage
dtype once, at the final store.  A float32 call therefore equals the float64 call on the widened input, rounded once - deliberately not
numpy's in-place float32 arithmetic - and ElasticDistortion returns the input dtype where the reference returns float64.  cos / sin
and the elastic grid's np.linspace axes are computed on the host; no transcendental runs on the device.

Passes.  A Compose is compiled into an op tape (opcodes + a [n_scenes, n_ops, 16] table of doubles; a gate that came out "off" is a
no-op for that scene only); consecutive ops run in ONE kernel pass, one thread per point.  Three ops need per-scene statistics of the
values in front of them - a flip the maximum of a coordinate, auto-contrast the colour extrema, elastic the coordinate extrema.  The
pass in front of such an op also reduces the per-scene minimum / maximum of the six columns on the device (exact integer atomics, NaN
aware) and a new pass starts - unless no op since the last reduction has written the columns asked for, then the op joins the
running pass.  So a chain without such ops (the S3DIS training chain) is one pass; a flip or an auto-contrast adds one pass and NO
read-back; ElasticDistortion costs one host read-back of the statistics table PER (granularity, magnitude) ENTRY, whatever the number
of scenes, because the size of its noise grid depends on the data.  `t.last_counts` reports passes and read-backs of the last call,
`plan_counts(t)` the same without a GPU.

Kept quirks: ChromaticAutoContrast on a constant channel divides by zero and yields NaN; HueSaturationTranslation keeps the two
astype('uint8') truncations (output quantised to 1 / 127.5; specified for feats in [-1, 1] - NaN and values that leave 0..255 give 0
where the reference's cast is undefined); the chromatic classes convert to 0..255 and back even when their gate is shut.  A flip's
maximum of -0.0 counts as +0.0.  ElasticDistortion refuses NaN coordinates (the reference's grid size is undefined there) and skips
empty scenes.  RandomHorizontalFlip(is_temporal=True) is refused.
"""
import numpy as np
import torch

from . import _lib

PARAMS, MAX_OPS, STAT_WORDS = 16, 32, 13        # POINTOPS2_AUGMENT_* of include/pointops2_hip.h
HAS_FEAT, STORE, STATS = 1, 2, 4
OP = {"rotate": 1, "scale": 2, "shift": 3, "jitter": 4, "feat_mul": 5, "flip": 6, "autocontrast": 7, "chroma_translate": 8,
      "chroma_jitter": 9, "hue_saturation": 10, "elastic": 11}
MAX_GRID_VALUES = 1 << 27                        # per ElasticDistortion entry, all scenes together (512 MB of float32)
_I64_MAX, _I64_MIN = np.iinfo(np.int64).max, np.iinfo(np.int64).min


class Draws:
    """What a call drew: `records` holds one dict per elementary transform, in chain order.  Host draws are numpy arrays with one
    leading entry per scene; per-point noise is a device tensor [N, 3] float64; ElasticDistortion's `noise` is, per entry, a list
    with one float32 device tensor [nx, ny, nz, 3] per scene (None where the scene drew none)."""

    def __init__(self, records=None):
        self.records = [] if records is None else list(records)


def _check_rows(coord, feat, offset):
    if not isinstance(coord, torch.Tensor) or not coord.is_cuda or coord.dim() != 2 or coord.shape[1] != 3 \
            or coord.dtype not in (torch.float32, torch.float64):
        raise RuntimeError("augment: coord must be a [N, 3] float32 / float64 GPU tensor (there is no CPU fallback)")
    if feat is not None and (not isinstance(feat, torch.Tensor) or feat.device != coord.device or feat.shape != coord.shape
                             or feat.dtype != coord.dtype):
        raise RuntimeError("augment: feat must be None or a tensor of coord's shape, dtype and device")
    if offset is not None and (not isinstance(offset, torch.Tensor) or offset.device != coord.device or offset.dtype != torch.int32
                               or offset.dim() != 1 or offset.shape[0] < 1):
        raise RuntimeError("augment: offset must be a non-empty 1-d int32 tensor on coord's device")


class _Call:
    """one call's inputs, random sources and the draws it records / replays"""

    def __init__(self, coord, feat, offset, draws, rng, generator):
        self.coord, self.feat = coord.contiguous(), None if feat is None else feat.contiguous()
        self.n, self.device = coord.shape[0], coord.device
        self.offset = offset.contiguous() if offset is not None else torch.tensor([self.n], dtype=torch.int32, device=self.device)
        self.b = self.offset.shape[0]
        self.rng = rng if rng is not None else np.random.default_rng()
        self.generator, self.replay, self.out = generator, draws, Draws()

    def record(self, leaf):
        if self.replay is not None:
            k = len(self.out.records)
            if k >= len(self.replay.records):
                raise ValueError("augment: the draws passed in belong to a shorter chain")
            rec = self.replay.records[k]
        else:
            rec = leaf._draw(self)
        self.out.records.append(rec)
        return rec

    def randn(self, shape, dtype):
        return torch.randn(shape, dtype=dtype, device=self.device, generator=self.generator)

    def noise_rows(self, rec):
        """the record's per-point noise; a replayed record that holds host draws only gets its noise drawn here"""
        if rec.get("noise") is None:
            rec["noise"] = self.randn((self.n, 3), torch.float64)
        z = rec["noise"]
        if not isinstance(z, torch.Tensor) or z.shape != (self.n, 3) or z.dtype != torch.float64 or z.device != self.device:
            raise ValueError("augment: replayed per-point noise must be a [N, 3] float64 tensor on coord's device")
        return z.contiguous()

    def host(self, rec, key, tail=()):
        if key not in rec:
            raise ValueError(f"augment: draw '{key}' is missing from the draws passed in")
        v = np.asarray(rec[key], dtype=np.float64)
        if v.shape != (self.b,) + tuple(tail):
            raise ValueError(f"augment: draw '{key}' has shape {v.shape}, expected {(self.b,) + tuple(tail)}")
        return v


class _Tape:
    """The pass compiler: ops are gathered until statistics are asked for that the running pass has made stale (or the tape is
    full), then the pass is launched.  call = None: a dry run that only counts."""

    def __init__(self, call):
        self.call, self.ops, self.keep = call, [], []
        self.dirty, self.stats = set(), None
        self.passes = self.readbacks = 0
        if call is not None:
            self.src, self.src_f64 = (call.coord, call.feat), call.coord.dtype == torch.float64
            self.work = None

    def require(self, cols):
        if self.stats is None or (set(cols) & self.dirty):
            self._flush(True, False)

    def add(self, code, writes, params=None, ptr0=0, ptr1=0, keep=()):
        if len(self.ops) == MAX_OPS:
            self._flush(False, False)
        self.ops.append((OP[code], params, ptr0, ptr1))
        self.keep += list(keep)
        self.dirty |= set(writes)

    def readback(self):
        """the statistics in front of the next op on the host: (min [B, 6], max [B, 6], nan bits [B], empty [B]); one synchronising copy"""
        self.readbacks += 1
        if self.call is None:
            return None
        t = self.stats.cpu().numpy()
        keys = np.where(t[:, :12] >= 0, t[:, :12], t[:, :12] ^ _I64_MAX)
        vals = np.ascontiguousarray(keys).view(np.float64)
        return vals[:, :6], vals[:, 6:12], t[:, 12], (t[:, 0] == _I64_MAX) & (t[:, 12] == 0)   # last: the scene has no point

    def finish(self):
        self._flush(False, True)

    def _flush(self, stats, final):
        self.passes += 1
        ops, self.ops = self.ops, []
        if stats:
            self.dirty = set()
            self.stats_prev, self.stats = self.stats, True
        if self.call is None:
            return
        c, n_ops = self.call, len(ops)
        store = final or n_ops > 0
        # one upload per pass: the preset statistics table, the ops' addresses, their parameters, the opcodes
        n_stat, n_ptr, n_par = (c.b * STAT_WORDS if stats else 0), 2 * n_ops, c.b * n_ops * PARAMS
        buf = np.zeros(n_stat + n_ptr + n_par + (n_ops + 1) // 2, dtype=np.int64)
        if stats:
            preset = buf[:n_stat].reshape(c.b, STAT_WORDS)
            preset[:, 0:6], preset[:, 6:12] = _I64_MAX, _I64_MIN
        par = buf[n_stat + n_ptr:n_stat + n_ptr + n_par].view(np.float64).reshape(c.b, n_ops, PARAMS)
        codes = buf[n_stat + n_ptr + n_par:].view(np.int32)
        for o, (code, params, ptr0, ptr1) in enumerate(ops):
            codes[o] = code
            buf[n_stat + 2 * o], buf[n_stat + 2 * o + 1] = ptr0, ptr1
            par[:, o, :params.shape[1]] = params
        dev = torch.from_numpy(buf).to(c.device)
        base = dev.data_ptr()
        stats_in = self.stats_prev if stats else self.stats
        stats_in = stats_in if isinstance(stats_in, torch.Tensor) else None
        if final:
            out = (torch.empty_like(c.coord), None if c.feat is None else torch.empty_like(c.feat))
            out_f64 = c.coord.dtype == torch.float64
        elif store:
            if self.work is None:
                self.work = (torch.empty(c.n, 3, dtype=torch.float64, device=c.device),
                             None if c.feat is None else torch.empty(c.n, 3, dtype=torch.float64, device=c.device))
            out, out_f64 = self.work, True
        else:
            out, out_f64 = (None, None), False
        flags = (HAS_FEAT if c.feat is not None else 0) | (STORE if store else 0) | (STATS if stats else 0)
        _lib.call("pointops2_augment_pass_launcher", c.n, c.b, n_ops, int(self.src_f64), int(out_f64), flags,
                  _lib.ptr(self.src[0]), _lib.ptr(self.src[1]), _lib.ptr(out[0]), _lib.ptr(out[1]), _lib.ptr(c.offset),
                  base + 8 * (n_stat + n_ptr + n_par), base + 8 * n_stat, base + 8 * (n_stat + n_ptr),
                  _lib.ptr(stats_in), base if stats else None, device=c.device)
        self.keep.append(dev)
        if stats:
            self.stats = dev[:n_stat].view(c.b, STAT_WORDS)
        if store:
            self.src, self.src_f64 = out, out_f64
        self.result = out


class Transform:
    """base of every transform: the call (see the module's docstring)"""
    needs, writes = "", ""

    def _leaves(self):
        return [self]

    def __call__(self, coord, feat=None, offset=None, draws=None, rng=None, generator=None):
        _check_rows(coord, feat, offset)
        leaves = self._leaves()
        if draws is not None and len(draws.records) != len(leaves):
            raise ValueError(f"augment: the draws passed in belong to a chain of {len(draws.records)} transforms, this one has {len(leaves)}")
        call = _Call(coord, feat, offset, draws, rng, generator)
        tape = _Tape(call)
        for leaf in leaves:
            leaf._emit(call, tape, call.record(leaf))
        tape.finish()
        self.last_draws, self.last_counts = call.out, {"passes": tape.passes, "readbacks": tape.readbacks}
        return tape.result

    def _draw(self, call):
        return {}

    def _emit(self, call, tape, rec):
        """append this transform's ops to the tape (call = None: dry run)"""
        if self.needs:
            tape.require(self.needs)
        tape.add(self.code, self.writes, *(() if call is None else self._params(call, rec)))

    def __repr__(self):
        return type(self).__name__ + "(" + ", ".join(f"{k}={v!r}" for k, v in vars(self).items() if not k.startswith("last_")) + ")"


def plan_counts(transform):
    """{'passes', 'readbacks'} of a call of `transform` on data with colours, with every gate open; needs no GPU"""
    tape = _Tape(None)
    for leaf in transform._leaves():
        leaf._emit(None, tape, None)
    tape.finish()
    return {"passes": tape.passes, "readbacks": tape.readbacks}


class Compose(Transform):
    def __init__(self, transforms):
        self.transforms = list(transforms)

    def _leaves(self):
        return [leaf for t in self.transforms for leaf in t._leaves()]


def _table(call, *columns):
    """[B, 1 + ...] parameter rows: the gate, then the columns ([B] or [B, k] arrays, or scalars)"""
    cols = [np.broadcast_to(np.asarray(c, dtype=np.float64), (call.b,))[:, None] if np.ndim(c) < 2 else np.asarray(c, dtype=np.float64)
            for c in columns]
    return np.concatenate(cols, 1)


def _rotate_matrix(angle, along_z):
    c, s = np.cos(angle), np.sin(angle)
    if along_z:
        return np.array([[c, s, 0], [-s, c, 0], [0, 0, 1]])
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


class RandomRotate(Transform):
    code, writes = "rotate", "cf"

    def __init__(self, rotate_angle=None, along_z=True, color_rotate=False):
        self.rotate_angle, self.along_z, self.color_rotate = rotate_angle, along_z, color_rotate
        self.writes = "cf" if color_rotate else "c"

    def _draw(self, call):
        return {} if self.rotate_angle is not None else {"u": call.rng.random(call.b)}

    def _params(self, call, rec):
        if self.rotate_angle is None:
            angles = call.host(rec, "u") * 2 * np.pi
        else:
            angles = np.full(call.b, self.rotate_angle, dtype=np.float64)
        R = np.stack([_rotate_matrix(a, self.along_z).reshape(9) for a in angles]).reshape(call.b, 9)
        return (_table(call, 1.0, R, 1.0, float(self.color_rotate and call.feat is not None)),)


class RandomRotatePerturbation(Transform):
    """normals=True: feat[:, :3] holds normals and is rotated too (the reference's rotation of columns 3:6 of its [N, 6] rows)"""
    code = "rotate"

    def __init__(self, angle_sigma=0.06, angle_clip=0.18, normals=False):
        self.angle_sigma, self.angle_clip, self.normals = angle_sigma, angle_clip, normals
        self.writes = "cf" if normals else "c"

    def _draw(self, call):
        return {"randn": call.rng.standard_normal((call.b, 3))}

    def _params(self, call, rec):
        angles = np.clip(self.angle_sigma * call.host(rec, "randn", (3,)), -self.angle_clip, self.angle_clip)
        R = np.empty((call.b, 9))
        for s, a in enumerate(angles):
            Rx = np.array([[1, 0, 0], [0, np.cos(a[0]), -np.sin(a[0])], [0, np.sin(a[0]), np.cos(a[0])]])
            Ry = np.array([[np.cos(a[1]), 0, np.sin(a[1])], [0, 1, 0], [-np.sin(a[1]), 0, np.cos(a[1])]])
            Rz = np.array([[np.cos(a[2]), -np.sin(a[2]), 0], [np.sin(a[2]), np.cos(a[2]), 0], [0, 0, 1]])
            R[s] = np.dot(Rz, np.dot(Ry, Rx)).reshape(9)
        return (_table(call, 1.0, R, 1.0, float(self.normals and call.feat is not None)),)


class RandomScale(Transform):
    code, writes = "scale", "c"

    def __init__(self, scale_low=0.8, scale_high=1.2):
        self.scale_low, self.scale_high = scale_low, scale_high

    def _draw(self, call):
        return {"scale": call.rng.uniform(self.scale_low, self.scale_high, call.b)}

    def _params(self, call, rec):
        return (_table(call, 1.0, call.host(rec, "scale")),)


class RandomShift(Transform):
    code, writes = "shift", "c"

    def __init__(self, shift_range=0.1):
        self.shift_range = shift_range

    def _draw(self, call):
        return {"shift": call.rng.uniform(-self.shift_range, self.shift_range, (call.b, 3))}

    def _params(self, call, rec):
        return (_table(call, 1.0, call.host(rec, "shift", (3,))),)


class RandomJitter(Transform):
    code, writes = "jitter", "c"

    def __init__(self, sigma=0.01, clip=0.05):
        if not clip > 0:
            raise ValueError("RandomJitter: clip must be positive")
        self.sigma, self.clip = sigma, clip

    def _draw(self, call):
        return {"noise": call.randn((call.n, 3), torch.float64)}

    def _params(self, call, rec):
        z = call.noise_rows(rec)
        return _table(call, 1.0, self.sigma, self.clip), z.data_ptr(), 0, [z]


class RandomDropColor(Transform):
    code, writes = "feat_mul", "f"

    def __init__(self, p=0.8, color_augment=0.0):
        self.p, self.color_augment = p, color_augment

    def _draw(self, call):
        return {} if call.feat is None else {"u": call.rng.random(call.b)}   # (the reference draws nothing without colours)

    def _params(self, call, rec):
        on = call.host(rec, "u") > self.p if call.feat is not None else np.zeros(call.b)
        return (_table(call, on, self.color_augment),)


class RandomHorizontalFlip(Transform):
    code, needs, writes = "flip", "c", "c"

    def __init__(self, upright_axis="z", is_temporal=False):
        if is_temporal:
            raise ValueError("RandomHorizontalFlip: is_temporal flips are not supported")
        if str(upright_axis).lower() not in ("x", "y", "z"):
            raise ValueError("RandomHorizontalFlip: upright_axis must be 'x', 'y' or 'z'")
        self.upright_axis = {"x": 0, "y": 1, "z": 2}[upright_axis.lower()]
        self.horz_axes = sorted(set(range(3)) - {self.upright_axis})

    def _draw(self, call):
        return {"gate": call.rng.random(call.b), "axes": call.rng.random((call.b, 2))}

    def _params(self, call, rec):
        flags = np.zeros((call.b, 3))
        flags[:, self.horz_axes] = call.host(rec, "axes", (2,)) < 0.5
        return (_table(call, call.host(rec, "gate") < 0.95, flags),)


class _Chromatic(Transform):
    writes = "f"

    def _emit(self, call, tape, rec):
        if call is not None and call.feat is None:
            raise ValueError(f"{type(self).__name__} needs feat")
        super()._emit(call, tape, rec)


class ChromaticAutoContrast(_Chromatic):
    code, needs = "autocontrast", "f"

    def __init__(self, randomize_blend_factor=True, blend_factor=0.5):
        self.randomize_blend_factor, self.blend_factor = randomize_blend_factor, blend_factor

    def _draw(self, call):
        return {"gate": call.rng.random(call.b), "blend": call.rng.random(call.b)}

    def _params(self, call, rec):
        blend = call.host(rec, "blend") if self.randomize_blend_factor else self.blend_factor
        return (_table(call, call.host(rec, "gate") < 0.2, blend),)


class ChromaticTranslation(_Chromatic):
    code = "chroma_translate"

    def __init__(self, trans_range_ratio=1e-1):
        self.trans_range_ratio = trans_range_ratio

    def _draw(self, call):
        return {"gate": call.rng.random(call.b), "u": call.rng.random((call.b, 3))}

    def _params(self, call, rec):
        tr = (call.host(rec, "u", (3,)) - 0.5) * 255 * 2 * self.trans_range_ratio
        return (_table(call, call.host(rec, "gate") < 0.95, tr),)


class ChromaticJitter(_Chromatic):
    code = "chroma_jitter"

    def __init__(self, std=0.01):
        self.std = std

    def _draw(self, call):
        return {"gate": call.rng.random(call.b), "noise": call.randn((call.n, 3), torch.float64)}

    def _params(self, call, rec):
        z = call.noise_rows(rec)
        return _table(call, call.host(rec, "gate") < 0.95, self.std * 255), z.data_ptr(), 0, [z]


class HueSaturationTranslation(_Chromatic):
    code = "hue_saturation"

    def __init__(self, hue_max, saturation_max):
        self.hue_max, self.saturation_max = hue_max, saturation_max

    def _draw(self, call):
        return {"hue_u": call.rng.random(call.b), "sat_u": call.rng.random(call.b)}

    def _params(self, call, rec):
        hue_val = (call.host(rec, "hue_u") - 0.5) * 2 * self.hue_max
        sat_ratio = 1 + (call.host(rec, "sat_u") - 0.5) * 2 * self.saturation_max
        return (_table(call, 1.0, hue_val, sat_ratio),)


class ElasticDistortion(Transform):
    """distortion_params: [(granularity, magnitude), ...] or None.  One host read-back of the per-scene coordinate extrema per entry
    (whatever the number of scenes): the noise grid's size depends on them."""

    def __init__(self, distortion_params):
        self.distortion_params = None if distortion_params is None else [(float(g), float(m)) for g, m in distortion_params]
        if any(not g > 0 for g, _ in self.distortion_params or []):
            raise ValueError("ElasticDistortion: a granularity must be positive")

    def _draw(self, call):
        return {"gate": call.rng.random(call.b)}                  # (the grids are drawn once their sizes are known: _entry)

    def _emit(self, call, tape, rec):
        for j, (granularity, magnitude) in enumerate(self.distortion_params or []):
            tape.require("c")
            table = tape.readback()
            if call is None:
                tape.add("elastic", "c")
                continue
            tape.add("elastic", "c", *self._entry(call, rec, j, granularity, magnitude, table))

    def _entry(self, call, rec, j, granularity, magnitude, table):
        lo, hi, nan_bits, empty = table
        on = (call.host(rec, "gate") < 0.95) & ~empty
        if np.any(nan_bits[on] & 7):
            raise ValueError("ElasticDistortion: a coordinate is NaN")
        if not np.all(np.isfinite(lo[on, :3])) or not np.all(np.isfinite(hi[on, :3])):
            raise ValueError("ElasticDistortion: a coordinate is infinite")
        noise = rec.setdefault("noise", [])                      # (a replayed record may hold host draws only: grids are drawn here)
        while len(noise) <= j:
            noise.append([None] * call.b)
        params = np.zeros((call.b, 7))
        grids, axes, desc, n_values, n_axis = [], [], [], 0, 0
        for s in np.nonzero(on)[0]:
            low = lo[s, :3]
            dim = np.floor_divide(hi[s, :3] - low, granularity).astype(np.int64) + 3
            values = int(dim[0]) * int(dim[1]) * int(dim[2]) * 3
            if n_values + values > MAX_GRID_VALUES:
                raise ValueError(f"ElasticDistortion: noise grids of more than {MAX_GRID_VALUES} values (granularity {granularity})")
            shape = tuple(int(d) for d in dim) + (3,)
            if noise[j][s] is None:
                noise[j][s] = call.randn(shape, torch.float32)
            g = noise[j][s]
            if not isinstance(g, torch.Tensor) or tuple(g.shape) != shape or g.dtype != torch.float32 or g.device != call.device:
                raise ValueError(f"ElasticDistortion: the replayed noise of scene {s}, entry {j} must be a float32 tensor {shape}")
            grids.append(g.contiguous().reshape(-1))
            axes += [np.linspace(a, b, n) for a, b, n in zip(low - granularity, low + granularity * (dim - 2), dim)]
            desc.append((n_values, dim[0], dim[1], dim[2]))
            params[s] = (1.0, magnitude, n_values, dim[0], dim[1], dim[2], n_axis)
            n_values, n_axis = n_values + values, n_axis + int(dim.sum())
        if not grids:
            return (params,)
        a = torch.cat(grids)
        b = torch.empty_like(a)
        host = np.concatenate([np.asarray(desc, dtype=np.int64).reshape(-1), np.concatenate(axes).view(np.int64)])
        dev = torch.from_numpy(host).to(call.device)
        for _ in range(2):
            for axis in range(3):
                _lib.call("pointops2_augment_blur_launcher", n_values, len(desc), axis, dev.data_ptr(), a.data_ptr(), b.data_ptr(),
                          device=call.device)
                a, b = b, a
        self.last_blurred = (a, desc)
        return params, a.data_ptr(), dev.data_ptr() + 8 * 4 * len(desc), [a, b, dev]
