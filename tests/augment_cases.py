"""The transform cases shared by the augmentation fixture (tests/golden/make_golden_augment.py), the oracle test and the device
test: which class with which arguments, on which input, and which `random.random()` / argument-less `np.random.rand()` values
the fixture forced so that every gate is seen open and shut.  Plain data and small helpers; nothing of the reference."""
import numpy as np

S3DIS_CHAIN = [
    ("RandomRotate", dict(along_z=True)),
    ("RandomScale", dict(scale_low=0.8, scale_high=1.2)),
    ("RandomJitter", dict(sigma=0.005, clip=0.02)),
    ("RandomDropColor", dict(color_augment=0.0)),
]
ELASTIC_PARAMS = [[0.2, 0.4], [0.8, 1.6]]
FULL_CHAIN = [
    ("ElasticDistortion", dict(distortion_params=ELASTIC_PARAMS)),
    ("RandomHorizontalFlip", dict(upright_axis="z")),
    ("RandomRotate", dict(along_z=True)),
    ("RandomScale", dict(scale_low=0.8, scale_high=1.2)),
    ("ChromaticAutoContrast", dict()),
    ("ChromaticTranslation", dict(trans_range_ratio=0.1)),
    ("ChromaticJitter", dict(std=0.05)),
    ("HueSaturationTranslation", dict(hue_max=0.5, saturation_max=0.2)),
]

# (case, class, arguments, input, forced gate values)
SINGLE = [
    ("rotate_z", "RandomRotate", dict(), "base", []),
    ("rotate_y_color", "RandomRotate", dict(along_z=False, color_rotate=True), "base", []),
    ("rotate_fixed", "RandomRotate", dict(rotate_angle=90), "base", []),
    ("perturb", "RandomRotatePerturbation", dict(), "base", []),
    ("perturb_normals", "RandomRotatePerturbation", dict(angle_sigma=0.2, angle_clip=0.18, normals=True), "base", []),
    ("scale", "RandomScale", dict(), "base", []),
    ("shift", "RandomShift", dict(shift_range=0.2), "base", []),
    ("jitter", "RandomJitter", dict(sigma=0.01, clip=0.015), "base", []),
    ("drop_on", "RandomDropColor", dict(p=0.8, color_augment=0.0), "base", [0.9]),
    ("drop_half", "RandomDropColor", dict(p=0.5, color_augment=0.5), "base", [0.7]),
    ("drop_off", "RandomDropColor", dict(), "base", [0.3]),
    ("elastic", "ElasticDistortion", dict(distortion_params=ELASTIC_PARAMS), "base", [0.5]),
    ("elastic_off", "ElasticDistortion", dict(distortion_params=ELASTIC_PARAMS), "base", [0.97]),
    ("flip_xy", "RandomHorizontalFlip", dict(upright_axis="z"), "base", [0.5, 0.1, 0.2]),
    ("flip_y", "RandomHorizontalFlip", dict(upright_axis="z"), "base", [0.5, 0.9, 0.2]),
    ("flip_upright_x", "RandomHorizontalFlip", dict(upright_axis="x"), "base", [0.1, 0.3, 0.7]),
    ("flip_off", "RandomHorizontalFlip", dict(upright_axis="z"), "base", [0.99]),
    ("contrast_on", "ChromaticAutoContrast", dict(), "narrow", [0.1, 0.37]),
    ("contrast_fixed", "ChromaticAutoContrast", dict(randomize_blend_factor=False, blend_factor=0.25), "narrow", [0.05]),
    ("contrast_off", "ChromaticAutoContrast", dict(), "narrow", [0.5]),
    ("contrast_const", "ChromaticAutoContrast", dict(), "const", [0.1, 0.6]),
    ("translate_on", "ChromaticTranslation", dict(trans_range_ratio=0.1), "base", [0.3]),
    ("translate_off", "ChromaticTranslation", dict(trans_range_ratio=0.1), "narrow", [0.96]),
    ("cjitter_on", "ChromaticJitter", dict(std=0.05), "narrow", [0.3]),
    ("cjitter_off", "ChromaticJitter", dict(std=0.05), "narrow", [0.99]),
    ("huesat", "HueSaturationTranslation", dict(hue_max=0.5, saturation_max=0.2), "base", []),
    ("huesat_wide", "HueSaturationTranslation", dict(hue_max=1.0, saturation_max=1.0), "base", [0.93, 0.08]),
]
# per scene of the three-scene batch: the forced gate values of the two chains
CHAINS = {
    "s3dis": (S3DIS_CHAIN, [[0.9], [0.3], [0.85]]),
    "full": (FULL_CHAIN, [[0.5, 0.5, 0.1, 0.2, 0.1, 0.6, 0.5, 0.5],
                          [0.97, 0.99, 0.5, 0.97, 0.5],
                          [0.2, 0.3, 0.8, 0.3, 0.15, 0.9, 0.2, 0.99]]),
}
BATCH_SIZES = (150, 250, 200)
ELEMENTWISE = {"RandomScale", "RandomShift", "RandomJitter", "RandomDropColor", "RandomHorizontalFlip", "ChromaticAutoContrast",
               "ChromaticTranslation", "ChromaticJitter", "HueSaturationTranslation"}
ROTATIONS = {"RandomRotate", "RandomRotatePerturbation"}


def cloud(n, seed):
    """a small room-like float64 cloud away from the origin, colours as feat = c / 127.5 - 1 with grey, black and white points"""
    if n < 16:
        xyz, feat = cloud(16, seed)
        return np.ascontiguousarray(xyz[:n]), np.ascontiguousarray(feat[:n])
    rng = np.random.default_rng(seed)
    xyz = rng.random((n, 3)) * np.array([2.4, 1.8, 1.2])
    which = rng.integers(0, 4, n)
    xyz[which == 0, 2] = 0.0
    xyz[which == 1, 0] = 0.0
    xyz += rng.normal(0, 0.004, (n, 3)) + np.array([3.0, -2.0, 0.5])
    rgb = rng.integers(0, 256, (n, 3)).astype(np.float64)
    k = n // 10
    rgb[:k] = rgb[:k, :1]          # grey
    rgb[k:k + 3] = 0.0             # black
    rgb[k + 3:k + 6] = 255.0       # white
    rgb[k + 6] = (255.0, 0.0, 0.0)
    rgb[k + 7] = (0.0, 255.0, 0.0)
    rgb[k + 8] = (0.0, 0.0, 255.0)
    return np.ascontiguousarray(xyz), np.ascontiguousarray(rgb / 127.5 - 1)


def narrow(feat):
    """colours that fill neither end of the range (auto-contrast then changes them) and do not convert to 0..255 and back exactly"""
    return feat * 0.8 - 0.1


def build(module, chain):
    """instances of `module`'s classes for [(class name, arguments)]"""
    return [getattr(module, name)(**kw) for name, kw in chain]


def scene_draws(records, s, lo, hi):
    """the oracle's draw dicts for scene s (rows lo:hi) out of the records of a device call (augment.Draws.records)"""
    out = []
    for rec in records:
        d = {}
        for k, v in rec.items():
            if k == "noise" and isinstance(v, list):          # elastic: per entry, one grid per scene
                d[k] = [e[s].cpu().numpy() for e in v if e[s] is not None]
            elif hasattr(v, "cpu"):                             # per-point noise
                d[k] = v[lo:hi].cpu().numpy()
            else:
                d[k] = np.asarray(v)[s]
        out.append(d)
    return out


def same_bits(got, want):
    """equal bit for bit outside NaNs, NaNs at equal positions"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and got[~nan].tobytes() == want[~nan].tobytes())


def load_draws(z, prefix, n_transforms):
    """the draw dicts stored under `prefix`.d<k>.<name>; noise<j> / blur<j> entries are gathered into the lists 'noise' / 'blur'"""
    out = []
    for k in range(n_transforms):
        head = f"{prefix}.d{k}."
        d, lists = {}, {}
        for key in z.files if hasattr(z, "files") else z:
            if not key.startswith(head):
                continue
            name = key[len(head):]
            v = z[key]
            v = v.item() if v.ndim == 0 else v
            for stem in ("noise", "blur"):
                if name.startswith(stem) and name[len(stem):].isdigit():
                    lists.setdefault(stem, {})[int(name[len(stem):])] = v
                    break
            else:
                d[name] = v
        for stem, items in lists.items():
            d[stem] = [items[j] for j in sorted(items)]
        out.append(d)
    return out
