"""Clouds for the exact furthest point sampling (csrc/sampling.hip, csrc/fps_bucket.hip, csrc/fps_lazy.hip): one case per kernel
path, size boundary, request length and degenerate geometry.  numpy only, except that the verified-prefix family asks the CPU
oracle for a selection order (an FPS-ordered cloud IS an oracle output).  tests/test_fps_cases_cpu.py proves the cases are what
they claim and pins the constants below to the sources; tests/test_fps_hip.py runs them.

The launcher picks its kernels from the LARGEST cloud of the batch (n), from whether a workspace was lent, whether the call
resumes an earlier one, and the process-wide switch P2_FPS_STEPWISE (furthestsampling_cuda_launcher, fps_bucket_launch,
fps_lazy_groups, fps_lazy_launch); `dispatch` below restates it:

    no workspace, or n < 2048        n <= 4096             fps_block_kernel<256>      the single-workgroup scan
                                     n >  4096             fps_block_kernel<1024>
    workspace and n >= 2048          BSZ = 64 * ceil(n / (64 * FPS_MAX_BUCKETS)):  64 to 131072 points, 128 to 262144, 192 ...
                                     NBL = buckets per lane = ceil(ceil(n / BSZ) / (FPS_NW * 64)):  1 to 65536 points, then 2
      step by step                   fps_bucket_kernel<NBL,16,BSZ == 64>
      in rounds                      G workgroups per cloud: ceil(n / 64) buckets, 100 per workgroup, rounded up to 1 2 4 8 16
                                       n <=   6400  G = 1      n <=  25600  G = 4      n <= 229376  G = 16
                                       n <=  12800  G = 2      n <=  51200  G = 8      n >  229376  G = 0: no rounds
                                     register slots per wave = ceil(ceil(ceil(n / 64) / G) / LZ_NW):
                                       <= 8 (n <= 131072)  fps_lazy_kernel<8>        else  fps_lazy_kernel<LZ_NSLOT>
    which of the two:                P2_FPS_STEPWISE set, or G == 0     step by step, the whole request (resume included)
                                     otherwise                          rounds; on a FRESH chain with n >= 8192 the first
                                                                        FPS_HEAD samples are taken step by step before them (the head)
    in front of either (not restated: they run on every workspace call): bbox, Morton keys, radix sort, gather on a fresh chain;
    the identity-prefix verification (probe of steps 1..63, then 256-sample tiles) unless the cloud carries the unordered hint.

`dispatch` returns G = None for the block kernels, G = 0 where the step-by-step kernel serves the whole request.

Families (CASES: name -> Case; every cloud is finite - the model never produces a non-finite coordinate and the round sampler's
workgroups wait for each other, so non-finite input is deliberately left out):

    size-*          both sides of every dispatch boundary, a room-style cloud (the n + 1 cloud is the n cloud plus a point);
                    above 131072 also a permuted integer lattice (-lattice), above 229376 a two-call resume (-resume), and one
                    ragged batch next to a 131073-point cloud (-ragged)
    bref-*          n = 2^k - 1, 2^k, 2^k + 1 (k = 1..11) on a permuted integer lattice, sampled to exhaustion: ties decide, and the
                    tie rule depends on ref_block_size(n); -plain: through the option-free launcher (block kernels)
    req-*           request lengths around the head on an 8192- and a 20000-point cloud, resumes, 0 / 1 samples in a batch
    degen-*         planar, collinear, coincident, the 1e10 clamp, 2^-70 and 2^40 scales, a translated 2^-8 grid, triplicates
    prefix-*        FPS-ordered clouds whose order breaks at a stated step, each with and without the unordered hint (-hint)
    many-*          130 clouds at G = 1: two launches of the round sampler
"""
import math
from collections import namedtuple

import numpy as np

# ---- the constants the dispatch rests on (tests/test_fps_cases_cpu.py reads them out of the sources) --------------------------
BUCKET_MIN_N = 2048          # sampling.hip: the bucketed path takes clouds from this size
BLOCK_1024_ABOVE = 4096      # sampling.hip: fps_block_kernel<1024> above this size
FPS_MAX_BUCKETS = 2048       # fps_bucket.hip
FPS_NW = 16                  # fps_bucket.hip: waves of the step-by-step kernel
FPS_HEAD = 256               # fps_bucket.hip: samples of the head
HEAD_MIN_N = 8192            # fps_bucket.hip: the head runs from this size
LZ_NW = 16                   # fps_lazy.hip
LZ_NSLOT = 14                # fps_common.h
LZ_GMAX = 16                 # fps_common.h
LZ_CAP = 512                 # fps_common.h
LZ_BUCKETS_PER_GROUP = 100   # fps_lazy.hip (fps_lazy_groups)
LZ_SMALL_SLOTS = 8           # fps_lazy.hip (fps_lazy_launch): fps_lazy_kernel<8> up to this many slots
LZ_CHUNK = 128               # fps_lazy.hip (fps_lazy_launch): workgroups of one launch, at most
DMAX = np.float32(1e10)      # the running minimum's start value (pointops.py:26): 2^10 * 5^10, exact in fp32

BLOCK256, BLOCK1024 = "fps_block_kernel<256>", "fps_block_kernel<1024>"
LAZY8, LAZYN = "fps_lazy_kernel<8>", "fps_lazy_kernel<LZ_NSLOT>"
ALL_KERNELS = (BLOCK256, BLOCK1024, "fps_bucket_kernel<1,16,true>", "fps_bucket_kernel<2,16,true>", "fps_bucket_kernel<2,16,false>",
               LAZY8, LAZYN)

Dispatch = namedtuple("Dispatch", "kernels G BSZ head")


def _div_up(a, b):
    return (a + b - 1) // b


def lazy_groups(n):
    nb, cap = _div_up(n, 64), LZ_NW * LZ_NSLOT
    need = _div_up(nb, cap)
    if need > LZ_GMAX:
        return 0
    g = max(max(need, 1), min(_div_up(nb, LZ_BUCKETS_PER_GROUP), LZ_GMAX))
    while g < LZ_GMAX and (LZ_NW * 64) % g != 0:
        g += 1
    return g


def dispatch(n_max, workspace=True, resumed=False, stepwise=False):
    """what one launcher call runs for a batch whose largest cloud has n_max points"""
    if not workspace or n_max < BUCKET_MIN_N:
        return Dispatch((BLOCK1024 if n_max > BLOCK_1024_ABOVE else BLOCK256,), None, None, False)
    bsz = 64 * _div_up(n_max, 64 * FPS_MAX_BUCKETS)
    nbl = 1 if _div_up(_div_up(n_max, bsz), FPS_NW * 64) <= 1 else 2
    bucket = "fps_bucket_kernel<%d,%d,%s>" % (nbl, FPS_NW, "true" if bsz == 64 else "false")
    g = 0 if stepwise else lazy_groups(n_max)
    if g == 0:
        return Dispatch((bucket,), 0, bsz, False)
    head = not resumed and n_max >= HEAD_MIN_N
    slots = _div_up(_div_up(_div_up(n_max, 64), g), LZ_NW)
    lazy = LAZY8 if slots <= LZ_SMALL_SLOTS else LAZYN
    return Dispatch(((bucket, lazy) if head else (lazy,)), g, bsz, head)


def ref_block_size(n):
    """cuda_utils.h:10-13 as sampling.hip restates it: the double-precision log quotient decides the tie rule"""
    if n < 1:
        return 1
    return max(min(1 << int(math.log(float(n)) / math.log(2.0)), 1024), 1)


# (lo | lo + 1): the dispatch differs between a cloud of lo and one of lo + 1 points
BOUNDARIES = (2047, 6400, 8191, 12800, 25600, 51200, 65536, 131072, 229376, 262144)

# name; family; xyz [n, 3] f32; offset [b] i32; requests: the new_offset arrays of the chain's calls (one: a fresh call; two: the
# second resumes the first); hint: the cloud carries the unordered hint; plain: through the option-free launcher (no workspace);
# exact: float64 evaluates every distance of the cloud exactly (integer or 2^-8-grid coordinates, or all points coincident);
# breaks: verified-prefix family, per batch element the step at which the selection order first breaks (None: never)
Case = namedtuple("Case", "name family xyz offset requests hint plain exact breaks")


def _case(name, family, xyz, sizes, requests, hint=False, plain=False, exact=False, breaks=None):
    xyz = np.ascontiguousarray(xyz, np.float32)
    offset = np.cumsum(sizes).astype(np.int32)
    assert offset[-1] == len(xyz) and np.isfinite(xyz).all()
    reqs = tuple(np.cumsum(r).astype(np.int32) for r in requests)
    assert all(len(r) == len(offset) for r in reqs)
    xyz.setflags(write=False)
    return Case(name, family, xyz, offset, reqs, hint, plain, exact, breaks)


def n_max_of(case):
    return int(np.diff(case.offset, prepend=0).max())


def dispatch_of(case, call=0, stepwise=False):
    return dispatch(n_max_of(case), workspace=not case.plain, resumed=call > 0, stepwise=stepwise)


# ---- clouds ----------------------------------------------------------------------------------------------------------------------
def room(n, seed):
    """a scanned room in small: points on the six faces of a 7 x 5.5 x 2.8 box (by area) with 2 cm of noise - surfaces, like the
    workload's clouds, and no exact ties"""
    rng = np.random.default_rng(seed)
    dims = np.array([7.0, 5.5, 2.8])
    area = np.array([dims[1] * dims[2], dims[0] * dims[2], dims[0] * dims[1]])
    axis = rng.choice(3, n, p=area / area.sum())
    pts = rng.random((n, 3)) * dims
    pts[np.arange(n), axis] = dims[axis] * rng.integers(0, 2, n)
    return (pts + rng.normal(0, 0.02, pts.shape)).astype(np.float32)


def lattice(dims, n, seed):
    """the integer lattice dims[0] x dims[1] x dims[2] in random index order, cut to its first n points: exact ties everywhere"""
    g = np.stack(np.meshgrid(*(np.arange(d) for d in dims), indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    assert len(g) >= n
    return g[np.random.default_rng(seed).permutation(len(g))[:n]]


def _m_of(n):
    return 700 if n >= 8192 else n // 4 + 1


LATTICE_DIMS = {131073: (66, 64, 32), 229376: (72, 64, 50), 229377: (72, 64, 50), 262144: (66, 64, 63), 262145: (66, 64, 63)}


def _size_cases():
    out = []
    for i, lo in enumerate(BOUNDARIES):
        cloud = room(lo + 1, 100 + i)
        for n in (lo, lo + 1):
            out.append(_case(f"size-{n}", "size", cloud[:n], [n], [[_m_of(n)]]))
            if n > 131072:
                out.append(_case(f"size-{n}-lattice", "size", lattice(LATTICE_DIMS[n], n, 200 + i), [n], [[700]], exact=True))
        if lo + 1 in (229377, 262145):
            out.append(_case(f"size-{lo + 1}-resume", "size", cloud, [lo + 1], [[300], [700]]))
    sizes = [131073, 40, 2048, 9000]   # the small clouds run with the large one's BSZ = 128 and G = 16
    xyz = np.concatenate([room(n, 120 + i) for i, n in enumerate(sizes)])
    out.append(_case("size-131073-ragged", "size", xyz, sizes, [[_m_of(n) for n in sizes]]))
    return out


BREF_SIZES = tuple(sorted({(1 << k) + d for k in range(1, 12) for d in (-1, 0, 1)}))   # 1 ... 2049
BREF_PLAIN_SIZES = (2048, 4096, 4097)


def _tight_dims(n):
    """the smallest s x s x c block that holds n points: the cut removes fewer than s * s of them, the lattice stays dense"""
    s = 1
    while s * s * s < n:
        s += 1
    return (s, s, _div_up(n, s * s))


def _bref_cases():
    out = []
    for n in BREF_SIZES:
        out.append(_case(f"bref-{n}", "bref", lattice(_tight_dims(n), n, 300 + n), [n], [[n]], exact=True))
    out.append(_case("bref-1-m3", "bref", lattice((1, 1, 1), 1, 301), [1], [[3]], exact=True))
    for n in BREF_PLAIN_SIZES:
        out.append(_case(f"bref-{n}-plain", "bref", lattice(_tight_dims(n), n, 310 + n), [n], [[n]], plain=True, exact=True))
    return out


REQ_SIZES = (8192, 20000)
REQ_LENGTHS = (1, 2, 255, 256, 257)
REQ_RESUMES = ((1, 600), (255, 600), (256, 600), (257, 258))


def _req_cases():
    out = []
    clouds = {n: room(n, 400 + n) for n in REQ_SIZES}
    for n, cloud in clouds.items():
        for m in REQ_LENGTHS + (n + 9,):
            out.append(_case(f"req-{n}-m{m}", "req", cloud, [n], [[m]]))
        for a, b in REQ_RESUMES:
            out.append(_case(f"req-{n}-resume{a}to{b}", "req", cloud, [n], [[a], [b]]))
    both = np.concatenate([clouds[8192], clouds[20000]])
    out.append(_case("req-batch-0-1", "req", both, list(REQ_SIZES), [[0, 1]]))
    # (the element that asks for nothing is never the last one: the reference writes every element's first slot)
    out.append(_case("req-batch-1-0-1", "req", np.concatenate([both, clouds[8192]]), [8192, 20000, 8192], [[1, 0, 1]]))
    return out


DEGEN_SIZES = (2048, 8192)
TRANSLATIONS = (0, 64, 1024, 16384)
CLAMP_EXTENT = np.float32(3e5)   # squared: 9e10 > 1e10, the running minimum's start value


def _degen_cases():
    out = []
    for n in DEGEN_SIZES:
        rng = np.random.default_rng(500 + n)
        base = rng.random((n, 3), dtype=np.float32)
        add = lambda name, xyz, m=600, size=n, **kw: out.append(_case(f"degen-{name}-{size}", "degen", xyz, [size], [[m]], **kw))
        planar = base.copy()
        planar[:, 2] = np.float32(0.375)
        add("planar", planar)
        line = base.copy()
        line[:, 1], line[:, 2] = np.float32(0.25), np.float32(-0.5)
        add("collinear", line)
        add("coincident", np.tile(np.array([0.3, -1.2, 2.5], np.float32), (n, 1)), m=70, exact=True)
        far = base.copy()
        far[n // 2:, 0] += CLAMP_EXTENT
        add("clusters3e5", far)
        add("extent3e5", base * CLAMP_EXTENT)
        add("scale2m70", base * np.float32(2.0 ** -70))
        add("scale2p40", base * np.float32(2.0 ** 40))
        # integers 0..39 per axis, in units of 2^-8: with T + 40/256 < 2^15 every translated coordinate, every difference
        # (the untranslated one) and every squared distance (a multiple of 2^-16 below 3 * 40^2 * 2^-16) is exact in fp32
        grid = rng.integers(0, 40, (n, 3)).astype(np.float32) / np.float32(256)
        for T in TRANSLATIONS:
            add(f"translate{T}", grid + np.float32(T), exact=True)
        # every point three times: n is no multiple of 3, so 683 / 2731 points -> 2049 / 8193 (the same dispatch rows)
        third = _div_up(n, 3)
        tri = np.tile(grid[:third] * np.float32(16), (3, 1))[rng.permutation(3 * third)]
        add("triple", tri, size=3 * third, exact=True)
    return out


PREFIX_N, PREFIX_BREAKS = 2304, (1, 2, 63, 64, 65, 255, 256, 257, 2303, None)


def _ordered(cloud, m):
    """the oracle's first m samples of `cloud`, kept in selection order"""
    from oracle import pointops_ref as ref
    order = ref.furthestsampling(cloud, np.array([len(cloud)], np.int32), np.array([m], np.int32))
    return np.ascontiguousarray(cloud[order])


def break_at(sub, j):
    """`sub` is in selection order; the copy's order first breaks at step j.  Swapping points j and j + 37 leaves steps 0..j-1
    alone (they see the same selected points and the same candidates) and moves step j's winner to index j + 37.  The LAST step
    of an exhaustive request cannot be broken by a swap - one point is left - so there the last point becomes a copy of point 5:
    every running minimum is 0 at that step and the tie rule, not the order, picks the sample."""
    out = sub.copy()
    if j is None:
        return out
    if j == len(sub) - 1:
        out[j] = out[5]
    else:
        k = min(j + 37, len(sub) - 1)
        out[[j, k]] = out[[k, j]]
    return out


def _prefix_cases():
    sub = _ordered(room(9000, 600), PREFIX_N)
    specs = [(f"prefix-break{j}", break_at(sub, j), [PREFIX_N], [[PREFIX_N]], (j,)) for j in PREFIX_BREAKS]
    trio = (2, 256, None)
    specs.append(("prefix-batch3", np.concatenate([break_at(sub, j) for j in trio]), [PREFIX_N] * 3, [[PREFIX_N] * 3], trio))
    lat = lattice((16, 16, 12), 3072, 601)
    specs.append(("prefix-lattice", _ordered(lat, 3072), [3072], [[1000]], None))
    full = _ordered(room(9000, 602), 9000)   # verification, head and rounds meet: n >= 8192, the order breaks inside / after the head
    for j in (100, 300):
        specs.append((f"prefix-9000-break{j}", break_at(full, j), [9000], [[1200]], (j,)))
    out = []
    for name, xyz, sizes, reqs, breaks in specs:
        for hint in (False, True):
            out.append(_case(name + ("-hint" if hint else ""), "prefix", xyz, sizes, reqs, hint=hint, exact=name == "prefix-lattice", breaks=breaks))
    return out


MANY_SIZES = tuple(2048 + (i * 7) % 53 for i in range(130))   # 2048 ... 2100


def _many_cases():
    xyz = np.concatenate([room(n, 700 + i) for i, n in enumerate(MANY_SIZES)])
    sizes, reqs = list(MANY_SIZES), [40] * len(MANY_SIZES)
    out = [_case("many-130", "many", xyz, sizes, [reqs])]
    sizes2, reqs2 = sizes[:65] + [0] + sizes[65:], reqs[:65] + [0] + reqs[65:]   # an empty element in the middle, asking for nothing
    out.append(_case("many-130-empty", "many", xyz, sizes2, [reqs2]))
    return out


def _build_all():
    cases = _size_cases() + _bref_cases() + _req_cases() + _degen_cases() + _prefix_cases() + _many_cases()
    out = {c.name: c for c in cases}
    assert len(out) == len(cases)
    return out


CASES = _build_all()

# what the P2_FPS_STEPWISE child of tests/test_fps_hip.py runs: the sizes at which the switch changes the dispatch
STEPWISE_CASES = tuple(["size-2048", "size-8192", "size-65537", "size-131073", "size-131073-lattice", "size-229376-lattice"]
                       + [f"req-{n}-resume{a}to600" for n in REQ_SIZES for a in (1, 256)]
                       + sorted(n for n in CASES if n.startswith("prefix-")))


# ---- a second statement of the selection rule (for the clouds float64 evaluates exactly) --------------------------------------
def tie_rank(n, n_max):
    """low word of the 64-bit key of sampling.hip's header for points 0..n-1 of a cloud in a batch whose largest cloud has n_max
    points: 0x7fffffff - (bitrev(rel mod B) << 21 | rel div B), B = ref_block_size(n_max)"""
    B = ref_block_size(n_max)
    log2b = B.bit_length() - 1
    rel = np.arange(n, dtype=np.uint64)
    tref, brev = rel & np.uint64(B - 1), np.zeros(n, np.uint64)
    for bit in range(log2b):
        brev |= ((tref >> np.uint64(bit)) & np.uint64(1)) << np.uint64(log2b - 1 - bit)
    return np.uint64(0x7fffffff) - ((brev << np.uint64(21)) | (rel >> np.uint64(log2b)))


def key_fps(xyz, offset, new_offset, limit=None):
    """FPS by the maximum of the 64-bit key (distance bits, then bit-reversed `rel mod B`, then `rel div B`), distances in
    float64.  -> (idx, tied, exact): tied[j] = how many points shared the largest running minimum when sample j was chosen;
    exact = every float64 distance was representable in fp32 (then it IS the fp32 fma chain's value: no rounding happened in
    either).  limit: at most this many samples per element."""
    offset, new_offset = np.asarray(offset, np.int64), np.asarray(new_offset, np.int64)
    n_max = int(np.diff(offset, prepend=0).max())
    idx, tied, exact = [], [], True
    lo, mlo = 0, 0
    for hi, mhi in zip(offset, new_offset):
        n, m = int(hi - lo), int(mhi - mlo)
        if limit is not None:
            m = min(m, limit)
        if m > 0:
            pts = xyz[lo:hi].astype(np.float64)
            low = tie_rank(n, n_max)
            d = np.full(n, float(DMAX))
            old = 0
            idx.append(lo)
            tied.append(1)
            for _ in range(1, m):
                dx, dy, dz = (pts - pts[old]).T
                d2 = dz * dz + (dx * dx + dy * dy)
                d = np.minimum(d, d2)
                d32 = d.astype(np.float32)
                exact = exact and bool((d32.astype(np.float64) == d).all())
                key = (d32.view(np.uint32).astype(np.uint64) << np.uint64(32)) | low
                old = int(np.argmax(key))
                idx.append(lo + old)
                tied.append(int((d32 == d32[old]).sum()))
        lo, mlo = int(hi), int(mhi)
    return np.asarray(idx, np.int32), np.asarray(tied), exact
