"""CPU: the FPS cases of tests/fps_cases.py are what they claim to be, so that a pass of tests/test_fps_hip.py cannot be hollow.
The constants of the restated dispatch are read out of the sources (a retuned constant fails here instead of silently moving a
case off its boundary), every boundary pair maps to two dispatch results, every kernel instance and workgroup count is reached,
and the C oracle is held against a second statement of the selection rule where float64 evaluates the distances exactly.
No HIP compute runs here."""
import os
import re

import numpy as np
import pytest

from oracle import pointops_ref as ref
from tests import fps_cases as C

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "stratified_transformer_amd", "csrc")
ALL = sorted(C.CASES)
_ORACLE = {}


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _one(pattern, text):
    found = re.findall(pattern, text)
    assert len(found) == 1, (pattern, found)
    return int(found[0])


def _oracle(name, call=-1):
    key = (name, call)
    if key not in _ORACLE:
        c = C.CASES[name]
        _ORACLE[key] = ref.furthestsampling(c.xyz, c.offset, c.requests[call])
        _ORACLE[key].setflags(write=False)
    return _ORACLE[key]


def _sq(a, b):
    """squared distance with the kernels' fma chain, evaluated in fp32 steps (dy*dy rounded, then the two fused adds emulated
    in float64 and rounded once each - exact products of fp32 values fit float64)"""
    d = (np.asarray(b, np.float32) - np.asarray(a, np.float32)).astype(np.float64)
    t = (d[..., 1] * d[..., 1]).astype(np.float32).astype(np.float64)
    t = (d[..., 0] * d[..., 0] + t).astype(np.float32).astype(np.float64)
    return (d[..., 2] * d[..., 2] + t).astype(np.float32)


# ---- constants against the source -----------------------------------------------------------------------------------------------
def test_the_constants_are_the_sources():
    sampling, bucket, lazy, common = _src("sampling.hip"), _src("fps_bucket.hip"), _src("fps_lazy.hip"), _src("fps_common.h")
    assert _one(r"if \(n >= (\d+) && fps_bucket_launch\(", sampling) == C.BUCKET_MIN_N
    assert _one(r"if \(n > (\d+)\)\s*\n\s*hipLaunchKernelGGL\(fps_block_kernel<1024>", sampling) == C.BLOCK_1024_ABOVE
    assert len(re.findall(r"else\s*\n\s*hipLaunchKernelGGL\(fps_block_kernel<256>", sampling)) == 1
    assert _one(r"constexpr int FPS_MAX_BUCKETS = (\d+);", bucket) == C.FPS_MAX_BUCKETS
    assert _one(r"constexpr int FPS_NW = (\d+);", bucket) == C.FPS_NW
    assert _one(r"constexpr int FPS_HEAD = (\d+);", bucket) == C.FPS_HEAD
    assert _one(r"pidx == nullptr && n >= (\d+)\)", bucket) == C.HEAD_MIN_N
    assert _one(r"constexpr int LZ_NW = (\d+);", lazy) == C.LZ_NW
    assert _one(r"constexpr int LZ_NSLOT = (\d+);", common) == C.LZ_NSLOT
    assert _one(r"constexpr int LZ_GMAX = (\d+);", common) == C.LZ_GMAX
    assert _one(r"constexpr int LZ_CAP = (\d+);", common) == C.LZ_CAP
    per = re.findall(r"int G = \(nb \+ (\d+)\) / (\d+);", lazy)
    assert per == [(str(C.LZ_BUCKETS_PER_GROUP - 1), str(C.LZ_BUCKETS_PER_GROUP))], per
    assert _one(r"if \(slots <= (\d+)\) \{", lazy) == C.LZ_SMALL_SLOTS
    assert _one(r"std::min\((\d+), num_cus\(\) / 2\) / G\)", lazy) == C.LZ_CHUNK
    # the formulas the restatement copies, literally
    assert "const int BSZ = 64 * div_up(n, 64 * FPS_MAX_BUCKETS);" in bucket
    assert "const int per_lane = div_up(nbuckets, FPS_NW * 64);" in bucket
    assert "if (per_lane <= 1) fps_stepwise_launch<1>" in bucket and "else fps_stepwise_launch<2>" in bucket
    assert "const int nb = (n_max + 63) / 64, cap = LZ_NW * LZ_NSLOT;" in lazy
    assert "const int slots = div_up(div_up(div_up(n_max, 64), G), LZ_NW);" in lazy
    assert 'getenv("P2_FPS_STEPWISE")' in bucket
    assert "1e10f);  // pointops.py:26" in bucket and float(C.DMAX) == 1e10     # the start value is exact in fp32


def test_every_boundary_pair_maps_to_two_dispatch_results_and_there_are_no_others():
    for lo in C.BOUNDARIES:
        assert C.dispatch(lo) != C.dispatch(lo + 1), lo
        assert f"size-{lo}" in C.CASES and f"size-{lo + 1}" in C.CASES
    prev, steps = C.dispatch(1), []
    for n in range(2, 300001):
        cur = C.dispatch(n)
        if cur != prev:
            steps.append(n - 1)
        prev = cur
    assert tuple(steps) == C.BOUNDARIES
    # the table of the module docstring
    assert [C.lazy_groups(n) for n in (2048, 6400, 6401, 12800, 12801, 25600, 25601, 51200, 51201, 229376, 229377)] == \
        [1, 1, 2, 2, 4, 4, 8, 8, 16, 16, 0]
    assert C.dispatch(2047) == ((C.BLOCK256,), None, None, False)
    assert C.dispatch(2048) == ((C.LAZY8,), 1, 64, False)
    assert C.dispatch(8192) == (("fps_bucket_kernel<1,16,true>", C.LAZY8), 2, 64, True)
    assert C.dispatch(8192, resumed=True) == ((C.LAZY8,), 2, 64, False)
    assert C.dispatch(65537) == (("fps_bucket_kernel<2,16,true>", C.LAZY8), 16, 64, True)
    assert C.dispatch(131073) == (("fps_bucket_kernel<2,16,false>", C.LAZYN), 16, 128, True)
    assert C.dispatch(131073, stepwise=True) == (("fps_bucket_kernel<2,16,false>",), 0, 128, False)
    assert C.dispatch(229377) == (("fps_bucket_kernel<2,16,false>",), 0, 128, False)
    assert C.dispatch(262145) == (("fps_bucket_kernel<2,16,false>",), 0, 192, False)
    assert C.dispatch(4096, workspace=False).kernels == (C.BLOCK256,) and C.dispatch(4097, workspace=False).kernels == (C.BLOCK1024,)


def test_every_kernel_instance_and_every_group_count_is_reached():
    kernels, groups, bsz = set(), set(), set()
    for c in C.CASES.values():
        for call in range(len(c.requests)):
            d = C.dispatch_of(c, call)
            kernels |= set(d.kernels)
            groups.add(d.G)
            bsz.add(d.BSZ)
    assert kernels == set(C.ALL_KERNELS), set(C.ALL_KERNELS) - kernels
    assert groups >= {1, 2, 4, 8, 16, 0}, groups
    assert bsz >= {64, 128, 192}
    # resumed calls on both sides of the round sampler's reach, and the head on and off
    assert C.dispatch_of(C.CASES["size-229377-resume"], 1).kernels == ("fps_bucket_kernel<2,16,false>",)
    for n in C.REQ_SIZES:
        c = C.CASES[f"req-{n}-resume256to600"]
        assert C.dispatch_of(c, 0).head and not C.dispatch_of(c, 1).head
    # the child with P2_FPS_STEPWISE: every case's dispatch differs from the default one, in every instance of the step kernel
    step = set()
    for name in C.STEPWISE_CASES:
        c = C.CASES[name]
        for call in range(len(c.requests)):
            d = C.dispatch_of(c, call, stepwise=True)
            assert d != C.dispatch_of(c, call) and d.G == 0 and len(d.kernels) == 1, name
            step |= set(d.kernels)
    assert step == {"fps_bucket_kernel<1,16,true>", "fps_bucket_kernel<2,16,true>", "fps_bucket_kernel<2,16,false>"}


# ---- cases are what they claim --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_offsets_and_requests_are_consistent(name):
    c = C.CASES[name]
    assert c.xyz.dtype == np.float32 and c.xyz.ndim == 2 and c.xyz.shape[1] == 3 and np.isfinite(c.xyz).all()
    assert c.offset.dtype == np.int32 and c.offset[-1] == len(c.xyz) and (np.diff(c.offset, prepend=0) >= 0).all()
    assert 1 <= len(c.requests) <= 2
    counts = [np.diff(r, prepend=0) for r in c.requests]
    for r, k in zip(c.requests, counts):
        assert r.dtype == np.int32 and len(r) == len(c.offset) and (k >= 0).all()
    sizes = np.diff(c.offset, prepend=0)
    assert counts[-1][-1] > 0 and sizes[-1] > 0     # the oracle writes every element's first slot: the last one must own it
    assert (counts[-1][sizes == 0] == 0).all()      # nothing is asked of an empty element
    if len(counts) == 2:
        assert (counts[1] >= counts[0]).all() and (counts[1] > counts[0]).any()   # a pure extension: the second call resumes


def test_size_cases_sit_on_their_boundaries():
    for lo in C.BOUNDARIES:
        a, b = C.CASES[f"size-{lo}"], C.CASES[f"size-{lo + 1}"]
        assert len(a.xyz) == lo and len(b.xyz) == lo + 1 and np.array_equal(a.xyz, b.xyz[:lo])    # one cloud on both sides
        for c in (a, b):
            m = int(c.requests[0][0])
            assert m == (700 if len(c.xyz) >= 8192 else len(c.xyz) // 4 + 1)
            assert m > C.FPS_HEAD                      # leaves the head and runs rounds
    lat = [n for n in ALL if n.endswith("-lattice") and n.startswith("size-")]
    assert sorted(int(n.split("-")[1]) for n in lat) == [131073, 229376, 229377, 262144, 262145]
    for n in (229377, 262145):
        c = C.CASES[f"size-{n}-resume"]
        assert [int(r[0]) for r in c.requests] == [300, 700]
    rag = C.CASES["size-131073-ragged"]
    assert np.diff(rag.offset, prepend=0).tolist() == [131073, 40, 2048, 9000]
    assert C.dispatch_of(rag).BSZ == 128 and C.dispatch_of(rag).G == 16


@pytest.mark.parametrize("name", [n for n in ALL if n.startswith("size-") and n.endswith("-lattice")])
def test_large_lattices_tie_at_sampled_steps_and_the_oracle_follows_the_key(name):
    """integer coordinates below 128: differences are integers, squared distances integers below 3 * 2^14 - every product and
    sum of the fma chain is exact in fp32 and in float64, so the two are the same number.  First 64 samples."""
    c = C.CASES[name]
    idx, tied, exact = C.key_fps(c.xyz, c.offset, c.requests[-1], limit=64)
    assert exact and np.array_equal(c.xyz, np.round(c.xyz)) and c.xyz.max() < 128
    assert (tied[1:] >= 2).sum() >= 10, tied                          # ten or more of the 63 choices were made among tied maxima
    assert np.array_equal(_oracle(name)[:64], idx)


def test_reference_block_size_family():
    assert C.BREF_SIZES[0] == 1 and C.BREF_SIZES[-1] == 2049 and len(C.BREF_SIZES) == 32
    for k in range(1, 12):
        assert C.ref_block_size((1 << k) - 1) == min(1 << (k - 1), 1024)
        assert C.ref_block_size(1 << k) == min(1 << k, 1024)           # the log quotient did not fall short of k
        assert C.ref_block_size((1 << k) + 1) == min(1 << k, 1024)
        for d in (-1, 0, 1):
            c = C.CASES[f"bref-{(1 << k) + d}"]
            assert len(c.xyz) == (1 << k) + d == int(c.requests[0][0]) and not c.plain
    assert int(C.CASES["bref-1-m3"].requests[0][0]) == 3 and len(C.CASES["bref-1-m3"].xyz) == 1
    assert [C.dispatch_of(C.CASES[f"bref-{n}-plain"]).kernels[0] for n in C.BREF_PLAIN_SIZES] == [C.BLOCK256, C.BLOCK256, C.BLOCK1024]


EXACT = [n for n in ALL if C.CASES[n].exact and (n.startswith("bref-") or n.startswith("degen-"))]


@pytest.mark.parametrize("name", EXACT)
def test_the_oracle_follows_the_64_bit_key_where_float64_is_exact(name):
    """Why float64 is exact here.  Coordinates are integers below 17 (bref), integers 0..39 in units of 2^-8 moved by T <= 2^14
    (translate: 23 bits, exact in fp32, and the translation cancels in every difference), the same integers in units of 2^-4
    (triple), or all equal (coincident).  Differences are therefore integers of magnitude below 40 in the cloud's unit, squares
    and the partial sums of the fma chain integers below 3 * 40^2 = 4800 < 2^24 in that unit squared: nothing is rounded, in
    fp32 or in float64, so the fp32 fma chain and the float64 sum are the same number (`exact` re-checks it on every running
    minimum).  The maximum of (distance bits, tie rank) must then be the C oracle's sample at every step."""
    c = C.CASES[name]
    idx, tied, exact = C.key_fps(c.xyz, c.offset, c.requests[-1])
    assert exact
    assert np.array_equal(_oracle(name), idx), np.flatnonzero(_oracle(name) != idx)[:8]
    if name.startswith(("bref-", "degen-translate", "degen-coincident", "degen-triple")) and len(idx) > 8:
        assert (tied[1:] >= 2).mean() >= 0.5, (tied[1:] >= 2).mean()  # ties, not distances, decide most samples


def test_degenerate_clouds_are_degenerate():
    for n in C.DEGEN_SIZES:
        get = lambda name: C.CASES[f"degen-{name}-{n}"]
        ext = lambda name: np.ptp(get(name).xyz, axis=0)
        assert (ext("planar") > 0.9).tolist() == [True, True, False] and ext("planar")[2] == 0
        assert ext("collinear")[0] > 0.9 and ext("collinear")[1] == 0 and ext("collinear")[2] == 0
        assert (ext("coincident") == 0).all() and int(get("coincident").requests[0][0]) == 70
        assert (_oracle(f"degen-coincident-{n}") == 0).all()             # every step is a tie of all points at 0: the first tie rank wins
        for name in ("planar", "collinear", "clusters3e5", "extent3e5", "scale2m70", "scale2p40", "translate0"):
            assert len(get(name).xyz) == n and int(get(name).requests[0][0]) == 600
        # the 1e10 clamp: pair distances above the running minimum's start value
        far = get("clusters3e5").xyz
        assert _sq(far[: n // 2][:, None, :][:64], far[n // 2:][None, :64, :]).min() > C.DMAX
        big = get("extent3e5").xyz
        d0 = _sq(big[0], big)
        assert 0.5 < (d0 > C.DMAX).mean() < 1.0                           # most points tie at the clamp after the first sample
        want = _oracle(f"degen-extent3e5-{n}")
        low = C.tie_rank(n, n)
        clamped = np.flatnonzero(d0 >= C.DMAX)
        assert want[1] == clamped[np.argmax(low[clamped])]                # the second sample is the tie rule's choice among them
        assert (_sq(get("scale2p40").xyz[0], get("scale2p40").xyz[1:]) > C.DMAX).all()   # nothing ever leaves the clamp
        # 2^-70: non-zero subnormal squares (below 2^-126, the smallest normal fp32)
        tiny = get("scale2m70").xyz
        dt = _sq(tiny[0], tiny[1:])
        assert (dt > 0).all() and (dt < np.float32(2.0 ** -126)).all()
        assert 64 < len(np.unique(dt)) <= 3 * 512                         # squares below 3 * 2^-140 = 1536 steps of 2^-149: coarse, tied, not flat
        # the 2^-8 grid: the translation is exact and the oracle does not see it
        base = get("translate0")
        assert np.array_equal(base.xyz * 256, np.round(base.xyz * 256))
        for T in C.TRANSLATIONS:
            c = get(f"translate{T}")
            assert np.array_equal(c.xyz.astype(np.float64) - T, base.xyz.astype(np.float64))
            assert np.array_equal(_oracle(c.name), _oracle(base.name)), T
        tri = C.CASES[f"degen-triple-{3 * ((n + 2) // 3)}"]
        _, counts = np.unique(tri.xyz, axis=0, return_counts=True)
        assert len(tri.xyz) == 3 * ((n + 2) // 3) and (counts % 3 == 0).all()
        assert C.dispatch_of(tri) == C.dispatch(n)


@pytest.mark.parametrize("name", [n for n in ALL if n.startswith("prefix-") and not n.endswith("-hint")])
def test_ordered_clouds_come_back_as_the_identity_up_to_exactly_the_stated_break(name):
    c, hinted = C.CASES[name], C.CASES[name + "-hint"]
    assert hinted.hint and not c.hint and hinted.xyz is c.xyz and hinted.breaks == c.breaks
    want = _oracle(name)
    if name == "prefix-lattice":
        # selection order of a lattice: genuine ties stop the identity early (the tie rule sees the new indices)
        stop = int(np.flatnonzero(want != np.arange(len(want)))[0])
        assert 1 <= stop < 64, stop
        return
    lo, mlo = 0, 0
    for hi, mhi, j in zip(c.offset, c.requests[0], c.breaks):
        got = want[mlo:mhi] - lo
        ident = np.arange(mhi - mlo)
        if j is None:
            assert np.array_equal(got, ident)
        else:
            assert np.array_equal(got[:j], ident[:j]) and got[j] != j, (j, got[max(j - 2, 0): j + 2])
        lo, mlo = int(hi), int(mhi)


def test_prefix_family_covers_probe_tiles_head_and_rounds():
    singles = [C.CASES[f"prefix-break{j}"] for j in C.PREFIX_BREAKS]
    assert [c.breaks[0] for c in singles] == [1, 2, 63, 64, 65, 255, 256, 257, 2303, None]
    assert all(len(c.xyz) == 2304 == int(c.requests[0][0]) for c in singles)
    assert C.CASES["prefix-batch3"].breaks == (2, 256, None) and len(C.CASES["prefix-batch3"].offset) == 3
    for j in (100, 300):
        c = C.CASES[f"prefix-9000-break{j}"]
        assert len(c.xyz) == 9000 and int(c.requests[0][0]) == 1200 and C.dispatch_of(c).head
        assert (j < C.FPS_HEAD) == (j == 100)


def test_request_lengths_surround_the_head():
    assert C.REQ_LENGTHS == (1, 2, C.FPS_HEAD - 1, C.FPS_HEAD, C.FPS_HEAD + 1)
    assert [a for a, _ in C.REQ_RESUMES] == [1, C.FPS_HEAD - 1, C.FPS_HEAD, C.FPS_HEAD + 1]
    for n in C.REQ_SIZES:
        assert C.dispatch(n).head and int(C.CASES[f"req-{n}-m{n + 9}"].requests[0][0]) == n + 9
    assert np.diff(C.CASES["req-batch-0-1"].requests[0], prepend=0).tolist() == [0, 1]
    assert np.diff(C.CASES["req-batch-1-0-1"].requests[0], prepend=0).tolist() == [1, 0, 1]


def test_many_clouds_need_two_launches_at_one_group_per_cloud():
    a, b = C.CASES["many-130"], C.CASES["many-130-empty"]
    sizes = np.diff(a.offset, prepend=0)
    assert len(sizes) == 130 > C.LZ_CHUNK and sizes.min() == 2048 and sizes.max() == 2100
    assert C.dispatch_of(a).G == 1 and (np.diff(a.requests[0], prepend=0) == 40).all()
    sizes_b, m_b = np.diff(b.offset, prepend=0), np.diff(b.requests[0], prepend=0)
    assert len(sizes_b) == 131 and np.flatnonzero(sizes_b == 0).tolist() == [65] and m_b[65] == 0
    assert np.array_equal(a.xyz, b.xyz) and C.dispatch_of(b).G == 1
    assert np.array_equal(_oracle("many-130"), _oracle("many-130-empty"))    # the empty element changes nobody's samples
