"""CPU check of the offset checks and the slice-and-chunk walk behind the segmented searches' host forms (colorid_amd/csrc/cid_segplan.hpp,
compiled with g++): every slice of seeded random layouts against a few-line restatement and against the properties the kernels rely on,
every malformed offset array refused with its rule and index, the kernels' segment lookup (segment_of) against numpy and in range whatever
the offsets hold — and, in a stand-alone program under AddressSanitizer, all of it within its bounds."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
OK, FIRST_NONZERO, DECREASES, TOO_LONG, WRONG_END = 0, 1, 2, 3, 4
u64p = C.POINTER(C.c_uint64)
LENGTHS = [0, 1, 63, 64, 65, 128, 200]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("shim") / "segplan_shim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, os.path.join(HERE, "cpu_shim", "segplan_shim.cpp")])
    L = C.CDLL(so)
    L.shim_check_seg_off.argtypes = [u64p, C.c_uint64, C.c_uint64, u64p]
    L.shim_check_seg_off.restype = None
    L.shim_check_group_off.argtypes = [u64p, C.c_uint64, C.c_uint64, u64p]
    L.shim_check_group_off.restype = None
    L.shim_plan_slice.argtypes = [u64p, C.c_uint64, C.c_uint64, C.c_uint64, u64p, C.c_uint64, u64p, C.c_uint64, u64p]
    L.shim_plan_slice.restype = None
    L.shim_segment_of.argtypes = [u64p, C.c_uint64, u64p, C.c_uint64, u64p]
    L.shim_segment_of.restype = None
    return L


def _ptr(a):
    return a.ctypes.data_as(u64p)


def check_seg(shim, off, max_len=2**32):
    off = np.array([int(x) % 2**64 for x in off], np.uint64)
    out = np.zeros(2, np.uint64)
    shim.shim_check_seg_off(_ptr(off), len(off) - 1, max_len, _ptr(out))
    return int(out[0]), int(out[1])


def check_group(shim, off, n_segs):
    off = np.array([int(x) % 2**64 for x in off], np.uint64)
    out = np.zeros(2, np.uint64)
    shim.shim_check_group_off(_ptr(off), len(off) - 1, n_segs, _ptr(out))
    return int(out[0]), int(out[1])


def plan(shim, off, s0, s1, chunk):
    """-> (loc as a list of ints, pieces as a list of (k0, nk, seg0, n_loc, loc0))"""
    off = np.ascontiguousarray(off, np.uint64)
    n_kmers = int(off[s1] - off[s0])
    loc_cap = (s1 - s0 + 1) + 2 * (n_kmers // chunk + 1) + 2 * (s1 - s0)     # a piece lists its segments + 1; a cut adds one segment
    piece_cap = n_kmers // chunk + 1
    loc = np.zeros(loc_cap, np.uint64)
    pieces = np.zeros(5 * piece_cap, np.uint64)
    out = np.zeros(2, np.uint64)
    shim.shim_plan_slice(_ptr(off), s0, s1, chunk, _ptr(loc), loc_cap, _ptr(pieces), piece_cap, _ptr(out))
    n_loc, n_pieces = int(out[0]), int(out[1])
    assert n_loc <= loc_cap and n_pieces <= piece_cap, (n_loc, loc_cap, n_pieces, piece_cap)
    return [int(x) for x in loc[:n_loc]], [tuple(int(x) for x in pieces[5 * i:5 * i + 5]) for i in range(n_pieces)]


def py_plan(off, s0, s1, chunk):
    """the restatement: a piece lists every segment from the one that holds its first k-mer to the one that holds its last"""
    off = [int(x) for x in off]
    loc, pieces = off[s0:s1 + 1], []
    holder = [s for s in range(s0, s1) for _ in range(off[s + 1] - off[s])]      # the segment of every k-mer of the slice
    for k0 in range(off[s0], off[s1], chunk):
        k1 = min(k0 + chunk, off[s1])
        sa, sb = holder[k0 - off[s0]], holder[k1 - 1 - off[s0]]
        pieces.append((k0, k1 - k0, sa, sb - sa + 1, len(loc)))
        loc += [min(max(off[s], k0), k1) - k0 for s in range(sa, sb + 2)]
    return loc, pieces


def offsets(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)


def random_lengths(rng, n_segs=40):
    """lengths around the chunk sizes, with runs of empty segments at the start, in the middle and at the end"""
    lens = rng.choice(LENGTHS, size=n_segs)
    lens[:int(rng.integers(1, 4))] = 0
    mid = int(rng.integers(10, 25))
    lens[mid:mid + int(rng.integers(2, 6))] = 0
    lens[n_segs - int(rng.integers(1, 4)):] = 0
    return lens


def check_slices(shim, off, per_slice, chunk):
    """every slice of per_slice segments: the restatement, and the properties one by one; -> the number of pieces"""
    n_segs, total = len(off) - 1, 0
    o = [int(x) for x in off]
    for s0 in range(0, n_segs, per_slice):
        s1 = min(n_segs, s0 + per_slice)
        loc, pieces = plan(shim, off, s0, s1, chunk)
        assert (loc, pieces) == py_plan(off, s0, s1, chunk)
        ns = s1 - s0
        assert loc[:ns + 1] == o[s0:s1 + 1]                       # the slice's true offsets come first
        if o[s0] == o[s1]:
            assert pieces == [] and len(loc) == ns + 1            # only empty segments: no pieces
        clipped = [0] * ns
        next_k, next_loc = o[s0], ns + 1
        for i, (k0, nk, seg0, n_loc, loc0) in enumerate(pieces):
            assert k0 == next_k and loc0 == next_loc              # in order, without gap or overlap
            assert 1 <= nk <= chunk and (nk == chunk or i == len(pieces) - 1)
            assert s0 <= seg0 and n_loc >= 1 and seg0 + n_loc <= s1
            mine = loc[loc0:loc0 + n_loc + 1]
            assert len(mine) == n_loc + 1 and mine[0] == 0 and mine[-1] == nk
            lens = np.diff(mine)
            assert (lens >= 0).all() and lens[0] > 0 and lens[-1] > 0
            for j, n in enumerate(lens):
                clipped[seg0 - s0 + j] += int(n)
            next_k, next_loc = k0 + nk, loc0 + n_loc + 1
        assert next_k == o[s1] and next_loc == len(loc)           # the pieces tile [seg_off[s0], seg_off[s1])
        assert clipped == [o[s + 1] - o[s] for s in range(s0, s1)]
        total += len(pieces)
    return total


@pytest.mark.parametrize("per_slice", [1, 3, 8, 40])
@pytest.mark.parametrize("chunk", [64, 128])
def test_every_slice_is_tiled_by_its_pieces(shim, chunk, per_slice):
    rng = np.random.default_rng(100 * chunk + per_slice)
    for trial in range(8):
        lens = random_lengths(rng)
        assert len(lens) == 40 and lens[0] == 0 and lens[-1] == 0
        n_pieces = check_slices(shim, offsets(lens), per_slice, chunk)
        assert n_pieces >= -(-int(lens.sum()) // chunk)
    # the layouts did hold what they are meant to hold
    lens = np.concatenate([random_lengths(np.random.default_rng(s)) for s in range(4)])
    assert set(lens.tolist()) == set(LENGTHS)


def test_only_empty_segments_give_no_pieces(shim):
    off = offsets([0] * 7)
    for per_slice in (1, 3, 7):
        assert check_slices(shim, off, per_slice, 64) == 0
    off = offsets([0, 0, 5, 0, 0, 0, 0])          # ... beside a slice that has k-mers
    assert check_slices(shim, off, 2, 64) == 1 and check_slices(shim, off, 7, 64) == 1


def test_a_chunk_boundary_on_a_segment_boundary(shim):
    off = offsets([64, 64, 0, 128, 1])
    loc, pieces = plan(shim, off, 0, 5, 64)
    assert loc[:6] == [0, 64, 128, 128, 256, 257]
    # no piece lists a neighbour it holds nothing of; the empty segment 2 lies between two pieces and is in neither
    assert pieces == [(0, 64, 0, 1, 6), (64, 64, 1, 1, 8), (128, 64, 3, 1, 10), (192, 64, 3, 1, 12), (256, 1, 4, 1, 14)]
    assert loc[6:] == [0, 64] * 4 + [0, 1]
    assert check_slices(shim, off, 5, 64) == 5 and check_slices(shim, off, 5, 128) == 3 and check_slices(shim, off, 2, 128) == 3


def test_one_segment_over_three_chunks(shim):
    off = offsets([3, 150, 5])
    loc, pieces = plan(shim, off, 0, 3, 64)
    assert pieces == [(0, 64, 0, 2, 4), (64, 64, 1, 1, 7), (128, 30, 1, 2, 9)]
    assert loc == [0, 3, 153, 158] + [0, 3, 64] + [0, 64] + [0, 25, 30]
    assert check_slices(shim, off, 3, 64) == 3 and check_slices(shim, off, 1, 64) == 5


@pytest.mark.parametrize("bad", [0, 4, 8])
def test_each_malformed_seg_off_is_refused_with_its_rule_and_index(shim, bad):
    good = [40 * s for s in range(10)]
    assert check_seg(shim, good) == (OK, 0)
    if bad == 0:
        assert check_seg(shim, [50] + good[1:]) == (FIRST_NONZERO, 0)        # it also decreases at segment 0: the first entry is looked at first
        assert check_seg(shim, [1] + good[1:]) == (FIRST_NONZERO, 0)
    else:
        off = list(good); off[bad + 1] = off[bad] - 1
        assert check_seg(shim, off) == (DECREASES, bad)
        assert check_seg(shim, [7] + off[1:]) == (FIRST_NONZERO, 0)
    for max_len in (2**32, 2**32 - 128):
        off = [x + (max_len - 40 if s > bad else 0) for s, x in enumerate(good)]    # segment `bad` has max_len entries: refused
        assert check_seg(shim, off, max_len) == (TOO_LONG, bad)
        off = [x - (1 if s > bad else 0) for s, x in enumerate(off)]                # one below the bound: accepted
        assert check_seg(shim, off, max_len) == (OK, 0)
    assert check_seg(shim, [x + (2**32 - 128 - 40 if s > bad else 0) for s, x in enumerate(good)], 2**32) == (OK, 0)   # the bounds differ
    # two rules broken: the lower segment is reported, and within a walk "decreases" is met before a later "too long"
    if bad < 8:
        off = list(good); off[bad + 1] = off[bad] + 2**32; off[bad + 2] = 0
        assert check_seg(shim, off) == (TOO_LONG, bad)
    if bad > 0:
        off = [x + (2**32 if s > bad else 0) for s, x in enumerate(good)]; off[1] = 50; off[2] = 45
        assert check_seg(shim, off) == (DECREASES, 1)


@pytest.mark.parametrize("bad", [0, 2, 5])
def test_each_malformed_group_off_is_refused_with_its_rule_and_index(shim, bad):
    n_segs, good = 18, [3 * g for g in range(7)]
    assert check_group(shim, good, n_segs) == (OK, 0)
    if bad == 0:
        assert check_group(shim, [2] + good[1:], n_segs) == (FIRST_NONZERO, 0)
        assert check_group(shim, [4] + good[1:], n_segs) == (FIRST_NONZERO, 0)      # decreases too
    else:
        off = list(good); off[bad + 1] = off[bad] - 1
        assert check_group(shim, off, n_segs) == (DECREASES, bad)
        assert check_group(shim, off, n_segs + 1) == (DECREASES, bad)               # ... and ends wrong: "decreases" comes first
        assert check_group(shim, [1] + off[1:], n_segs) == (FIRST_NONZERO, 0)
    for end in (n_segs - 1, n_segs + 1, 2**40):
        assert check_group(shim, good[:-1] + [end], n_segs) == (WRONG_END, end)     # `at` is where the array ends
    assert check_group(shim, [0], 0) == (OK, 0) and check_group(shim, [0, 0, 0], 0) == (OK, 0)


def segment_of(shim, off, n_segs, kmers):
    off = np.ascontiguousarray(off, np.uint64)
    kmers = np.ascontiguousarray(kmers, np.uint64)
    out = np.full(len(kmers), 2**64 - 1, np.uint64)
    shim.shim_segment_of(_ptr(off), n_segs, _ptr(kmers), len(kmers), _ptr(out))
    return out


@pytest.mark.parametrize("lens", [[5], [0, 0, 3, 0, 0, 0, 64, 1, 0, 63, 0, 0], [0, 1], [1, 0], [64, 64, 0, 128, 1], "random"],
                         ids=["one", "empties-everywhere", "leading", "trailing", "tile-edges", "random"])
def test_the_segment_of_every_kmer(shim, lens):
    """the kernels' lookup (segment_of): the last segment whose offset is <= the k-mer, so an empty segment never holds one"""
    if lens == "random":
        lens = random_lengths(np.random.default_rng(7))
    off = offsets(lens)
    n_segs, n_kmers = len(lens), int(off[-1])
    kmers = np.arange(n_kmers, dtype=np.uint64)
    got = segment_of(shim, off, n_segs, kmers)
    assert np.array_equal(got, np.searchsorted(off[:n_segs], kmers, side="right") - 1)
    assert (np.asarray(lens)[got.astype(np.int64)] > 0).all()                    # the segment that really holds the k-mer
    assert np.array_equal(np.bincount(got.astype(np.int64), minlength=n_segs), lens)


@pytest.mark.parametrize("n_segs", [1, 2, 3, 8, 33])
def test_the_segment_stays_in_range_whatever_the_offsets_hold(shim, n_segs):
    """any contents — decreasing, all equal, huge, a first entry that is not 0 — and any k-mer: the result indexes the kernels' outputs"""
    rng = np.random.default_rng(n_segs)
    arrays = [rng.integers(0, 300, n_segs + 1), np.sort(rng.integers(0, 300, n_segs + 1))[::-1], np.full(n_segs + 1, 2**64 - 1, np.uint64),
              np.zeros(n_segs + 1), np.full(n_segs + 1, 150), rng.integers(0, 2**63, n_segs + 1)]
    kmers = np.array(list(range(310)) + [2**32 - 1, 2**32, 2**63, 2**64 - 1], np.uint64)
    for off in arrays:
        got = segment_of(shim, np.asarray(off).astype(np.uint64), n_segs, kmers)
        assert (got < n_segs).all(), (off, got)


def test_the_checks_and_the_walk_stay_inside_their_arrays(tmp_path):
    """the stand-alone program (its own main, exactly-sized heap arrays) under AddressSanitizer + UBSan, as a child process"""
    exe = str(tmp_path / "segplan_main")
    # (both runtimes linked statically: the program's own, whatever else the process loads)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-o", exe, os.path.join(HERE, "cpu_shim", "segplan_main.cpp")])
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "ERROR" not in p.stderr and "runtime error" not in p.stderr, p.stderr
