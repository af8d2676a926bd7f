"""The report epilogues called directly, on device arrays the test chose (tests/report_refs.py): cid_unique_freq_modes_dev against
ref_modes over every depth of the mode table, and cid_search_unique_finalize_dev against ref_finalize over its three code shapes
(a per-workgroup LDS histogram, the same past 64 KiB, global atomics).  Every comparison is exact: everything is an integer."""
import itertools

import numpy as np
import pytest
import torch

import report_refs as rr
from report_refs import SENTINEL, U32_MAX
from util import random_index, random_kmers, to_hip_index

pytestmark = pytest.mark.gpu

GUARD = 64                      # elements past the end of every output: they keep what they held
INVALID = -1                    # CID_ERR_INVALID


def dev(a):
    """u32 / u64 host array -> int32 / int64 device tensor of the same bits"""
    a = np.array(a, copy=True)
    return torch.from_numpy(a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])).cuda()


def host(t, dtype):
    return t.cpu().numpy().view(dtype)


def ptr(t):
    return t.data_ptr() if t is not None and t.numel() else 0


def gpu_modes(ctx, uc, fq, C):
    d_uc, d_fq = dev(uc), (None if fq is None else dev(fq))
    out = torch.full((C + GUARD,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")     # fully written: starts as garbage
    torch.cuda.synchronize()
    ctx.unique_freq_modes_dev(ptr(d_uc), ptr(d_fq), len(uc), C, out.data_ptr())
    ctx.synchronize()
    got = host(out, np.uint64)
    assert (got[C:] == 0x5A5A5A5A5A5A5A5A).all()
    return got[:C]


def assert_modes(ctx, uc, fq, C):
    got, want = gpu_modes(ctx, uc, fq, C), rr.ref_modes(uc, fq, C)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, (C, len(uc), bad[:8], got[bad[:8]], want[bad[:8]])


# ---------------------------------------------------------------------------------------------- modes

@pytest.mark.parametrize("C", rr.MODE_COLOUR_COUNTS)
def test_modes_every_table_depth(hip_ctx, C):
    uc, fq, _ = rr.get_mode_case(C, rr.MODE_N)
    assert_modes(hip_ctx, uc, fq, C)


@pytest.mark.parametrize("n", rr.MODE_SIZES)
@pytest.mark.parametrize("C", rr.MODE_SIZE_COLOURS)
def test_modes_sizes(hip_ctx, C, n):
    uc, fq, _ = rr.get_mode_case(C, n)
    assert_modes(hip_ctx, uc, fq, C)


@pytest.mark.parametrize("C", [256, 3000, 16384, 70_000])     # multiplicity 1: in the table, in the table, in the list, no table
def test_modes_without_multiplicities(hip_ctx, C):
    uc, _, _ = rr.get_mode_case(C, rr.MODE_N)
    got = gpu_modes(hip_ctx, uc, None, C)
    assert np.array_equal(got, rr.ref_modes(uc, None, C))
    assert np.array_equal(got, gpu_modes(hip_ctx, uc, np.ones(len(uc), np.uint32), C))
    assert set(got.tolist()) <= {0, 1} and got.any()


@pytest.mark.parametrize("C", [256, 70_000])
def test_modes_all_sentinel(hip_ctx, C):
    rng = np.random.default_rng(C)
    uc = np.full(rr.MODE_N, SENTINEL, np.uint32)
    fq = rng.integers(0, 1 << 32, rr.MODE_N, dtype=np.uint64).astype(np.uint32)
    assert not gpu_modes(hip_ctx, uc, fq, C).any()
    assert not gpu_modes(hip_ctx, uc, None, C).any()


def test_modes_all_in_the_overflow_list(hip_ctx):
    C, n = 70_000, 300_000
    rng = np.random.default_rng(7)
    uc, fq = rr.random_entries(C, n, rng, 0)
    assert_modes(hip_ctx, uc, fq, C)
    # ... and with a table that none of the entries reaches
    C = 300
    fq = np.maximum(fq, 32).astype(np.uint32)
    assert_modes(hip_ctx, (uc % C).astype(np.uint32), fq, C)


@pytest.mark.parametrize("C,c,f", [(256, 17, 5), (256, 255, 63), (3000, 2999, 3), (16384, 16383, 0)])
def test_modes_all_in_one_cell(hip_ctx, C, c, f):
    n = rr.MODE_N
    got = gpu_modes(hip_ctx, np.full(n, c, np.uint32), np.full(n, f, np.uint32), C)
    want = np.zeros(C, np.uint64)
    want[c] = f
    assert np.array_equal(got, want)
    assert np.array_equal(want, rr.ref_modes(np.full(n, c, np.uint32), np.full(n, f, np.uint32), C))


def test_modes_twice_on_one_context_and_a_search_afterwards(orc, hip_ctx):
    """the work arrays go back to the context's block cache: a stale `best` or table would show in the second call, and a search on
    the same context afterwards still matches the oracle"""
    a = rr.get_mode_case(3000, rr.MODE_N)
    b = rr.get_mode_case(257, rr.MODE_N)
    for uc, fq, feat in (a, b, a, a, b):
        assert_modes(hip_ctx, uc, fq, feat["C"])
    rng = np.random.default_rng(11)
    oix = random_index(orc, rng, 10_007, 3, 31, 100, density=0.05, zero_row_frac=0.1)
    kmers = random_kmers(rng, 3000, 31)
    for km in kmers[:1500]:
        oix.insert(int(rng.integers(0, 100)), km.tobytes())
    freq = rng.integers(1, 9, len(kmers)).astype(np.uint32)
    hx = to_hip_index(hip_ctx, oix)
    got, want = hx.search_count(kmers, freq), oix.search_count(kmers, freq)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    assert want[1].sum() > 500
    uc = got[3]
    assert np.array_equal(gpu_modes(hip_ctx, uc, freq, 100), orc.unique_modes(uc, freq, 100))
    hx.close()


def test_modes_argument_errors(hip_ctx):
    uc, fq, feat = rr.get_mode_case(256, 2049)
    d_uc, d_fq = dev(uc), dev(fq)
    out = torch.zeros(256, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    call = hip_ctx.lib.cid_unique_freq_modes_dev
    from colorid_amd._lib import vp
    assert call(hip_ctx.h, vp(d_uc.data_ptr()), vp(d_fq.data_ptr()), len(uc), 256, None) == INVALID
    assert call(hip_ctx.h, vp(d_uc.data_ptr()), vp(d_fq.data_ptr()), len(uc), 0, vp(out.data_ptr())) == INVALID
    assert call(hip_ctx.h, None, vp(d_fq.data_ptr()), len(uc), 256, vp(out.data_ptr())) == INVALID
    assert call(None, vp(d_uc.data_ptr()), vp(d_fq.data_ptr()), len(uc), 256, vp(out.data_ptr())) == INVALID
    hip_ctx.synchronize()
    assert not host(out, np.uint64).any()                       # a refused call writes nothing
    from colorid_amd import CidError
    with pytest.raises(CidError):
        hip_ctx.unique_freq_modes_dev(d_uc.data_ptr(), d_fq.data_ptr(), len(uc), 256, 0)
    assert_modes(hip_ctx, uc, fq, 256)
    # no colours at all with n == 0 is fine: every mode 0
    assert not gpu_modes(hip_ctx, np.zeros(0, np.uint32), None, 5).any()


# ---------------------------------------------------------------------------------------------- finalize

def gpu_finalize(ctx, fact, freq, C, want=(True, True, True), calls=1):
    """-> (n_unique, sum, unique_colour) as u64 / u64 / u32 arrays, None where the pointer was NULL.  n_unique and sum start zeroed
    (the header's "zeroed"); unique_colour is fully written and starts as garbage."""
    from colorid_amd._lib import check, vp
    n = len(fact)
    d_fact, d_fq = dev(fact), (None if freq is None else dev(freq))
    nu = torch.zeros(C + GUARD, dtype=torch.int64, device="cuda") if want[0] else None
    sf = torch.zeros(C + GUARD, dtype=torch.int64, device="cuda") if want[1] else None
    uc = torch.full((n + GUARD,), 0x5A5A5A5A, dtype=torch.int32, device="cuda") if want[2] else None
    torch.cuda.synchronize()
    for _ in range(calls):
        check(ctx.lib.cid_search_unique_finalize_dev(ctx.h, vp(ptr(d_fact)) if n else None, vp(ptr(d_fq)) if d_fq is not None and n else None, n, C,
                                                     vp(nu.data_ptr()) if want[0] else None, vp(sf.data_ptr()) if want[1] else None,
                                                     vp(uc.data_ptr()) if want[2] else None))
    ctx.synchronize()
    out = []
    for t, dt, m in ((nu, np.uint64, C), (sf, np.uint64, C), (uc, np.uint32, n)):
        if t is None:
            out.append(None)
            continue
        h = host(t, dt)
        assert (h[m:] == h[-1]).all() and h[-1] == (0x5A5A5A5A if dt == np.uint32 else 0)      # nothing past the end
        out.append(h[:m])
    return out


def assert_finalize(ctx, fact, freq, C, want=(True, True, True)):
    got = gpu_finalize(ctx, fact, freq, C, want)
    ref = rr.ref_finalize(fact, freq, C)
    for g, r, w, name in zip(got, ref, want, ("n_unique", "sum", "unique_colour")):
        if not w:
            assert g is None
            continue
        bad = np.flatnonzero(g != r)
        assert len(bad) == 0, (name, C, len(fact), bad[:8], g[bad[:8]], r[bad[:8]])


@pytest.mark.parametrize("C,n", rr.fact_cases())
def test_finalize_colour_counts_and_sizes(hip_ctx, C, n):
    fact, freq, feat = rr.get_fact_case(C, n)
    assert_finalize(hip_ctx, fact, freq, C)


def test_finalize_more_than_4096_per_workgroup(hip_ctx):
    C, n = rr.FACT_BIG
    fact, freq, feat = rr.get_fact_case(C, n)
    assert_finalize(hip_ctx, fact, freq, C)


@pytest.mark.parametrize("C", [300, 8192, 8193])               # one per code shape
def test_finalize_null_pointers(hip_ctx, C):
    fact, freq, _ = rr.get_fact_case(C, 10_000)
    for want in ((False, True, True), (True, False, True), (True, True, False), (False, False, True), (True, True, True)):
        assert_finalize(hip_ctx, fact, freq, C, want)
    assert_finalize(hip_ctx, fact, None, C)
    nu, sf, _ = gpu_finalize(hip_ctx, fact, None, C)
    assert np.array_equal(nu, sf) and nu.sum() > 1000


@pytest.mark.parametrize("C", [300, 5462, 1 << 20])
def test_finalize_adds_onto_its_outputs(hip_ctx, C):
    """n_unique and sum are ADDED onto ("zeroed" in the header is the caller's job): two calls give exactly double"""
    fact, freq, _ = rr.get_fact_case(C, rr.FACT_N)
    nu, sf, uc = rr.ref_finalize(fact, freq, C)
    got = gpu_finalize(hip_ctx, fact, freq, C, calls=2)
    assert np.array_equal(got[0], 2 * nu) and np.array_equal(got[1], 2 * sf) and np.array_equal(got[2], uc)
    assert int(sf.max()) > 1 << 32


def test_finalize_argument_errors(hip_ctx):
    from colorid_amd._lib import vp
    fact, freq, _ = rr.get_fact_case(300, 4097)
    d_fact, d_fq = dev(fact), dev(freq)
    o = torch.zeros(300, dtype=torch.int64, device="cuda")
    u = torch.zeros(len(fact), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    call = hip_ctx.lib.cid_search_unique_finalize_dev
    args = (vp(o.data_ptr()), vp(o.data_ptr()), vp(u.data_ptr()))
    assert call(hip_ctx.h, None, vp(d_fq.data_ptr()), len(fact), 300, *args) == INVALID
    assert call(hip_ctx.h, vp(d_fact.data_ptr()), vp(d_fq.data_ptr()), len(fact), 0, *args) == INVALID
    assert call(None, vp(d_fact.data_ptr()), vp(d_fq.data_ptr()), len(fact), 300, *args) == INVALID
    hip_ctx.synchronize()
    assert not host(o, np.uint64).any() and not host(u, np.uint32).any()
    assert_finalize(hip_ctx, fact, freq, 300)


# ---------------------------------------------------------------------------------------------- stripes in any order

def test_stripe_order_does_not_matter(orc, hip_ctx):
    """three 64-colour stripes searched in all six orders into a zeroed d_fact, then finalized: every order gives the whole index's
    n_unique, sum and unique_colour.  The k-mers cover every combination of (0, 1, at least 2) colours hit in the three stripes: the
    fact word saturates at 2 and keeps its colour only while the count is 1, which is where an order could matter."""
    from colorid_amd._lib import check, vp
    from test_gpu_striped import stripe_indices
    rng = np.random.default_rng(192)
    C, K, k = 192, 2000, 31
    oix = random_index(orc, rng, 30_011, 3, k, C, density=0.01, zero_row_frac=0.0)
    kmers = random_kmers(rng, K, k)
    for j, km in enumerate(kmers):
        for s, d in enumerate(((j % 27) // 9, (j % 27) // 3 % 3, j % 3)):          # colours to plant in stripes A, B, C: 0, 1 or 2-3
            for c in rng.choice(64, size=(0, 1, int(rng.integers(2, 4)))[d], replace=False):
                oix.insert(64 * s + int(c), km.tobytes())
    member = np.array([[oix.contains(c, kb) for c in range(C)] for kb in (km.tobytes() for km in kmers)], bool)
    pops = np.minimum(member.reshape(K, 3, 64).sum(axis=2), 2)
    assert len({tuple(p) for p in pops.tolist()}) == 27                            # all of {0, 1, >= 2}^3 in the oracle's own popcounts
    freq = rng.integers(0, 1 << 32, K, dtype=np.uint64).astype(np.uint32)
    freq[:50] = U32_MAX
    want = oix.search_count(kmers, freq.astype(np.uint64))
    assert np.array_equal(want[3] != SENTINEL, member.sum(axis=1) == 1) and (want[3] != SENTINEL).sum() > 200
    stripes = stripe_indices(hip_ctx, orc, oix, [(0, 64), (64, 128), (128, 192)])
    dk = torch.from_numpy(kmers.reshape(-1).copy()).cuda().reshape(K, k)
    for order in itertools.permutations(range(3)):
        fact = torch.zeros(K, dtype=torch.int32, device="cuda")
        hits = torch.full((C,), -1, dtype=torch.int64, device="cuda")             # each stripe call zeroes and fills its own slice
        torch.cuda.synchronize()
        for s in order:
            hx, base = stripes[s]
            check(hip_ctx.lib.cid_search_count_stripe_dev(hip_ctx.h, hx.h, vp(dk.data_ptr()), None, K, base, vp(hits.data_ptr() + 8 * base),
                                                          vp(fact.data_ptr())))
        hip_ctx.synchronize()
        assert np.array_equal(host(hits, np.uint64), want[0]), order
        f = host(fact, np.uint32)
        assert np.array_equal(np.minimum(f >> 26, 2), np.minimum(member.sum(axis=1), 2)), order
        got = gpu_finalize(hip_ctx, f, freq, C)
        for g, w, name in zip(got, want[1:], ("n_unique", "sum", "unique_colour")):
            assert np.array_equal(g, w), (order, name)
    for hx, _ in stripes:
        hx.close()
