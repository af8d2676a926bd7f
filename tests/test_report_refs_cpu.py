"""tests/report_refs.py proved without a GPU: ref_modes against the oracle's orc_unique_modes (the reference implementation's rule,
ties to the smallest value) and against hand-written expectations, ref_finalize on hand-written fact words, and every feature a
builder says it planted re-derived from the arrays it returned — a builder that stops planting one fails HERE and does not pass
silently on the GPU."""
import numpy as np
import pytest

import report_refs as rr
from report_refs import SENTINEL, U32_MAX


def orc_modes(orc, uc, freq, C, span=8):
    """orc.unique_modes in a form that can take these inputs, and nothing but it:
      * on the multiplicities' dense ranks (from 1; 0 stays "no entry"), mapped back: the oracle allocates a histogram of
        max(freq) + 1 counters per colour — 32 GiB at 2^32 - 1 — and its rule depends on the multiplicities' order and equality only
        (the most frequent, the first of them in ascending order), which the ranks keep;
      * one call per range of `span` colours on the entries of that range: the oracle scans every entry once per colour (20 s at
        3000 colours x 2 M entries), and a colour's mode depends on that colour's entries only."""
    uc = np.asarray(uc, np.uint32)
    if freq is None:
        vals, ranks = np.array([1], np.uint64), np.ones(len(uc), np.uint64)
    else:
        live = uc != SENTINEL            # (the entries without a colour are skipped by the oracle: their multiplicities get no rank)
        vals, inv = np.unique(np.asarray(freq, np.uint32)[live], return_inverse=True)
        ranks = np.ones(len(uc), np.uint64)
        ranks[live] = (inv.reshape(-1) + 1).astype(np.uint64)
    order = np.argsort(uc, kind="stable")
    u, r = uc[order], ranks[order]
    out = np.zeros(C, np.uint64)
    for lo in range(0, C, span):
        hi = min(lo + span, C)
        a, b = np.searchsorted(u, [lo, hi])
        out[lo:hi] = orc.unique_modes(u[a:b] - np.uint32(lo), r[a:b], hi - lo)
    return np.concatenate(([0], vals)).astype(np.uint64)[out.astype(np.int64)]


# ---------------------------------------------------------------------------------------------- ref_modes

def test_rank_form_of_the_oracle_equals_the_oracle(orc):
    rng = np.random.default_rng(5)
    uc = np.where(rng.random(3000) < 0.2, SENTINEL, rng.integers(0, 40, 3000)).astype(np.uint32)
    fq = rng.choice([0, 1, 2, 3, 7, 63, 64, 65, 900], size=3000).astype(np.uint32)
    want = orc.unique_modes(uc, fq, 40)
    assert want.any() and np.array_equal(orc_modes(orc, uc, fq, 40), want) and np.array_equal(orc_modes(orc, uc, fq, 40, span=16), want)
    assert np.array_equal(orc_modes(orc, uc, None, 40, span=7), orc.unique_modes(uc, None, 40))


@pytest.mark.parametrize("C,n", rr.mode_cases())
def test_ref_modes_equals_oracle(orc, C, n):
    uc, fq, _ = rr.get_mode_case(C, n)
    want = orc_modes(orc, uc, fq, C)
    assert np.array_equal(rr.ref_modes(uc, fq, C), want)
    assert np.array_equal(rr.ref_modes(uc, None, C), orc_modes(orc, uc, None, C))


def test_ref_modes_by_hand():
    S = SENTINEL
    # colour 0: 5 twice, 2 twice -> 2 (tie to the smaller); colour 1: nothing -> 0; colour 2: one 2^32-1; colour 3: 0 beats 9 two to one
    uc = np.array([0, 0, 0, 0, S, 2, 3, 3, 3, S], np.uint32)
    fq = np.array([5, 2, 5, 2, 7, U32_MAX, 0, 9, 0, 1], np.uint32)
    assert rr.ref_modes(uc, fq, 5).tolist() == [2, 0, U32_MAX, 0, 0]
    # no multiplicities: 1 wherever a colour has an entry
    assert rr.ref_modes(uc, None, 4).tolist() == [1, 0, 1, 1]
    # the highest count wins over the smaller value; the last colour; only sentinels; nothing at all
    uc = np.array([6, 6, 6, 6, 6, 6], np.uint32)
    fq = np.array([1, 8, 8, 8, 1, 0], np.uint32)
    assert rr.ref_modes(uc, fq, 7).tolist() == [0, 0, 0, 0, 0, 0, 8]
    assert rr.ref_modes(np.full(9, S, np.uint32), np.arange(9, dtype=np.uint32), 3).tolist() == [0, 0, 0]
    assert rr.ref_modes(np.zeros(0, np.uint32), np.zeros(0, np.uint32), 2).tolist() == [0, 0]
    assert rr.ref_modes(uc, fq, 7).dtype == np.uint64


# ---------------------------------------------------------------------------------------------- mode_tiers and the builders' features

def test_mode_tiers_table():
    """the documented depths: 64 up to 256 colours, then 32, 16, 8, 4, 2, 1, and no table above 16 384"""
    want = {1: (6, 64), 63: (6, 64), 64: (6, 64), 65: (7, 64), 256: (8, 64), 257: (9, 32), 512: (9, 32), 513: (10, 16), 1024: (10, 16),
            1025: (11, 8), 2048: (11, 8), 2049: (12, 4), 3000: (12, 4), 4096: (12, 4), 4097: (13, 2), 8192: (13, 2), 8193: (14, 1),
            16384: (14, 1), 16385: (15, 0), 70_000: (17, 0)}
    for C, t in want.items():
        assert rr.mode_tiers(C) == t, C
    assert {rr.mode_tiers(C)[1] for C in rr.MODE_COLOUR_COUNTS} == {64, 32, 16, 8, 4, 2, 1, 0}
    assert {rr.finalize_shape(C) for C in rr.FACT_COLOUR_COUNTS} == {"lds", "lds_over_64k", "global_atomics"}
    assert [rr.finalize_shape(C) for C in (5461, 5462, 8192, 8193)] == ["lds", "lds_over_64k", "lds_over_64k", "global_atomics"]


def colour_counts(uc, fq, c):
    """[(multiplicity, count)] of colour c, ascending multiplicity"""
    v, n = np.unique(fq[uc == c], return_counts=True)
    return list(zip(v.tolist(), n.tolist()))


def scan_blocks(uc, fq, FL):
    """the aligned 64-blocks (one wave of k_mode_hist each) by what their lanes hold"""
    nb = len(uc) // 64
    U, F = uc[:nb * 64].reshape(nb, 64), fq[:nb * 64].reshape(nb, 64)
    sent = U == SENTINEL
    small = ~sent & (F.astype(np.uint64) < FL)
    big = ~sent & ~small
    key = (U.astype(np.uint64) << np.uint64(32)) | F.astype(np.uint64)
    kmin = np.where(small, key, np.uint64(2**64 - 1)).min(axis=1)
    kmax = np.where(small, key, np.uint64(0)).max(axis=1)
    one = small.any(axis=1) & (kmin == kmax)
    distinct = (np.diff(np.sort(key, axis=1), axis=1) != 0).sum(axis=1) + 1
    return {"sentinel": set(np.flatnonzero(sent.all(axis=1)).tolist()),
            "one_cell": set(np.flatnonzero(small.all(axis=1) & one).tolist()),
            "two_cells": set(np.flatnonzero(small.all(axis=1) & (distinct == 2)).tolist()),
            "small_one_cell_rest_overflow": set(np.flatnonzero(one & ~small.all(axis=1) & big.any(axis=1)).tolist())}


def expected_ties(C, FL):
    if C < 8:
        return {"cross_equal"}
    return {"overflow"} | ({"cross_equal", "cross_overflow_wins"} if FL else set()) | ({"table"} if FL >= 2 else set())


@pytest.mark.parametrize("C,n", rr.mode_cases())
def test_mode_case_features(C, n):
    uc, fq, feat = rr.get_mode_case(C, n)
    cp_log, FL = rr.mode_tiers(C)
    assert len(uc) == len(fq) == n and uc.dtype == fq.dtype == np.uint32
    live = uc != SENTINEL
    assert (uc[live] < C).all()                                   # the API's precondition
    ref = rr.ref_modes(uc, fq, C)
    # the final partial wave: its live lanes all name one (small) cell
    tail = n % 64 if n >= 64 else 0
    assert feat["final_partial_lanes"] == tail
    if tail:
        t_uc, t_fq = uc[n - tail:], fq[n - tail:]
        assert (t_uc == t_uc[0]).all() and (t_fq == t_fq[0]).all() and t_uc[0] != SENTINEL and (FL == 0 or t_fq[0] < FL)
    # a colour that a run (or the final partial wave) has to itself: one count more or less in the run changes its mode
    small_runs = 8 if (FL and n >= rr.MIN_PLANT) else 0
    assert len(feat["run_modes"]) == ((small_runs + (tail > 0) if C >= 32 else 0) if n >= rr.MIN_PLANT else int(tail > 0 and C > 1))
    for c, want in feat["run_modes"].items():
        (f0, k0), (f1, k1) = colour_counts(uc, fq, c)
        assert f1 == FL + 2 and (f0 < FL or (FL == 0 and f0 == 1)) and k1 - k0 in (0, 1) and want == ref[c] == (f0 if k1 == k0 else f1), (c, f0, k0, f1, k1)
    assert feat["planted"] == (n >= rr.MIN_PLANT)
    if not feat["planted"]:
        assert not feat["ties"] and not feat["runs"]
        return
    # both tiers are fed wherever there is a table
    n_small, n_big = int((live & (fq < FL)).sum()), int((live & (fq >= FL)).sum())
    assert n_big > 0 and (n_small > 0) == (FL > 0) and int((~live).sum()) > 64
    # every special multiplicity occurs, colours 0 and C - 1 occur
    for f in {0, 1, max(FL - 1, 0), FL, FL + 1, U32_MAX}:
        assert (live & (fq == f)).any(), f
    assert (uc == 0).any() and (uc == C - 1).any()
    # cells whose rotated index wraps, wherever the colour count allows one
    wraps = int((live & (fq < FL) & (uc.astype(np.uint64) + fq >= (1 << cp_log))).sum())
    assert (wraps > 0) == (FL >= 1 and C - 1 + FL - 1 >= (1 << cp_log)), wraps
    # the ties
    assert set(feat["ties"]) == expected_ties(C, FL)
    for kind, (c, want) in feat["ties"].items():
        cc = colour_counts(uc, fq, c)
        top = max(k for _, k in cc)
        winners = [f for f, k in cc if k == top]
        assert want == min(winners) == ref[c], (kind, cc)
        if kind == "table":
            assert len(winners) >= 2 and all(f < FL for f in winners)
        elif kind == "overflow":
            assert len(winners) >= 2 and all(f >= FL for f in winners)
        elif kind == "cross_equal":
            assert min(winners) < FL <= max(winners)
        else:
            assert len(winners) == 1 and winners[0] >= FL and max(k for f, k in cc if f < FL) == top - 1
    if C >= 8:
        if FL:
            assert feat["ties"]["cross_equal"][0] == C - 1 and feat["ties"]["cross_overflow_wins"][0] == 0
        else:
            assert feat["ties"]["overflow"][0] == 0 and feat["modes"]["in_overflow"][0] == C - 1
    # a clear winner in each tier, and a colour that lives in the list only
    assert set(feat["modes"]) == (set() if C < 8 else {"in_overflow", "overflow_only"} | ({"in_table"} if FL else set()))
    for kind, (c, want) in feat["modes"].items():
        cc = colour_counts(uc, fq, c)
        top = max(k for _, k in cc)
        winners = [f for f, k in cc if k == top]
        assert winners == [want] and ref[c] == want, (kind, cc)
        if kind == "in_table":
            assert want < FL and any(f >= FL for f, _ in cc)
        elif kind == "in_overflow":
            assert want >= FL and (FL == 0 or any(f < FL for f, _ in cc))
        else:
            assert all(f >= FL for f, _ in cc) and len(cc) >= 2
    # the runs
    found = scan_blocks(uc, fq, FL)
    assert set(feat["runs"]) == ({"one_cell", "two_cells", "small_one_cell_rest_overflow", "sentinel"} if FL else {"sentinel"})
    for kind, blocks in feat["runs"].items():
        assert len(blocks) == 2 and set(blocks) <= found[kind], (kind, blocks)


@pytest.mark.parametrize("C,n", rr.fact_cases())
def test_fact_case_features(C, n):
    fact, freq, feat = rr.get_fact_case(C, n)
    assert len(fact) == len(freq) == n and fact.dtype == freq.dtype == np.uint32
    nf, field = fact >> 26, fact & ((1 << 26) - 1)
    assert nf.max(initial=0) <= 62
    uniq = nf == 1
    assert (field[uniq] >= 1).all() and (field[uniq] <= C).all()   # the API's precondition: a unique entry's colour is below C
    got = {"0": int((nf == 0).sum()), "1": int(uniq.sum()), "2": int((nf == 2).sum()), "3..62": int((nf >= 3).sum())}
    assert feat["n_field"] == got
    assert feat["not_unique_zero_field"] == int((~uniq & (field == 0)).sum())
    assert feat["not_unique_garbage_field"] == int((~uniq & (field != 0)).sum())
    assert feat["colour_0"] == int((uniq & (field == 1)).sum()) and feat["colour_last"] == int((uniq & (field == C)).sum())
    if n >= 1000:
        assert all(v > 0 for v in got.values()) and feat["not_unique_zero_field"] > 0 and feat["not_unique_garbage_field"] > 0
        assert feat["colour_0"] > 0 and feat["colour_last"] > 0
        assert ((nf >= 3) & (field != 0)).any() and ((nf == 0) & (field != 0)).any() and (~uniq & (field > C)).any()
        assert (freq[uniq] == 0).any() and (freq[uniq] == 1).any() and (freq[uniq] == U32_MAX).any()
    if n >= 8:
        heavy, n_heavy = feat["heavy"]
        total = sum(int(f) for f in freq[uniq & (field == heavy + 1)])                    # Python integers
        assert total >= n_heavy * U32_MAX > 1 << 32 and n_heavy == max(2, min(3000, n // 4))
        assert rr.ref_finalize(fact, freq, C)[1][heavy] == total
    else:
        assert feat["heavy"] is None


# ---------------------------------------------------------------------------------------------- ref_finalize

def test_ref_finalize_by_hand():
    S = SENTINEL

    def w(n, field):
        return (n << 26) | field
    # three ranks' words summed: 1 + 0 + 0 keeps the colour, 1 + 1 + 0 and 2 + 1 + 2 do not (their colour fields add up to garbage)
    summed = w(1, 5) + w(0, 0) + w(0, 0)
    fact = np.array([summed, w(1, 5) + w(1, 9) + w(0, 0), w(2, 0) + w(1, 3) + w(2, 0), w(0, 0), w(1, 1), w(1, 7), w(62, 123456), w(0, 77),
                     w(1, 7), w(2, 5)], np.uint32)
    freq = np.array([10, 99, 99, 99, U32_MAX, 3, 99, 99, U32_MAX, 99], np.uint32)
    nu, sf, uc = rr.ref_finalize(fact, freq, 7)
    assert uc.tolist() == [4, S, S, S, 0, 6, S, S, 6, S]
    assert nu.tolist() == [1, 0, 0, 0, 1, 0, 2]
    assert sf.tolist() == [U32_MAX, 0, 0, 0, 10, 0, 3 + U32_MAX]
    assert nu.dtype == sf.dtype == np.uint64 and uc.dtype == np.uint32
    nu, sf, uc = rr.ref_finalize(fact, None, 7)
    assert nu.tolist() == sf.tolist() == [1, 0, 0, 0, 1, 0, 2]
    # sums past 2^32 stay exact
    fact = np.full(5000, w(1, 2), np.uint32)
    nu, sf, uc = rr.ref_finalize(fact, np.full(5000, U32_MAX, np.uint32), 2)
    assert int(sf[1]) == 5000 * U32_MAX and int(nu[1]) == 5000 and sf[0] == 0 and (uc == 1).all()
    nu, sf, uc = rr.ref_finalize(np.zeros(0, np.uint32), np.zeros(0, np.uint32), 3)
    assert nu.tolist() == sf.tolist() == [0, 0, 0] and len(uc) == 0
