"""Plain references and input builders for the report epilogues (numpy only, no GPU):
    cid_unique_freq_modes_dev       -> ref_modes     (the mode of the unique-hit multiplicities per colour, reports.rs:65-77)
    cid_search_unique_finalize_dev  -> ref_finalize  (the exactly-one-colour rule on summed fact words, include/colorid_hip.h)
The builders aim their inputs at the places where the two kernel families change shape; each returns its arrays together with a
dict of the features it planted, and tests/test_report_refs_cpu.py re-derives every feature from the arrays alone."""
import functools

import numpy as np

SENTINEL = 0xFFFFFFFF          # "no unique colour"
U32_MAX = 0xFFFFFFFF
FACT_SHIFT = 26                # fact word: n << 26 | colour + 1
FACT_COLOUR_MASK = (1 << FACT_SHIFT) - 1
MIN_PLANT = 4096               # mode_case plants its ties and runs from this n on; below it the entries are a random mix

# the cases of tests/test_gpu_report_tails.py (the CPU tests prove the builders on exactly these)
MODE_COLOUR_COUNTS = (1, 63, 64, 65, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193, 16384, 16385, 70_000)
MODE_N = 50_000
MODE_SIZE_COLOURS = (256, 3000)
MODE_SIZES = (0, 1, 63, 64, 65, 2047, 2048, 2049, 1024 * 2048 + 1)
FACT_COLOUR_COUNTS = (1, 64, 300, 5461, 5462, 8192, 8193, 1 << 20)
FACT_N = 50_000
FACT_SIZES = (0, 1, 255, 256, 4095, 4096, 4097, 100_000)
FACT_BIG = (300, 4096 * 4096 + 1)


# ---------------------------------------------------------------------------------------------- references

def ref_modes(uc, freq, C):
    """u64[C]: per colour the multiplicity that occurs most often among the entries with uc != 0xFFFFFFFF; ties go to the smallest
    multiplicity; 0 where a colour has no entry.  freq None = every multiplicity 1."""
    uc = np.asarray(uc, np.uint32)
    f = np.ones(len(uc), np.uint32) if freq is None else np.asarray(freq, np.uint32)
    keep = uc != SENTINEL
    keys, counts = np.unique((uc[keep].astype(np.uint64) << np.uint64(32)) | f[keep].astype(np.uint64), return_counts=True)
    colour = (keys >> np.uint64(32)).astype(np.int64)
    value = keys & np.uint64(U32_MAX)
    order = np.lexsort((value, -counts.astype(np.int64), colour))     # by colour, then the highest count, then the smallest value
    colour, value = colour[order], value[order]
    first = np.ones(len(colour), bool)
    first[1:] = colour[1:] != colour[:-1]
    modes = np.zeros(C, np.uint64)
    modes[colour[first]] = value[first]
    return modes


def ref_finalize(fact, freq, C):
    """(n_unique u64[C], sum u64[C], unique_colour u32[n]): an entry is unique exactly when fact >> 26 == 1, its colour is then
    (fact & (2^26 - 1)) - 1; otherwise unique_colour is 0xFFFFFFFF.  freq None = every multiplicity 1."""
    fact = np.asarray(fact, np.uint32)
    f = np.ones(len(fact), np.uint64) if freq is None else np.asarray(freq, np.uint32).astype(np.uint64)
    unique = (fact >> np.uint32(FACT_SHIFT)) == 1
    colour = (fact[unique] & np.uint32(FACT_COLOUR_MASK)).astype(np.int64) - 1
    uc = np.full(len(fact), SENTINEL, np.uint32)
    uc[unique] = colour.astype(np.uint32)
    nu = np.zeros(C, np.uint64)
    sf = np.zeros(C, np.uint64)
    np.add.at(nu, colour, np.uint64(1))
    np.add.at(sf, colour, f[unique])
    return nu, sf, uc


def mode_tiers(C):
    """(cp_log, FL) of the mode step: the colours padded to a power of two 2^cp_log of at least 64, and the depth of the table of small
    multiplicities, the largest FL <= 64 (a power of two) with FL << cp_log <= 16384, else 0 (no table).  It MUST FOLLOW
    unique_freq_modes_begin (colorid_amd/csrc/cid_reports.hip).  It only aims the builders' inputs at the boundary between the table
    and the overflow list: no assertion on a result may depend on it."""
    cp_log = 6
    while (1 << cp_log) < C:
        cp_log += 1
    FL = 64
    while FL > 1 and (FL << cp_log) > 16384:
        FL >>= 1
    if (FL << cp_log) > 16384:
        FL = 0
    return cp_log, FL


def finalize_shape(C):
    """which of k_unique_finalize's three code shapes n_colors_total = C selects (launch_unique_finalize, cid_search.hip): it only
    labels the cases, like mode_tiers"""
    lds = 12 * C
    return "lds" if lds <= 64 * 1024 else "lds_over_64k" if lds <= 96 * 1024 else "global_atomics"


# ---------------------------------------------------------------------------------------------- mode inputs

def _special_freqs(FL):
    return sorted({0, 1, max(FL - 1, 0), FL, FL + 1, U32_MAX})


def random_entries(C, n, rng, FL, colours=None):
    """n (colour, multiplicity) pairs: colours from a small pool (so that counts grow and natural ties occur) or uniform, among them
    0 and C - 1; multiplicities from the special values, a few small ones and a few large ones"""
    allowed = np.arange(C, dtype=np.int64) if colours is None else np.asarray(colours, np.int64)
    pool = rng.choice(allowed, size=min(len(allowed), 96), replace=False)
    c = np.where(rng.random(n) < 0.7, pool[rng.integers(0, len(pool), n)], allowed[rng.integers(0, len(allowed), n)])
    special = np.array(_special_freqs(FL), np.uint64)
    f = special[rng.integers(0, len(special), n)]
    r = rng.random(n)
    f = np.where(r < 0.15, rng.integers(0, 70, n).astype(np.uint64), f)
    large = rng.integers(1 << 20, 1 << 32, 64, dtype=np.uint64)       # few enough to repeat within a colour
    f = np.where(r > 0.9, large[rng.integers(0, 64, n)], f)
    return c.astype(np.uint32), f.astype(np.uint32)


def mode_case(C, n, rng):
    """(uc u32[n], freq u32[n], features) for cid_unique_freq_modes_dev with n_colors = C.  Every colour is below C or 0xFFFFFFFF.
    Entries i .. i + 63 with i % 64 == 0 are one wave of k_mode_hist, so the runs below are aligned blocks of 64.

    From n = MIN_PLANT on it plants, and names in `features`:
      ties        {kind: (colour, expected mode)}: 'table' (two multiplicities below FL with the same top count), 'overflow' (two at or
                  above FL), 'cross_equal' (FL - 1 in the table and FL in the list with equal counts: FL - 1 wins), 'cross_overflow_wins'
                  (FL in the list one ahead of FL - 1 in the table: FL wins).  Colour C - 1 carries cross_equal (its cell index wraps
                  where C - 1 + FL - 1 >= 2^cp_log, and losing that cell changes the mode), colour 0 cross_overflow_wins.  With fewer than 8 colours there is
                  one tie only, cross_equal on colour 0; without a table (FL == 0) only 'overflow', on colour 0 (and the list's
                  clear winner on colour C - 1); 'table' needs FL >= 2.
      modes       {'in_table' | 'in_overflow' | 'overflow_only': (colour, expected mode)}: a clear winner in each tier, and a colour
                  whose entries all sit in the list (C >= 8)
      runs        {kind: [block index, ...]}: 'one_cell' (64 lanes, one small cell), 'two_cells', 'small_one_cell_rest_overflow'
                  (20 lanes of one small cell, the other 44 at or above FL), all three only with a table; 'sentinel' (64 x 0xFFFFFFFF)
      final_partial_lanes   the n % 64 live lanes of the last wave, all one cell (planted at every n >= 64 with n % 64 != 0)
      run_modes   {colour: expected mode} (C >= 32): a run's cell and the final partial wave's have their colour to themselves, with as
                  many scattered entries of FL + 2 (the tie goes to the run's multiplicity unless the run lost a count) or one more
                  (FL + 2 wins unless the run gained one): a wave that adds its count once must add exactly its lanes
    Sentinel entries carry random multiplicities: they must be ignored whatever these are."""
    cp_log, FL = mode_tiers(C)
    uc = np.full(n, SENTINEL, np.uint32)
    fq = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    feat = {"C": C, "n": n, "cp_log": cp_log, "FL": FL, "planted": n >= MIN_PLANT, "ties": {}, "modes": {}, "runs": {}, "run_modes": {}, "final_partial_lanes": 0}
    tail = n % 64 if n >= 64 else 0
    body = n - tail
    small_f = (FL - 1) if FL else 1          # the final partial wave: one cell (one key where there is no table)
    g_run = FL + 2                           # the multiplicity (in the list) that competes with a run's cell
    if not feat["planted"]:
        ct = (C - 1) // 2
        if body:
            live = rng.random(body) < 0.8
            c, f = random_entries(C, body, rng, FL, np.setdiff1d(np.arange(C), [ct]) if C > 1 else None)
            uc[:body], fq[:body] = np.where(live, c, SENTINEL), np.where(live, f, fq[:body])
        if tail:
            uc[body:], fq[body:] = ct, small_f
            feat["final_partial_lanes"] = tail
            if C > 1:                        # as many entries of a larger multiplicity elsewhere: the tail's count decides the tie
                at = rng.choice(body, size=tail, replace=False)
                uc[at], fq[at] = ct, g_run
                feat["run_modes"][ct] = small_f
        return uc, fq, feat

    few = C < 8
    pivots = C >= 32                         # colours to spare: every run gets colours of its own, where its count decides the mode
    k = 37
    reserved, run_colours = {}, []
    if not few:
        mid = rng.choice(np.arange(1, C - 1), size=5 + (9 if pivots else 0), replace=False)
        reserved = {"cross_equal": C - 1, "cross_overflow_wins": 0, "table": int(mid[0]), "overflow": int(mid[1]),
                    "in_table": int(mid[2]), "in_overflow": int(mid[3]), "overflow_only": int(mid[4])}
        if not FL:     # no table, so no cross-tier plant: colours 0 and C - 1 go to the list's tie and the list's clear winner
            reserved = {"overflow": 0, "in_overflow": C - 1, "overflow_only": int(mid[4])}
        run_colours = [int(c) for c in mid[5:]]
    free_colours = np.setdiff1d(np.arange(C), np.array(sorted(set(reserved.values()) | set(run_colours)), np.int64))
    if len(free_colours) == 0:
        free_colours = np.arange(C)

    # ---- the scattered plants: (colour, multiplicity, count)
    plants = []
    if not few:
        if FL >= 2:
            c = reserved["table"]
            plants += [(c, 0, k), (c, FL - 1, k), (c, FL, k - 1)]
            feat["ties"]["table"] = (c, 0)
        c = reserved["overflow"]
        plants += [(c, FL + 1, k), (c, U32_MAX, k)] + ([(c, 0, k - 1)] if FL else [])
        feat["ties"]["overflow"] = (c, FL + 1)
        if FL:
            c = reserved["cross_equal"]
            plants += [(c, FL - 1, k), (c, FL, k), (c, FL + 1, k - 1)]
            feat["ties"]["cross_equal"] = (c, FL - 1)
            c = reserved["cross_overflow_wins"]
            plants += [(c, FL - 1, k), (c, FL, k + 1)]
            feat["ties"]["cross_overflow_wins"] = (c, FL)
            c = reserved["in_table"]
            f_tab = 1 if FL > 1 else 0
            plants += [(c, f_tab, k), (c, FL + 1, k - 2), (c, U32_MAX, 1)]
            feat["modes"]["in_table"] = (c, f_tab)
        c = reserved["in_overflow"]
        plants += [(c, U32_MAX, k), (c, FL, k - 1)] + ([(c, 0, k - 5)] if FL else [])
        feat["modes"]["in_overflow"] = (c, U32_MAX)
        c = reserved["overflow_only"]
        plants += [(c, FL, 3), (c, FL + 5, 5)]
        feat["modes"]["overflow_only"] = (c, FL + 5)

    def pivot(c, f, m, over):
        """colour c holds nothing but m entries of f in one run: scatter m entries of g_run > f (the tie goes to f unless the run lost
        a count) or m + 1 of them (g_run wins unless the run gained one)"""
        plants.append((c, g_run, m + 1 if over else m))
        feat["run_modes"][c] = g_run if over else f

    # ---- the runs: aligned blocks of 64, two of each kind
    n_blocks = body // 64
    kinds = (["one_cell", "two_cells", "small_one_cell_rest_overflow"] if FL else []) + ["sentinel"]
    blocks = rng.choice(n_blocks, size=2 * len(kinds), replace=False)
    taken = np.zeros(n, bool)
    taken[body:] = True
    for j, b in enumerate(blocks):
        kind = kinds[j // 2]
        s = slice(int(b) * 64, int(b) * 64 + 64)
        taken[s] = True
        feat["runs"].setdefault(kind, []).append(int(b))
        if kind == "sentinel":               # the block stays 0xFFFFFFFF with random multiplicities
            continue
        if pivots:
            ca, cb = run_colours.pop(), (run_colours.pop() if kind == "two_cells" else None)
        else:
            ca, cb = (int(x) for x in free_colours[rng.integers(0, len(free_colours), 2)])
        fa = int(rng.integers(0, FL))
        if kind == "one_cell":
            uc[s], fq[s] = ca, fa
            lanes = np.ones(64, bool)
        elif kind == "two_cells":            # the same colour twice needs two multiplicities
            fb = (fa + 1) % FL if ca == cb else fa
            lanes = rng.random(64) < 0.6
            lanes[0], lanes[1] = True, False
            uc[s], fq[s] = np.where(lanes, ca, cb), np.where(lanes, fa, fb)
            if pivots:
                pivot(cb, fb, 64 - int(lanes.sum()), over=not j % 2)
        else:
            lanes = np.zeros(64, bool)
            lanes[rng.choice(64, size=20, replace=False)] = True
            co, fo = random_entries(C, 64, rng, FL, free_colours)
            fo = np.maximum(fo, FL).astype(np.uint32)
            uc[s], fq[s] = np.where(lanes, ca, co), np.where(lanes, fa, fo)
        if pivots:
            pivot(ca, fa, int(lanes.sum()), over=bool(j % 2))
    if tail:
        ct = run_colours.pop() if pivots else int(free_colours[len(free_colours) // 2])
        uc[body:], fq[body:] = ct, small_f
        feat["final_partial_lanes"] = tail
        if pivots:
            pivot(ct, small_f, tail, over=False)

    # ---- the scattered plants and the random background share the other positions; what is left stays 0xFFFFFFFF
    free = rng.permutation(np.flatnonzero(~taken))
    at = 0
    for c, f, count in plants:
        uc[free[at:at + count]], fq[free[at:at + count]] = c, f
        at += count
    n_bg = int((len(free) - at) * (0.25 if few else 0.75))
    uc[free[at:at + n_bg]], fq[free[at:at + n_bg]] = random_entries(C, n_bg, rng, FL, free_colours)
    at += n_bg
    if few:    # one colour range for everything: raise FL - 1 (table) and FL (list) of colour 0 to one count above every other
        own = uc == 0
        top = int(np.unique(fq[own], return_counts=True)[1].max()) + 1
        for f in (FL - 1, FL):
            need = top - int((own & (fq == f)).sum())
            uc[free[at:at + need]], fq[free[at:at + need]] = 0, f
            at += need
        feat["ties"]["cross_equal"] = (0, FL - 1)
    assert at <= len(free), "mode_case: n too small for its plants"
    return uc, fq, feat


def seed_of(*parts):
    return [int(p) & 0xFFFFFFFF for p in parts] + [int(p) >> 32 for p in parts]


@functools.lru_cache(maxsize=4)
def get_mode_case(C, n):
    """the mode_case of (C, n) the GPU tests and the CPU tests share (arrays are read-only)"""
    uc, fq, feat = mode_case(C, n, np.random.default_rng(seed_of(0x6D6F6465, C, n)))
    uc.setflags(write=False)
    fq.setflags(write=False)
    return uc, fq, feat


def mode_cases():
    return [(C, MODE_N) for C in MODE_COLOUR_COUNTS] + [(C, n) for C in MODE_SIZE_COLOURS for n in MODE_SIZES]


# ---------------------------------------------------------------------------------------------- fact inputs

def fact_case(C, n, rng):
    """(fact u32[n], freq u32[n], features) for cid_search_unique_finalize_dev with n_colors_total = C: fact words as they look after
    the stripes of one GPU (n fields 0, 1, 2) and after a sum across GPUs (3 .. 62).  An n field of 1 carries colour + 1 with
    colour < C, 0 and C - 1 among them; every other n field carries a colour field that is zero or garbage (any 26 bits).  From
    n = 8 on, one colour ('heavy') takes more than 2^32 in summed multiplicity: min(3000, n // 4) entries with freq = 2^32 - 1."""
    r = rng.random(n, dtype=np.float32)
    nf = np.select([r < 0.3, r < 0.7, r < 0.85], [0, 1, 2], default=0).astype(np.uint32)
    wide = r >= 0.85
    nf[wide] = rng.integers(3, 63, int(wide.sum())).astype(np.uint32)
    pool = rng.integers(0, C, 64)
    c = np.where(rng.random(n, dtype=np.float32) < 0.6, pool[rng.integers(0, 64, n)], rng.integers(0, C, n))
    edge = rng.random(n, dtype=np.float32)
    c = np.where(edge < 0.05, 0, np.where(edge > 0.95, C - 1, c)).astype(np.uint32)
    garbage = np.where(rng.random(n, dtype=np.float32) < 0.5, 0, rng.integers(1, 1 << FACT_SHIFT, n)).astype(np.uint32)
    freq = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    s = rng.random(n, dtype=np.float32)
    freq[s < 0.2] = 1
    freq[(s >= 0.2) & (s < 0.25)] = 0
    freq[(s >= 0.25) & (s < 0.3)] = U32_MAX
    feat = {"C": C, "n": n, "heavy": None}
    if n >= 8:
        n_heavy = max(2, min(3000, n // 4))
        heavy = int(pool[0])
        at = rng.choice(n, size=n_heavy, replace=False)
        nf[at], c[at], freq[at] = 1, heavy, U32_MAX
        feat["heavy"] = (heavy, n_heavy)
    field = np.where(nf == 1, c + np.uint32(1), garbage).astype(np.uint32)
    fact = (nf << np.uint32(FACT_SHIFT)) | field
    feat["n_field"] = {"0": int((nf == 0).sum()), "1": int((nf == 1).sum()), "2": int((nf == 2).sum()), "3..62": int((nf >= 3).sum())}
    feat["not_unique_zero_field"] = int(((nf != 1) & (field == 0)).sum())
    feat["not_unique_garbage_field"] = int(((nf != 1) & (field != 0)).sum())
    feat["colour_0"] = int(((nf == 1) & (c == 0)).sum())
    feat["colour_last"] = int(((nf == 1) & (c == C - 1)).sum())
    return fact, freq, feat


@functools.lru_cache(maxsize=2)
def get_fact_case(C, n):
    fact, freq, feat = fact_case(C, n, np.random.default_rng(seed_of(0x66616374, C, n)))
    fact.setflags(write=False)
    freq.setflags(write=False)
    return fact, freq, feat


def fact_cases():
    return [(C, FACT_N) for C in FACT_COLOUR_COUNTS] + [(300, n) for n in FACT_SIZES] + [(8192, n) for n in (1, 4097)]
