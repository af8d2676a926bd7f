"""The oracle pinned against every golden vector / known-answer test available for the path
(SURVEY.md §8c): published XXH3 KATs, src/seq.rs:72-76, src/simple_bloom.rs:60-66, the BitVec bit layout
(bit-vec_serde/src/lib.rs:335-363, :465-474), the sizing KAT for test_data/refs/Listeria_phage_B056.fasta,
the bincode .bxi layout, and an independent pure-Python restatement of the search loop."""
import json
import os
import struct

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REFS = os.path.join(HERE, "golden", "refs")
PHAGES = ["Listeria_phage_B021", "Listeria_phage_B051", "Listeria_phage_B056", "Listeria_phage_B545"]


def test_xxh3_published_kats(orc):
    with open(os.path.join(HERE, "golden", "xxh3_kat.json")) as f:
        kat = json.load(f)
    assert len(kat["vectors"]) > 1000
    for v in kat["vectors"]:
        assert orc.xxh3(bytes.fromhex(v["hex"]), v["seed"]) == v["h"]


def test_xxh3_survey_appendix_c(orc):
    # hex digests for seeds 0..3 and `% 50_000_000`
    want = {
        b"ATGC": ("caaf223612b989e9 1fe32407d1d902a7 0179b9fcb0a2e122 1f867a716405d144", [23535593, 43116071, 16278946, 32989892]),
        b"A" * 21: ("1b772345efdb0578 805f68dc5fe80a71 0d2d650c1021f29b 359baf9f25b4d395", [36446328, 3424497, 29715867, 17600789]),
        b"TAATTAAATCTAACAATTTCGTTACAGATTT": ("2c624549743ccc73 df0b2df1ea809a28 0a197e76821ed30b 76a89e4cd5fef317", [21544179, 46411816, 1344651, 7845143]),
    }
    for b, (hx, mods) in want.items():
        hs = [orc.xxh3(b, s) for s in range(4)]
        assert [f"{h:016x}" for h in hs] == hx.split()
        assert [h % 50_000_000 for h in hs] == mods


def test_seq_rs_can_detect_no_n(orc):  # src/seq.rs:72-76
    L = orc.lib()
    assert L.orc_has_no_n(b"AAGT", 4)
    assert not L.orc_has_no_n(b"NAGT", 4)
    assert L.orc_has_no_n(b"acgtACGT", 8)
    for bad in b"NnUuRY-*\n\r xX":
        assert not L.orc_is_good_base(bad)


def test_revcomp_switch_base(orc):  # src/kmer.rs:839-863
    assert orc.revcomp(b"ACGTacgt") == b"acgtACGT"
    assert orc.revcomp(b"AUuNnXx-") == b"NNNnNaAT"
    assert orc.revcomp(b"") == b""


def test_qual_mask(orc):  # src/seq.rs:36-56
    seq, qual = b"ACGTACGT", b"II#I0/5I"
    assert orc.qual_mask(seq, qual, 0) == seq
    # threshold 15 -> chars < chr(48) = '0' are masked
    assert orc.qual_mask(seq, qual, 15) == b"ACNTANGT"


def test_simple_bloom_use_filter(orc):  # src/simple_bloom.rs:60-66 (m = 250_000_000, 4 hashes)
    ix = orc.Index(250_000_000, 4, 4, 1)
    ix.insert(0, b"ATGC")
    assert ix.contains(0, b"ATGC") is True
    assert ix.contains(0, b"ATGT") is False
    rows = np.flatnonzero(ix.rows()[:, 0])
    assert sorted(rows.tolist()) == sorted(orc.xxh3(b"ATGC", s) % 250_000_000 for s in range(4))


def test_bitvec_bit_layout(orc):
    # lib.rs:465-474/492-500: bit i lives at storage[i/32] >> (i%32); from_bytes (lib.rs:335-363) is MSB-first per byte
    ix = orc.Index(4, 1, 4, 40)
    assert ix.w32 == 2
    rows = ix.rows()
    # BitVec::from_bytes(&[0b10100000, 0b00010010]) == bits {0, 2, 11, 14}
    for c in (0, 2, 11, 14, 33):
        rows[1, c // 32] |= np.uint32(1 << (c % 32))
    assert rows[1, 0] == (1 << 0) | (1 << 2) | (1 << 11) | (1 << 14)
    assert rows[1, 1] == 1 << 1


def test_canonical_choice_and_case(orc):
    km = orc.Kmers(4)
    km.kmerize_vector(b"ACGTTNAAAC", 1)      # windows with N dropped; upper-cased after the raw compare
    d = km.as_dict()
    assert b"ACGT" in d and d[b"ACGT"] == 1   # palindrome: takes the rc branch, same string
    assert b"AACG" in d                        # CGTT -> rc AACG is smaller
    assert all(b"N" not in k for k in d)
    km = orc.Kmers(4)
    km.kmerize_vector(b"acgaACGA", 1)          # compare is case-sensitive, THEN upper-cased
    d = km.as_dict()
    assert set(d) == {b"ACGA", b"CGAA", b"GAAC", b"AACG", b"TCGT"} or all(k == k.upper() for k in d)
    assert all(k == k.upper() for k in d)
    km = orc.Kmers(4)
    km.kmerize_skip_n_set(b"acgaACGA", 1)      # read_id path: no upper-casing (Q2)
    assert any(k != k.upper() for k in km.as_dict())
    km = orc.Kmers(4)
    assert km.kmerize_string(b"ACNT") == 0     # kmerize_string has no N filter (Q3)
    assert len(km) == 1
    assert orc.Kmers(5).kmerize_string(b"ACGT") == -1   # None


def test_sizing_kat_phage_b056(orc):  # 42 records, 33 726 bp, 32 634 distinct canonical 27-mers
    seqs = orc.read_fasta(os.path.join(REFS, "Listeria_phage_B056.fasta"))
    assert len(seqs) == 42 and sum(map(len, seqs)) == 33726
    km = orc.Kmers(27)
    for s in seqs:
        km.kmerize_vector(s, 1)
    assert len(km) == 32634


def test_sizing_kat_egd_e(orc, tmp_path):
    """the 2 912 954 distinct canonical 31-mers of refs/LmonoEGDe.fasta (configs[0]'s query genome, 2.94 Mbp) — the
    second sizing KAT the survey asked the C oracle to re-derive.  The genome is stored xz-compressed (0.8 MB) under tests/golden/genomes/
    and unpacked for the oracle's plain-file reader."""
    import lzma
    path = tmp_path / "LmonoEGDe.fasta"
    path.write_bytes(lzma.open(os.path.join(HERE, "golden", "genomes", "LmonoEGDe.fasta.xz")).read())
    seqs = orc.read_fasta(str(path))
    km = orc.Kmers(31)
    for s in seqs:
        km.kmerize_vector(s, 1)
    assert len(km) == 2_912_954


def _write_ref_tsv(tmp_path):
    p = tmp_path / "ref_file.txt"
    # same shape as test_data/ref_file.txt (accession \t path), deliberately unsorted
    p.write_text("".join(f"{n}\t{os.path.join(REFS, n + '.fasta')}\n" for n in reversed(PHAGES)))
    return str(p)


@pytest.fixture(scope="module")
def phage_index(orc, tmp_path_factory):
    # test.sh:3 parameters: build -s 750000 -n 4 -k 27
    return orc.Index.build_single(_write_ref_tsv(tmp_path_factory.mktemp("phage")), 750000, 4, 27)


def test_build_single_colours_sorted(phage_index):
    assert phage_index.colors() == sorted(PHAGES)          # build.rs:102-113
    assert phage_index.n_ref_kmers()[2] == 32634            # B056, build.rs:92
    assert phage_index.w32 == 1


def test_bxi_layout_and_roundtrip(orc, phage_index, tmp_path):
    p = str(tmp_path / "phage.bxi")
    phage_index.save(p)
    raw = open(p, "rb").read()
    m, n, k, nc = struct.unpack_from("<4Q", raw, 0)
    assert (m, n, k, nc) == (750000, 4, 27, 4)
    off = 32
    for c in range(4):
        cid, ln = struct.unpack_from("<2Q", raw, off)
        name = raw[off + 16: off + 16 + ln].decode()
        assert (cid, name) == (c, sorted(PHAGES)[c])
        off += 16 + ln
    (nrows,) = struct.unpack_from("<Q", raw, off)
    off += 8
    rows = phage_index.rows()
    assert nrows == int((rows[:, 0] != 0).sum())
    r0, w32 = struct.unpack_from("<2Q", raw, off)
    (word,) = struct.unpack_from("<I", raw, off + 16)
    (nbits,) = struct.unpack_from("<Q", raw, off + 20)
    assert w32 == 1 and nbits == 4 and word == rows[r0, 0] and word != 0
    assert len(raw) == off + nrows * 28 + 8 + sum(8 + len(n_) + 8 for n_ in PHAGES)
    back = orc.Index.read(p)
    assert np.array_equal(back.rows(), rows)
    assert back.colors() == phage_index.colors() and back.n_ref_kmers() == phage_index.n_ref_kmers()
    p2 = str(tmp_path / "again.bxi")
    back.save(p2)
    assert open(p2, "rb").read() == raw


def _py_search_count(rows, m, n_hash, n_colors, kmers, freq):
    """Independent restatement of batch_search_pe.rs:45-84 with python-xxhash (a second opinion on the oracle)."""
    import xxhash
    hits = [0] * n_colors
    nu = [0] * n_colors
    sf = [0] * n_colors
    for km, f in zip(kmers, freq):
        acc = None
        for s in range(n_hash):
            r = xxhash.xxh3_64_intdigest(km, seed=s) % m
            word = int(rows[r, 0])
            if word == 0:
                acc = None
                break
            acc = word if acc is None else acc & word
        if acc is None:
            continue
        cs = [c for c in range(n_colors) if acc >> c & 1]
        for c in cs:
            hits[c] += 1
        if len(cs) == 1:
            nu[cs[0]] += 1
            sf[cs[0]] += f
    return hits, nu, sf


def test_search_count_vs_independent_python(orc, phage_index):
    xxhash = pytest.importorskip("xxhash")  # noqa: F841
    seqs = orc.read_fasta(os.path.join(REFS, "Listeria_phage_B056.fasta"))
    km = orc.Kmers(27)
    for s in seqs[:6]:
        km.kmerize_vector(s, 1)
    keys, counts = km.keys(), km.counts()
    rng = np.random.default_rng(5)
    extra = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=(500, 27))]
    keys = np.concatenate([keys, extra])
    counts = np.concatenate([counts, rng.integers(1, 9, size=500).astype(np.uint64)])
    hits, nu, sf, uc = phage_index.search_count(keys, counts)
    ph, pn, ps = _py_search_count(phage_index.rows(), 750000, 4, 4, [k.tobytes() for k in keys], counts.tolist())
    assert hits.tolist() == ph and nu.tolist() == pn and sf.tolist() == ps
    assert hits[2] >= len(km)                       # every B056 k-mer hits colour B056
    assert int((uc != 0xFFFFFFFF).sum()) == int(nu.sum())


def test_perfect_search(orc, phage_index):
    seqs = orc.read_fasta(os.path.join(REFS, "Listeria_phage_B056.fasta"))
    km = orc.Kmers(27)
    km.kmerize_vector(seqs[0], 1)
    words, missing = phage_index.search_perfect(km.keys())
    assert not missing and words[0] >> 2 & 1        # B056 = colour 2 contains all its own k-mers
    keys = np.concatenate([km.keys(), np.frombuffer(b"ACGT" * 6 + b"ACG", np.uint8)[None, :]])
    words2, _ = phage_index.search_perfect(keys)
    assert words2[0] & ~words[0] == 0


def test_report_formats(orc, phage_index):
    seqs = orc.read_fasta(os.path.join(REFS, "Listeria_phage_B056.fasta"))
    km = orc.Kmers(27)
    for s in seqs:
        km.kmerize_vector(s, 1)
    hits, nu, sf, uc = phage_index.search_count(km.keys(), km.counts())
    modes = orc.unique_modes(uc, km.counts(), 4)
    rep = phage_index.generate_report("q.fasta", hits, nu, sf, modes, len(km), 0.35)
    row = [r for r in rep.splitlines() if "B056" in r][0].split("\t")
    assert row[:4] == ["q.fasta", "32634", "Listeria_phage_B056", "1.00"]   # reports.rs:39-42 {:.2}
    gene = phage_index.generate_report_gene("q.fasta", hits, len(km), 0.35)
    assert "q.fasta\tListeria_phage_B056\t32634\t1.000" in gene.splitlines()  # reports.rs:59 {:.3}


def test_auto_cutoff(orc):  # src/kmer.rs:866-942
    km = orc.Kmers(5)
    km.kmerize_vector(b"AAAAACCCCC", 1)
    assert len(km) == 6 and km.auto_cutoff() == 0    # mean multiplicity < 1.5
    km = orc.Kmers(3)
    km.kmerize_vector(b"ACGTAC", 1)                  # {ACG: 2, GTA: 2}: `d1.len() - 1` underflows in the reference
    assert km.as_dict() == {b"ACG": 2, b"GTA": 2} and km.auto_cutoff() == -1
    # multiplicities: histogram {1: 30, 2: 4, 3: 1, 4: 2, 5: 6, 6: 9, 7: 6, 8: 2, 9: 1}
    h = orc.lib()
    km = orc.Kmers(4)
    import itertools
    keys = ["".join(p).encode() for p in itertools.product("ACGT", repeat=4)]
    mult = [1] * 30 + [2] * 4 + [3] + [4] * 2 + [5] * 6 + [6] * 9 + [7] * 6 + [8] * 2 + [9]
    for key, mu in zip(keys, mult):
        h.orc_kmers_insert(km.h, key, mu)
    # coverages = [30,4,1,2,6,9,6,2]; d1 = [4, .5, .33, .67, 1.5, 3]; first_pos_d1 = 2; mean = (0*4+1*1+2*2+3*6+4*9+5*6+6*2)/30 = 3.37
    assert km.auto_cutoff() == 2
    assert len(km.clean_map(2)) == 1 + 2 + 6 + 9 + 6 + 2 + 1


def test_search_index_order_semantics(orc):
    # read_id_mt_pe.rs:104-165 with start_sample: colours outside the sampled set are never counted later
    ix = orc.Index(1 << 12, 2, 5, 3)
    for c in range(3):
        ix.set_color(c, f"c{c}", 100)
    a, b, c_ = b"AAAAC", b"AAACC", b"AACCC"
    ix.insert(0, a); ix.insert(0, b); ix.insert(1, b); ix.insert(1, c_); ix.insert(0, c_)
    ks = np.frombuffer(a + b + c_, np.uint8).reshape(3, 5)
    assert ix.search_index_classic(ks).tolist() == [3, 2, 0, 0]
    assert ix.search_index(ks, 1).tolist() == [3, 0, 0, 0]      # sampled set = {0} after the first k-mer
    assert ix.search_index(ks, 2).tolist() == [3, 2, 0, 0]
    miss = np.frombuffer(a + b"GGGGG" + c_, np.uint8).reshape(3, 5)
    assert ix.search_index_classic(miss).tolist() == [1, 0, 0, 1]  # absent row: report[C] += 1; break


def test_kmer_poll_plus(orc):  # read_id_mt_pe.rs:187-251, SURVEY.md App. E1
    ix = orc.Index(750000, 4, 27, 4)
    for c, n in enumerate([30000, 31000, 32634, 29000]):
        ix.set_color(c, f"phage{c}", n)
    assert ix.kmer_poll_plus(np.array([0, 0, 0, 0, 1], np.uint64), 50) == ("no_hits", 0, 50, "accept", 0)
    assert ix.kmer_poll_plus(np.array([0, 0, 0, 0, 0], np.uint64), 0) == ("no_hits", 0, 0, "accept", 0)
    assert ix.kmer_poll_plus(np.array([0, 0, 40, 0, 0], np.uint64), 50) == ("phage2", 40, 50, "accept", 1)
    assert ix.kmer_poll_plus(np.array([40, 0, 40, 0, 0], np.uint64), 50) == ("phage0,phage2", 40, 50, "reject", 2)
    # one hit out of 1000 k-mers with p_false ~ 6e-4: hits(1) > critical(0.6) and pmf >= 1e-3 -> not significant
    assert ix.kmer_poll_plus(np.array([1, 0, 0, 0, 0], np.uint64), 1000) == ("no_significant_hits", 0, 1000, "reject", 0)
    p = orc.false_prob(750000, 4, 30000)
    assert abs(p - (1 - np.exp(-4 * 30000.5 / 749999)) ** 4) < 1e-15


def _py_find_minimizer(kmer: bytes, m: int) -> bytes:
    """Independent restatement of kmer.rs:971-986: window 0 contributes its forward m-mer only, later windows also their
    reverse-complement m-mer; strict `<` keeps the first minimum."""
    comp = {65: 84, 67: 71, 71: 67, 84: 65, 97: 116, 99: 103, 103: 99, 116: 97}   # switch_base keeps the case (kmer.rs:847-863)
    rc = bytes(comp.get(c, c) for c in reversed(kmer))
    n = len(kmer)
    best = kmer[:m]
    for i in range(1, n - m + 1):
        best = min(best, kmer[i:i + m], rc[n - (i + m):n - i])
    return best


def test_find_minimizer(orc):  # src/kmer.rs:971-986
    assert orc.find_minimizer(b"TTTTA", 3) == b"AAA"            # revcomp of window 1 (TTT) wins
    assert orc.find_minimizer(b"TTTAC", 3) == b"GTA"            # revcomp GTAAA: its AAA sits over window 0 and is never compared
    assert orc.find_minimizer(b"TTTGG", 5) == b"TTTGG"          # m == k: the forward k-mer, its revcomp is never compared
    assert orc.find_minimizer(b"ACGTACGTAC", 4) == b"ACGT"
    rng = np.random.default_rng(5)
    for k, m in ((27, 15), (31, 15), (21, 7), (35, 19), (16, 16), (64, 33)):
        for _ in range(300):
            km = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), k))
            assert orc.find_minimizer(km, m) == _py_find_minimizer(km, m)


def test_minimizer_set_of_read(orc):  # src/kmer.rs:363-394: canonical k-mers without N, one minimizer each, -d stride
    rng = np.random.default_rng(6)
    read = bytearray(rng.choice(np.frombuffer(b"ACGT", np.uint8), 120))
    read[40] = ord("N")
    read = bytes(read)
    for d in (1, 3):
        km = orc.Kmers(27)
        km.kmerize_skip_n_set(read, d)
        want = []
        for key in km.keys():
            mm = _py_find_minimizer(key.tobytes(), 15)
            if mm not in want:
                want.append(mm)
        got = [r.tobytes() for r in orc.minimizer_set([read], 27, 15, d).keys()]
        assert got == want and 0 < len(want) < len(km)


def test_mxi_layout_and_roundtrip(orc, tmp_path):  # bigsi.rs:40-49, 71-83: BigsyMapMiniNew = BigsyMapNew + m_size after k_size
    tsv = _write_ref_tsv(tmp_path)
    mix = orc.Index.build_single_mini(tsv, 750000, 4, 27, 15)
    full = orc.Index.build_single(tsv, 750000, 4, 27)
    assert mix.m_size == 15 and mix.colors() == sorted(PHAGES)
    assert mix.n_ref_kmers() == full.n_ref_kmers()              # FASTA accessions: distinct k-mers, not minimizers (build.rs:444)
    assert 0 < int((mix.rows()[:, 0] != 0).sum()) < int((full.rows()[:, 0] != 0).sum())
    # every k-mer of an accession is found again through its minimizer, under that accession's colour
    seqs = orc.read_fasta(os.path.join(REFS, PHAGES[1] + ".fasta"))
    km = orc.Kmers(27)
    km.kmerize_vector(seqs[0], 1)
    import xxhash
    for key in km.keys()[:200]:
        mm = _py_find_minimizer(key.tobytes(), 15)
        for s in range(4):
            assert int(mix.rows()[xxhash.xxh3_64_intdigest(mm, seed=s) % 750000, 0]) >> 1 & 1
    p = str(tmp_path / "phage.mxi")
    mix.save(p)
    raw = open(p, "rb").read()
    assert struct.unpack_from("<5Q", raw, 0) == (750000, 4, 27, 15, 4)
    back = orc.Index.read(p)
    assert back.m_size == 15 and np.array_equal(back.rows(), mix.rows())
    assert back.colors() == mix.colors() and back.n_ref_kmers() == mix.n_ref_kmers()
    p2 = str(tmp_path / "again.mxi")
    back.save(p2)
    assert open(p2, "rb").read() == raw


def test_sparse_structure_variant_equals_dense(orc, phage_index):
    """the bench's "faithful structure" CPU figure runs the same loop over an FNV-hashed row map: same counts"""
    seqs = orc.read_fasta(os.path.join(REFS, PHAGES[3] + ".fasta"))
    km = orc.Kmers(27)
    for s in seqs:
        km.kmerize_vector(s, 1)
    keys = km.keys()[:4000]
    freq = km.counts()[:4000].astype(np.uint64)
    rng = np.random.default_rng(2)
    noise = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (500, 27))]
    keys = np.concatenate([keys, noise])
    freq = np.concatenate([freq, np.ones(500, np.uint64)])
    want = phage_index.search_count(keys, freq)
    sp = phage_index.sparse_map()
    got = phage_index.search_count_sparse(sp, keys, freq)
    orc.sparse_free(sp)
    assert all(np.array_equal(w, g) for w, g in zip(want[:3], got)) and want[0].sum() >= 4000


def _py_readid(rows, m, n_hash, n_colors, k, msz, mates, d, S):
    """Independent restatement (python-xxhash, python sets) of parallel_vec's per-read work — kmer.rs:221-243 / :363-394
    for the set (first-occurrence order, the documented normalisation), read_id_mt_pe.rs:66-102 (S == 0) / :104-165 for the
    search — returning (report[C+1], n_kmers, too_short)."""
    import xxhash
    comp = {65: 84, 67: 71, 71: 67, 84: 65, 97: 116, 99: 103, 103: 99, 116: 97}
    if len(mates[0]) < k:
        return None, 0, True
    keys = []
    seen = set()
    for l in mates:
        if len(l) < k:
            continue
        rc = bytes(comp.get(c, c) for c in reversed(l))
        L = len(l)
        for i in range(0, L - k + 1, d):
            w = l[i:i + k]
            if any(c not in b"ACGTacgt" for c in w):
                continue
            r = rc[L - (i + k):L - i]
            canon = w if w < r else r
            if msz:
                canon = _py_find_minimizer(canon, msz).upper()
            if canon not in seen:
                seen.add(canon)
                keys.append(canon)
    report = [0] * (n_colors + 1)
    sampled = set()
    for counter, key in enumerate(keys):
        acc = None
        for s in range(n_hash):
            word = 0
            r = xxhash.xxh3_64_intdigest(key, seed=s) % m
            for w in range(rows.shape[1]):
                word |= int(rows[r, w]) << (32 * w)
            if word == 0:
                acc = None
                break
            acc = word if acc is None else acc & word
        if acc is None:
            report[n_colors] += 1
            break
        cols = [c for c in range(n_colors) if acc >> c & 1]
        if S == 0:
            for c in cols:
                report[c] += 1
        elif counter < S:
            for c in cols:
                sampled.add(c)
                report[c] += 1
        else:
            for c in cols:
                if c in sampled:
                    report[c] += 1
    return report, len(keys), False


@pytest.mark.parametrize("msz", [0, 11])
def test_readid_counts_vs_independent_python(orc, msz):
    rng = np.random.default_rng(31 + msz)
    m, n_hash, k, C = 20_011, 3, 21, 40
    genome = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 6000)].tobytes()
    oix = orc.Index(m, n_hash, k, C)
    if msz:
        oix.set_minimizer(msz)
    for c in range(C):
        oix.set_color(c, f"a{c}", 100)
    km = orc.Kmers(k)
    km.kmerize_vector(genome[:4000], 1)
    for i, key in enumerate(km.keys()):
        oix.insert(i % 7, key.tobytes())
        if i % 3 == 0:
            oix.insert(20 + i % 11, key.tobytes())
    reads = []
    for i in range(120):
        L = int(rng.integers(15, 200))
        st = int(rng.integers(0, len(genome) - L))
        a = bytearray(genome[st:st + L])
        if i % 5 == 0:
            a[int(rng.integers(0, L))] = ord("N")
        if i % 7 == 0:
            a = bytearray(bytes(a).lower())
        if i % 11 == 0:
            for p in rng.integers(0, L, 4):
                a[p] = ord("acgt"[int(rng.integers(0, 4))])
        mates = [bytes(a)]
        if i % 2:
            mates.append(genome[st + 50:st + 50 + int(rng.integers(5, 150))])
        reads.append(mates)
    from test_gpu_readid import pack_reads
    bases, seq_off, read_seq0 = pack_reads(reads)
    for d, S in ((1, 3), (1, 0), (4, 2), (2, 1000)):
        rep, nk, st = oix.readid_counts(bases, seq_off, read_seq0, d, S)
        for i, mates in enumerate(reads):
            want, n_keys, short = _py_readid(oix.rows(), m, n_hash, C, k, msz, mates, d, S)
            assert bool(st[i]) == short, i
            if short:
                continue
            assert nk[i] == n_keys and list(rep[i]) == want, (i, d, S)
        assert rep[:, :C].sum() > 0 and rep[:, C].sum() > 0
        # the rayon analogue (contiguous slices of the batch on pthreads) returns the same rows
        for nt in (2, 7, 200):
            rep_mt, nk_mt, st_mt = oix.readid_counts(bases, seq_off, read_seq0, d, S, n_threads=nt)
            assert np.array_equal(rep, rep_mt) and np.array_equal(nk, nk_mt) and np.array_equal(st, st_mt)


def _py_canon_windows(l: bytes, k: int, d: int = 1):
    comp = {65: 84, 67: 71, 71: 67, 84: 65, 97: 116, 99: 103, 103: 99, 116: 97, 117: 97, 85: 65, 110: 110}
    rc = bytes(comp.get(c, 78) for c in reversed(l))
    L = len(l)
    for i in range(0, L - k + 1, d):
        w = l[i:i + k]
        if all(c in b"ACGTacgt" for c in w):
            r = rc[L - (i + k):L - i]
            yield w if w < r else r


def _py_qual_mask(seq: bytes, qual: bytes, q: int) -> bytes:   # seq.rs:36-56
    if q == 0:
        return seq
    return bytes(78 if qc < q + 33 else seq[i] for i, qc in enumerate(qual))


def test_kmer_maps_vs_independent_python(orc, tmp_path):
    """kmerize_vector (kmer.rs:87-125, upper-cases), kmers_from_fq_qual (:461-510) and kmers_fq_pe_qual (:581-655, stops
    with the shorter file, keeps the case) restated with python dicts and gzip, against the oracle's C."""
    import gzip
    from collections import Counter
    from util import synth_fastq_records, write_fastq_gz
    rng = np.random.default_rng(12)
    genomes = [np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 5000)].tobytes() for _ in range(2)]
    mixed = bytearray(genomes[0][:900])
    mixed[100:180] = bytes(mixed[100:180]).lower()
    mixed[300] = ord("N"); mixed[301] = ord("n"); mixed[500] = ord("R")
    for k, d in ((21, 1), (5, 3), (31, 7)):
        km = orc.Kmers(k)
        km.kmerize_vector(bytes(mixed), d)
        want = Counter(w.upper() for w in _py_canon_windows(bytes(mixed), k, d))
        assert km.as_dict() == dict(want)
    r1 = synth_fastq_records(rng, genomes, 120, 100, mate=0)
    r2 = synth_fastq_records(rng, genomes, 110, 100, mate=1)
    f1, f2 = str(tmp_path / "x_1.fastq.gz"), str(tmp_path / "x_2.fastq.gz")
    write_fastq_gz(f1, r1, multi_member=True)
    write_fastq_gz(f2, r2)

    def records(path):
        lines = gzip.open(path, "rb").read().split(b"\n")
        return [(lines[i + 1], lines[i + 3]) for i in range(0, len(lines) - 3, 4)]
    for q in (0, 15, 30):
        want = Counter()
        for seq, qual in records(f1):
            want.update(_py_canon_windows(_py_qual_mask(seq, qual, q), 27))
        assert orc.kmers_from_fq_qual(f1, 27, q).as_dict() == dict(want)
        want = Counter()
        for (s1, q1), (s2, q2) in zip(records(f1), records(f2)):          # zip stops with the shorter file, like the reference
            for seq, qual in ((s1, q1), (s2, q2)):
                want.update(_py_canon_windows(_py_qual_mask(seq, qual, q), 27))
        assert orc.kmers_fq_pe_qual(f1, f2, 27, q).as_dict() == dict(want)
        assert len(want) > 2000


def _py_auto_cutoff(mults):
    """kmer.rs:866-942 restated; None where the reference would panic (usize underflow, index out of range) and float
    semantics as in Rust (x/0 = inf, 0/0 = NaN, comparisons with NaN false)."""
    import math
    from collections import Counter

    def div(a, b):
        if b == 0:
            return math.nan if a == 0 else math.inf
        return a / b
    histo = Counter(mults)
    max_cov = max(mults)
    total_mean = sum(i * p for i, p in histo.items()) / len(mults)
    if total_mean < 1.5:
        return 0
    cov = [histo.get(c, 0) for c in range(1, max_cov)]
    if len(cov) < 1:                      # `1..coverages.len() - 1` underflows
        return None
    d1 = [div(float(cov[i]), float(cov[i + 1])) for i in range(1, len(cov) - 1)]
    if len(d1) < 1:                       # `0..d1.len() - 1` underflows
        return None
    d2 = []
    for i in range(len(d1) - 1):
        a, b = d1[i], d1[i + 1]
        if math.isnan(a) or math.isnan(b):
            d2.append(math.nan)
        elif math.isinf(a) and math.isinf(b):
            d2.append(math.nan)
        elif math.isinf(b):
            d2.append(0.0)
        elif b == 0:
            d2.append(math.nan if a == 0 else math.inf)
        else:
            d2.append(a / b)
    p1 = next((i + 1 for i, p in enumerate(d1) if p < 1.0), 0)
    p2 = next((i + 1 for i, p in enumerate(d2) if p < 1.0), 0)
    bigsum = sum(i * p for i, p in enumerate(cov[1:]))
    num = sum(cov[1:])
    mean = div(float(bigsum), float(num))
    if p1 > 0 and p1 < mean * 0.75:
        return p1
    if p2 > 0:
        return p2
    if math.isnan(mean):
        return 1                          # `NaN.ceil() as usize` saturates to 0; max(1, 0)
    return max(1, math.ceil(mean / 2.0))


def test_auto_cutoff_vs_independent_python(orc):
    import itertools
    rng = np.random.default_rng(77)
    keys = ["".join(p).encode() for p in itertools.product("ACGT", repeat=6)]
    n_cases = n_panic = 0
    for case in range(300):
        shape = case % 5
        n = int(rng.integers(3, 600))
        if shape == 0:        # sequencing-like: error k-mers at 1-2, a coverage peak
            mults = np.concatenate([rng.integers(1, 3, n), rng.poisson(int(rng.integers(5, 40)), n) + 1])
        elif shape == 1:
            mults = rng.integers(1, int(rng.integers(2, 12)), n)
        elif shape == 2:
            mults = rng.geometric(0.3, n)
        elif shape == 3:
            mults = np.full(n, int(rng.integers(1, 6)))
        else:
            mults = rng.choice([1, 2, 3, 9, 10, 30], n)
        mults = [int(x) for x in mults[:len(keys)]]
        km = orc.Kmers(6)
        for key, mu in zip(keys, mults):
            orc.lib().orc_kmers_insert(km.h, key, mu)
        want = _py_auto_cutoff(mults)
        got = km.auto_cutoff()
        if want is None:
            assert got == -1, (case, mults[:20])
            n_panic += 1
        else:
            assert got == want, (case, sorted(mults)[:30], want, got)
        n_cases += 1
    assert n_cases == 300 and n_panic >= 1


def test_kmer_poll_plus_vs_independent_python(orc):
    """read_id_mt_pe.rs:168-251 restated with scipy's binomial pmf standing in for `probability::Binomial::mass`: random sparse
    reports, cases within 5 % of the pmf == fp_correct boundary skipped (two correct pmf implementations may differ in the
    last bits there); ties keep ascending colour id (the documented normalisation of the reference's arbitrary order)."""
    from scipy.stats import binom
    rng = np.random.default_rng(55)
    C, m, n_hash = 12, 750_000, 4
    ix = orc.Index(m, n_hash, 27, C)
    n_ref = [int(x) for x in rng.integers(5_000, 120_000, C)]
    for c in range(C):
        ix.set_color(c, f"acc{c:02d}", n_ref[c])
    p_false = [orc.false_prob(m, n_hash, n) for n in n_ref]
    for c in range(C):      # read_id_mt_pe.rs:695-698
        assert abs(p_false[c] - (1.0 - np.exp(-(n_hash * (n_ref[c] + 0.5)) / (m - 1.0))) ** n_hash) < 1e-15
    n_done = 0
    outcomes = set()
    for case in range(600):
        klen = int(rng.integers(1, 300))
        report = np.zeros(C + 1, np.uint64)
        for c in rng.choice(C, size=int(rng.integers(0, 5)), replace=False):
            report[c] = int(rng.integers(1, klen + 1)) if case % 3 else int(rng.integers(1, 4))
        if case % 4 == 0:
            report[C] = 1
        if case % 7 == 0 and report[:C].any():       # force a tie at the top
            top = int(report[:C].max())
            report[int(rng.integers(0, C))] = top
        if not report.any():
            continue
        fp_correct = float(rng.choice([1e-3, 1e-2, 1e-6, 0.05]))
        near_boundary = False
        sig = []
        for c in sorted(range(C), key=lambda c: (-int(report[c]), c)):
            h = int(report[c])
            if h == 0:
                continue
            crit = klen * p_false[c]
            mpf = float(binom.pmf(h, klen, p_false[c]))
            if abs(mpf - fp_correct) <= 0.05 * fp_correct or h == crit:
                near_boundary = True
            if h < crit or (h > crit and mpf >= fp_correct):
                continue
            sig.append((c, h))
        if near_boundary:
            continue
        if not report[:C].any():
            want = ("no_hits", 0, klen, "accept", 0)
        elif not sig:
            want = ("no_significant_hits", 0, klen, "reject", 0)
        else:
            tops = [f"acc{c:02d}" for c, h in sig if h == sig[0][1]]
            want = (",".join(tops), sig[0][1], klen, "accept" if len(tops) == 1 else "reject", len(tops))
        assert ix.kmer_poll_plus(report, klen, fp_correct) == want, (case, report, klen, fp_correct)
        outcomes.add(want[0] if want[0].startswith("no_") else want[3])
        n_done += 1
    assert n_done > 400 and outcomes == {"no_hits", "no_significant_hits", "accept", "reject"}


def test_reports_vs_independent_python(orc):
    """reports.rs:8-62 restated with python formatting: a row per colour with hits (ascending colour id, the documented
    normalisation), `{:.2}` / `{:.3}` proportions, mean = Σfreq / n_unique, thresholds `>` (default) and `>=` (-g)."""
    rng = np.random.default_rng(91)
    C = 9
    for case in range(200):
        ix = orc.Index(1000, 2, 21, C)
        n_ref = [int(x) for x in rng.integers(0 if case % 10 == 0 else 1, 5000, C)]
        for c in range(C):
            ix.set_color(c, f"genome_{c}", n_ref[c])
        num_kmers = int(rng.integers(1, 6000))
        hits = rng.integers(0, 5000, C).astype(np.uint64)
        hits[rng.random(C) < 0.3] = 0
        nu = np.minimum(hits, rng.integers(0, 3000, C).astype(np.uint64))
        nu[rng.random(C) < 0.3] = 0
        sf = (nu * rng.integers(1, 400, C).astype(np.uint64) + rng.integers(0, 7, C).astype(np.uint64)) * (nu > 0)
        modes = rng.integers(1, 300, C).astype(np.uint64) * (nu > 0)
        cov = float(rng.choice([0.35, 0.0, 0.9, 0.5, 1.0]))
        want = []
        for c in range(C):
            if hits[c] == 0:
                continue
            g = float("inf") if n_ref[c] == 0 else int(hits[c]) / n_ref[c]
            if g > cov:
                mean = int(sf[c]) / int(nu[c]) if nu[c] else 0.0
                want.append(f"q.fq\t{num_kmers}\tgenome_{c}\t{g:.2f}\t{mean:.2f}\t{int(modes[c])}\t{int(nu[c])}")
        got = ix.generate_report("q.fq", hits, nu, sf, modes, num_kmers, cov)
        assert got.splitlines() == want, case
        want = [f"q.fq\tgenome_{c}\t{num_kmers}\t{int(hits[c]) / num_kmers:.3f}" for c in range(C)
                if hits[c] and int(hits[c]) / num_kmers >= cov]
        assert ix.generate_report_gene("q.fq", hits, num_kmers, cov).splitlines() == want, case
    # mode (reports.rs:65-77): the most frequent multiplicity among a colour's unique k-mers; ties -> the smallest value
    uc = np.array([0, 0, 0, 1, 1, 0xFFFFFFFF, 2, 2], np.uint32)
    fr = np.array([5, 7, 5, 9, 8, 5, 4, 4], np.uint64)
    assert list(orc.unique_modes(uc, fr, 4)) == [5, 8, 4, 0]
