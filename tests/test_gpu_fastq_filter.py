"""cid_fastq_filter: the kept records of a classified step, written by the device as block-gzip members, against a restatement of the
reference's read_filter (src/read_filter.rs:60-116 / :154-178): the lines as lines() gives them, four per record, a kept record written
as `header\\nsequence\\n+\\nquality\\n` — the sequence as the input has it, whatever followed the '+' dropped."""
import ctypes as C
import zlib

import numpy as np
import pytest

import colorid_amd
from colorid_amd._lib import CID_ERR_INVALID, CID_ERR_STATE
from test_gpu_fastq import line_loop_records, world  # noqa: F401  (the toy index of the front end's tests)

pytestmark = pytest.mark.gpu


def make_text(rng, genomes, n, mate, last_newline):
    out = bytearray()
    for i in range(n):
        g = genomes[int(rng.integers(len(genomes)))]
        L = int(rng.integers(30, 151))
        a = int(rng.integers(0, len(g) - L))
        seq = g[a:a + L]
        if i == 7:
            seq = b""                                                            # an empty sequence
        if i == 150:
            seq = (g * 12)[:70_000]                                              # a record that spans block-gzip members
        qual = bytes(rng.integers(35, 74, len(seq)).astype(np.uint8))
        eol = b"\r\n" if i % 5 == 2 else b"\n"
        plus = b"+read%d" % i if i % 3 == 1 else b"+"
        out += b"@read%d/%d some description" % (i, mate) + eol + seq + eol + plus + eol + qual + eol
    if not last_newline:
        out = out[:-1]                                                           # an unterminated last line (the last record ends in "\n")
    return bytes(out)


def restated(records, keep):
    return b"".join(h + b"\n" + s + b"\n+\n" + q + b"\n" for (h, s, q), k in zip(records, keep) if k)


def gunzip(blob):
    out, rest = [], blob
    while rest:
        d = zlib.decompressobj(31)
        out.append(d.decompress(rest))
        assert d.eof
        rest = d.unused_data
    return b"".join(out)


def patterns(rng, n):
    return {"none": np.zeros(n, np.uint8), "all": np.ones(n, np.uint8), "alternating": (np.arange(n) % 2).astype(np.uint8),
            "random": (rng.random(n) < 0.4).astype(np.uint8)}


@pytest.mark.parametrize("n_files,q", [(1, 15), (2, 0)])
def test_filter_equals_the_restated_read_filter(hip_ctx, world, n_files, q):
    oix, hx, genomes = world
    rng = np.random.default_rng(5 + n_files)
    texts = [make_text(rng, genomes, 300, f + 1, last_newline=(f == 1)) for f in range(n_files)]
    records = [line_loop_records(t) for t in texts]
    assert all(len(r) == 300 for r in records)
    fr = colorid_amd.FastqReader(hip_ctx, n_files, q)
    fr.keep_steps()
    got = {name: [b""] * n_files for name in ("none", "all", "alternating", "random")}
    kept = {name: 0 for name in got}
    want_keep = {name: [] for name in got}
    done = 0
    for part in range(2):                                                        # two pushes, cut inside a record
        for f in range(n_files):
            cut = len(texts[f]) * 2 // 5 + 11 * f
            fr.push_text(f, texts[f][:cut] if part == 0 else texts[f][cut:], last=(part == 1))
        ids = fr.classify(hx, 1, 3)[0]
        n = len(ids)
        assert n and ids == [r[0] for r in records[0][done:done + n]]
        for name, keep in patterns(rng, n).items():
            want_keep[name] += keep.tolist()
            for f in range(n_files):
                blob, n_members, n_kept = fr.filter(keep, f)
                assert n_kept == int(keep.sum())
                text = gunzip(blob)
                assert n_members == (len(text) + 65279) // 65280
                got[name][f] += text
            kept[name] += int(keep.sum())
        done += n
    assert done == 300
    for name in got:
        for f in range(n_files):
            assert got[name][f] == restated(records[f], want_keep[name]), (name, f)
    assert got["none"] == [b""] * n_files and kept["all"] == 300
    fr.close()


def test_filter_of_a_step_while_the_next_one_runs(hip_ctx, world):
    oix, hx, genomes = world
    rng = np.random.default_rng(9)
    text = make_text(rng, genomes, 300, 1, True)
    records = line_loop_records(text)
    cut = len(text) // 2 + 3
    fr = colorid_amd.FastqReader(hip_ctx, 1, 0)
    fr.keep_steps()
    fr.push_text(0, text[:cut])
    fr.classify_begin(hx, 1, 3)
    n1 = fr.classify_end()[0].value
    keep1 = (rng.random(n1) < 0.5).astype(np.uint8)
    fr.push_text(0, text[cut:], last=True)
    fr.classify_begin(hx, 1, 3)                                                 # step 2 is in flight: step 1 is still the one to filter
    blob, _, n_kept = fr.filter(keep1, 0)
    assert n_kept == int(keep1.sum()) and gunzip(blob) == restated(records[:n1], keep1)
    n2 = fr.classify_end()[0].value
    assert n1 + n2 == 300
    blob, _, n_kept = fr.filter(np.ones(n2, np.uint8), 0)
    assert n_kept == n2 and gunzip(blob) == restated(records[n1:], [1] * n2)
    fr.close()


def test_the_c_entry_point_without_a_record_and_without_room(hip_ctx, world):
    """what a caller of cid_fastq_filter itself relies on, for either file of a pair: a step without a complete record answers CID_OK with
    zeros whatever `keep` is; too little room answers CID_ERR_INVALID with the buffer untouched, *n_kept set and *members_bytes the very
    size with which the same call then succeeds"""
    oix, hx, genomes = world
    lib = hip_ctx.lib
    rng = np.random.default_rng(10)
    texts = []
    for mate in (1, 2):
        out = bytearray()
        for i in range(12):
            L = int(rng.integers(40, 61))
            a = int(rng.integers(0, len(genomes[i % 5]) - L))
            out += b"@s%d/%d\n" % (i, mate) + genomes[i % 5][a:a + L] + b"\n+\n" + bytes(rng.integers(35, 74, L).astype(np.uint8)) + b"\n"
        texts.append(bytes(out))
    records = [line_loop_records(t) for t in texts]
    fr = colorid_amd.FastqReader(hip_ctx, 2, 0)
    fr.keep_steps()
    nb, nm, nk = C.c_size_t(7), C.c_size_t(7), C.c_uint64(7)

    def call(keep, f, buf):
        return lib.cid_fastq_filter(fr.h, keep.ctypes.data_as(C.c_void_p) if keep is not None else None, f, buf.ctypes.data_as(C.c_void_p), buf.size,
                                    C.byref(nb), C.byref(nm), C.byref(nk))
    for f in range(2):
        fr.push_text(f, texts[f][:20])                                           # half a record
    assert len(fr.classify(hx, 1, 3)[0]) == 0
    out = np.full(64, 0xAB, np.uint8)
    for f in range(2):
        nb.value = nm.value = nk.value = 7
        assert call(None, f, out) == 0 and (nb.value, nm.value, nk.value) == (0, 0, 0) and np.all(out == 0xAB)
    for f in range(2):
        fr.push_text(f, texts[f][20:], last=True)
    assert len(fr.classify(hx, 1, 3)[0]) == 12
    keep = np.array([1, 0, 1, 1, 0, 1, 1, 1, 0, 1, 1, 0], np.uint8)
    for f in range(2):
        assert call(keep, f, out) == CID_ERR_INVALID and nb.value > out.size and np.all(out == 0xAB)
        assert (nk.value, nm.value) == (8, 1)
        room = np.full(nb.value, 0xAB, np.uint8)
        nk.value = 0
        assert call(keep, f, room) == 0 and nb.value == room.size and (nk.value, nm.value) == (8, 1)
        assert gunzip(room.tobytes()) == restated(records[f], keep)              # (gunzip takes every byte: the members end at the buffer's last)
    fr.close()


def test_filter_without_a_finished_step(hip_ctx, world):
    oix, hx, genomes = world
    fr = colorid_amd.FastqReader(hip_ctx, 1, 0)
    with pytest.raises(colorid_amd.CidError) as e:                               # the reader keeps no steps
        fr.filter(np.ones(4, np.uint8), 0)
    assert e.value.code == CID_ERR_STATE
    fr.keep_steps()
    with pytest.raises(colorid_amd.CidError) as e:                               # no step has ended
        fr.filter(np.ones(4, np.uint8), 0)
    assert e.value.code == CID_ERR_STATE
    fr.push_text(0, b"@r\nACGT\n+\nIIII\n", last=True)
    fr.classify_begin(hx, 1, 3)
    with pytest.raises(colorid_amd.CidError) as e:                               # begun, not ended
        fr.filter(np.ones(4, np.uint8), 0)
    assert e.value.code == CID_ERR_STATE
    assert fr.classify_end()[0].value == 1
    blob, n_members, n_kept = fr.filter(np.ones(1, np.uint8), 0)
    assert (gunzip(blob), n_members, n_kept) == (b"@r\nACGT\n+\nIIII\n", 1, 1)
    fr.close()
