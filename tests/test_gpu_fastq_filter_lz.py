"""cid_fastq_filter_matches: cid_fastq_filter with the LZ77 coder behind it — the same records as the restated read_filter gives, every
member under the rules of tests/deflate_lz_props.py, today's bytes again once the setting is off, and the setting refused while a step
is in flight."""
import zlib

import numpy as np
import pytest

import colorid_amd
from colorid_amd._lib import CID_ERR_STATE
from deflate_lz_props import check_lz_member
from deflate_props import split_members
from test_gpu_fastq import line_loop_records, world  # noqa: F401  (the toy index of the front end's tests)
from test_gpu_fastq_filter import gunzip, make_text, restated

pytestmark = pytest.mark.gpu


def checked_text(blob):
    """every member through check_lz_member against what zlib reads from it -> the members' text"""
    out = []
    for m in split_members(blob):
        piece = zlib.decompressobj(31).decompress(m)
        check_lz_member(m, piece)
        out.append(piece)
    assert all(len(p) == 65280 for p in out[:-1])
    return b"".join(out)


def patterns(n):
    return {"all": np.ones(n, np.uint8), "none": np.zeros(n, np.uint8), "every_third": (np.arange(n) % 3 == 0).astype(np.uint8)}


@pytest.mark.parametrize("n_files,q", [(1, 15), (2, 0)])
def test_filter_with_matches_equals_the_restated_read_filter(hip_ctx, world, n_files, q):
    from colorid_amd.hip import bgzf_deflate
    oix, hx, genomes = world
    rng = np.random.default_rng(50 + n_files)
    texts = [make_text(rng, genomes, 300, f + 1, last_newline=(f == 1)) for f in range(n_files)]
    records = [line_loop_records(t) for t in texts]
    fr = colorid_amd.FastqReader(hip_ctx, n_files, q)
    fr.keep_steps()
    fr.filter_matches(1)
    got = {name: [b""] * n_files for name in patterns(1)}
    want_keep = {name: [] for name in got}
    sizes = {"with matches": 0, "without": 0}
    done = 0
    for part in range(2):                                                        # two steps, cut inside a record
        for f in range(n_files):
            cut = len(texts[f]) * 2 // 5 + 11 * f
            fr.push_text(f, texts[f][:cut] if part == 0 else texts[f][cut:], last=(part == 1))
        n = len(fr.classify(hx, 1, 3)[0])
        assert n
        for name, keep in patterns(n).items():
            want_keep[name] += keep.tolist()
            for f in range(n_files):
                blob, n_members, n_kept = fr.filter(keep, f)
                assert n_kept == int(keep.sum())
                text = checked_text(blob)
                assert n_members == (len(text) + 65279) // 65280
                got[name][f] += text
                # off again: today's bytes, which are cid_bgzf_deflate's of the same text; and on again: the bytes from before
                fr.filter_matches(0)
                off = fr.filter(keep, f)[0]
                assert off == bgzf_deflate(hip_ctx, text)[0]
                fr.filter_matches(1)
                assert fr.filter(keep, f)[0] == blob == bgzf_deflate(hip_ctx, text, matches=True)[0]
                assert len(blob) <= len(off)
                sizes["with matches"] += len(blob); sizes["without"] += len(off)
        done += n
    assert done == 300
    for name in got:
        for f in range(n_files):
            assert got[name][f] == restated(records[f], want_keep[name]), (name, f)
    assert got["none"] == [b""] * n_files
    print(f"{n_files} file(s): {sizes}")
    assert sizes["with matches"] < sizes["without"]                               # headers repeat from record to record
    fr.close()


def test_the_setting_is_refused_while_a_step_is_in_flight(hip_ctx, world):
    oix, hx, genomes = world
    fr = colorid_amd.FastqReader(hip_ctx, 1, 0)
    fr.keep_steps()
    fr.push_text(0, b"@r\nACGT\n+\nIIII\n", last=True)
    fr.classify_begin(hx, 1, 3)
    for on in (1, 0):
        with pytest.raises(colorid_amd.CidError) as e:
            fr.filter_matches(on)
        assert e.value.code == CID_ERR_STATE
    assert fr.classify_end()[0].value == 1
    fr.filter_matches(1)
    blob, n_members, n_kept = fr.filter(np.ones(1, np.uint8), 0)
    assert (gunzip(blob), n_members, n_kept) == (b"@r\nACGT\n+\nIIII\n", 1, 1)
    fr.close()
