"""Every host-offset entry point of read_id on one small batch: the malformed batches each of them must refuse before anything is
launched, the slices of cid_readid_count and the shards of the replica group, and both staging modes — all against the oracle.
One index (m = 5003, 2 hashes, k = 21, 40 colours) serves every call but the striped group's: two ranks need a 64-colour word each,
so that call has an index of the same shape with 104 colours, and its own oracle answer for the same batch."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

from test_gpu_readid import pack_reads
from util import random_index, to_hip_index

pytestmark = pytest.mark.gpu

INVALID = -1
N_COLORS = 40
N_COLORS_STRIPED = 104


@pytest.fixture(scope="module")
def world(orc, hip_ctx):
    import torch

    import colorid_amd
    rng = np.random.default_rng(2)
    oix = random_index(orc, rng, 5003, 2, 21, N_COLORS, density=0.3, zero_row_frac=0.1)

    def seq(n):
        return bytes(rng.choice(list(b"ACGT"), size=n).astype(np.uint8))
    # paired and single reads of 150 bases, a read with no sequence, one whose first mate is shorter than k, one of 600 bases
    reads = [[seq(150), seq(150)], [seq(150)], [], [seq(10), seq(150)], [seq(600)], [seq(150), seq(150)], [seq(150)], [seq(150), seq(150)],
             [seq(150)], [seq(150), seq(150)], [seq(150)]]
    assert len(reads) == 11
    bases, so, r0 = pack_reads(reads)
    want = oix.readid_counts(bases, so, r0, 1, 3)
    # an all-zero result cannot pass
    assert want[0][:, :N_COLORS].sum() > 0 and want[1].sum() > 0 and {0, 1} <= set(want[2].tolist())
    hx = to_hip_index(hip_ctx, oix)
    g = colorid_amd.Group([0, 0])
    gx = to_hip_index(g.ctxs[0], oix)
    g.replicate(gx)
    oix_s = random_index(orc, rng, 5003, 2, 21, N_COLORS_STRIPED, density=0.3, zero_row_frac=0.1)
    want_s = oix_s.readid_counts(bases, so, r0, 1, 3)
    assert want_s[0][:, :N_COLORS_STRIPED].sum() > 0 and want_s[1].sum() > 0 and {0, 1} <= set(want_s[2].tolist())
    stp = g.stripes(oix_s.m, oix_s.n_hash, oix_s.k, oix_s.n_colors)
    rows = oix_s.rows()
    ids = np.nonzero(rows.any(axis=1))[0].astype(np.uint64)
    stp.put_rows(ids, np.ascontiguousarray(rows[ids.astype(np.int64)], np.uint32))
    stp.finalize()
    for cx in g.ctxs:
        cx.tune("readid_long_from", 200)   # the 600-base read takes the long-read path, the others the LDS kernels
    d_bases = torch.from_numpy(bases.copy()).cuda()
    yield SimpleNamespace(oix=oix, hx=hx, g=g, stp=stp, bases=bases, so=so, r0=r0, want=want, want_s=want_s, d_bases=d_bases, ctx=hip_ctx,
                          lib=hip_ctx.lib)
    g.close()
    hx.close()


def _sparse_equals(want, got):
    rs, col, cnt, nk, st = got
    assert np.array_equal(nk, want[1]) and np.array_equal(st, want[2])
    rows, cols = np.nonzero(want[0])
    assert np.array_equal(rs, np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=len(want[0])))]).astype(np.uint64))
    assert np.array_equal(col, cols.astype(np.uint32)) and np.array_equal(cnt, want[0][rows, cols])


def _dense_equals(want, rep, nk, st):
    assert np.array_equal(st, want[2]) and np.array_equal(nk, want[1]) and np.array_equal(rep, want[0])


def _resident(w, bases_t, so, r0, d=1):
    """cid_readid_count_resident into fresh device arrays -> (rc, rep, nk, st)"""
    import torch
    n = len(r0) - 1
    rep = torch.full((n, N_COLORS + 1), 77, dtype=torch.int32, device="cuda")
    nk = torch.full((n,), 77, dtype=torch.int32, device="cuda")
    st = torch.full((n,), 77, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc = w.lib.cid_readid_count_resident(w.ctx.h, w.hx.h, bases_t.data_ptr(), so.ctypes.data, len(so) - 1, r0.ctypes.data, n, d, 3, rep.data_ptr(),
                                         nk.data_ptr(), st.data_ptr())
    w.ctx.synchronize()
    return rc, rep.cpu().numpy().view(np.uint32), nk.cpu().numpy().view(np.uint32), st.cpu().numpy()


def _stripe_passes(w, bases_t, so, r0, n_seqs, n_reads, d, n_words):
    """cid_readid_stripe_zero, then _count, of the whole index as one stripe -> (rc_zero, rc_count, rep, nk, st)"""
    import torch
    zero = torch.full((max(n_words, 1),), -1, dtype=torch.int32, device="cuda")
    rep = torch.zeros((max(n_reads, 1), N_COLORS + 1), dtype=torch.int32, device="cuda")
    nk = torch.zeros(max(n_reads, 1), dtype=torch.int32, device="cuda")
    st = torch.zeros(max(n_reads, 1), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    args = (w.ctx.h, w.hx.h, bases_t.data_ptr(), so.ctypes.data, n_seqs, r0.ctypes.data, n_reads, d)
    rc_zero = w.lib.cid_readid_stripe_zero(*args, zero.data_ptr(), nk.data_ptr(), st.data_ptr())
    rc_count = w.lib.cid_readid_stripe_count(*args, 3, 0, N_COLORS, 1, zero.data_ptr(), rep.data_ptr(), nk.data_ptr(), st.data_ptr())
    w.ctx.synchronize()
    return rc_zero, rc_count, rep.cpu().numpy().view(np.uint32), nk.cpu().numpy().view(np.uint32), st.cpu().numpy()


def _mask_words(w, so, r0, n_reads, d):
    nw = C.c_uint64(0)
    return w.lib.cid_readid_stripe_mask_words(21, d, so.ctypes.data, r0.ctypes.data, n_reads, C.byref(nw)), nw.value


def test_every_entry_refuses_malformed_batches_and_works_afterwards(world, tune):
    """the three malformed batches of test_more_error_behaviour and stride 0: CID_ERR_INVALID with a message from every entry that
    takes offsets on the host — refused on the host, before any launch — and the oracle's answer from the same context afterwards"""
    import torch
    w = world
    lib = w.lib
    tune("readid_long_from", 200)
    one = np.frombuffer(b"ACGT" * 50, np.uint8)
    d_one = torch.from_numpy(one.copy()).cuda()
    rep = np.zeros((1, N_COLORS + 1), np.uint32); nk = np.zeros(1, np.uint32); st = np.zeros(1, np.uint8)
    ne = C.c_uint64(0)

    def refused(name, rc):
        assert rc == INVALID, (name, rc)
        assert lib.cid_last_error(), name

    # (seq_off, read_seq0, n_seqs, n_reads, stride, has a meaning without n_seqs)
    cases = [([0, 200], [0, 1], 1, 1, 0, True),          # stride 0
             ([200, 0], [0, 1], 1, 1, 1, True),          # seq_off not monotonic
             ([0, 200], [0, 2], 1, 1, 1, False),         # read_seq0 points past n_seqs
             ([0, 200], [1, 0], 1, 1, 1, True)]          # read_seq0 not monotonic
    for seq_off, read0, n_seqs, n_reads, d, without_n_seqs in cases:
        so = np.array(seq_off, np.uint64); r0 = np.array(read0, np.uint64)
        host = (one.ctypes.data, so.ctypes.data, n_seqs, r0.ctypes.data, n_reads, d, 3)
        refused("count", lib.cid_readid_count(w.ctx.h, w.hx.h, *host, rep.ctypes.data, nk.ctypes.data, st.ctypes.data))
        refused("count_sparse", lib.cid_readid_count_sparse(w.ctx.h, w.hx.h, *host, nk.ctypes.data, st.ctypes.data, C.byref(ne)))
        refused("count_resident", _resident(w, d_one, so, r0, d)[0])
        rc_zero, rc_count = _stripe_passes(w, d_one, so, r0, n_seqs, n_reads, d, 256)[:2]
        refused("stripe_zero", rc_zero)
        refused("stripe_count", rc_count)
        if without_n_seqs:
            refused("stripe_mask_words", _mask_words(w, so, r0, n_reads, d)[0])
        refused("group count_sparse", lib.cid_group_readid_count_sparse(w.g.h, w.g._replica_handles, *host, nk.ctypes.data, st.ctypes.data, C.byref(ne)))
        refused("striped group count_sparse", lib.cid_group_stripes_readid_count_sparse(w.g.h, w.stp.arr, *host, nk.ctypes.data, st.ctypes.data,
                                                                                         C.byref(ne)))
    # the same contexts and indices afterwards
    want, bases, so, r0 = w.want, w.bases, w.so, w.r0
    _dense_equals(want, *w.hx.readid_count(bases, so, r0, 1, 3))
    _sparse_equals(want, w.hx.readid_count_sparse(bases, so, r0, 1, 3))
    rc, *got = _resident(w, w.d_bases, so, r0)
    assert rc == 0
    _dense_equals(want, *got)
    rc, n_words = _mask_words(w, so, r0, len(r0) - 1, 1)
    assert rc == 0 and n_words == sum(max(0, int(n) - 21 + 1) for n in np.diff(so.astype(np.int64))) + 1
    rc_zero, rc_count, *got = _stripe_passes(w, w.d_bases, so, r0, len(so) - 1, len(r0) - 1, 1, n_words)
    assert rc_zero == 0 and rc_count == 0
    _dense_equals(want, *got)
    _sparse_equals(want, w.g.readid_count_sparse(bases, so, r0, 1, 3))
    _sparse_equals(w.want_s, w.stp.readid_count_sparse(bases, so, r0, 1, 3))


def test_slices_and_shards_equal_the_oracle(world, tune):
    """cid_readid_count in slices of 3 reads (4 slices, the last short) and the replica group's shards: row for row the oracle's"""
    w = world
    tune("readid_long_from", 200)
    tune("dense_report_bytes", 3 * (N_COLORS + 1) * 4)
    _dense_equals(w.want, *w.hx.readid_count(w.bases, w.so, w.r0, 1, 3))
    _sparse_equals(w.want, w.g.readid_count_sparse(w.bases, w.so, w.r0, 1, 3))


@pytest.mark.parametrize("pin", [1, 0])
def test_both_staging_modes_equal_the_oracle(world, tune, pin):
    """pin_staging 1 (through the pinned arena) and 0 (straight from the caller's memory): _count, _count_sparse + _sparse_fetch,
    _count_resident and the striped group call"""
    w = world
    tune("readid_long_from", 200)
    tune("pin_staging", pin)
    for cx in w.g.ctxs:
        cx.tune("pin_staging", pin)
    try:
        _dense_equals(w.want, *w.hx.readid_count(w.bases, w.so, w.r0, 1, 3))
        _sparse_equals(w.want, w.hx.readid_count_sparse(w.bases, w.so, w.r0, 1, 3))
        rc, *got = _resident(w, w.d_bases, w.so, w.r0)
        assert rc == 0
        _dense_equals(w.want, *got)
        _sparse_equals(w.want_s, w.stp.readid_count_sparse(w.bases, w.so, w.r0, 1, 3))
    finally:
        for cx in w.g.ctxs:
            cx.tune("pin_staging", 1)
