"""The host-to-host entry (csrc/host_batch.cpp, pa_map_tiles_host) at its seams: batch sizes around a tile, chunk sizes and stream counts at their
clamps, NULL outputs, a packed buffer that fits exactly and one word short, stages parked on the handle that must grow and are then too large, reads at
and beyond what the compact records hold. What the reads map to is the oracle's answer; the raw bits of the records and of the packed stream are
what the model (tests/compact_model.py, written from the header) makes of that answer, chunk by chunk. Pinned host buffers, every one with a guard
region behind it; all integers, equality."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import compact_model as cm
import helpers

pa = helpers.pa
pytestmark = pytest.mark.gpu

GUARD_BYTES = 512
PAT64, PAT32, PATC, PATW = 0x5A5A5A5A5A5A5A5A, 0xA5A5A5A5, 0x7777777777777777, 0x1122334455667788
TILE_JUNK = 0xC6C6C6C6C6C6C6C6              # what the tile words hold beyond a read's length, and in the rows behind the last read
OK, INVALID_ARG, ERR_HIP, ARENA_FULL = 0, -1, -5, -7
READ_LEN, PPM, SEED, N = 100, 20000, 6, 1000
CLEAN_N, CLEAN_SEED = 129, 50               # error-free reads none of which has a class that is no index class (chosen on the CPU; asserted below)

_cache = {}


@pytest.fixture(scope="module")
def ctx(small_index):
    if pa.lib().pa_device_count() < 1:
        raise RuntimeError("the gpu tier needs a GPU and the HIP library: %s" % pa.lib().pa_last_error().decode())
    assert (pa._ffi.PA_ERR_INVALID_ARG, pa._ffi.PA_ERR_ARENA_FULL) == (INVALID_ARG, ARENA_FULL)      # (ERR_HIP: PA_ERR_HIP of the header)
    host = small_index(24)
    return SimpleNamespace(host=host, al=pa.Pseudoaligner(host, 0), arrays=host.arrays(), oracle=helpers.Oracle(host), tx=pa.Txome.from_host_index(host),
                           wpr=pa.lib().pa_words_per_read(READ_LEN))


class Pinned:
    """page-locked host memory: `arr`'s bytes, a guard region behind them"""

    def __init__(self, arr):
        import torch
        b = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
        self.n, self.dtype = len(b), arr.dtype
        self.t = torch.empty(self.n + GUARD_BYTES, dtype=torch.uint8).pin_memory()
        v = self.t.numpy()
        v[:self.n] = b
        v[self.n:] = 0xEE
        self.ptr = self.t.data_ptr()

    def get(self, what):
        v = self.t.numpy()
        assert (v[self.n:] == 0xEE).all(), "%s: a byte behind it was written" % what
        return v[:self.n].view(self.dtype).copy()


def tiles_with_junk(tiles, lens, wpr, junk):
    """the batch's tiles with every bit that belongs to no base of a read — beyond its length, and the rows of the last tile behind the last read — set from `junk`"""
    t = np.asarray(tiles, np.uint64).copy().reshape(-1, wpr, 64)
    n = len(lens)
    r = np.arange(n)
    for w in range(wpr):
        bases = np.clip(np.asarray(lens, np.int64) - 32 * w, 0, 32)
        keep = np.where(bases >= 32, np.uint64(0xFFFFFFFFFFFFFFFF), (np.uint64(1) << (2 * np.minimum(bases, 31)).astype(np.uint64)) - np.uint64(1))
        t[r >> 6, w, r & 63] = (t[r >> 6, w, r & 63] & keep) | (np.uint64(junk) & ~keep)
    if n % 64:
        t[-1, :, n % 64:] = np.uint64(junk)
    return t.reshape(-1)


def call(ctx, tiles, n, wpr, lens=None, uniform=0, chunk=64, streams=3, packed_cap=1 << 15, counts=True, null_pw=False, null_packed=False, null_tiles=False,
         null_compact=False, al=None):
    """pa_map_tiles_host on fresh pinned buffers, the outputs pre-filled with patterns -> rc, words, compact, packed[packed_cap], counts, error text.
    Every guard is looked at; a HIP error ends the session: nothing more is started on a GPU that may have faulted"""
    al = al or ctx.al
    L = pa.lib()
    h_tiles = Pinned(np.asarray(tiles, np.uint64) if len(tiles) else np.zeros(8, np.uint64))
    h_lens = Pinned(np.asarray(lens, np.uint32) if len(lens) else np.zeros(4, np.uint32)) if lens is not None else None
    h_compact = Pinned(np.full(n, PAT64, np.uint64))
    h_packed = Pinned(np.full(packed_cap, PAT32, np.uint32))
    h_counts = Pinned(np.full(al.counts_len(), PATC, np.uint64))
    pw = C.c_uint64(PATW)
    rc = L.pa_map_tiles_host(al._h, None if null_tiles else h_tiles.ptr, h_lens.ptr if h_lens else None, uniform, n, wpr, 2, None if null_compact else h_compact.ptr,
                             None if null_packed else h_packed.ptr, packed_cap, None if null_pw else C.byref(pw), h_counts.ptr if counts else None, chunk, streams)
    err = L.pa_last_error().decode() if rc != OK else ""
    if rc == ERR_HIP:
        pytest.exit("host-to-host entry: %s" % err, returncode=3)
    assert np.array_equal(h_tiles.get("h_tiles"), np.asarray(tiles, np.uint64) if len(tiles) else np.zeros(8, np.uint64))
    if h_lens:
        h_lens.get("h_lens")
    return SimpleNamespace(rc=rc, words=pw.value, compact=h_compact.get("h_compact"), packed=h_packed.get("h_packed"), counts=h_counts.get("h_counts"), err=err)


def effective_chunk(chunk, n):
    """chunks of chunk_reads reads (0: 1 M), whole tiles, no more than the batch and no less than one tile"""
    return max(64, min(chunk or 1000000, max(n, 64)) // 64 * 64)


def expected(host, oracle, tiles, lens, wpr, chunk):
    """the oracle's answer for the batch and what the entry returns for it when it maps chunks of `chunk` reads"""
    res, coff, ids, _ = oracle.map_tiles(np.asarray(tiles, np.uint64), np.asarray(lens, np.uint32), wpr, 2, 8)
    compact, packed, words = cm.host_batch(res["mapped"], res["coverage"], res["mismatches"], coff, ids, host.arrays(), chunk)
    return SimpleNamespace(res=res, coff=coff, ids=ids, compact=compact, packed=packed, words=words, total=int(sum(words)),
                           counts=helpers.counts_reference_fast(res, coff, ids, host))


def same(host, got, want, what, counts=True, words=True):
    assert got.rc == OK, (what, got.rc, got.err)
    if words:
        assert got.words == want.total, (what, got.words, want.total)
    bad = np.flatnonzero(got.compact != want.compact)
    assert len(bad) == 0, "%s: record %d is %s, expected %s (%d differ)" % (what, bad[0], cm.fields(got.compact[bad[0]]), cm.fields(want.compact[bad[0]]), len(bad))
    assert np.array_equal(got.packed[:want.total], want.packed), what + ": packed stream"
    assert (got.packed[want.total:] == PAT32).all(), what + ": a word behind the packed stream was written"
    if counts:
        assert np.array_equal(got.counts.astype(np.int64), want.counts), what + ": count table"
    else:
        assert (got.counts == PATC).all()
    res, coff, ids = pa.unpack_compact(got.compact, got.packed[:want.total], host)
    helpers.assert_same_as_oracle(res, coff, ids, want.res, want.coff, want.ids, what)


def batch(ctx):
    """N simulated reads of READ_LEN bases with substitutions (so that classes that are no index classes occur) -> (tiles, lens)"""
    if "batch" not in _cache:
        tiles, lens = ctx.tx.simulate_host(READ_LEN, SEED, N, PPM, 0, ctx.wpr)
        assert (lens == READ_LEN).all()
        _cache["batch"] = (tiles, lens)
    return _cache["batch"]


def want_of_batch(ctx, chunk):
    key = ("want", chunk)
    if key not in _cache:
        tiles, lens = batch(ctx)
        _cache[key] = expected(ctx.host, ctx.oracle, tiles, lens, ctx.wpr, chunk)
    return _cache[key]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 129])
def test_batches_around_a_tile(ctx, n):
    """nothing, one read, a tile less one, a tile, a tile and one read, two tiles and one; the rows of the last tile behind the last read hold junk"""
    tiles, lens = batch(ctx)
    t = tiles_with_junk(tiles[:pa.lib().pa_tiles_words(n, ctx.wpr)], lens[:n], ctx.wpr, TILE_JUNK)
    for uniform in (False, True):
        got = call(ctx, t, n, ctx.wpr, lens=None if uniform else lens[:n], uniform=READ_LEN if uniform else 0, chunk=64, streams=3)
        if n == 0:
            assert got.rc == OK and got.words == 0 and (got.counts == 0).all() and len(got.compact) == 0 and (got.packed == PAT32).all()
            continue
        want = expected(ctx.host, ctx.oracle, tiles_with_junk(tiles[:len(t)], lens[:n], ctx.wpr, 0), lens[:n], ctx.wpr, 64)
        same(ctx.host, got, want, "n = %d, uniform = %s" % (n, uniform))
    if n == 0:      # h_compact is not touched: the same call with a buffer it could write to
        h = Pinned(np.full(64, PAT64, np.uint64))
        z = Pinned(np.zeros(8, np.uint64))
        pw = C.c_uint64(PATW)
        assert pa.lib().pa_map_tiles_host(ctx.al._h, z.ptr, None, READ_LEN, 0, ctx.wpr, 2, h.ptr, None, 0, C.byref(pw), None, 64, 3) == OK
        assert pw.value == 0 and (h.get("h_compact") == PAT64).all()


CONFIGS = [(64, 1), (64, 2), (64, 8), (64, 9), (64, -1), (100, 3), (1, 2), (0, 0), (4096, 4)]


def test_chunk_sizes_and_stream_counts_at_their_clamps(ctx):
    """one stage that every chunk reuses; the stream count clamped to 8 and defaulted; chunk_reads rounded down to whole tiles, raised to one tile, defaulted
    and clamped to the batch; fewer chunks than streams. Every arrangement returns the oracle's answer in the model's bits. Arrangements with the same chunk
    size return the same bytes; between the two chunk sizes that occur (64 and 960) only `hi` of packed records may differ — it is an offset in the packed
    stream of the record's launch — and the model says by how much"""
    tiles, lens = batch(ctx)
    w64 = want_of_batch(ctx, 64)
    assert sum(1 for w in w64.words if w) >= 3, "at least three chunks of the reference result hold packed classes"
    t = tiles_with_junk(tiles, lens, ctx.wpr, TILE_JUNK)
    outs = {}
    for chunk, streams in CONFIGS:
        eff = effective_chunk(chunk, N)
        assert eff == (960 if chunk in (0, 4096) else 64)
        got = call(ctx, t, N, ctx.wpr, uniform=READ_LEN, chunk=chunk, streams=streams)
        same(ctx.host, got, want_of_batch(ctx, eff), "chunk_reads = %d, n_streams = %d" % (chunk, streams))
        outs[(chunk, streams)] = got
    first = outs[CONFIGS[0]]
    packed_rec = (first.compact & np.uint64(pa.PA_COMPACT_PACKED)) != 0
    for key, got in outs.items():
        assert got.words == first.words and np.array_equal(got.packed, first.packed) and np.array_equal(got.counts, first.counts), key
        assert np.array_equal(got.compact & np.uint64(0xFFFFFFFF), first.compact & np.uint64(0xFFFFFFFF)) and np.array_equal(got.compact[~packed_rec], first.compact[~packed_rec]), key
        if effective_chunk(key[0], N) == 64:
            assert np.array_equal(got.compact, first.compact), key
        else:
            assert np.array_equal(got.compact, outs[(0, 0)].compact), key


def test_offsets_of_packed_records_restart_in_every_chunk(ctx):
    """`hi` of a packed record is the word offset of its entry in the packed stream of its launch: 0 for the first of every chunk; a reader that walks the
    records in read order finds every entry where the one before it ended, and the stream ends with the last"""
    tiles, lens = batch(ctx)
    got = call(ctx, tiles, N, ctx.wpr, lens=lens, chunk=64, streams=2)
    assert got.rc == OK
    want = want_of_batch(ctx, 64)
    at = 0
    chunks_with_entries = 0
    for c in range(0, N, 64):
        base = at
        for i in range(c, min(N, c + 64)):
            f = cm.fields(got.compact[i])
            if f["packed"] and not f["by_ref"]:
                assert f["hi"] == at - base, (i, f, at, base)
                ln = int(got.packed[at])
                assert ln == int(want.res["class_len"][i]) and got.packed[at + 1:at + 1 + ln].tolist() == want.ids[int(want.coff[i]):int(want.coff[i + 1])].tolist()
                at += 1 + ln
        chunks_with_entries += at > base
        assert at - base == want.words[c // 64]
    assert at == got.words and chunks_with_entries >= 3


def test_ragged_and_uniform(ctx):
    """the same batch through a length array with lengths below K (0, 1, 23), at K, and up to the full length mixed in, and through uniform_len; the tile
    words hold junk beyond every read's length"""
    tiles, lens = batch(ctx)
    ragged = lens.copy()
    mix = np.array([0, 1, 23, 24, 25, 99, 100], np.uint32)
    ragged[::3] = mix[np.arange(len(ragged[::3])) % len(mix)]
    assert set(mix.tolist()) <= set(ragged.tolist()) and ctx.host.k == 24
    for what, ll in (("ragged", ragged), ("uniform", lens)):
        want = expected(ctx.host, ctx.oracle, tiles_with_junk(tiles, ll, ctx.wpr, 0), ll, ctx.wpr, 64)
        got = call(ctx, tiles_with_junk(tiles, ll, ctx.wpr, TILE_JUNK), N, ctx.wpr, lens=ll if what == "ragged" else None, uniform=0 if what == "ragged" else READ_LEN,
                   chunk=64, streams=3)
        same(ctx.host, got, want, what)
        if what == "ragged":
            short = ragged < 24
            assert short.sum() > 100 and not want.res["mapped"][short].any() and (got.compact[short] == 0).all()


def test_null_outputs(ctx):
    tiles, lens = batch(ctx)
    want = want_of_batch(ctx, 64)
    same(ctx.host, call(ctx, tiles, N, ctx.wpr, uniform=READ_LEN, counts=False), want, "h_counts NULL", counts=False)
    got = call(ctx, tiles, N, ctx.wpr, uniform=READ_LEN, null_pw=True)
    assert got.words == PATW
    same(ctx.host, got, want, "packed_words NULL", words=False)
    # no room for packed classes, and none needed
    c_tiles, c_lens = ctx.tx.simulate_host(READ_LEN, CLEAN_SEED, CLEAN_N, 0, 0, ctx.wpr)
    c_want = expected(ctx.host, ctx.oracle, c_tiles, c_lens, ctx.wpr, 64)
    assert c_want.total == 0 and int(c_want.res["mapped"].sum()) == CLEAN_N and (c_want.res["class_len"] > 0).all(), "the reference result has no packed class"
    got = call(ctx, c_tiles, CLEAN_N, ctx.wpr, uniform=READ_LEN, packed_cap=0, null_packed=True)
    same(ctx.host, got, c_want, "packed_cap 0, h_packed NULL")
    assert ((got.compact & np.uint64(pa.PA_COMPACT_BY_REF)) != 0).all()
    # ... and needed
    assert want.total > 0
    got = call(ctx, tiles, N, ctx.wpr, uniform=READ_LEN, packed_cap=0, null_packed=True)
    assert got.rc == ARENA_FULL, (got.rc, got.err)
    same(ctx.host, call(ctx, tiles, N, ctx.wpr, uniform=READ_LEN), want, "after PA_ERR_ARENA_FULL")


def test_packed_cap_at_the_edge(ctx):
    """room for exactly the words the batch needs; one word less is PA_ERR_ARENA_FULL, nothing is written behind h_packed[packed_cap] (the guard of the
    pinned buffer begins there), and the handle goes on working"""
    tiles, lens = batch(ctx)
    want = want_of_batch(ctx, 64)
    assert want.total > 3
    exact = call(ctx, tiles, N, ctx.wpr, uniform=READ_LEN, packed_cap=want.total)
    same(ctx.host, exact, want, "packed_cap == words")
    short = call(ctx, tiles, N, ctx.wpr, uniform=READ_LEN, packed_cap=want.total - 1)
    assert short.rc == ARENA_FULL, (short.rc, short.err)
    again = call(ctx, tiles, N, ctx.wpr, uniform=READ_LEN, packed_cap=want.total)
    same(ctx.host, again, want, "after PA_ERR_ARENA_FULL")
    assert np.array_equal(again.compact, exact.compact) and np.array_equal(again.packed, exact.packed) and np.array_equal(again.counts, exact.counts)


def wide_reads(ctx, n, length, seed):
    """n reads of `length` bases cut from transcripts at least that long, 2 % substitutions -> (tiles, lens, wpr)"""
    packed, tx_start = ctx.tx.arrays()
    starts = tx_start.astype(np.int64)
    tlen = starts[1:] - starts[:-1]
    longs = np.flatnonzero(tlen >= length)
    assert len(longs) >= 20
    codes = helpers.unpack_bases(packed, int(starts[-1]))
    rng = np.random.RandomState(seed)
    lut = np.frombuffer(b"ACGT", np.uint8)
    reads = []
    for _ in range(n):
        t = int(longs[rng.randint(len(longs))])
        s = int(starts[t]) + int(rng.randint(0, tlen[t] - length + 1))
        c = codes[s:s + length].copy()
        flip = rng.rand(length) < 0.02
        c[flip] = (c[flip] + rng.randint(1, 4, int(flip.sum()))) % 4
        reads.append(lut[c].tobytes())
    return helpers.pack_reads_tiles(reads, (length + 31) // 32)


def test_parked_stages_grow_and_are_reused(ctx):
    """three calls on one handle: 100-base reads in chunks of 64; 600-base reads (19 words per read, the map kernel's wide-read path) in chunks of 512 — the
    stages parked by the first call are too small in every buffer; the first call again, on stages that are now too large. Each is its oracle's answer, and the
    count table of the third is that of the first: overwritten, not accumulated"""
    tiles, lens = batch(ctx)
    want = want_of_batch(ctx, 64)
    w_tiles, w_lens, w_wpr = wide_reads(ctx, 700, 600, 13)
    assert w_wpr == 19 > ctx.wpr and (w_lens == 600).all()
    w_want = expected(ctx.host, ctx.oracle, w_tiles, w_lens, w_wpr, 512)
    assert int(w_want.res["mapped"].sum()) > 600
    al = pa.Pseudoaligner(ctx.host, 0)       # a handle of this test's own: nothing is parked on it yet
    first = call(ctx, tiles, N, ctx.wpr, uniform=READ_LEN, chunk=64, streams=2, al=al)
    same(ctx.host, first, want, "first call")
    wide = call(ctx, w_tiles, 700, w_wpr, lens=w_lens, chunk=512, streams=2, packed_cap=1 << 17, al=al)
    same(ctx.host, wide, w_want, "wide reads, larger chunks")
    third = call(ctx, tiles, N, ctx.wpr, uniform=READ_LEN, chunk=64, streams=2, al=al)
    same(ctx.host, third, want, "the first call again")
    assert np.array_equal(third.counts, first.counts) and np.array_equal(third.compact, first.compact) and np.array_equal(third.packed, first.packed)


def test_refused_arguments(ctx):
    tiles, lens = batch(ctx)
    w = ctx.wpr
    for what, kw in (("no h_lens and uniform_len 0", dict(wpr=w, uniform=0)),
                     ("uniform_len beyond the tile words", dict(wpr=w, uniform=32 * w + 1)),
                     ("words_per_read 0", dict(wpr=0, uniform=READ_LEN)),
                     ("h_tiles NULL", dict(wpr=w, uniform=READ_LEN, null_tiles=True)),
                     ("h_compact NULL", dict(wpr=w, uniform=READ_LEN, null_compact=True))):
        wpr = kw.pop("wpr")
        got = call(ctx, tiles, N, wpr, **kw)
        assert got.rc == INVALID_ARG, (what, got.rc, got.err)
        assert (got.compact == PAT64).all() and (got.packed == PAT32).all() and (got.counts == PATC).all(), what
    same(ctx.host, call(ctx, tiles, N, w, uniform=READ_LEN), want_of_batch(ctx, 64), "after the refused calls")


def test_reads_at_and_beyond_what_the_records_hold(ctx):
    """14 bits of coverage: a read of 16 383 bases (PA_COMPACT_MAX_READ_LEN) that maps over its whole length comes back exact, one of 16 384 bases is refused
    before anything is copied — as uniform_len and in a length array — and the handle goes on working.
    (Before the check existed the 16 384-base call returned PA_OK with the coverage modulo 2^14.)"""
    limit = pa.PA_COMPACT_MAX_READ_LEN
    assert limit == 16383
    rng = np.random.RandomState(31)
    codes = [rng.randint(0, 4, 20000).astype(np.uint8), rng.randint(0, 4, 300).astype(np.uint8)]
    host = pa.HostIndex.build_packed(helpers.pack_bases(np.concatenate(codes)), np.array([0, 20000, 20300], np.uint64), 24, 2)
    al, oracle = pa.Pseudoaligner(host, 0), helpers.Oracle(host)
    lut = np.frombuffer(b"ACGT", np.uint8)
    seq = lambda c: lut[c].tobytes()
    wpr = (limit + 31) // 32
    assert wpr == 512 and 32 * wpr == limit + 1

    def run(reads, uniform):
        tiles, lens, _ = helpers.pack_reads_tiles(reads, wpr)
        return tiles, lens, call(ctx, tiles, len(reads), wpr, lens=None if uniform else lens, uniform=uniform, chunk=64, streams=2, packed_cap=256, al=al)

    fits = [seq(codes[0][:limit]), seq(codes[0][20000 - limit:])]
    for uniform, reads in ((limit, fits), (0, fits + [seq(codes[1])])):
        tiles, lens, got = run(reads, uniform)
        want = expected(host, oracle, tiles, lens, wpr, 64)
        assert want.res["mapped"][0] and int(want.res["coverage"][0]) > 8191, "the top bit of the field is exercised"
        assert int(want.res["coverage"][0]) == limit and want.ids[int(want.coff[0]):int(want.coff[1])].tolist() == [0]
        same(host, got, want, "16 383 bases, uniform_len = %d" % uniform)
        assert cm.fields(got.compact[0])["coverage"] == limit
    beyond = [seq(codes[0][:limit]), seq(codes[0][:limit + 1])]
    for uniform, reads in ((limit + 1, [beyond[1]] * 2), (0, beyond + [seq(codes[1])])):
        tiles, lens, got = run(reads, uniform)
        assert got.rc == INVALID_ARG, (got.rc, got.err)
        assert str(limit) in got.err and ("uniform_len %d" % (limit + 1) if uniform else "read 1 ") in got.err, got.err
        assert (got.compact == PAT64).all() and (got.packed == PAT32).all() and (got.counts == PATC).all() and got.words == PATW
        tiles, lens, got = run(fits, limit)                                   # the next valid call
        same(host, got, expected(host, oracle, tiles, lens, wpr, 64), "after the refused call")
