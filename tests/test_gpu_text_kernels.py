"""The text kernels of process_reads at their edges, through tests/text/text_probe.hip (the product's launch functions on host arrays)
against tests/text_model.py (pure Python, none of the kernels' arithmetic): record finding and in-place encode (csrc/fastq_scan.hip), tuple
rendering (csrc/render.hip). Every comparison is exact, on bytes or integers.

What pa_process_reads cannot aim at (the host's scan takes the end of every text, windows start at record starts, files hold no class id
of ten digits): line breaks planted just outside the window, windows that begin and end anywhere in a 16-byte lane, line breaks on a
chunk's last and first byte, chunks without a line break and chunks of nothing else, line tables and record tables that are too small by
one entry (guard words behind every output), headers and sequences of every awkward shape at record 0, in the second wave and last, every
power of ten as class id and coverage, classes that end with the arena and one entry beyond it, every byte value in an id, a text
buffer one byte too small, the progress buckets with flag_mark in the middle of a wave.

Left unpinned: the clamp into the last flag bucket (it takes 62 M records), and blanks at the end of a SEQUENCE line (what bio does with
them cannot be settled without its source: DESIGN.md §6)."""

import numpy as np
import pytest

import helpers
import text_model as tm

pytestmark = pytest.mark.gpu

PAT32 = 0xDEADBEEF
PAT64 = 0xDEADBEEFCAFEF00D
SENTINEL = 0xA5
GUARD = 4
SLACK = b"\n" * 32   # behind every window: line breaks the scan must not count (it loads whole 16-byte groups)
INFO = np.dtype([("lines", "<u8"), ("n", "<u8"), ("consumed", "<u8"), ("max_seq", "<u4"), ("odd", "<u4"), ("overflow", "<u4"), ("pad", "<u4")])


@pytest.fixture(scope="module")
def lib():
    """the probe, built once (nothing here needs the product library)"""
    L = helpers.text_lib()
    if L.tp_device_count() < 1:
        raise RuntimeError("the gpu tier needs a GPU")
    assert L.tp_guard() == GUARD and L.tp_info_bytes() == INFO.itemsize and L.tp_flag_buckets() == tm.FLAG_BUCKETS
    return L


def ok(L, rc):
    if rc == -5:   # PA_ERR_HIP: a launch or a copy failed. Nothing more is started on a GPU that may have faulted
        pytest.exit("text probe: %s" % L.tp_last_error().decode(), returncode=3)
    assert rc == 0, (rc, L.tp_last_error().decode())


# ---------------------------------------------------------------- scan ----
def gpu_scan(L, buf, begin, end, cap_lines, cap_recs, rescan=None):
    """-> (info, line_start, rec, chunk, first[, info2, line_start2, rec2]): the arrays with their guard elements, pre-filled with PAT32"""
    assert len(buf) >= end + 32
    text = np.frombuffer(bytes(buf), np.uint8)
    nch = L.tp_chunks(begin, end)
    out = lambda n: np.full(n, PAT32, np.uint32)
    ls, rec, chunk, first = out(cap_lines + GUARD), out(4 * (cap_recs + GUARD)), out(nch + 1 + GUARD), out(nch + 1 + GUARD)
    info, info2 = np.zeros(1, INFO), np.zeros(1, INFO)
    info["lines"] = info2["lines"] = 12345   # (the launch zeroes the block itself)
    cl2, cr2 = rescan or (0, 0)
    ls2, rec2 = out(cl2 + GUARD), out(4 * (cr2 + GUARD))
    ok(L, L.tp_scan(text.ctypes.data, len(text), begin, end, ls.ctypes.data, cap_lines, rec.ctypes.data, cap_recs, info.ctypes.data, ls2.ctypes.data, cl2,
                    rec2.ctypes.data, cr2, info2.ctypes.data, chunk.ctypes.data, first.ctypes.data))
    res = (info[0], ls, rec.reshape(-1, 4), chunk, first)
    return res + (info2[0], ls2, rec2.reshape(-1, 4)) if rescan else res


def assert_full_answer(m, info, ls, rec, what):
    """a scan whose tables were large enough: everything is the model's, and nothing is written where nothing belongs"""
    got = {k: int(info[k]) for k in ("lines", "n", "consumed", "max_seq", "odd", "overflow")}
    want = {k: int(m[k]) for k in got}
    assert got == want, (what, got, want)
    L_, n = m["lines"], m["n"]
    assert np.array_equal(ls[: L_ + 1], m["line_start"]), what
    assert (ls[L_ + 1:] == PAT32).all(), (what, "line starts behind the last line")
    assert np.array_equal(rec[:n], m["recs"]), (what, np.flatnonzero((rec[:n] != m["recs"]).any(axis=1))[:5])
    assert (rec[n:] == PAT32).all(), (what, "records behind the last record")


def check_scan(L, buf, begin, end, what="", spare_lines=3, spare_recs=2):
    """the window buf[begin, end) with tables that hold everything (and a little more): the GPU's answer is the model's"""
    m = tm.scan(buf, begin, end, None, None)
    info, ls, rec, chunk, first = gpu_scan(L, buf, begin, end, m["lines"] + 1 + spare_lines, m["n"] + spare_recs)
    assert_full_answer(m, info, ls, rec, what)
    # the chunk tables: line breaks of the window per 4 KiB counted from begin & ~15, their exclusive prefix, the total last
    nch = len(chunk) - 1 - GUARD
    base = begin & ~15
    counts = [bytes(buf[max(begin, base + 4096 * c):max(begin, min(end, base + 4096 * (c + 1)))]).count(b"\n") for c in range(nch)]
    assert nch == (end - base + 4095) // 4096 and chunk[:nch].tolist() == counts and chunk[nch] == 0, what
    assert first[: nch + 1].tolist() == np.concatenate([[0], np.cumsum(counts)]).tolist(), what
    assert (chunk[nch + 1:] == PAT32).all() and (first[nch + 1:] == PAT32).all(), what
    return m


def records(ids, seqs, nl=b"\n", plus=b"+", qual=None):
    return b"".join(b"@" + i + nl + s + nl + plus + nl + (qual if qual is not None else b"I" * len(s)) + nl for i, s in zip(ids, seqs))


def plain(n, rng, lo=0, hi=40):
    ids = [b"r%d/%d extra words" % (i, int(rng.integers(0, 1000))) for i in range(n)]
    seqs = [bytes(rng.choice(np.frombuffer(b"ACGTacgtN", np.uint8), int(rng.integers(lo, hi))).tolist()) for _ in range(n)]
    return ids, seqs


def text_of_size(size, rng, at=None):
    """four-line records, exactly `size` bytes, the last byte a line break; at: the header of one record is stretched so that ITS line break
    is byte `at`"""
    out = bytearray()
    i = 0
    while len(out) + 200 < (at if at is not None and len(out) < at else size):
        ids, seqs = plain(1, rng, 0, 60)
        out += records([b"%d_" % i + ids[0]], seqs)
        i += 1
    if at is not None and len(out) < at:
        out += b"@" + b"h" * (at - len(out) - 1) + b"\nACGTN\n+\nIIIII\n"
        return bytes(out) + text_of_size(size - len(out), rng)
    tail = b"\nAC\n+\nII\n"
    out += b"@" + b"x" * (size - len(out) - 1 - len(tail)) + tail
    assert len(out) == size
    return bytes(out)


def test_window_end_anywhere_in_a_lane(lib):
    """an aligned begin, end % 16 in {0, 1, 15}: the line breaks planted in [end, end + 16) do not count. The text ends inside a line (its
    last bytes belong to the next window)"""
    rng = np.random.default_rng(1)
    for e in (0, 1, 15):
        body = records(*plain(9, rng))
        body += b"@unfinished" + b"x" * ((e - len(body) - 11) % 16)
        buf = b"\n" * 64 + body + SLACK
        assert (64 + len(body)) % 16 == e
        m = check_scan(lib, buf, 64, 64 + len(body), "end %% 16 = %d" % e)
        assert m["n"] == 9 and m["lines"] == 36


def test_window_begin_anywhere_in_a_lane(lib):
    """begin % 16 in {1, 15} (0: the test above) x end % 16 in {0, 1, 15}: line breaks planted in [begin & ~15, begin) and in [end, end + 16)
    do not count, and every position is counted from `begin`"""
    rng = np.random.default_rng(2)
    for b in (1, 15):
        for e in (0, 1, 15):
            begin = 48 + b
            body = records(*plain(7, rng)) + b"@r\nACGT\n"
            body += b"+" * ((e - begin - len(body)) % 16)
            buf = b"\n" * begin + body + SLACK
            assert (begin + len(body)) % 16 == e
            m = check_scan(lib, buf, begin, begin + len(body), "begin %% 16 = %d, end %% 16 = %d" % (b, e))
            assert m["n"] == 7 and m["lines"] == 30


def test_window_inside_one_lane(lib):
    """begin and end in the same 16-byte lane, line breaks on both sides of it in that lane"""
    for begin, body in ((35, b"\nA\n\nGG"), (33, b"@\n\n+\n\n"), (33, b"@i d\nAc\r\n+\n!!\n"), (40, b"none")):
        buf = b"\n" * begin + body + SLACK
        assert begin // 16 == (begin + len(body) - 1) // 16
        check_scan(lib, buf, begin, begin + len(body), repr(body))


def test_window_of_whole_chunks_and_one_byte_more(lib):
    """exactly 4096 and 8192 bytes from an aligned begin; 4097 bytes: with the last line break as byte 0 of chunk 1, and with the first byte of
    the next record there"""
    rng = np.random.default_rng(3)
    for name, body in (("4096", text_of_size(4096, rng)), ("8192", text_of_size(8192, rng)), ("4097", text_of_size(4097, rng)),
                       ("4096 + '@'", text_of_size(4096, rng) + b"@")):
        buf = b"\n" * 64 + body + SLACK
        m = check_scan(lib, buf, 64, 64 + len(body), name)
        assert m["lines"] % 4 == 0 and m["consumed"] == len(body) - (name == "4096 + '@'")


def test_chunk_seams(lib):
    """a header whose line break is the last byte of chunk 0, one whose line break is the first byte of chunk 1, a header of 9000 bytes (two
    chunks without any line break)"""
    rng = np.random.default_rng(4)
    for at in (4095, 4096):
        body = text_of_size(10000, rng, at=at)
        assert body[at] == 10 and body[at - 50:at].count(b"\n") == 0
        check_scan(lib, body + SLACK, 0, len(body), "line break at %d" % at)
    body = records(*plain(3, rng)) + records([b"H" * 8999], [b"ACG"]) + records(*plain(3, rng))
    m = check_scan(lib, b"\n" * 16 + body + SLACK, 16, 16 + len(body), "header of 9000 bytes")
    assert 9000 in (m["recs"][:, 2] - m["recs"][:, 0]).tolist()


def test_chunk_of_line_breaks(lib):
    """4096 consecutive line breaks: every lane counts 16, the workgroup's scan runs at its maximum; 1024 'records' of empty lines: odd"""
    m = check_scan(lib, b"\n" * 4096 + SLACK, 0, 4096, "4096 line breaks")
    assert m["lines"] == 4096 and m["n"] == 1024 and m["odd"] == 1 and m["max_seq"] == 0


def test_chunk_of_line_breaks_from_an_odd_begin(lib):
    """the same from byte 17, between line breaks that do not count"""
    m = check_scan(lib, b"\n" * 17 + b"\n" * 4096 + b"@" + SLACK, 17, 17 + 4097, "4096 line breaks from byte 17")
    assert m["lines"] == 4096 and m["n"] == 1024 and m["odd"] == 1


def test_only_0x0a_is_a_line_break(lib):
    """bytes that differ from 0x0A in one bit or one nibble, 0x00 and 0xFF, next to real line breaks, in every order: exact per byte"""
    rng = np.random.default_rng(5)
    alphabet = np.array([0x8A, 0x0B, 0x1A, 0x4A, 0x00, 0xFF, 0x0A, 0x0A, 0x2A, 0x0E, 0x09, 0x40, 0x2B], np.uint8)
    body = bytes(rng.choice(alphabet, 9000).tolist())
    m = check_scan(lib, b"\x8a" * 16 + body + SLACK, 16, 16 + len(body), "look-alikes")
    assert m["lines"] == body.count(b"\n") > 1000
    for x in (0x8A, 0x0B, 0x1A, 0x4A, 0x00, 0xFF):   # every arrangement of one look-alike and line breaks in a 32-bit word
        body = b"".join(bytes(x if (k >> j) & 1 else 10 for j in range(4)) for k in range(16)) * 3
        m = check_scan(lib, body + SLACK, 0, len(body), "0x%02x" % x)
        assert m["lines"] == 3 * 32


def test_line_counts(lib):
    """lines % 4 in {0, 1, 2, 3}: only whole records count, consumed lies behind them; no record: consumed = 0; no line at all"""
    rng = np.random.default_rng(6)
    base = records(*plain(5, rng))
    extra = [b"", b"@h x\n", b"@h x\nACGT\n", b"@h x\nACGT\n+\n", b"@h x\nACGT\n+\nIII"]
    for k, tail in enumerate(extra):
        m = check_scan(lib, b"\n" * 32 + base + tail + SLACK, 32, 32 + len(base + tail), "5 records + %d lines" % (k % 4))
        assert m["n"] == 5 and m["lines"] == 20 + (k if k < 4 else 3) and m["consumed"] == len(base)
    for tail in extra[1:] + [b"no line break in here", b"\n", b"x"]:
        m = check_scan(lib, b"\n" * 32 + tail + SLACK, 32, 32 + len(tail), repr(tail))
        assert m["n"] == 0 and m["consumed"] == 0 and m["lines"] == tail.count(b"\n") < 4


@pytest.mark.parametrize("extra_lines", [0, 2])
def test_tables_too_small_by_one(lib, extra_lines):
    """L lines, n records: cap_lines in {L, L + 1, L + 2} x cap_recs in {n - 1, n, n + 1}. overflow exactly when the line table does not hold
    L + 1 starts or the record table n records; lines and n are right either way; nothing is written behind either table; what IS written is
    right; and the second call, rescan = true on the same chunk tables with tables that fit exactly, gives the full answer."""
    rng = np.random.default_rng(7)
    body = records(*plain(70, rng)) + [b"", b"", b"@next\nACGT\n"][extra_lines]
    buf = b"\n" * 21 + body + SLACK
    begin, end = 21, 21 + len(body)
    full = tm.scan(buf, begin, end)
    Ln, n = full["lines"], full["n"]
    assert Ln == 280 + extra_lines and n == 70
    seen = set()
    for cap_lines in (Ln, Ln + 1, Ln + 2):
        for cap_recs in (n - 1, n, n + 1):
            what = "cap_lines %d, cap_recs %d" % (cap_lines, cap_recs)
            m = tm.scan(buf, begin, end, cap_lines, cap_recs)
            assert m["overflow"] == int(cap_lines == Ln or cap_recs == n - 1)
            seen.add(m["overflow"])
            info, ls, rec, chunk, first, info2, ls2, rec2 = gpu_scan(lib, buf, begin, end, cap_lines, cap_recs, rescan=(Ln + 1, n))
            assert (int(info["lines"]), int(info["n"]), int(info["overflow"])) == (Ln, n, m["overflow"]), what
            assert (ls[cap_lines:] == PAT32).all() and (rec[cap_recs:] == PAT32).all(), (what, "a write behind a table")
            if not m["overflow"]:
                assert_full_answer(m, info, ls, rec, what)
            else:
                k = min(cap_lines, Ln + 1)
                assert np.array_equal(ls[:k], m["line_start"][:k]), what
                for r in range(min(n, cap_recs)):
                    assert (rec[r] == PAT32).all() or np.array_equal(rec[r], m["recs"][r]), (what, r)
            assert_full_answer(tm.scan(buf, begin, end, Ln + 1, n), info2, ls2, rec2, what + ", scanned again")
    assert seen == {0, 1}


HEADERS = [b"@", b"@\r", b"@ x", b"@id", b"@id\r", b"@id \t \r", b"@a\tb c", b"@   ", b"@id\x0b", b"@id\x0c\r", b"@id\x0b desc", b"@id\x0c", b"@id\x0b\x0c \t\r",
           b'@q"uote', b"@back\\slash", b"@c\x01tl", b"@del\x7f", b'@"\\\x01\x7f x']


@pytest.mark.parametrize("header", HEADERS, ids=[repr(h)[2:-1] for h in HEADERS])
def test_headers(lib, header):
    """record.id() = header[1..].trim_end().splitn(2, ' ').next() for the header as record 0, as record 64 (second wave) and as the last"""
    rng = np.random.default_rng(8)
    ids, seqs = plain(130, rng)
    lines = [b"@" + i for i in ids]
    for j in (0, 64, 129):
        lines[j] = header
    body = b"".join(h + b"\n" + s + b"\n+\n" + b"I" * len(s) + b"\n" for h, s in zip(lines, seqs))
    m = check_scan(lib, b"\n" * 16 + body + SLACK, 16, 16 + len(body), repr(header))
    want = tm.record_id(header)
    for j in (0, 64, 129):
        o, l = int(m["recs"][j, 0]), int(m["recs"][j, 1])
        assert (b"\n" * 16 + body)[o:o + l] == want
    assert m["odd"] == 0


def test_vt_and_ff_are_trimmed(lib):
    """Rust's trim_end strips White_Space: VT and FF go with blank, tab and CR (bio 1.5 gives `read7` for `@read7\\x0c`)"""
    body = records([b"read7\x0c", b"read8\x0b", b"read9 \x0b\x0c", b"in\x0bside", b"in\x0cside\x0b d"], [b"ACGT"] * 5)
    buf = body + SLACK
    info, ls, rec, chunk, first = gpu_scan(lib, buf, 0, len(body), 32, 8)
    assert [buf[int(o):int(o) + int(l)] for o, l in rec[:5, :2]] == [b"read7", b"read8", b"read9", b"in\x0bside", b"in\x0cside\x0b"]


def test_sequences(lib):
    """empty, CR alone, ACGT + CR, lower case, N, IUPAC letters; the longest sequence held by lane 63 of a wave, by lane 63 of the second wave,
    by the last record, by record 0"""
    rng = np.random.default_rng(9)
    special = [b"", b"\r", b"ACGT\r", b"acgtn", b"N", b"NNNN\r", b"RYKMSWBDHVN", b"rykmswbdhvn\r", b"acgu", b"X*-."]
    for holder in (63, 127, 129, 0):
        ids, seqs = plain(130, rng, 0, 30)
        for j, s in enumerate(special):
            seqs[3 + 11 * j] = s
        seqs[holder] = b"ACGTN" * 9 + b"\r"
        body = b"".join(b"@" + i + b"\n" + s + b"\n+\n" + b"I" * len(s) + b"\n" for i, s in zip(ids, seqs))
        m = check_scan(lib, body + SLACK, 0, len(body), "longest in record %d" % holder)
        assert m["max_seq"] == 45 and int(m["recs"][holder, 3]) == 45
        assert [int(m["recs"][3 + 11 * j, 3]) for j in range(6)] == [0, 0, 4, 5, 1, 4]


def test_odd_marking(lib):
    """'@' or '+' missing in record 0, in record 64, in the last record: odd. A quality line that starts with '@' or '+' does not matter"""
    rng = np.random.default_rng(10)
    ids, seqs = plain(130, rng, 1, 30)
    for line, repl in ((0, b"r"), (0, b">"), (2, b"-"), (2, b"@")):
        for j in (0, 64, 129):
            lines = records(ids, seqs).split(b"\n")
            lines[4 * j + line] = repl + lines[4 * j + line][1:]
            body = b"\n".join(lines)
            m = check_scan(lib, body + SLACK, 0, len(body), "line %d of record %d starts with %r" % (line, j, repl))
            assert m["odd"] == 1 and m["n"] == 130
    for q in (b"@", b"+"):
        lines = records(ids, seqs).split(b"\n")
        for j in (0, 64, 129):
            lines[4 * j + 3] = q + lines[4 * j + 3][1:]
        body = b"\n".join(lines)
        m = check_scan(lib, body + SLACK, 0, len(body), "quality lines that start with %r" % q)
        assert m["odd"] == 0 and m["n"] == 130


def test_seventy_thousand_short_records(lib):
    """more records than one row of 256-thread groups covers, about a megabyte of text, sequences of 1..3 bases"""
    rng = np.random.default_rng(11)
    n = 70000
    lens = rng.integers(1, 4, n)
    body = b"".join(b"@r%d\n%s\n+\n%s\n" % (i, b"ACG"[:l], b"III"[:l]) for i, l in enumerate(lens.tolist()))
    m = check_scan(lib, b"\n" * 7 + body + SLACK, 7, 7 + len(body), "70 000 records")
    assert m["n"] == n and m["max_seq"] == 3 and m["odd"] == 0 and m["consumed"] == len(body)


# -------------------------------------------------------------- encode ----
def check_encode(L, seqs, wpr, what):
    body = records([b"id%d d" % i for i in range(len(seqs))], seqs)
    buf = b"\n" * 5 + body + b"@" + SLACK
    m = tm.scan(buf, 5, 5 + len(body) + 1)
    n = len(seqs)
    assert m["n"] == n and [buf[int(o):int(o) + int(l)] for o, l in m["recs"][:, 2:]] == seqs
    want_tiles, want_lens = tm.encode(seqs, wpr)
    text = np.frombuffer(buf, np.uint8)
    rec = np.ascontiguousarray(m["recs"], np.uint32) if n else np.zeros((1, 4), np.uint32)
    tiles, lens = np.full(len(want_tiles) + GUARD, PAT64, np.uint64), np.full(n + GUARD, PAT32, np.uint32)
    ok(L, L.tp_encode_rec(text.ctypes.data, len(text), rec.ctypes.data, n, wpr, tiles.ctypes.data, lens.ctypes.data))
    assert np.array_equal(lens[:n], want_lens) and (lens[n:] == PAT32).all(), what
    assert np.array_equal(tiles[: len(want_tiles)], want_tiles), (what, np.flatnonzero(tiles[: len(want_tiles)] != want_tiles)[:5])
    assert (tiles[len(want_tiles):] == PAT64).all(), what


@pytest.mark.parametrize("wpr", [1, 2, 5])
def test_encode_in_place(lib, wpr):
    """n in {0, 1, 63, 64, 65, 257} x lengths {0, 1, 31, 32, 33, 32 wpr - 1, 32 wpr, 32 wpr + 1, 32 wpr + 40}: either case, N and IUPAC letters as
    A, a read cut at 32 wpr bases (lens too), the lanes of the last tile beyond n zero, nothing written behind tiles or lens"""
    rng = np.random.default_rng(20 + wpr)
    lengths = [0, 1, 31, 32, 33, 32 * wpr - 1, 32 * wpr, 32 * wpr + 1, 32 * wpr + 40]
    letters = np.frombuffer(b"ACGTACGTacgtNnRY", np.uint8)
    seq = lambda l: bytes(rng.choice(letters, l).tolist())
    for l in lengths:
        check_encode(lib, [seq(l)], wpr, "one read of %d bases" % l)
        check_encode(lib, [b"T" * l], wpr, "one read of %d T" % l)
    for n in (0, 63, 64, 65, 257):
        shift = int(rng.integers(0, 9))
        check_encode(lib, [seq(lengths[(i + shift) % 9]) for i in range(n)], wpr, "%d reads" % n)


# -------------------------------------------------------------- render ----
def gpu_render(L, results, arena, arena_cap, ids, cls_text, flag_mark, form, text_cap, windows=None, flagged0=0):
    """-> (len, off, flagged, text): len / off with their guards; text = the device's whole buffer (text_cap + slack bytes), or the windows
    ((offset, bytes), (offset, bytes)) of it"""
    n = len(results)
    results = np.ascontiguousarray(results, tm.RESULT_DTYPE) if n else np.zeros(1, tm.RESULT_DTYPE)
    arena = np.ascontiguousarray(arena, np.uint32)
    assert len(arena) >= arena_cap
    if isinstance(ids, tuple):
        id_bytes, id_off, rec = ids   # already laid out
    elif form == "off":
        id_bytes = b"".join(ids)
        id_off, rec = np.concatenate([[0], np.cumsum([len(i) for i in ids])]).astype(np.uint64), None
    else:   # where they lie in a text: "@id description\n..." with the record's other fields unused
        parts, rec, at = [], np.zeros((max(n, 1), 4), np.uint32), 3
        for i, rid in enumerate(ids):
            rec[i] = (at + 1, len(rid), 0xFFFFFFFF, 0xFFFFFFFF)
            parts.append(b"@" + rid + b" d\n")
            at += len(parts[-1])
        id_bytes, id_off = b"###" + b"".join(parts), None
    idb = np.frombuffer(id_bytes, np.uint8) if id_bytes else np.zeros(1, np.uint8)
    cls_off = np.concatenate([[0], np.cumsum([len(c) for c in cls_text])]).astype(np.uint64)
    cls_txt = np.frombuffer(b"".join(cls_text) or b"\0", np.uint8)
    ln, off = np.full(n + 1 + GUARD, PAT32, np.uint32), np.full(n + 1 + GUARD, PAT64, np.uint64)
    flagged = np.full(tm.FLAG_BUCKETS, flagged0, np.uint64)
    alloc = text_cap + L.tp_text_slack()
    (w0, l0), (w1, l1) = windows or ((0, alloc), (0, 0))
    out0, out1 = np.zeros(max(l0, 1), np.uint8), np.zeros(max(l1, 1), np.uint8)
    ok(L, L.tp_render(results.ctypes.data, n, arena.ctypes.data, arena_cap, idb.ctypes.data, len(id_bytes), id_off.ctypes.data if id_off is not None else None,
                      rec.ctypes.data if rec is not None else None, cls_off.ctypes.data, len(cls_text), cls_txt.ctypes.data, flag_mark, text_cap, SENTINEL,
                      ln.ctypes.data, off.ctypes.data, flagged.ctypes.data, w0, l0, out0.ctypes.data, w1, l1, out1.ctypes.data))
    return ln, off, flagged, (out0[:l0].tobytes() if windows is None else (out0[:l0].tobytes(), out1[:l1].tobytes()))


def check_render(L, results, arena, arena_cap, ids, cls_text, flag_mark, what, forms=("off", "rec")):
    """both id forms, a text buffer of exactly the text's size: lengths, offsets, flag buckets (added to what they held) and bytes are the
    model's, the bytes behind the text untouched"""
    lines, flagged = tm.render(results, arena, arena_cap, ids, cls_text, flag_mark)
    n, total = len(lines), sum(len(l) for l in lines)
    for form in forms:
        ln, off, fl, text = gpu_render(L, results, arena, arena_cap, ids, cls_text, flag_mark, form, total, flagged0=5)
        w = (what, form)
        assert ln[:n].tolist() == [len(l) for l in lines] and ln[n] == 0 and (ln[n + 1:] == PAT32).all(), w
        assert off[: n + 1].tolist() == np.concatenate([[0], np.cumsum([len(l) for l in lines], dtype=np.int64)]).tolist() and (off[n + 1:] == PAT64).all(), w
        assert fl.tolist() == [5 + f for f in flagged], w
        got = text[:total].split(b"\n")[:-1] if total else []
        assert len(got) == n and [g + b"\n" for g in got] == lines, (w, [(i, g, l) for i, (g, l) in enumerate(zip(got, lines)) if g + b"\n" != l][:3])
        assert text[:total] == b"".join(lines), w
        assert text[total:] == bytes([SENTINEL]) * (len(text) - total), (w, "bytes behind the text")
    return lines, flagged


def res_of(rows):
    """rows of (mapped, coverage, class_off, class_len)"""
    r = np.zeros(len(rows), tm.RESULT_DTYPE)
    for i, (mapped, cov, off, cl) in enumerate(rows):
        r[i] = (cov, (tm.MAPPED_BIT if mapped else 0) | (i % 3), off, cl)
    return r


POWERS = sorted({0, 2 ** 32 - 1} | {10 ** p - 1 for p in range(1, 10)} | {10 ** p for p in range(1, 10)})


def test_render_numbers(lib):
    """class ids at 0, 9, 10, 99, 100 ... 999 999 999, 1 000 000 000, 4 294 967 295 in classes of 0, 1, 2 and 300 ids in the arena; coverages
    over the same list up to PA_MAX_READ_LEN = 1 048 575; index classes whose text is empty, one id, 2000 ids"""
    assert POWERS[:4] == [0, 9, 10, 99] and POWERS[-3:] == [999999999, 1000000000, 4294967295] and len(POWERS) == 20
    arena, rows = [], []
    for v in POWERS:                                   # classes of one id
        rows.append((True, 40, len(arena), 1))
        arena.append(v)
    for a, b in zip(POWERS, POWERS[1:]):               # of two
        rows.append((True, 33, len(arena), 2))
        arena += [a, b]
    for s in range(3):                                 # of 300
        rows.append((True, 150, len(arena), 300))
        arena += [POWERS[(s + 7 * j) % 20] for j in range(300)]
    rows.append((True, 31, 5, 0))                      # of none
    covs = [v for v in POWERS if v <= 1048575] + [1048575, 1048574, 31, 32]
    rows += [(True, c, 0, 1) for c in covs] + [(True, c, tm.CLASS_REF | 1, 1) for c in covs]
    cls_text = [b"", b"7", b", ".join(b"%d" % (3 * i) for i in range(2000)), b"4294967295"]
    rows += [(True, 100, tm.CLASS_REF | c, [0, 1, 2000, 1][c]) for c in (0, 1, 2, 3, 2, 0)]
    ids = [b"r%d" % i for i in range(len(rows))]
    arena = np.array(arena, np.uint32)
    lines, _ = check_render(lib, res_of(rows), arena, len(arena), ids, cls_text, 0, "numbers")
    assert lines[19] == b'(false, "r19", [4294967295], 40)\n' and lines[20] == b'(false, "r20", [0, 9], 33)\n' and len(lines[39]) > 300 * 3
    assert any(l.endswith(b"], 1048575)\n") for l in lines) and lines[-4].count(b",") == 1999 + 3 and lines[-1] == b'(true, "r%d", [], 100)\n' % (len(rows) - 1)


def test_render_flag_rule(lib):
    """(mapped, coverage >= 32, no class) and nothing else flags a read; an unmapped read prints coverage 0 whatever its record holds"""
    rows = [(m, c, off, cl) for m in (True, False) for c in (31, 32, 0, 1000) for off, cl in ((0, 0), (0, 1), (tm.CLASS_REF | 0, 0), (tm.CLASS_REF | 1, 1))]
    ids = [b"f%d" % i for i in range(len(rows))]
    for mark in (0, 3, len(rows)):
        lines, flagged = check_render(lib, res_of(rows), np.array([17], np.uint32), 1, ids, [b"", b"9"], mark, "flag rule, flag_mark %d" % mark)
        want = [m and c >= 32 and cl == 0 for m, c, off, cl in rows]
        assert [l.startswith(b"(true") for l in lines] == want and sum(want) == 4 == sum(flagged)
        assert all(l.endswith(b", 0)\n") for l in lines[16:]) and lines[4].endswith(b"[], 32)\n") and lines[21] == b'(false, "f21", [17], 0)\n'


def test_render_arena_edge(lib):
    """a class that ends with the arena is printed; one that ends one entry beyond it — or begins beyond it — is printed empty and does not flag
    its read; the arena lies at the end of its allocation"""
    cap = 1024 + 300
    arena = (np.arange(cap, dtype=np.uint64) * 2654435761 % 2 ** 32).astype(np.uint32)
    rows = [(True, 50, cap - 300, 300), (True, 50, cap - 299, 300), (True, 50, cap - 1, 1), (True, 50, cap, 1), (True, 50, cap, 0), (True, 50, cap + 1, 0),
            (True, 50, 0x7FFFFFFF, 0x7FFFFFFF), (True, 50, 0x7FFFFFFF, 0xFFFFFFFF), (True, 50, 0, cap), (True, 50, 0, cap + 1), (False, 50, cap, 1)]
    ids = [b"a%d" % i for i in range(len(rows))]
    lines, flagged = check_render(lib, res_of(rows), arena, cap, ids, [b""], 0, "arena edge")
    nums = lambda l: [int(x) for x in l[l.index(b"[") + 1:l.index(b"]")].split(b", ") if x]
    assert [len(nums(l)) for l in lines] == [300, 0, 1, 0, 0, 0, 0, 0, cap, 0, 0] and nums(lines[0]) == arena[-300:].tolist() and nums(lines[2]) == [int(arena[-1])]
    assert lines[1] == b'(false, "a1", [], 50)\n' and lines[4] == b'(true, "a4", [], 50)\n' and sum(flagged) == 2
    check_render(lib, res_of(rows[3:8]), arena[:0], 0, ids[3:8], [b""], 0, "no arena at all")


def test_render_ids(lib):
    """every byte value as an id of one byte, all 256 in one id, the empty id: Rust's Debug for str below 0x80, bytes from 0x80 on copied"""
    ids = [bytes([c]) for c in range(256)] + [bytes(range(256)), b"", b"it's", bytes(range(255, -1, -1)) * 3, b""]
    rows = [(i % 2 == 0, 40, 0, i % 2) for i in range(len(ids))]
    lines, _ = check_render(lib, res_of(rows), np.array([3], np.uint32), 1, ids, [b""], 0, "ids")
    body = lambda l: l[l.index(b'"') + 1:l.rindex(b'"')]
    assert [body(lines[c]) for c in (0, 9, 10, 13, 0x22, 0x27, 0x5C)] == [b"\\0", b"\\t", b"\\n", b"\\r", b'\\"', b"'", b"\\\\"]
    assert [body(lines[c]) for c in (1, 0x0B, 0x0C, 0x0F, 0x10, 0x1F, 0x7F, 0x80, 0xFF)] == [b"\\u{1}", b"\\u{b}", b"\\u{c}", b"\\u{f}", b"\\u{10}", b"\\u{1f}", b"\\u{7f}",
                                                                                             b"\x80", b"\xff"]
    assert lines[257] == b'(false, "", [3], 0)\n' and lines[260] == b'(true, "", [], 40)\n'


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_render_sizes(lib, n):
    rng = np.random.default_rng(30 + n)
    arena = rng.integers(0, 2 ** 32, 64, dtype=np.uint64).astype(np.uint32)
    cls_text = [b"", b"1, 2", b"77"]
    rows = []
    for i in range(n):
        kind = int(rng.integers(0, 4))
        cl = int(rng.integers(0, 5))
        rows.append((kind != 0, int(rng.integers(0, 200)), tm.CLASS_REF | int(rng.integers(0, 3)), cl) if kind == 1 else (kind != 0, int(rng.integers(0, 200)), int(rng.integers(0, 60)), cl))
    ids = [bytes(rng.integers(0, 128, int(rng.integers(0, 12)), dtype=np.uint8).tolist()) for _ in range(n)]
    check_render(lib, res_of(rows), arena, 64, ids, cls_text, n // 2, "%d reads" % n)


def test_render_text_cap(lib):
    """a text buffer one byte too small: nothing is written at all (the host sees the length and renders again); exactly large enough: the
    text, and nothing behind it. off[] is the model's in both cases"""
    rows = [(True, 40 + i, i % 7, i % 3) for i in range(300)]
    ids = [b"cap%d" % i for i in range(300)]
    arena = np.arange(100, 110, dtype=np.uint32)
    lines, _ = tm.render(res_of(rows), arena, 10, ids, [b""], 0)
    total = sum(len(l) for l in lines)
    offs = np.concatenate([[0], np.cumsum([len(l) for l in lines])]).tolist()
    for form in ("off", "rec"):
        for cap in (total - 1, total, total + 1, 0):
            ln, off, fl, text = gpu_render(lib, res_of(rows), arena, 10, ids, [b""], 0, form, cap)
            assert off[:301].tolist() == offs and ln[:300].tolist() == [len(l) for l in lines], (form, cap)
            written = b"".join(lines) if cap >= total else b""
            assert text == written + bytes([SENTINEL]) * (len(text) - len(written)), (form, cap)


_big = {}


def big_batch():
    if not _big:
        n = 2000100
        res = np.zeros(n, tm.RESULT_DTYPE)
        res["coverage"], res["mismatches"] = 32, tm.MAPPED_BIT
        rec = np.zeros((n, 4), np.uint32)
        rec[:, 0], rec[:, 1] = np.arange(n), 1
        _big.update(n=n, res=res, ids={"off": (b"x" * n, np.arange(n + 1, dtype=np.uint64), None), "rec": (b"x" * n, None, rec)})
    return _big


@pytest.mark.parametrize("flag_mark", [0, 37, 1000000, 2000100, 5000000])
def test_render_flag_buckets(lib, flag_mark):
    """2 000 100 flagged reads: those before flag_mark in bucket 0, the j-th million behind it in bucket j — flag_mark in the middle of a wave
    (37), on a wave's edge (10^6 = 15 625 x 64), at and beyond the batch's end; all 64 buckets and off[n]. The text: its first and last 4 KiB.
    (Not pinned: the clamp into bucket 63, which takes 62 M reads.)"""
    b = big_batch()
    n = b["n"]
    line = b'(true, "x", [], 32)\n'
    total = n * len(line)
    i = np.arange(n, dtype=np.int64)
    want = np.bincount(np.where(i < flag_mark, 0, np.minimum(tm.FLAG_BUCKETS - 1, 1 + (i - flag_mark) // tm.FLAG_BUCKET_READS)), minlength=tm.FLAG_BUCKETS)
    assert want.sum() == n and (flag_mark != 37 or want[:5].tolist() == [37, 1000000, 1000000, 63, 0])
    for form in ("off", "rec"):
        ln, off, fl, (head, tail) = gpu_render(lib, b["res"], np.zeros(1, np.uint32), 0, b["ids"][form], [b""], flag_mark, form, total,
                                               windows=((0, 4096), (total - 4096, 4096 + 64)))
        assert fl.tolist() == want.tolist(), form
        assert int(off[n]) == total and (ln[:n] == len(line)).all() and ln[n] == 0, form
        assert np.array_equal(off[: n + 1], np.arange(n + 1, dtype=np.uint64) * np.uint64(len(line))) and (off[n + 1:] == PAT64).all() and (ln[n + 1:] == PAT32).all(), form
        assert head == (line * 205)[:4096] and tail == (line * 205)[-4096:] + bytes([SENTINEL]) * 64, form
