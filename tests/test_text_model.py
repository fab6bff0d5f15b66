"""tests/text_model.py — the independent model the text kernels are compared with (tests/test_gpu_text_kernels.py) — pinned on the CPU tier
against what the suite already knows: the host's scan (pa_fastq_scan_host; and, through the text probe, the id lengths it keeps to
itself), the tuples tests/test_gpu_ingest.py expects literally, the host's 2-bit packing. Also the CPU-tier case of the id rule: the
host's scan cuts record.id() as bio 1.5 does, trailing VT / FF included."""
import ctypes as C

import numpy as np
import pytest

import helpers
import test_fastq_scan as tfs
import text_model as tm

pa = helpers.pa


def test_constants_are_the_products():
    assert tm.RESULT_DTYPE == pa.RESULT_DTYPE and tm.CLASS_REF == pa.PA_CLASS_REF and tm.MAPPED_BIT == pa.PA_MAPPED_BIT
    assert tm.COVERAGE_THRESHOLD == pa.PA_READ_COVERAGE_THRESHOLD


@pytest.mark.parametrize("nl", ["\n", "\r\n"])
def test_scan_equals_the_host_scan(tmp_path, nl):
    """the LF / CRLF / empty-sequence texts of tests/test_fastq_scan.py: starts, header lengths, sequence lengths"""
    rng = np.random.default_rng(11)
    ids, seqs = tfs._records(3000, rng, empty_every=97)
    raw = tfs._text(ids, seqs, nl=nl).encode()
    p = tmp_path / "t.fq"
    p.write_bytes(raw)
    starts, hdr, seq, kind = pa.fastq_scan(str(p), 3)
    m = tm.scan(raw, 0, len(raw))
    assert kind == 0 and m["n"] == len(ids) == len(starts) and m["lines"] == 4 * len(ids) and m["consumed"] == len(raw) and not m["odd"]
    recs = m["recs"].astype(np.int64)
    assert np.array_equal(recs[:, 0] - 1, starts.astype(np.int64))
    assert np.array_equal(recs[:, 2] - recs[:, 0], hdr.astype(np.int64))        # the header line: from the '@' to its line break
    assert np.array_equal(recs[:, 3], seq.astype(np.int64))
    assert m["max_seq"] == max(len(s) for s in seqs)
    for i in (0, 97, 2999):
        assert raw[recs[i, 0]:recs[i, 0] + recs[i, 1]].decode() == ids[i] and raw[recs[i, 2]:recs[i, 2] + recs[i, 3]].decode() == seqs[i]


HEADERS = [b"@", b"@\r", b"@ x", b"@id", b"@id\r", b"@id \t \r", b"@a\tb c", b"@   ", b"@id\x0b", b"@id\x0c", b"@id\x0c\r", b"@id\x0b desc", b"@id\x0b\x0c \t",
           b'@q"\\\x01\x7f', b"@\x0bid", b"@id\x0bx"]
IDS = [b"", b"", b"", b"id", b"id", b"id", b"a\tb", b"", b"id", b"id", b"id", b"id\x0b", b"id", b'q"\\\x01\x7f', b"\x0bid", b"id\x0bx"]


def test_id_rule_is_bios():
    """header[1..].trim_end().splitn(2, ' ').next(): trailing White_Space — VT and FF too — goes, the cut is at the first SPACE only"""
    assert [tm.record_id(h) for h in HEADERS] == IDS


def test_host_scan_cuts_ids_as_the_model(built, tmp_path):
    """the host's scan (csrc/fastq_text.cpp, through the text probe: pa_fastq_scan_host does not hand the id lengths out) on every header
    of the list, LF and CRLF: starts, header, id and sequence lengths are the model's. `@id\\x0b` and `@id\\x0c` give `id`."""
    lib = helpers.text_lib()
    for nl in (b"\n", b"\r\n"):
        raw = b"".join(h + nl + b"ACGT"[: i % 5] + nl + b"+" + nl + b"IIII"[: i % 5] + nl for i, h in enumerate(HEADERS * 3))
        p = tmp_path / "h.fq"
        p.write_bytes(raw)
        cap = 3 * len(HEADERS)
        n = C.c_uint64()
        starts, hdr, idl, seq = np.zeros(cap, np.uint64), np.zeros(cap, np.uint32), np.zeros(cap, np.uint32), np.zeros(cap, np.uint32)
        rc = lib.tp_host_scan(str(p).encode(), 2, C.byref(n), starts.ctypes.data, hdr.ctypes.data, idl.ctypes.data, seq.ctypes.data, cap)
        assert rc == 0 and n.value == cap, lib.tp_last_error()
        m = tm.scan(raw, 0, len(raw))
        recs = m["recs"].astype(np.int64)
        assert m["n"] == cap and np.array_equal(recs[:, 0] - 1, starts.astype(np.int64)) and np.array_equal(recs[:, 2] - recs[:, 0], hdr.astype(np.int64))
        assert idl.tolist() == recs[:, 1].tolist() == [len(i) for i in IDS * 3], nl
        assert seq.tolist() == recs[:, 3].tolist() == [i % 5 for i in range(cap)]


def test_render_gives_the_lines_the_ingest_test_expects():
    """tests/test_gpu_ingest.py::test_gpu_scan_and_host_scan_agree, literally"""
    res = np.zeros(5, tm.RESULT_DTYPE)
    res["mismatches"] = [tm.MAPPED_BIT, 0, tm.MAPPED_BIT | 1, tm.MAPPED_BIT, 0]
    res["coverage"] = [40, 7, 31, 32, 0]
    res["class_off"] = [tm.CLASS_REF | 1, 0, 0, 0, 0]
    res["class_len"] = [3, 0, 2, 0, 0]
    ids = [b'qu"ote', b"back\\slash\x01ctl", b"tab\tinside", b"it's", b"nul\x00\x7f\x1f\r\n"]
    lines, flagged = tm.render(res, np.array([4, 17], np.uint32), 2, ids, [b"", b"1, 5, 9"], 3)
    assert lines == [b'(false, "qu\\"ote", [1, 5, 9], 40)\n', b'(false, "back\\\\slash\\u{1}ctl", [], 0)\n', b'(false, "tab\\tinside", [4, 17], 31)\n',
                     b'(true, "it\'s", [], 32)\n', b'(false, "nul\\0\\u{7f}\\u{1f}\\r\\n", [], 0)\n']
    assert flagged == [0, 1] + [0] * 62
    assert tm.render(res, np.array([4, 17], np.uint32), 1, ids, [b"", b"1, 5, 9"], 4)[0][2] == b'(false, "tab\\tinside", [], 31)\n'
    assert tm.render(res, np.array([4, 17], np.uint32), 2, ids, [b"", b"1, 5, 9"], 4)[1] == [1] + [0] * 63
    assert tm.escape_debug(bytes([0x0B, 0x0C, 0x0F, 0x10, 0x80, 0xFF])) == b"\\u{b}\\u{c}\\u{f}\\u{10}\x80\xff"


def test_encode_equals_the_host_packing():
    """the reads of tests/test_gpu_parity.py::test_encode_kernel_equals_host_packing, and a read cut at 32 * wpr bases"""
    _, seqs = helpers.read_fastq()
    reads = seqs[:1000] + ["acgtnNRY" * 9, "", "T"]
    h_tiles, h_lens, wpr = pa.encode_reads_host(reads)
    tiles, lens = tm.encode([r.encode() for r in reads], wpr)
    assert np.array_equal(tiles, h_tiles) and np.array_equal(lens, h_lens)
    tiles, lens = tm.encode([b"T" * 70, b"c" * 64, b"g" * 63], 2)
    assert lens.tolist() == [64, 64, 63] and len(tiles) == 128
    assert int(tiles[0]) == 2 ** 64 - 1 and int(tiles[64]) == 2 ** 64 - 1 and int(tiles[1]) == int("01" * 32, 2) and int(tiles[66]) == int("10" * 31, 2)
