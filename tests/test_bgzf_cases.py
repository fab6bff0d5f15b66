"""BGZF on the CPU tier: the vectors of tests/bgzf_cases.py pinned by zlib (not by the product), pa_bgzf_scan against a Python walk of
the headers, and the DEFLATE decoder of csrc/inflate_core.hpp run on every vector as a stand-alone program under ASan + UBSan
(tests/inflate/): every corrupt payload has been through the decoder's decisions on a CPU before tests/test_gpu_inflate.py sends it to a
GPU. Every comparison is exact."""
import importlib.util
import struct
import subprocess
import zlib

import numpy as np
import pytest

import bgzf_cases as bc
import helpers


def _members(data):
    rows = bc.walk(data)
    assert rows is not None
    return rows


def test_vectors_are_pinned_by_zlib():
    import gzip
    for name, data, text in bc.valid_cases():
        rows = _members(data)
        got = b""
        for r in rows:
            ok, t = bc.zlib_verdict(data[r["in_off"]:r["in_off"] + r["in_len"]], r["out_len"], r["crc32"])
            assert ok, (name, r)
            got += t
        assert got == text, name
        assert gzip.decompress(data) == text, name
    sizes = [r["out_len"] for r in _members(dict((n, d) for n, d, _ in bc.valid_cases())["ISIZE 1 .. 65536 interleaved"])]
    assert {1, 2, 3, 5, 63, 64, 65, 65280, 65536} <= set(sizes)
    names = set()
    for name, data, bad, texts in bc.corrupt_cases():
        rows = _members(data)
        assert len(rows) == 4 and bad == 1, name   # left neighbour, the corrupt member, right neighbour, EOF block
        for i, r in enumerate(rows):
            ok, t = bc.zlib_verdict(data[r["in_off"]:r["in_off"] + r["in_len"]], r["out_len"], r["crc32"])
            assert ok == (i != bad), (name, i)
            if i in (0, 2):
                assert t == texts[i], name
        names.add(name)
    assert len(names) == 16
    for name, data in bc.not_bgzf_cases():
        assert bc.walk(data) is None, name
        if name in ("ordinary gzip", "gzip with FNAME only", "first member BGZF, second ordinary"):
            gzip.decompress(data)   # ... while zlib reads them


def test_scan_is_the_python_walk(built):
    pa = helpers.pa
    for name, data, text in bc.valid_cases():
        rows = _members(data)
        got = pa.bgzf_scan(data)
        assert got is not None, name
        members, text_bytes = got
        assert text_bytes == len(text) and len(members) == len(rows), name
        for f in ("in_off", "out_off", "file_off", "in_len", "out_len", "crc32"):
            assert members[f].tolist() == [r[f] for r in rows], (name, f)
        assert not members["reserved"].any()
    for name, data, _, _ in bc.corrupt_cases():   # corrupt payloads are still BGZF: the scan does not inflate
        assert len(pa.bgzf_scan(data)[0]) == 4, name
    for name, data in bc.not_bgzf_cases():
        assert pa.bgzf_scan(data) is None, name
    # members == NULL only counts; a table that is too small is said to be
    import ctypes as C
    data = bc.valid_cases()[1][1]
    buf = np.frombuffer(data, np.uint8)
    n, tb = C.c_uint64(), C.c_uint64()
    assert pa.lib().pa_bgzf_scan(buf.ctypes.data, len(buf), None, 0, C.byref(n), C.byref(tb)) == 0 and n.value == 3 and tb.value == 3000
    two = np.zeros(3, pa.BGZF_MEMBER_DTYPE)
    two["crc32"][2] = 0xDEAD
    rc = pa.lib().pa_bgzf_scan(buf.ctypes.data, len(buf), two.ctypes.data_as(C.POINTER(pa._ffi.BgzfMember)), 2, C.byref(n), C.byref(tb))
    assert rc == pa._ffi.PA_ERR_BUFFER_TOO_SMALL and n.value == 3 and two["crc32"][2] == 0xDEAD and two["out_off"][1] == 1000
    assert pa.lib().pa_bgzf_scan(buf.ctypes.data, len(buf) - 1, None, 0, C.byref(n), C.byref(tb)) == pa._ffi.PA_ERR_NOT_BGZF and n.value == 0


def case_file(path, files):
    """the members of several BGZF files as one case file of tests/inflate/inflate_host_check.cpp -> the rows, file by file"""
    rows_by_file = [_members(d) for d in files]
    with open(path, "wb") as f:
        f.write(b"PAIC" + struct.pack("<I", sum(len(r) for r in rows_by_file)))
        for d, rows in zip(files, rows_by_file):
            for r in rows:
                f.write(struct.pack("<III", r["in_len"], r["out_len"], r["crc32"]) + d[r["in_off"]:r["in_off"] + r["in_len"]])
    return rows_by_file


def fnv1a(b):
    h = 0xcbf29ce484222325
    for x in b:
        h = ((h ^ x) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


def test_decoder_under_sanitizers(tmp_path):
    spec = importlib.util.spec_from_file_location("pa_inflate_build", str(helpers.ROOT / "tests" / "inflate" / "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    exe = mod.build_check()
    valid, corrupt = bc.valid_cases(), bc.corrupt_cases()
    files = [d for _, d, _ in valid] + [d for _, d, _, _ in corrupt]
    rows_by_file = case_file(tmp_path / "cases.bin", files)
    out = subprocess.run([str(exe), str(tmp_path / "cases.bin")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stderr == "", (out.returncode, out.stderr[-3000:])   # the sanitizers stay silent
    lines = [l.split() for l in out.stdout.splitlines()]
    assert len(lines) == sum(len(r) for r in rows_by_file)
    at = 0
    for k, rows in enumerate(rows_by_file):
        got = lines[at:at + len(rows)]
        at += len(rows)
        if k < len(valid):
            name, _, text = valid[k]
            for r, (st, crc, h) in zip(rows, got):
                piece = text[r["out_off"]:r["out_off"] + r["out_len"]]
                assert int(st) == 0 and int(crc, 16) == r["crc32"] == zlib.crc32(piece) and int(h, 16) == fnv1a(piece), (name, r, st, crc)
        else:
            name, _, bad, texts = corrupt[k - len(valid)]
            for i, (r, (st, crc, h)) in enumerate(zip(rows, got)):
                if i == bad:
                    assert int(st) != 0, name
                else:
                    assert int(st) == 0 and int(crc, 16) == r["crc32"], (name, i, st)
    statuses = {corrupt[k][0]: int(lines[sum(len(r) for r in rows_by_file[:len(valid) + k]) + 1][0]) for k in range(len(corrupt))}
    names = helpers.pa._ffi.INFLATE_STATUS_NAMES
    assert {k: names[v] for k, v in statuses.items()} == bc.EXPECTED_STATUS   # the codes are distinct and say what is wrong
