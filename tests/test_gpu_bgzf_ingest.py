"""`-m gpu`: pa_process_reads / pa_process_reads_multi on BGZF input. The members' compressed bytes cross the link, the text first exists
in HBM (csrc/inflate.hip on the copy stream), and the output is byte for byte what the plain-text file gives, whatever the window size, the
number of lanes and wherever the member boundaries fall. Reads are made as tests/test_gpu_ingest.py makes them (its two helpers copied)."""
import numpy as np
import pytest

import bgzf_cases as bc
import helpers

pa = helpers.pa
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def aligner(small_index):
    if pa.lib().pa_device_count() < 1:
        raise RuntimeError("the gpu tier needs a GPU and the HIP library: %s" % pa.lib().pa_last_error().decode())
    return pa.Pseudoaligner(small_index(24), 0)


def expected_lines(a, ids, seqs):
    res, coff, cids, _ = helpers.Oracle(a.host).map_reads(seqs, 2, 8)
    want = []
    for i, rid in enumerate(ids):
        cl = cids[int(coff[i]):int(coff[i + 1])].tolist()
        flag = bool(res["mapped"][i]) and res["coverage"][i] >= 32 and not cl
        want.append('(%s, "%s", [%s], %d)' % ("true" if flag else "false", rid, ", ".join(map(str, cl)), res["coverage"][i] if res["mapped"][i] else 0))
    return want


def make_reads(n, seed, lo=1, hi=181):
    ids, seqs = helpers.read_fastq()
    rng = np.random.default_rng(seed)
    pick = rng.integers(0, len(seqs), n)
    out_ids, out_seqs = [], []
    for j, i in enumerate(pick):
        s = seqs[i] + seqs[(i + 1) % len(seqs)] + seqs[(i + 2) % len(seqs)]
        out_seqs.append(s[: int(rng.integers(lo, hi))])
        out_ids.append("%s/%d" % (ids[i], j))
    return out_ids, out_seqs


def fastq_text(ids, seqs, eol="\n", tail=""):
    return ("".join("@%s some description%s%s%s+%s%s%s" % (i, eol, s, eol, eol, "I" * len(s), eol) for i, s in zip(ids, seqs)) + tail).encode()


def run(aligner, path, out, lanes=0, threads=4):
    if lanes == 0:
        n, flagged = pa.process_reads(str(path), aligner, str(out), threads)
    else:
        n, flagged = pa.process_reads_multi(str(path), [aligner] * lanes, str(out), threads)
    return n, flagged, out.read_bytes(), pa.process_reads_input_stats()


@pytest.fixture(scope="module")
def reads20k(aligner):
    ids, seqs = make_reads(20000, 3)
    return ids, seqs, expected_lines(aligner, ids, seqs), fastq_text(ids, seqs)


@pytest.mark.parametrize("window", [700, 65536, 200000])
def test_windows_and_lanes(aligner, reads20k, tmp_path, monkeypatch, window):
    ids, seqs, want, text = reads20k
    plain, gz = tmp_path / "r.fq", tmp_path / "r.fq.gz"
    plain.write_bytes(text)
    gz.write_bytes(bc.bgzf(text))
    monkeypatch.setenv("PA_INGEST_WINDOW", str(window))
    n, flagged, ref, st = run(aligner, plain, tmp_path / "p.txt")
    assert n == len(ids) and st["text_kind"] == 0 and ref.decode().splitlines() == want
    for lanes in (1, 2, 3):
        n2, f2, got, st = run(aligner, gz, tmp_path / ("o%d.txt" % lanes), lanes)
        assert (n2, f2) == (n, flagged) and got == ref, (window, lanes)
        assert st["text_kind"] == 2 and st["members_total"] == len(bc.walk(gz.read_bytes())) and st["members_gpu"] > 0, st
        assert st["bytes_h2d"] < st["text_bytes_gpu"], st


def test_default_window_keeps_the_text_off_the_host(aligner, tmp_path, monkeypatch):
    monkeypatch.delenv("PA_INGEST_WINDOW", raising=False)
    ids, seqs = make_reads(60000, 7)
    ids[31000] = "L" * 5000
    text = fastq_text(ids, seqs)
    plain, gz = tmp_path / "r.fq", tmp_path / "r.fq.gz"
    plain.write_bytes(text)
    gz.write_bytes(bc.bgzf(text))
    n, flagged, ref, _ = run(aligner, plain, tmp_path / "p.txt")
    n2, f2, got, st = run(aligner, gz, tmp_path / "o.txt")
    assert n == n2 == len(ids) and flagged == f2 and got == ref
    print("input stats:", st)
    assert st["text_kind"] == 2 and st["members_total"] > 200
    assert st["members_host"] * 8 <= st["members_total"], st


def test_switch_forces_the_host_path(aligner, reads20k, tmp_path, monkeypatch):
    ids, seqs, want, text = reads20k
    gz = tmp_path / "r.fq.gz"
    gz.write_bytes(bc.bgzf(text))
    monkeypatch.setenv("PA_INGEST_BGZF", "0")
    n, _, got, st = run(aligner, gz, tmp_path / "o.txt")
    assert st["text_kind"] == 1 and st["members_gpu"] == 0 and n == len(ids) and got.decode().splitlines() == want


@pytest.mark.parametrize("shape", ["crlf", "wrapped", "trailing blank lines", "no final line break"])
def test_shapes_the_host_handles(aligner, tmp_path, monkeypatch, shape):
    monkeypatch.setenv("PA_INGEST_WINDOW", "100000")
    ids, seqs = make_reads(6000, 11, 30, 181)
    if shape == "crlf":
        text = fastq_text(ids, seqs, "\r\n")
    elif shape == "wrapped":
        text = "".join("@%s d\n%s\n%s\n+\n%s\n%s\n" % (i, s[:len(s) // 2], s[len(s) // 2:], "I" * (len(s) // 2), "I" * (len(s) - len(s) // 2))
                       if j >= 3000 and len(s) > 1 else "@%s d\n%s\n+\n%s\n" % (i, s, "I" * len(s)) for j, (i, s) in enumerate(zip(ids, seqs))).encode()
    elif shape == "trailing blank lines":
        text = fastq_text(ids, seqs, "\n", "\n\n\n")
    else:
        text = fastq_text(ids, seqs)[:-1]
    plain, gz = tmp_path / "r.fq", tmp_path / "r.fq.gz"
    plain.write_bytes(text)
    gz.write_bytes(bc.bgzf(text, 30000))
    n, flagged, ref, _ = run(aligner, plain, tmp_path / "p.txt")
    n2, f2, got, st = run(aligner, gz, tmp_path / "o.txt", 2)
    assert n == n2 == len(ids) and flagged == f2 and got == ref and st["text_kind"] == 2


def test_corrupt_member_is_an_error_and_the_next_call_works(aligner, reads20k, tmp_path, monkeypatch):
    ids, seqs, want, text = reads20k
    monkeypatch.setenv("PA_INGEST_WINDOW", "200000")
    good = bc.bgzf(text, 20000)
    rows = bc.walk(good)
    r = rows[len(rows) // 2]
    bad = bytearray(good)
    bad[r["in_off"] + r["in_len"] // 2] ^= 0x10
    ok, _ = bc.zlib_verdict(bytes(bad[r["in_off"]:r["in_off"] + r["in_len"]]), r["out_len"], r["crc32"])
    assert not ok
    (tmp_path / "bad.fq.gz").write_bytes(bytes(bad))
    (tmp_path / "good.fq.gz").write_bytes(good)
    with pytest.raises(pa.PaError) as e:
        pa.process_reads(str(tmp_path / "bad.fq.gz"), aligner, str(tmp_path / "b.txt"), 4)
    assert e.value.code == pa._ffi.PA_ERR_FORMAT and "corrupt gzip stream" in str(e.value) and "byte %d:" % r["file_off"] in str(e.value), str(e.value)
    n, _, got, st = run(aligner, tmp_path / "good.fq.gz", tmp_path / "g.txt")
    assert n == len(ids) and got.decode().splitlines() == want and st["text_kind"] == 2


def test_member_boundaries_in_every_kind_of_line(aligner, tmp_path, monkeypatch):
    """members cut by hand: exactly at a record start, one byte behind it, inside the id, on the header's line break, inside the sequence, on the '+', inside
    the qualities, on the record's last line break — and a window that holds a few members only"""
    monkeypatch.setenv("PA_INGEST_WINDOW", "65536")
    ids, seqs = make_reads(3000, 13, 60, 181)
    text = fastq_text(ids, seqs)
    starts = [0]
    for i, s in zip(ids, seqs):
        starts.append(starts[-1] + len("@%s some description\n" % i) + 2 * len(s) + 4)
    assert starts[-1] == len(text)
    cuts = []
    for k, rec in enumerate(range(40, 2900, 40)):
        a, hdr, ls = starts[rec], len("@%s some description" % ids[rec]), len(seqs[rec])
        cuts.append(a + [0, 1, 5, hdr, hdr + 1, hdr + 1 + ls // 2, hdr + 1 + ls, hdr + 2 + ls, hdr + 3 + ls, hdr + 4 + ls + ls // 2, hdr + 4 + 2 * ls][k % 11])
    cuts = sorted(set(cuts))
    chunks = [text[a:b] for a, b in zip([0] + cuts, cuts + [len(text)])]
    assert max(map(len, chunks)) <= 65280
    plain, gz = tmp_path / "r.fq", tmp_path / "r.fq.gz"
    plain.write_bytes(text)
    gz.write_bytes(bc.bgzf_chunks(chunks))
    n, flagged, ref, _ = run(aligner, plain, tmp_path / "p.txt")
    for lanes in (1, 3):
        n2, f2, got, st = run(aligner, gz, tmp_path / ("o%d.txt" % lanes), lanes)
        assert n == n2 == len(ids) and flagged == f2 and got == ref and st["text_kind"] == 2 and st["members_gpu"] > 0
