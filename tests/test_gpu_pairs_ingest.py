"""The paired drivers on their device path (csrc/window_feed.cpp, csrc/pair_scan.hip: windows of both files to HBM, records found, ids
compared and R2 / the R1 prefix gathered on the GPU) against the SAME call on the host path (PA_PAIRS_HOST_SCAN=1): output files byte for
byte, the count table, the stats and the number of pairs. The device path is the default for two BGZF files; a plain file takes it on request
(PA_PAIRS_DEVICE_PLAIN=1), which the cases with plain files make. The cases come from the existing builders (cells_model, bus_model, pairs_cases);
BGZF files are written with Python's zlib (tests/bgzf_cases.py)."""
import gzip

import numpy as np
import pytest

import bgzf_cases as bc
import bus_model as bm
import cells_model as cm
import helpers
import pairs_cases

pa = helpers.pa
pytestmark = pytest.mark.gpu

BC, UMI = 16, 12
_cache = {}


def _gencode():
    if "gencode" not in _cache:
        host = pa.build_index(str(helpers.FASTA), 24, 8)
        tx_gene, names = host.genes()
        _, seqs = helpers.read_fasta()
        _cache["gencode"] = (host, pa.Pseudoaligner(host), np.asarray(tx_gene, np.uint32), seqs)
    return _cache["gencode"]


def _reads(kind, n):
    """-> (R1 strings, R2 strings, whitelist or None) of `kind`'s own case builder, the first n pairs"""
    key = (kind, n)
    if key not in _cache:
        host, al, tx_gene, seqs = _gencode()
        if kind == "cells":
            case = cm.make_case(71, seqs, tx_gene, BC, UMI, n_cells=120)
            _cache[key] = (case["r1"][:n], case["r2"][:n], case["whitelist"])
        elif kind == "bus":
            case = bm.make_case(72, seqs, BC, UMI, n_pairs=n)
            _cache[key] = (case["r1"][:n], case["r2"][:n], None)
        else:
            _, r1, r2, _ = pairs_cases.case("gencode_k20_fr")
            _cache[key] = (r1[:n], r2[:n], None)
        assert len(_cache[key][0]) >= 1000
    return _cache[key]


def _pairs_aligner():
    if "pairs_al" not in _cache:
        host, _, _, _ = pairs_cases.case("gencode_k20_fr")
        _cache["pairs_al"] = (host, pa.Pseudoaligner(host))
    return _cache["pairs_al"]


def fastq(ids, seqs, eol="\n", wrap=0, final_eol=True, trailing=""):
    """wrap > 0: sequence and quality lines cut into pieces of `wrap` bytes (a multi-line record)"""
    def lines(s):
        return eol.join(s[i:i + wrap] for i in range(0, len(s), wrap)) if wrap and s else s
    text = "".join("@%s extra words%s%s%s+%s%s%s" % (i, eol, lines(s), eol, eol, lines("I" * len(s)), eol) for i, s in zip(ids, seqs))
    if not final_eol:
        text = text[:-len(eol)]
    return (text + trailing).encode()


def write(tmp_path, name, text, form, chunk=4000):
    p = tmp_path / (name + {"plain": "", "bgzf": ".gz", "gzip": ".gz"}[form])
    p.write_bytes(text if form == "plain" else bc.bgzf(text, chunk) if form == "bgzf" else gzip.compress(text, 1))
    return p


def run(kind, p1, p2, tmp_path, tag, whitelist=None):
    """one call of the driver -> everything it answers, comparable with =="""
    out = tmp_path / ("out_" + tag)
    out.mkdir(exist_ok=True)
    if kind == "cells":
        host, al, _, _ = _gencode()
        wl = tmp_path / "wl.txt"
        wl.write_text("\n".join(whitelist) + "\n")
        st = al.count_cells(host, p1, p2, wl, out, BC, UMI, num_threads=4)
        files = [(out / f).read_bytes() for f in ("matrix.mtx", "barcodes.tsv", "features.tsv")]
    elif kind == "bus":
        host, al, _, _ = _gencode()
        st = al.write_bus(host, p1, p2, out, BC, UMI, num_threads=4)
        files = [(out / f).read_bytes() for f in ("output.bus", "matrix.ec", "transcripts.txt")]
    else:
        host, al = _pairs_aligner()
        counts, st = al.count_pairs(str(p1), str(p2), "un" if kind == "un" else "fr")
        files = [counts.tobytes()]
    n_pairs = int(list(pa.process_reads_stage_seconds().values())[7])
    return st, files, n_pairs, pa.pairs_input_stats()


def both(kind, p1, p2, tmp_path, monkeypatch, whitelist=None, device_expected=True, request_plain=True):
    """the call on the host path and on the device path (request_plain: plain files are asked to take it too): equal answers; -> the second
    call's input stats"""
    monkeypatch.setenv("PA_PAIRS_HOST_SCAN", "1")
    h_st, h_files, h_n, h_in = run(kind, p1, p2, tmp_path, "host", whitelist)
    assert not h_in["device_path"]
    monkeypatch.delenv("PA_PAIRS_HOST_SCAN")
    if request_plain:
        monkeypatch.setenv("PA_PAIRS_DEVICE_PLAIN", "1")
    else:
        monkeypatch.delenv("PA_PAIRS_DEVICE_PLAIN", raising=False)
    d_st, d_files, d_n, d_in = run(kind, p1, p2, tmp_path, "dev", whitelist)
    assert d_in["device_path"] == device_expected
    assert d_st == h_st and d_n == h_n and h_n > 0
    for k, (a, b) in enumerate(zip(d_files, h_files)):
        assert a == b, "output %d differs between the device path and the host path" % k
    return d_in


MIXES = {"plain_plain": ("plain", "plain"), "bgzf_bgzf": ("bgzf", "bgzf"), "plain_bgzf": ("plain", "bgzf")}


@pytest.mark.parametrize("window", ["700", "65536", None])
@pytest.mark.parametrize("mix", list(MIXES))
@pytest.mark.parametrize("kind", ["cells", "bus", "pairs"])
def test_windows(kind, mix, window, tmp_path, monkeypatch):
    """small windows: many segments per batch, a head at every window, R1 and R2 windows that end at different pairs"""
    n = 2000 if window == "700" else 6000
    r1, r2, wl = _reads(kind, n)
    ids = ["pair%d" % i for i in range(len(r1))]
    f1, f2 = MIXES[mix]
    p1 = write(tmp_path, "R1.fq", fastq([i + "/1" for i in ids], r1), f1)
    p2 = write(tmp_path, "R2.fq", fastq([i + "/2" for i in ids], r2), f2)
    if window:
        monkeypatch.setenv("PA_INGEST_WINDOW", window)
    stats = both(kind, p1, p2, tmp_path, monkeypatch, wl)
    assert stats["r1"]["text_kind"] == (2 if f1 == "bgzf" else 0) and stats["r2"]["text_kind"] == (2 if f2 == "bgzf" else 0)
    # (with the default window these files are shorter than the part of a text that the host keeps for itself: no member reaches the GPU's inflate)
    assert stats["r2"]["bytes_h2d"] > 0 and (f2 != "bgzf" or window is None or stats["r2"]["members_gpu"] > 0)


@pytest.mark.parametrize("kind", ["cells", "bus", "pairs", "un"])   # ("un": four streams, the gathered bytes consumed on two of them)
def test_batch_seam_inside_small_windows(kind, tmp_path, monkeypatch):
    r1, r2, wl = _reads(kind, 2000)
    ids = ["p%d" % i for i in range(len(r1))]
    p1 = write(tmp_path, "R1.fq", fastq(ids, r1), "plain")
    p2 = write(tmp_path, "R2.fq", fastq(ids, r2), "plain")
    monkeypatch.setenv("PA_INGEST_BATCH", "333")
    monkeypatch.setenv("PA_INGEST_WINDOW", "700")
    both(kind, p1, p2, tmp_path, monkeypatch, wl)


SHAPES = {"crlf": (dict(eol="\r\n"), dict(eol="\r\n")), "no_final_line_break": (dict(final_eol=False), dict(final_eol=False)),
          "trailing_blank_lines": (dict(trailing="\n\n\n"), dict(trailing="\n")), "wrapped_r2": (dict(), dict(wrap=37)),
          "wrapped_both": (dict(wrap=11), dict(wrap=60))}


@pytest.mark.parametrize("window", ["3000", None])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_shapes(shape, window, tmp_path, monkeypatch):
    r1, r2, _ = _reads("bus", 2000)
    ids = ["s%d" % i for i in range(len(r1))]
    k1, k2 = SHAPES[shape]
    p1 = write(tmp_path, "R1.fq", fastq([i + "/1" for i in ids], r1, **k1), "plain")
    p2 = write(tmp_path, "R2.fq", fastq([i + "/2" for i in ids], r2, **k2), "plain")
    if window:
        monkeypatch.setenv("PA_INGEST_WINDOW", window)
    both("bus", p1, p2, tmp_path, monkeypatch)


def _error(kind, p1, p2, tmp_path, monkeypatch, host):
    if host:
        monkeypatch.setenv("PA_PAIRS_HOST_SCAN", "1")
    else:
        monkeypatch.delenv("PA_PAIRS_HOST_SCAN", raising=False)
        monkeypatch.setenv("PA_PAIRS_DEVICE_PLAIN", "1")
    with pytest.raises(pa.PaError) as e:
        run(kind, p1, p2, tmp_path, "err")
    return e.value


def test_errors_are_the_host_path_errors(tmp_path, monkeypatch):
    _, r1, r2, _ = pairs_cases.case("gencode_k20_fr")
    r1, r2 = r1[:200], r2[:200]
    ids = ["pair%d" % i for i in range(200)]
    monkeypatch.setenv("PA_INGEST_BATCH", "64")
    monkeypatch.setenv("PA_INGEST_WINDOW", "700")
    p1 = write(tmp_path, "R1.fq", fastq([i + "/1" for i in ids], r1), "plain")
    renamed = [i + "/2" if k != 137 else "pair731/2" for k, i in enumerate(ids)]
    p2 = write(tmp_path, "R2.fq", fastq(renamed, r2), "plain")
    for kind in ("pairs", "bus"):
        e, h = _error(kind, p1, p2, tmp_path, monkeypatch, False), _error(kind, p1, p2, tmp_path, monkeypatch, True)
        assert e.code == pa._ffi.PA_ERR_FORMAT and "record 137:" in str(e) and str(e) == str(h)
    p2 = write(tmp_path, "R2.fq", fastq([i + "/2" for i in ids[:150]], r2[:150]), "plain")
    e, h = _error("pairs", p1, p2, tmp_path, monkeypatch, False), _error("pairs", p1, p2, tmp_path, monkeypatch, True)
    assert e.code == pa._ffi.PA_ERR_FORMAT and "record 150 has no mate" in str(e) and str(e) == str(h)
    # ... and the other way round: R1 is the shorter file
    e, h = _error("pairs", p2, p1, tmp_path, monkeypatch, False), _error("pairs", p2, p1, tmp_path, monkeypatch, True)
    assert "record 150 has no mate" in str(e) and str(e) == str(h)


def test_a_corrupt_bgzf_member_is_named_and_the_next_call_works(tmp_path, monkeypatch):
    r1, r2, _ = _reads("bus", 2000)
    ids = ["c%d" % i for i in range(len(r1))]
    p1 = write(tmp_path, "R1.fq", fastq(ids, r1), "bgzf")
    good = bc.bgzf(fastq(ids, r2), 4000)
    rows = bc.walk(good)
    k = 5
    at = rows[k]["in_off"] + rows[k]["in_len"] // 2            # a byte in the middle of member 5's payload
    bad = bytearray(good)
    bad[at] ^= 0x55
    p2 = tmp_path / "R2.fq.gz"
    p2.write_bytes(bytes(bad))
    monkeypatch.delenv("PA_PAIRS_HOST_SCAN", raising=False)
    with pytest.raises(pa.PaError) as e:
        run("bus", p1, p2, tmp_path, "bad")
    assert e.value.code == pa._ffi.PA_ERR_FORMAT and "corrupt gzip stream: member at byte %d:" % rows[k]["file_off"] in str(e.value)
    p2.write_bytes(good)
    both("bus", p1, p2, tmp_path, monkeypatch)


@pytest.mark.parametrize("mix", list(MIXES))
def test_which_input_takes_which_path_by_default(mix, tmp_path, monkeypatch):
    """without PA_PAIRS_DEVICE_PLAIN: two BGZF files take the device path, a plain file on either side keeps the host path"""
    r1, r2, _ = _reads("bus", 2000)
    ids = ["d%d" % i for i in range(len(r1))]
    f1, f2 = MIXES[mix]
    p1 = write(tmp_path, "R1.fq", fastq(ids, r1), f1)
    p2 = write(tmp_path, "R2.fq", fastq(ids, r2), f2)
    monkeypatch.setenv("PA_INGEST_WINDOW", "65536")
    both("bus", p1, p2, tmp_path, monkeypatch, device_expected=mix == "bgzf_bgzf", request_plain=False)


def test_ordinary_gzip_on_one_side_takes_the_host_path(tmp_path, monkeypatch):
    r1, r2, _ = _reads("bus", 2000)
    ids = ["g%d" % i for i in range(len(r1))]
    p1 = write(tmp_path, "R1.fq", fastq(ids, r1), "bgzf")
    p2 = write(tmp_path, "R2.fq", fastq(ids, r2), "gzip")
    stats = both("bus", p1, p2, tmp_path, monkeypatch, device_expected=False)
    assert stats["r1"]["text_kind"] == 1 and stats["r2"]["text_kind"] == 1 and stats["r1"]["members_gpu"] == 0
    # the same pairs, both files BGZF: the same output on the device path
    want = run("bus", p1, p2, tmp_path, "gz")
    p2b = tmp_path / "R2b.fq.gz"
    p2b.write_bytes(bc.bgzf(fastq(ids, r2), 4000))
    got = run("bus", p1, p2b, tmp_path, "bgzf")
    assert got[3]["device_path"] and got[:3] == want[:3]


def test_the_host_stays_off_the_text(tmp_path, monkeypatch):
    """120 000 pairs (28-base R1, 90-base R2) as BGZF with 65 280-byte members, the default window, through write_bus: both files are inflated on
    the GPU, fewer bytes cross the link than the text has, and the host inflates at most a quarter of the members (its part is the tail of each file:
    the last KEEP bytes and the members they start in)"""
    host, al, tx_gene, seqs = _gencode()
    rng = np.random.default_rng(5)
    n = 120000
    long_tx = [s for s in seqs if len(s) >= 200]
    cells = ["".join("ACGT"[x] for x in rng.integers(0, 4, BC)) for _ in range(150)]
    umis = rng.integers(0, 4, (n, UMI))
    which, start = rng.integers(0, len(long_tx), n), rng.integers(0, 100, n)
    r1 = [cells[int(c)] + "".join("ACGT"[x] for x in u) for c, u in zip(rng.integers(0, 150, n), umis)]
    r2 = [long_tx[int(t)][int(a):int(a) + 90] for t, a in zip(which, start)]
    ids = ["read%d" % i for i in range(n)]
    p1 = write(tmp_path, "R1.fq", fastq([i + "/1" for i in ids], r1), "bgzf", 65280)
    p2 = write(tmp_path, "R2.fq", fastq([i + "/2" for i in ids], r2), "bgzf", 65280)
    stats = both("bus", p1, p2, tmp_path, monkeypatch, request_plain=False)   # (two BGZF files: the device path without being asked)
    for side in ("r1", "r2"):
        s = stats[side]
        assert s["text_kind"] == 2 and s["members_gpu"] > 0 and s["bytes_h2d"] < s["text_bytes_gpu"] and s["members_host"] * 4 <= s["members_total"], (side, s)
