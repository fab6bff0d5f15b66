"""The BUS writer (pa_bus, csrc/bus.hip) at the edges its code has branches and arithmetic for, with no aligner in the loop: the tests write
the mapping's records and arenas themselves (bus_model.directed), so every (barcode, UMI, class, reads) is chosen exactly. Every case
equals the pure-Python model in the records, the ec table and all eight stats, and first shows on the model's side alone that it
reaches the path it is named for. All integers: equality, no tolerance."""
import ctypes as C

import numpy as np
import pytest

import bus_model as bm
import helpers

pa = helpers.pa
pytestmark = pytest.mark.gpu

_cache = {}


def _setup():
    """the gencode_small index at K = 24 on the GPU: (host index, aligner, HostIndex.arrays(), index classes)"""
    if "ix" not in _cache:
        host = pa.build_index(str(helpers.FASTA), 24, 8)
        ix = host.arrays()
        _cache["ix"] = (host, pa.Pseudoaligner(host), ix, bm.index_classes(ix))
        assert bm.RESULT_DTYPE == pa.RESULT_DTYPE and bm.CLASS_REF == pa.PA_CLASS_REF and bm.MAPPED_BIT == pa.PA_MAPPED_BIT
        assert bm.RECORD_DTYPE == pa.BUS_RECORD_DTYPE and bm.STAT_NAMES == pa._ffi.BUS_STAT_NAMES
    return _cache["ix"]


def _feed(writer, r1, records, arena, arena_len=None):
    """one batch: the records, the arena and the R1 text uploaded as they are (8 bytes of padding behind the text)"""
    import torch
    if len(r1) == 0:
        writer.add_device(0, 0, 0, 0, 0, 0)
        return
    text, off = pa.concat_reads(r1)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()
    d = [up(records), up(arena), up(np.concatenate([text, np.zeros(8, np.uint8)])), up(off)]
    torch.cuda.synchronize()
    writer.add_device(d[0].data_ptr(), d[1].data_ptr(), len(arena) if arena_len is None else arena_len, d[2].data_ptr(), d[3].data_ptr(), len(r1))


def _result(writer):
    records = bm.records_from_array(writer.records())
    table = bm.table_from_csr(*writer.ecs())
    st = writer.stats()
    assert writer.finish() == (len(records), len(table)) and st["records"] == len(records)
    return records, table, st


def _gpu(batches, bc_len, umi_len):
    """a fresh writer fed the batches [(r1, records, arena)] -> (records, ec table, stats)"""
    host, al, _, _ = _setup()
    writer = pa.BusWriter(al, host, bc_len, umi_len)
    for r1, records, arena in batches:
        _feed(writer, r1, records, arena)
    return _result(writer)


def _model(r1, mapping, bc_len, umi_len):
    _, _, ix, classes = _setup()
    records, table, st, fates = bm.model(r1, mapping, int(ix["num_transcripts"]), classes, bc_len, umi_len)
    return (records, table, st), fates


def _check(reads, bc_len, umi_len, seed=0, shuffle=True):
    r1, records, arena, mapping = bm.directed(reads, _setup()[2], seed, shuffle)
    want, fates = _model(r1, mapping, bc_len, umi_len)
    got = _gpu([(r1, records, arena)], bc_len, umi_len)
    assert got[2] == want[2]
    assert got[0] == want[0]
    assert got[1] == want[1]
    return want, fates


def _novel(k, length=2):
    """the k-th list of `length` ids that is no index class"""
    _, _, ix, classes = _setup()
    have, T = set(classes), int(ix["num_transcripts"])
    out = []
    a = 0
    while len(out) <= k:
        cand = tuple(range(a, a + 2 * length, 2))
        assert cand[-1] < T
        if cand not in have:
            out.append(cand)
        a += 1
    return list(out[k])


# ---- widths and key values ----
def test_all_ones_key_is_counted():
    """bc_len + umi_len = 32 with an all-T barcode and UMI: 64 one bits in the key's high word, beside reads that drop"""
    _, _, ix, classes = _setup()
    (c1, t1), = bm.singleton_classes(ix)[:1]
    cm, ids_m, j = bm.multi_classes(ix)[0]
    nov = _novel(0, 3)
    T16 = "T" * 16
    reads = [(T16 + T16, c1, 3), (T16 + T16, cm, 2), (T16 + T16, nov, 4), (T16 + T16, None, 5), (T16 + "T" * 15 + "N", c1, 2), ("T" * 31, c1, 1),
             ("A" * 32, c1, 1), (T16 + "T" * 15 + "G", ("fresh", nov), 1)]
    want, _ = _check(reads, 16, 16)
    T, M = int(ix["num_transcripts"]), len(bm.multi_classes(ix))
    ones = (1 << 32) - 1
    assert want[0][-3:] == [(ones, ones, t1, 3), (ones, ones, T + j, 2), (ones, ones, T + M, 4)] and want[0][0] == (0, 0, t1, 1)
    assert want[2]["unmapped"] == 5 and want[2]["umi_n"] == 2 and want[2]["r1_short"] == 1
    # the same at 31 + 1 and 1 + 31 bases: barcode and UMI split the 64 bits elsewhere
    for bc in (31, 1):
        w, _ = _check(reads[:4] + reads[6:7], bc, 32 - bc)
        assert w[0][-1][:2] == ((1 << 2 * bc) - 1, (1 << 2 * (32 - bc)) - 1)


def test_one_base_each():
    _, _, ix, _ = _setup()
    (c0, t0), (c1, t1) = bm.singleton_classes(ix)[:2]
    reads = [(b + u, c, 1 + (i % 3)) for i, (b, u, c) in enumerate((b, u, c) for b in "ACGT" for u in "ACGT" for c in (c0, c1))]
    reads += [("A", c0, 1), ("", c0, 1), ("NA", c0, 1), ("AN", c0, 1), ("TTACGT", c1, 1)]
    want, _ = _check(reads, 1, 1)
    assert len(want[0]) == 32 and want[0][0][:2] == (0, 0) and want[0][-1][:2] == (3, 3) and want[2]["r1_short"] == 2
    assert sum(n for _, _, _, n in want[0]) == want[2]["recorded"]


# ---- the R1 text ----
def test_r1_fates():
    _, _, ix, _ = _setup()
    (c0, t0), = bm.singleton_classes(ix)[:1]
    reads = [("ACGTAGGA", c0, 1),            # exactly bc_len + umi_len bytes
             ("ACGTAGG", c0, 1),             # one byte shorter
             ("", c0, 1),
             ("NCGTAGGA", c0, 1), ("ACGTNGGA", c0, 1),     # N at the first and at the last base of the barcode
             ("ACGTANGA", c0, 1), ("ACGTAGGN", c0, 1),     # ... of the UMI
             ("NCGTAGGN", c0, 1),                          # both: the barcode's rule comes first
             ("aCGTAGGA", c0, 1), ("ACGTAGGa", c0, 1), ("acgtagga", c0, 1),   # lower case is no base
             ("NCGTAGGA", None, 1), ("ACGTAGGN", None, 1),   # an N comes before "unmapped"
             ("ACGTAGG", None, 1),
             ("ACGTAGGATTTTNNNN", c0, 2),    # (longer: the tail is not read)
             ("ACGTAGGA", c0, 1)]
    r1, records, arena, mapping = bm.directed(reads, ix, shuffle=False)
    assert len(r1[-1]) == 8   # the last record of the buffer is an R1 of exactly bc_len + umi_len bytes
    want, fates = _model(r1, mapping, 5, 3)
    assert fates == ["recorded", "r1_short", "r1_short", "barcode_n", "barcode_n", "umi_n", "umi_n", "barcode_n", "barcode_n", "umi_n", "barcode_n", "barcode_n",
                     "umi_n", "r1_short", "recorded", "recorded", "recorded"]
    assert want[0] == [(bm.pack("ACGTA"), bm.pack("GGA"), t0, 4)]
    assert _gpu([(r1, records, arena)], 5, 3) == want


# ---- what a record can say about its class ----
def test_class_references():
    _, _, ix, classes = _setup()
    T, num_classes = int(ix["num_transcripts"]), int(ix["num_classes"])
    (c0, t0), (c1, t1) = bm.singleton_classes(ix)[:2]
    multi = bm.multi_classes(ix)
    (cm, ids_m, j), (cm2, ids_m2, j2) = multi[0], multi[-1]
    M = len(multi)
    nov = _novel(0)
    bc, umi = "ACGTAC", "GGTT"
    reads = [(bc + umi, None, 2),                              # unmapped
             (bc + umi, ("unmapped", c0), 1), (bc + umi, ("unmapped", list(ids_m)), 1),
             (bc + umi, [], 2),                                # mapped with an empty class
             (bc + umi, c0, 3),                                # a singleton class -> ec t
             (bc + umi, [t0], 2),                              # an arena list of length 1 -> the same record
             (bc + umi, cm, 4),                                # a class of two ids or more -> T + j
             (bc + umi, list(ids_m), 5),                       # an arena list equal by content to that class: merges into its record
             (bc + "GGTA", list(ids_m2), 1),                   # ... alone under its UMI
             (bc + umi, nov, 1),
             (bc + umi, [T - 1], 1), (bc + umi, num_classes - 1, 1),   # (the last transcript, the last class)
             (bc + umi, num_classes, 2),                       # a reference = num_classes
             (bc + umi, 0x7FFFFFFF, 1),
             (bc + umi, [3, T], 1), (bc + umi, [T], 1),        # an id = T
             (bc + umi, [7, 5, 9], 1), (bc + umi, [5, 5], 1)]  # descending; repeated
    want, fates = _check(reads, 6, 4)
    st = want[2]
    assert len(classes[-1]) >= 1
    assert st["unmapped"] == 6 and st["bad_class"] == 7 and st["recorded"] == 3 + 2 + 4 + 5 + 1 + 1 + 1 + 1
    b, u = bm.pack(bc), bm.pack(umi)
    assert (b, u, t0, 5) in want[0] and (b, u, T + j, 9) in want[0] and (b, bm.pack("GGTA"), T + j2, 1) in want[0] and (b, u, T + M, 1) in want[0]
    assert want[1][T + M:] == [tuple(nov)] and len(want[1]) == T + M + 1
    # an arena range that ends one past arena_len: the list's last word is not read; the rest of the batch is unharmed
    r1, records, arena, mapping = bm.directed([(bc + umi, c0, 2), (bc + umi, ("fresh", list(ids_m)), 1), (bc + "AAAA", nov, 1)], ix, shuffle=False)
    last = int(records["class_off"][3])
    assert last + int(records["class_len"][3]) == len(arena) and records["class_len"][3] == 2
    host, al, _, _ = _setup()
    for cut, n_bad in ((0, 0), (1, 1)):
        writer = pa.BusWriter(al, host, 6, 4)
        _feed(writer, r1, records, arena, arena_len=len(arena) - cut)
        m = [x if not (cut and i == 3) else (True, bm.BAD) for i, x in enumerate(mapping)]
        assert _result(writer) == _model(r1, m, 6, 4)[0] and writer.stats()["bad_class"] == n_bad
    # ... and a range that begins past it, in a raw record
    r1, records, arena, mapping = bm.directed([(bc + umi, c0, 2), (bc + umi, ("raw", 0x7FFFFFF0, 4), 1), (bc + umi, ("raw", 1, 0x7FFFFFFF), 1)], ix)
    want = _model(r1, mapping, 6, 4)[0]
    assert want[2]["bad_class"] == 2 and want[0] == [(b, u, t0, 2)]
    assert _gpu([(r1, records, arena)], 6, 4) == want


def test_novel_lists():
    _, _, ix, classes = _setup()
    T, M = int(ix["num_transcripts"]), len(bm.multi_classes(ix))
    # three lists that pin the lexicographic order: {a, b} < {a, b, c} < {a', b'} with a < a'
    lo = _novel(0)
    mid = lo + [lo[-1] + 1]
    k = 1
    while _novel(k)[0] == lo[0]:
        k += 1
    hi = _novel(k)
    assert tuple(mid) not in set(classes) and lo < mid < hi and len(mid) > len(hi)
    bc = "ACGTACGTAC"
    first = bm.directed([(bc + "AAAAAA", ("fresh", hi), 2), (bc + "AAAAAA", ("fresh", hi), 3),      # the same list at two offsets of one batch
                         (bc + "CCCCCC", hi, 1), (bc + "AAAAAA", mid, 1)], ix, seed=1, pad=1)
    later = bm.directed([(bc + "AAAAAA", hi, 4), (bc + "GGGGGG", lo, 1), (bc + "AAAAAA", ("fresh", mid), 1)], ix, seed=2, pad=7)   # other offsets
    offs = lambda case: {int(o) for o, l in zip(case[1]["class_off"], case[1]["class_len"]) if l == len(hi)}
    assert len(offs(first)) == 2 and not offs(first) & offs(later)
    want, _ = _model(first[0] + later[0], first[3] + later[3], 10, 6)
    assert want[1][T + M:] == [tuple(lo), tuple(mid), tuple(hi)]
    b = bm.pack(bc)
    assert want[0] == [(b, 0, T + M + 1, 2), (b, 0, T + M + 2, 9), (b, bm.pack("CCCCCC"), T + M + 2, 1), (b, bm.pack("GGGGGG"), T + M, 1)]
    assert _gpu([first[:3], later[:3]], 10, 6) == want
    assert _gpu([later[:3], first[:3]], 10, 6) == want


# ---- sizes ----
def test_batch_sizes():
    _, _, ix, _ = _setup()
    singles = bm.singleton_classes(ix)[:4]
    rng = np.random.default_rng(3)
    rand = lambda n: "".join(bm.BASES[x] for x in rng.integers(0, 4, n))
    nov = _novel(2)
    zero = dict.fromkeys(bm.STAT_NAMES, 0)
    T, M = int(ix["num_transcripts"]), len(bm.multi_classes(ix))
    base_table = _model([], [], 8, 6)[0][1]
    assert len(base_table) == T + M
    # nothing added; a batch of no reads, null pointers
    assert _gpu([], 8, 6) == ([], base_table, zero)
    assert _gpu([([], None, None)], 8, 6) == ([], base_table, zero)
    for n in (1, 63, 64, 65, 257):
        reads = [(rand(3) + "A" * 5 + rand(2) + "C" * 4, singles[i % 4][0] if i % 5 else nov, 1) for i in range(n)]
        want, _ = _check(reads, 8, 6, seed=n)
        assert want[2]["reads"] == n == want[2]["recorded"]
    # a batch of dropped reads only (one of each fate), then a recording one; and the dropped batch alone
    c0 = singles[0][0]
    dropped = bm.directed([("ACGTACG", c0, 1), ("ACGTACGNACGTAC", c0, 1), ("ACGTACGTACGTAN", c0, 1), ("ACGTACGTACGTAC", None, 1), ("ACGTACGTACGTAC", [9, 3], 1)], ix)
    recording = bm.directed([("ACGTACGTACGTAC", c0, 2), ("TTTTTTTTTTTTTT", nov, 1)], ix)
    want_d, _ = _model(dropped[0], dropped[3], 8, 6)
    assert want_d[0] == [] and want_d[2]["recorded"] == 0 and all(want_d[2][k] == 1 for k in bm.STAT_NAMES[1:6])
    assert _gpu([dropped[:3]], 8, 6) == want_d
    want, _ = _model(dropped[0] + recording[0], dropped[3] + recording[3], 8, 6)
    assert _gpu([dropped[:3], recording[:3]], 8, 6) == want and len(want[0]) == 2


def test_seventy_thousand_identical_reads():
    """one record whose count crosses blocks and 16 bits, beside a neighbour that differs in the ec alone"""
    _, _, ix, _ = _setup()
    (c0, t0), (c1, t1) = bm.singleton_classes(ix)[:2]
    want, _ = _check([("GATTACAGATTACAGATTACAGATTACA", c0, 70000), ("GATTACAGATTACAGATTACAGATTACA", c1, 3)], 16, 12)
    b, u = bm.pack("GATTACAGATTACAGA"), bm.pack("TTACAGATTACA")
    assert sorted(want[0]) == sorted([(b, u, t0, 70000), (b, u, t1, 3)])


@pytest.mark.parametrize("n", [255, 256, 257])
def test_distinct_records(n):
    _, _, ix, _ = _setup()
    singles = bm.singleton_classes(ix)
    reads = [("ACGT" + bm.BASES[i % 4] + bm.BASES[(i // 4) % 4] + "ACG" + bm.BASES[(i // 16) % 4], singles[(i // 64) % 5][0], 1 + (i % 2)) for i in range(n)]
    want, _ = _check(reads, 6, 4, seed=n)
    assert len(want[0]) == n


def test_twelve_growing_batches_equal_one():
    _, _, ix, _ = _setup()
    singles = bm.singleton_classes(ix)[:3]
    multi = bm.multi_classes(ix)[:2]
    novs = [_novel(k) for k in range(4)]
    rng = np.random.default_rng(21)
    sizes = [1, 2, 3, 10, 12, 40, 45, 150, 160, 500, 520, 1600]
    batches, carry = [], []
    for jb, size in enumerate(sizes):
        fresh = {("".join(bm.BASES[x] for x in rng.integers(0, 4, 5)), int(rng.integers(5)), int(rng.integers(9))) for _ in range(size)}
        mols = sorted(fresh | set(carry))
        reads = []
        for umi, cell, g in mols:
            # a class by reference, the same class as a list (at an offset of this batch), a novel list
            cls = singles[g][0] if g < 3 else multi[g - 3][0] if g < 5 and jb % 2 else list(multi[g - 3][1]) if g < 5 else novs[g - 5]
            reads.append(("ACG" + bm.BASES[cell % 4] + umi, cls, 1))
        batches.append(bm.directed(reads, ix, seed=jb, pad=1 + jb))
        carry = mols[: len(mols) // 3]   # a record comes again in the batch after its own
    all_r1, all_map = sum((b[0] for b in batches), []), sum((b[3] for b in batches), [])
    want, _ = _model(all_r1, all_map, 4, 5)
    assert len(want[1]) == len(_model([], [], 4, 5)[0][1]) + 4 and max(n for _, _, _, n in want[0]) >= 2
    assert _gpu([b[:3] for b in batches], 4, 5) == want
    # one batch: the twelve arenas back to back, every offset moved
    shift, recs = 0, []
    for b in batches:
        r = b[1].copy()
        in_arena = (r["class_off"] & bm.CLASS_REF) == 0
        r["class_off"][in_arena] += shift
        recs.append(r)
        shift += len(b[2])
    assert _gpu([(all_r1, np.concatenate(recs), np.concatenate([b[2] for b in batches]))], 4, 5) == want


# ---- protocol ----
def test_protocol():
    host, al, ix, _ = _setup()
    L = pa.lib()
    (c0, t0), = bm.singleton_classes(ix)[:1]
    nov = _novel(1)
    r1, records, arena, mapping = bm.directed([("ACGTACGT", c0, 2), ("ACGTACGA", nov, 1)], ix)
    want, _ = _model(r1, mapping, 4, 4)
    writer = pa.BusWriter(al, host, 4, 4)
    _feed(writer, r1, records, arena)
    assert writer.finish() == writer.finish() == (2, len(want[1]))
    with pytest.raises(pa.PaError) as e:
        _feed(writer, r1, records, arena)
    assert e.value.code == pa._ffi.PA_ERR_INVALID_ARG
    assert _result(writer) == want   # the refused batch left no trace
    buf = np.zeros(2, pa.BUS_RECORD_DTYPE)
    assert L.pa_bus_records(writer._h, buf.ctypes.data, 1) == pa._ffi.PA_ERR_BUFFER_TOO_SMALL
    assert L.pa_bus_records(writer._h, buf.ctypes.data, 2) == pa._ffi.PA_OK and bm.records_from_array(buf) == want[0]
    n_ids = C.c_uint64()
    assert L.pa_bus_ecs(writer._h, None, None, 0, C.byref(n_ids)) == pa._ffi.PA_OK and n_ids.value == sum(len(x) for x in want[1])
    off, ids = np.zeros(len(want[1]) + 1, np.uint64), np.zeros(n_ids.value, np.uint32)
    assert L.pa_bus_ecs(writer._h, off.ctypes.data, ids.ctypes.data, n_ids.value - 1, C.byref(n_ids)) == pa._ffi.PA_ERR_BUFFER_TOO_SMALL
    assert L.pa_bus_ecs(writer._h, off.ctypes.data, ids.ctypes.data, n_ids.value, C.byref(n_ids)) == pa._ffi.PA_OK and bm.table_from_csr(off, ids) == want[1]
    # before finish there is nothing to read
    fresh = pa.BusWriter(al, host, 4, 4)
    assert L.pa_bus_records(fresh._h, buf.ctypes.data, 2) == pa._ffi.PA_ERR_INVALID_ARG
    # the lengths: each at least 1, together at most 32
    for bc_len, umi_len in ((0, 4), (4, 0), (17, 16), (32, 1), (33, 0)):
        with pytest.raises(pa.PaError) as e:
            pa.BusWriter(al, host, bc_len, umi_len)
        assert e.value.code == pa._ffi.PA_ERR_UNSUPPORTED
