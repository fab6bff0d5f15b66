"""The pure-Python model of the BUS output (tests/bus_model.py) pinned on hand cases: the bytes of a two-record file against a hex literal
written by hand from the format's description, the ec numbering, the fates in their order, and a read-back round trip. No GPU, no library."""
import bus_model as bm

CLASSES = [(3,), (1, 5), (), (2, 3, 4), (0, 6), (6,)]   # index classes 0..5 of a toy index of T = 8 transcripts: M = 3
T = 8


def test_two_record_file_bytes():
    # barcode ACGT = 0b00011011 = 0x1b, UMI GA = 0b1000 = 8, ec 5, 3 reads; barcode TTTT = 0xff, UMI TT = 0xf, ec 9, 70 000 reads
    records = [(bm.pack("ACGT"), bm.pack("GA"), 5, 3), (bm.pack("TTTT"), bm.pack("TT"), 9, 70000)]
    assert records == [(0x1B, 8, 5, 3), (0xFF, 0xF, 9, 70000)]
    want = bytes.fromhex(
        "42555300"                  # B U S \0
        "01000000"                  # version 1
        "04000000" "02000000"       # bclen 4, umilen 2
        "00000000"                  # tlen 0
        "1b00000000000000" "0800000000000000" "05000000" "03000000" "00000000" "00000000"
        "ff00000000000000" "0f00000000000000" "09000000" "70110100" "00000000" "00000000")
    got = bm.bus_bytes(records, 4, 2)
    assert got == want and len(got) == 20 + 2 * 32
    assert bm.read_bus(want) == (4, 2, b"", records)
    # free text moves the records behind it
    with_text = bm.bus_bytes(records, 4, 2, b"hello")
    assert with_text[16:20] == bytes.fromhex("05000000") and with_text[20:25] == b"hello" and bm.read_bus(with_text) == (4, 2, b"hello", records)


def test_ec_numbering():
    lists = [(1, 5), (5,), (2, 3), (1, 5, 7), (1, 7), (2, 3), (0, 6)]
    ec_of, table, novel = bm.number_ecs(T, CLASSES, lists)
    assert table[:T] == [(t,) for t in range(T)]
    assert table[T:T + 3] == [(1, 5), (2, 3, 4), (0, 6)]                   # the classes of two ids or more, in class-id order
    assert novel == [(1, 5, 7), (1, 7), (2, 3)] and table[T + 3:] == novel   # {1,5} < {1,5,7} < {1,7} < {2,3}
    assert ec_of[(1, 5)] == T and ec_of[(0, 6)] == T + 2 and ec_of[(2, 3)] == T + 5 and ec_of[(1, 5, 7)] == T + 3
    assert (5,) not in ec_of                                                # a list of one id is ec t
    # a pure function of the set of recorded lists: order and repeats do not matter
    assert bm.number_ecs(T, CLASSES, list(reversed(lists)) + lists)[1] == table
    assert bm.matrix_ec_text(table).splitlines()[T:T + 2] == ["8\t1,5", "9\t2,3,4"] and bm.read_matrix_ec(bm.matrix_ec_text(table)) == table
    # no novel list: T + M lines
    assert len(bm.number_ecs(T, CLASSES, [(1, 5), (3,)])[1]) == T + 3


def test_fates_in_order_and_records():
    bc, umi = 3, 2
    r1s = ["ACGT",            # one byte short
           "ANGTT",           # N in the barcode (and a valid UMI)
           "NCGNT",           # N in both: the barcode's rule comes first
           "ACGNT",           # N in the UMI
           "ACGtT",           # lower case is no base
           "ACGTT",           # unmapped
           "ACGTT",           # mapped, empty class
           "ACGTT",           # an id that is no transcript
           "ACGTT",           # descending
           "ACGTT",           # repeated id: not strictly ascending
           "ACGTT",           # a class the record cannot name
           "ACGTTAAAA",       # recorded: the tail is not read
           "ACGTT", "ACGTT",  # ... the same record, by content of index class 1 and as a list of one id
           "AAAAA", "TTTTT", "ACGTT"]
    mapping = [(True, [3])] * 5 + [(False, [3]), (True, []), (True, [3, T]), (True, [5, 1]), (True, [1, 1]), (True, bm.BAD),
                                   (True, [1, 5]), (True, [1, 5]), (True, [3]), (True, [2, 3]), (True, [1, 7]), (True, [3])]
    records, table, st, fates = bm.model(r1s, mapping, T, CLASSES, bc, umi)
    assert fates[:11] == ["r1_short", "barcode_n", "barcode_n", "umi_n", "umi_n", "unmapped", "unmapped", "bad_class", "bad_class", "bad_class", "bad_class"]
    assert st == dict(reads=17, r1_short=1, barcode_n=2, umi_n=2, unmapped=2, bad_class=4, recorded=6, records=4)
    acg, tt = bm.pack("ACG"), bm.pack("TT")
    assert table[T + 3:] == [(1, 7), (2, 3)]
    assert records == [(0, 0, T + 4, 1), (acg, tt, 3, 2), (acg, tt, T, 2), (bm.pack("TTT"), tt, T + 3, 1)]
    # the three files, written and read back
    data = bm.bus_bytes(records, bc, umi)
    assert bm.read_bus(data) == (bc, umi, b"", records)
    assert bm.transcripts_text(["a", "b c"]) == "a\nb c\n"


def test_count_clamp_and_dtype():
    records, _, st, _ = bm.model(["AC"] * 5, [(True, [0])] * 5, T, CLASSES, 1, 1)
    assert records == [(0, 1, 0, 5)] and st["records"] == 1
    assert bm.RECORD_DTYPE.itemsize == 32 and bm.RECORD_DTYPE.fields["ec"][1] == 16 and bm.RECORD_DTYPE.fields["pad"][1] == 28
    assert bm.COUNT_MAX == 2 ** 32 - 1
