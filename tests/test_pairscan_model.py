"""tests/pairscan_model.py pinned on hand-written cases: the id cut, the first bad position, lengths, offsets, bytes and maxima, as
pair_id_len (csrc/fastq_text.hpp) and HostPairReader::gather (csrc/pair_reader.cpp) define them (spelled out here case by case: the gather lives in an
unnamed namespace of the library; the id rule is an inline function, which tests/pairplan/pairplan_check.cpp runs over the cases of test_id_cut),
and the two rules of the device entry point (rows outside the text,
pieces beyond the capacity). The GPU tests compare pa_pairs_gather_device with this model bit for bit."""
import pairscan_model as pm


def test_id_cut():
    assert pm.cut_id(b"read7/1") == b"read7" and pm.cut_id(b"read7/2") == b"read7"
    assert pm.cut_id(b"read7/3") == b"read7/3" and pm.cut_id(b"read7/") == b"read7/" and pm.cut_id(b"read71") == b"read71"
    assert pm.cut_id(b"/1") == b"" and pm.cut_id(b"/2") == b""          # exactly two bytes: cut to nothing
    assert pm.cut_id(b"1") == b"1" and pm.cut_id(b"/") == b"/" and pm.cut_id(b"") == b""   # shorter than two bytes: never cut
    assert pm.cut_id(b"a/1/1") == b"a/1"                                  # once


def test_one_segment_by_hand():
    t1, r1 = pm.layout([(b"a/1", b"ACGTACGT"), (b"b", b"GG"), (b"c/3", b""), (b"/1", b"TTTTT")])
    t2, r2 = pm.layout([(b"a/2", b"CCC"), (b"b/2", b""), (b"c", b"AAAA"), (b"", b"G")], lead=b"xyz")
    assert r1[0] == (1, 3, 5, 8) and t1[5:13] == b"ACGTACGT" and r2[0] == (4, 3, 8, 3)
    b = pm.Batch(16, 16, 5)
    b.add_segment(t1, r1, t2, r2, 4, 0)
    # a/1 ~ a/2, b ~ b/2, c/3 != c (not cut), "/1" ~ "" (cut to nothing)
    assert b.ctl_words() == [2, 4, 4, 4 + 2 + 0 + 4, 3 + 0 + 4 + 1, pm.NONE]
    assert b.off1 == [0, 4, 6, 6, 10] and b.off2 == [0, 3, 3, 7, 8]
    assert bytes(b.bytes1) == b"ACGTGGTTTT" + b"\xee" * 6 and bytes(b.bytes2) == b"CCCAAAAG" + b"\xee" * 8
    whole = pm.Batch(16, 16, 5)
    whole.add_segment(t1, r1, t2, r2, pm.WHOLE_READ, 0)
    assert whole.off1 == [0, 8, 10, 10, 15] and whole.ctl["max_len1"] == 8 and bytes(whole.bytes1[:15]) == b"ACGTACGTGGTTTTT"


def test_first_bad_is_the_smallest_position_and_a_batch_continues_across_segments():
    recs = [(b"r%d" % i, b"A" * (i % 5)) for i in range(140)]
    mates = [(b"r%d/2" % i if i not in (5, 70, 130) else b"q%d" % i, b"C" * (i % 3)) for i in range(140)]
    t1, r1 = pm.layout(recs)
    t2, r2 = pm.layout(mates)
    one = pm.Batch(400, 400, 141)
    one.add_segment(t1, r1, t2, r2, pm.WHOLE_READ, 0)
    assert one.ctl["first_bad"] == 5
    # the same pairs as two segments out of different texts: positions, offsets and bytes are the batch's
    ta, ra = pm.layout(recs[:37])
    tb, rb = pm.layout(recs[37:], lead=b"....")
    t2a, r2a = pm.layout(mates[:37], lead=b"-")
    t2b, r2b = pm.layout(mates[37:])
    two = pm.Batch(400, 400, 141)
    two.add_segment(ta, ra, t2a, r2a, pm.WHOLE_READ, 0)
    assert two.ctl["first_bad"] == 5 and two.off1[37] == two.ctl["bytes1"] == sum(i % 5 for i in range(37))
    two.add_segment(tb, rb, t2b, r2b, pm.WHOLE_READ, 37)
    assert (two.off1, two.off2, two.bytes1, two.bytes2, two.ctl) == (one.off1, one.off2, one.bytes1, one.bytes2, one.ctl)
    late = pm.Batch(400, 400, 141)
    late.add_segment(t1, r1[:131], t2, r2[:130] + [r2[0]], pm.WHOLE_READ, 0)   # only the last pair differs
    assert late.ctl["first_bad"] == 5
    last = pm.Batch(64, 64, 4)
    last.add_segment(t1, r1[:3], t2, r2[:2] + [r2[9]], pm.WHOLE_READ, 0)
    assert last.ctl["first_bad"] == 2
    # a call at base 0 opens a new batch
    last.add_segment(t1, r1[:3], t2, r2[:3], 2, 0)
    assert last.ctl_words() == [pm.NONE, 2, 2, 0 + 1 + 2, 0 + 1 + 2, pm.NONE]


def test_rows_outside_the_text_and_pieces_beyond_the_capacity():
    t1, r1 = pm.layout([(b"a", b"ACGT"), (b"b", b"GGGG"), (b"c", b"TT")])
    t2, r2 = pm.layout([(b"a", b"AC"), (b"b", b"GGGGGG"), (b"c", b"T")])
    bad = list(r1)
    bad[1] = (r1[1][0], r1[1][1], r1[1][2], len(t1))           # the sequence runs beyond the text
    b = pm.Batch(32, 32, 4)
    b.add_segment(t1, bad, t2, r2, pm.WHOLE_READ, 0)
    assert b.ctl_words() == [pm.NONE, 4, 2, 6, 3, 1] and b.off1 == [0, 4, 4, 6] and b.off2 == [0, 2, 2, 3]
    small = pm.Batch(7, 5, 4)                                    # R1: piece 1 would end at 8; R2: piece 1 would end at 8
    small.add_segment(t1, r1, t2, r2, pm.WHOLE_READ, 0)
    assert small.ctl["bytes1"] == 10 and small.ctl["bytes2"] == 9
    assert bytes(small.bytes1) == b"ACGT\xee\xee\xee" and bytes(small.bytes2) == b"AC\xee\xee\xee"
