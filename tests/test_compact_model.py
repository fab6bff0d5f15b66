"""The model of the compact records (tests/compact_model.py, written from the header) against the one reader of those records the package has,
pa.unpack_compact: what the model packs, the reader unpacks. No GPU; the GPU tests (test_gpu_compact_edges.py, test_gpu_host_batch_edges.py) compare
the kernel with this model."""
import numpy as np
import pytest

import compact_model as cm
import helpers

pa = helpers.pa

_cache = {}


def tiny_index():
    """five transcripts over three shared segments at K = 11: index classes of one, two and three ids"""
    if "host" not in _cache:
        rng = np.random.RandomState(7)
        seg = [rng.randint(0, 4, 60).astype(np.uint8) for _ in range(5)]
        tx = [np.concatenate(p) for p in ((seg[0], seg[1]), (seg[1], seg[2]), (seg[0], seg[1], seg[2]), (seg[3],), (seg[4], seg[2]))]
        starts = np.concatenate([[0], np.cumsum([len(t) for t in tx])]).astype(np.uint64)
        _cache["host"] = pa.HostIndex.build_packed(helpers.pack_bases(np.concatenate(tx)), starts, 11, 1)
    return _cache["host"]


def hand_made(a):
    """records of the four kinds a reader accepts -> (records, arena, arena_cap, the classes they stand for (None: unmapped))"""
    off = a["ec_offset"].astype(np.int64)
    nc = int(a["num_classes"])
    assert nc >= 3 and int((off[1:] - off[:-1]).max()) >= 2
    cls = lambda c: a["ec_ids"][off[c]:off[c + 1]].tolist()
    novel = [[0, 3], [2], [0, 1, 2, 3, 4], [1, 3, 4]]                # (transcript 2 has no k-mer of its own: {2} is no index class)
    table = cm.class_table(a)
    assert not any(tuple(x) in table for x in novel)
    arena = [0xABCD0000, 0xABCD0001]
    rec, want = [], []
    place = {}
    for j, ids in enumerate(novel):                                  # the arena is not in read order
        place[j] = len(arena)
        arena += ids + [0xEEEE0000]
    for i in range(23):
        cov, mm = (i * 701) % 16384, (i * 37) % 16384
        k = i % 4
        if k == 0:
            rec.append((cov, mm, 0x80000005, 7)); want.append(None)                                  # unmapped, garbage in the class fields
        elif k == 1:
            rec.append((cov, mm | cm.MAPPED_BIT, cm.CLASS_REF if i % 8 == 1 else 0, 0)); want.append([])   # mapped, empty
        elif k == 2:
            c = i % nc
            rec.append((cov, mm | cm.MAPPED_BIT, cm.CLASS_REF | c, len(cls(c)))); want.append(cls(c))
        else:
            j = (3 - i // 4) % len(novel)
            rec.append((cov, mm | cm.MAPPED_BIT, place[j], len(novel[j]))); want.append(novel[j])
    return np.array(rec, cm.RESULT_DTYPE).reshape(-1), np.array(arena, np.uint32), len(arena), want


def test_model_output_unpacks_to_the_classes_it_was_built_from(built):
    host = tiny_index()
    rec, arena, cap, want = hand_made(host.arrays())
    compact, packed, written, need = cm.compact(rec, arena, cap, 1 << 20)
    assert written.all() and need == len(packed) == sum(1 + len(w) for r, w in zip(rec, want) if w and not r["class_off"] & cm.CLASS_REF)
    res, coff, ids = pa.unpack_compact(compact, packed, host)
    for i, w in enumerate(want):
        assert bool(res["mismatches"][i] >> 31) == (w is not None), i
        assert int(res["coverage"][i]) == int(rec["coverage"][i]) and int(res["mismatches"][i] & 0x7FFFFFFF) == int(rec["mismatches"][i] & 0x3FFF), i
        assert ids[int(coff[i]):int(coff[i + 1])].tolist() == (w or []), i
        assert int(res["class_len"][i]) == len(w or [])
    # the kinds, and what `hi` is for each
    kinds = [cm.kind(r, cap) for r in rec]
    assert set(kinds) == {"unmapped", "empty", "by_ref", "packed"}
    at = 0
    for i, k in enumerate(kinds):
        f = cm.fields(compact[i])
        assert (f["mapped"], f["by_ref"], f["packed"], f["bit31"]) == (k != "unmapped", k == "by_ref", k == "packed", False), (i, k, f)
        if k == "packed":
            assert f["hi"] == at and packed[at] == len(want[i])
            at += 1 + len(want[i])
        else:
            assert f["hi"] == (int(rec["class_off"][i]) & 0x7FFFFFFF if k == "by_ref" else 0)
    assert at == need


def test_reader_refuses_a_lost_record_and_a_truncated_stream(built):
    host = tiny_index()
    rec, arena, cap, want = hand_made(host.arrays())
    last = max(i for i in range(len(rec)) if cm.kind(rec[i], cap) == "packed")
    compact, packed, written, need = cm.compact(rec, arena, cap, 1 << 20)
    # one word short: the last entry is not written, `need` and the records stay what they were
    c2, p2, w2, need2 = cm.compact(rec, arena, cap, need - 1)
    assert need2 == need and np.array_equal(c2, compact) and len(p2) == need - 1
    tail = 1 + len(want[last])
    assert w2[:need - tail].all() and not w2[need - tail:].any() and np.array_equal(p2[:need - tail], packed[:need - tail])
    with pytest.raises(AssertionError, match="packed stream"):
        pa.unpack_compact(compact, packed[:need - 1], host)                       # (the stream without the last id of its last entry)
    # a record whose ids lie beyond the arena: lost, both bits, no room in the stream
    lost = rec.copy()
    lost["class_off"][last] = cap - int(lost["class_len"][last]) + 1
    c3, p3, w3, need3 = cm.compact(lost, arena, cap, 1 << 20)
    f = cm.fields(c3[last])
    assert cm.kind(lost[last], cap) == "lost" and f["by_ref"] and f["packed"] and f["mapped"] and f["hi"] == 0 and need3 == need - tail
    assert np.array_equal(np.delete(c3, last), np.delete(compact, last))       # (it was the last entry: no other offset moves)
    with pytest.raises(AssertionError, match="lost to a full arena"):
        pa.unpack_compact(c3, p3, host)
    # at the boundary it is packed
    edge = rec.copy()
    edge["class_off"][last] = cap - int(edge["class_len"][last])
    assert cm.kind(edge[last], cap) == "packed"
    # the sum is not taken in 32 bits
    wrap = np.array([(1, 1 | cm.MAPPED_BIT, 0x7FFFFFFF, 0xFFFFFFFF)], cm.RESULT_DTYPE)
    assert cm.kind(wrap[0], cap) == "lost"


@pytest.mark.parametrize("cov,mm", [(a, b) for a in (0, 1, 16383) for b in (0, 1, 16383)])
def test_fields_round_trip(built, cov, mm):
    """14 bits each, side by side, nothing in bits 28 - 31 but the flags"""
    host = tiny_index()
    assert pa.PA_COMPACT_MAX_READ_LEN == cm.FIELD_MAX == 16383
    assert (pa.PA_COMPACT_MAPPED, pa.PA_COMPACT_BY_REF, pa.PA_COMPACT_PACKED) == (cm.COMPACT_MAPPED, cm.COMPACT_BY_REF, cm.COMPACT_PACKED)
    rec = np.array([(cov, mm | cm.MAPPED_BIT, 0, 0), (cov, mm, 0, 0)], cm.RESULT_DTYPE)
    compact, packed, written, need = cm.compact(rec, np.zeros(1, np.uint32), 1, 0)
    assert need == 0 and len(packed) == 0
    assert int(compact[0]) == cov | (mm << 14) | (1 << 28) and int(compact[1]) == cov | (mm << 14)
    res, coff, ids = pa.unpack_compact(compact, packed, host)
    assert res["coverage"].tolist() == [cov, cov] and res["mismatches"].tolist() == [mm | cm.MAPPED_BIT, mm]
    assert coff.tolist() == [0, 0, 0] and len(ids) == 0
