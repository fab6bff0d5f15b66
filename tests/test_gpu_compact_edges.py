"""The compact step (csrc/compact.hip, pa_results_compact_device) at its edges, with no aligner in the loop beyond the handle the call needs: records
and arena are written by hand, every output lies between sentinel words and is pre-filled with a pattern, the scratch has exactly the bytes the
library asks for. Everything is compared with the model (tests/compact_model.py, written from the header): all integers, equality; what the model
says is not written keeps its pattern."""
import numpy as np
import pytest

import compact_model as cm
import helpers

pa = helpers.pa
pytestmark = pytest.mark.gpu

GUARD = 64                                   # sentinel words in front of and behind every output
SENT64, PAT64 = 0xDEADBEEFCAFEF00D, 0x5A5A5A5A5A5A5A5A
SENT32, PAT32 = 0xDEADBEEF, 0xA5A5A5A5
SCR_GUARD = 512                              # bytes behind (and in front of) the scratch
INVALID_ARG, ERR_HIP = -1, -5


@pytest.fixture(scope="module")
def handle(small_index):
    if pa.lib().pa_device_count() < 1:
        raise RuntimeError("the gpu tier needs a GPU and the HIP library: %s" % pa.lib().pa_last_error().decode())
    assert pa._ffi.PA_ERR_INVALID_ARG == INVALID_ARG                                                 # (ERR_HIP: PA_ERR_HIP of the header)
    host = small_index(24)
    return pa.Pseudoaligner(host, 0), host.arrays()


def _guarded(n, sent, pat, dtype):
    import torch
    a = np.full(GUARD + n + GUARD, pat, dtype)
    a[:GUARD] = sent
    a[GUARD + n:] = sent
    return torch.from_numpy(a.view(np.uint8).copy()).cuda()


def _body(t, n, sent, dtype, what):
    a = t.cpu().numpy().view(dtype)
    assert (a[:GUARD] == sent).all(), "%s: a word in front of it was written" % what
    assert (a[GUARD + n:] == sent).all(), "%s: a word behind it was written" % what
    return a[GUARD:GUARD + n].copy()


def _run(handle, rec, arena, arena_cap, packed_cap, null_packed=False, null_pw=False, scratch_short=0, runs=1):
    """the call on guarded, pre-filled buffers -> (rc, compact u64[n], packed u32[packed_cap], *d_packed_words) of every run; a HIP error ends the session"""
    import torch
    al = handle[0]
    rec = np.asarray(rec, cm.RESULT_DTYPE).reshape(-1)
    n = len(rec)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy() if a.size else np.zeros(16, np.uint8)).cuda()
    d_rec, d_arena = up(rec), up(np.asarray(arena, np.uint32))
    d_compact = _guarded(n, SENT64, PAT64, np.uint64)
    d_packed = _guarded(packed_cap, SENT32, PAT32, np.uint32)
    d_pw = _guarded(1, SENT64, PAT64, np.uint64)
    sb = pa.lib().pa_compact_scratch_bytes(n)
    d_scr = torch.full((SCR_GUARD + 256 + sb + SCR_GUARD,), 0xC3, dtype=torch.uint8, device="cuda")
    pad = SCR_GUARD + (-(d_scr.data_ptr() + SCR_GUARD)) % 256
    out = []
    try:
        for _ in range(runs):
            torch.cuda.synchronize()
            rc = pa.lib().pa_results_compact_device(al._h, d_rec.data_ptr(), d_arena.data_ptr(), arena_cap, n, d_compact.data_ptr() + GUARD * 8,
                                                    None if null_packed else d_packed.data_ptr() + GUARD * 4, packed_cap, None if null_pw else d_pw.data_ptr() + GUARD * 8,
                                                    d_scr.data_ptr() + pad, sb - scratch_short, None)
            if rc == ERR_HIP:
                raise RuntimeError(pa.lib().pa_last_error().decode())
            torch.cuda.synchronize()
            scr = d_scr.cpu().numpy()
            assert (scr[:pad] == 0xC3).all() and (scr[pad + sb:] == 0xC3).all(), "a byte outside the %d scratch bytes was written" % sb
            out.append((rc, _body(d_compact, n, SENT64, np.uint64, "d_compact"), _body(d_packed, packed_cap, SENT32, np.uint32, "d_packed"),
                        int(_body(d_pw, 1, SENT64, np.uint64, "d_packed_words")[0])))
    except RuntimeError as e:   # a launch, a copy or the synchronisation failed: nothing more is started on a GPU that may have faulted
        pytest.exit("compact kernels: %s" % e, returncode=3)
    return out if runs > 1 else out[0]


def _check(handle, rec, arena, arena_cap, packed_cap, **kw):
    """one batch against the model -> (the model's tuple, the GPU's)"""
    want = cm.compact(rec, arena, arena_cap, packed_cap)
    w_compact, w_packed, w_written, need = want
    got = _run(handle, rec, arena, arena_cap, packed_cap, **kw)
    rc, compact, packed, pw = got
    assert rc == 0, pa.lib().pa_last_error().decode()
    assert pw == need
    bad = np.flatnonzero(compact != w_compact)
    assert len(bad) == 0, "record %d: %s, the model %s (%s)" % (bad[0], cm.fields(compact[bad[0]]), cm.fields(w_compact[bad[0]]), rec[bad[0]])
    m = len(w_packed)
    assert m == min(need, packed_cap)
    assert np.array_equal(packed[:m][w_written], w_packed[w_written]), "packed stream"
    assert (packed[:m][~w_written] == PAT32).all() and (packed[m:] == PAT32).all(), "a word of an entry that does not fit, or behind the stream, was written"
    return want, got


def _batch(arrays, n, seed):
    """n records, kind i % 5 (unmapped, empty, by reference, packed, lost), packed classes of 1 .. 130 ids at shuffled arena offsets, two records on one range"""
    rng = np.random.RandomState(seed)
    off = arrays["ec_offset"].astype(np.int64)
    nc = int(arrays["num_classes"])
    T = int(arrays["num_transcripts"])
    packed_at = [i for i in range(n) if i % 5 == 3]
    lens = {i: 1 + j % 130 for j, i in enumerate(packed_at)}
    shared = (packed_at[len(packed_at) // 2], packed_at[-1]) if len(packed_at) >= 2 else None
    if shared:
        lens[shared[1]] = lens[shared[0]]                           # the last packed record names the arena range of the one in the middle
    arena = [0xABCD0000, 0xABCD0001, 0xABCD0002]
    place = {}
    for i in rng.permutation(packed_at[:-1] if shared else packed_at):   # the arena order is not the read order
        place[int(i)] = len(arena)
        arena += sorted(rng.choice(max(T, 200), lens[int(i)], replace=False).tolist()) + [0xEEEE0000 + int(i)]
    if shared:
        place[shared[1]] = place[shared[0]]
    cap = len(arena)
    rec = np.zeros(n, cm.RESULT_DTYPE)
    for i in range(n):
        cov, mm = int(rng.randint(0, 16384)), int(rng.randint(0, 16384))
        k = i % 5
        if k == 0:
            rec[i] = (cov, mm, 0x80000005, 7) if i % 10 else (cov, mm, 3, 2)
        elif k == 1:
            rec[i] = (cov, mm | cm.MAPPED_BIT, cm.CLASS_REF | 9 if i % 10 == 1 else 0, 0)
        elif k == 2:
            c = int(rng.randint(0, nc))
            rec[i] = (cov, mm | cm.MAPPED_BIT, cm.CLASS_REF | c, max(1, int(off[c + 1] - off[c])))
        elif k == 3:
            rec[i] = (cov, mm | cm.MAPPED_BIT, place[i], lens[i])
        else:
            ln = 1 + i % 130
            rec[i] = (cov, mm | cm.MAPPED_BIT, cap - ln + 1 + i % 7, ln)   # ends 1 .. 7 words beyond the arena: never dereferenced
    assert [cm.kind(r, cap) for r in rec] == [cm.KINDS[i % 5] for i in range(n)]
    return rec, np.array(arena, np.uint32), cap, shared


@pytest.mark.parametrize("n", [0, 1, 254, 255, 256, 257, 511, 512, 1025])
def test_sizes_around_the_blocks_of_256(handle, n):
    """n + 1 threads write the lengths (len[n] = 0 closes the scan), the same n + 1 threads write the records: compact[n] — the first sentinel word — is
    nobody's, also where n + 1 fills its last block exactly (n = 255) and where thread n opens a block of its own (n = 256)"""
    rec, arena, cap, shared = _batch(handle[1], n, 100 + n)
    (w_compact, w_packed, w_written, need), _ = _check(handle, rec, arena, cap, cap + n + 8)
    assert w_written.all() and need == sum(1 + int(r["class_len"]) for i, r in enumerate(rec) if i % 5 == 3)
    assert (shared is not None) == (n >= 254)
    if shared:                                                      # one arena range, two entries
        at = [int(w_compact[i] >> np.uint64(32)) for i in shared]
        ln = int(rec["class_len"][shared[0]])
        assert at[0] < at[1] and ln > 1 and np.array_equal(w_packed[at[0]:at[0] + 1 + ln], w_packed[at[1]:at[1] + 1 + ln])


def test_the_arena_boundary(handle):
    """class_off + class_len == arena_cap is packed and copied; one more is lost (both bits, hi == 0, no room in the stream); the sum is not taken in 32 bits"""
    arena = np.arange(1000, 1040, dtype=np.uint32)
    cap = len(arena)
    M = cm.MAPPED_BIT
    rec = np.array([(100, M | 1, cap - 5, 5),                   # ends at the last word of the arena
                    (101, M | 2, cap - 5 + 1, 5),               # one beyond
                    (102, M | 0, 0x7FFFFFFF, 0xFFFFFFFF),       # the sum is beyond 2^32
                    (103, M | 3, cap - 1, 1),                   # the last word alone
                    (104, M | 0, cap, 1),                       # starts at arena_cap
                    (105, M | 1, 0, cap),                       # the whole arena
                    (106, M | 1, 0, cap + 1),
                    (107, M | 2, 7, 4),
                    (108, M | 0, 0x7FFFFFFF, 0x80000006)], cm.RESULT_DTYPE)   # a sum that would be 5 if it were taken in 32 bits
    assert [cm.kind(r, cap) for r in rec] == ["packed", "lost", "lost", "packed", "lost", "packed", "lost", "packed", "lost"]
    (w_compact, w_packed, w_written, need), (rc, compact, packed, pw) = _check(handle, rec, arena, cap, 200)
    assert need == 6 + 2 + (cap + 1) + 5
    for i in (1, 2, 4, 6, 8):
        f = cm.fields(compact[i])
        assert f["by_ref"] and f["packed"] and f["mapped"] and f["hi"] == 0 and f["coverage"] == 100 + i
    assert packed[:6].tolist() == [5] + arena[cap - 5:].tolist() and packed[6:8].tolist() == [1, int(arena[cap - 1])]
    assert [cm.fields(compact[i])["hi"] for i in (0, 3, 5, 7)] == [0, 6, 8, 8 + cap + 1]


def test_garbage_behind_the_flags(handle):
    """an unmapped record's class fields and an empty class's offset mean nothing; MAPPED comes from bit 31 of mismatches alone"""
    arena = np.arange(50, 60, dtype=np.uint32)
    M = cm.MAPPED_BIT
    rec = np.array([(3, 4, 0x80000005, 7),                     # unmapped: the fields of a by-reference class
                    (5, 6, 2, 3),                              # unmapped: the fields of a packed class
                    (7, 8, 0x7FFFFFFF, 0xFFFFFFFF),            # unmapped: the fields of a lost one
                    (9, M | 1, 0x80000011, 0),                 # mapped, empty, REF bit set
                    (10, M | 2, 4, 0),                         # mapped, empty, an arena offset
                    (0xFFFFFFFF, 0, 0, 0),                     # every bit of coverage, none of mismatches: not mapped
                    (0x80000000, 0x7FFFFFFF, 0x80000001, 1),   # bit 31 of coverage, every bit of mismatches but 31: not mapped
                    (0, M, 0, 0),                              # bit 31 of mismatches and nothing else: mapped, empty
                    (0, M, 0x80000001, 1)], cm.RESULT_DTYPE)
    _, (rc, compact, packed, pw) = _check(handle, rec, arena, len(arena), 16)
    assert pw == 0 and (packed == PAT32).all()
    f = [cm.fields(c) for c in compact]
    assert [x["mapped"] for x in f] == [False, False, False, True, True, False, False, True, True]
    assert all(not x["by_ref"] and not x["packed"] and x["hi"] == 0 for x in f[:8]) and not any(x["bit31"] for x in f)
    assert int(compact[0]) == 3 | (4 << 14) and int(compact[3]) == 9 | (1 << 14) | (1 << 28)
    assert int(compact[5]) == 0x3FFF and int(compact[6]) == 0x3FFF << 14 and int(compact[7]) == 1 << 28 and int(compact[8]) == (1 << 28) | (1 << 29) | (1 << 32)


PACKED_CAP_LENS = (3, 1, 130, 2)
PACKED_CAP_NEED = sum(1 + l for l in PACKED_CAP_LENS)      # 140


@pytest.mark.parametrize("packed_cap", [PACKED_CAP_NEED, PACKED_CAP_NEED - 1, 4 + 2 + 57, 4 + 2, 1, 0])
def test_packed_cap_cuts_the_stream(handle, packed_cap):
    """four entries of 1 + {3, 1, 130, 2} words: an entry that would end beyond packed_cap is not written, none behind it is, those in front of it are exact;
    *d_packed_words is the need and the records keep PA_COMPACT_PACKED and their offsets whatever fits (packed_cap == 0: d_packed is NULL)"""
    rng = np.random.RandomState(5)
    arena, rec = [0xABCD0000], [(1, 2, 0, 0)]                  # (an unmapped record in front and between)
    for j, l in enumerate(PACKED_CAP_LENS):
        rec.append((20 + j, cm.MAPPED_BIT | j, len(arena), l))
        arena += rng.randint(0, 5000, l).tolist() + [0xEEEE0000]
        rec.append((30 + j, cm.MAPPED_BIT, cm.CLASS_REF | j, 2))
    rec, arena = np.array(rec, cm.RESULT_DTYPE), np.array(arena, np.uint32)
    full = cm.compact(rec, arena, len(arena), PACKED_CAP_NEED)
    (w_compact, w_packed, w_written, need), (rc, compact, packed, pw) = _check(handle, rec, arena, len(arena), packed_cap, null_packed=packed_cap == 0)
    assert need == pw == PACKED_CAP_NEED and np.array_equal(compact, full[0])
    assert [cm.fields(compact[1 + 2 * j]) for j in range(4)] == [dict(coverage=20 + j, mismatches=j, mapped=True, by_ref=False, packed=True, bit31=False, hi=h)
                                                                  for j, h in enumerate((0, 4, 6, 137))]
    fits = {140: 4, 139: 3, 63: 2, 6: 2, 1: 0, 0: 0}[packed_cap]
    end = sum(1 + l for l in PACKED_CAP_LENS[:fits])
    assert int(w_written.sum()) == min(end, packed_cap) == end and w_written[:end].all()
    assert np.array_equal(packed[:end], full[1][:end]) and (packed[end:] == PAT32).all()


def test_fields_side_by_side(handle):
    """coverage and mismatches at 0, 1 and 16383 (PA_COMPACT_MAX_READ_LEN): exact, neither reaches the other's bits or bits 28 - 30"""
    vals = (0, 1, 16383)
    rec = np.array([(c, m | f, 0, 0) for f in (0, cm.MAPPED_BIT) for c in vals for m in vals], cm.RESULT_DTYPE)
    _, (rc, compact, packed, pw) = _check(handle, rec, np.zeros(4, np.uint32), 4, 4)
    want = [c | (m << 14) | (1 << 28 if f else 0) for f in (0, 1) for c in vals for m in vals]
    assert [int(x) for x in compact] == want
    assert 16383 in want and 16383 << 14 in want and (1 << 28) | 16383 in want and (1 << 28) | (16383 << 14) in want    # one field full, the other empty


def test_refused_arguments_launch_nothing(handle):
    """a scratch one byte short, a packed_cap without a buffer, no place for the stream's length: PA_ERR_INVALID_ARG and every output keeps its pattern"""
    rec, arena, cap, _ = _batch(handle[1], 300, 9)
    for kw in (dict(scratch_short=1), dict(null_packed=True), dict(null_pw=True)):
        rc, compact, packed, pw = _run(handle, rec, arena, cap, 4096, **kw)
        assert rc == INVALID_ARG, (kw, rc)
        assert (compact == PAT64).all() and (packed == PAT32).all() and pw == PAT64, kw
    _check(handle, rec, arena, cap, 4096)                     # (the same batch with nothing wrong)


def test_a_repeat_run_gives_the_same_bytes(handle):
    rec, arena, cap, _ = _batch(handle[1], 700, 11)
    want = cm.compact(rec, arena, cap, 3000)                  # (a packed_cap inside the stream: the second run must not write more than the first)
    assert want[3] > 3000
    a, b = _run(handle, rec, arena, cap, 3000, runs=2)
    assert a[0] == b[0] == 0 and a[3] == b[3] == want[3]
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[1], want[0])
    assert np.array_equal(a[2][want[2]], want[1][want[2]]) and (a[2][~want[2]] == PAT32).all()
