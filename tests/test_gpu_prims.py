"""csrc/device_prims.hpp through tests/prims/prims_probe.hip — one export per wrapper instantiation the product makes — against numpy and
Python integers. Everything is exact. What the callers rely on and the suite's shapes never showed: scans are summed in the OUTPUT type,
sorts are stable and look at [begin_bit, end_bit) alone, n = 0 is a no-op, nothing is written past the end, the scratch buffer of a
chain of operations never shrinks. The two host-side helpers (bits_for, grid_for) are checked on the CPU tier too: those tests carry no
gpu mark."""
import ctypes as C
from collections import Counter

import numpy as np
import pytest

import helpers

gpu = pytest.mark.gpu
PA_OK = 0
GUARD = 4   # elements behind every sort / scan output of the probe (probe_guard())
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 100003, 1000003]
FILL = {np.dtype(np.uint32): 0xDEADBEEF, np.dtype(np.uint64): 0xDEADBEEFCAFEF00D}


def L():
    return helpers.prims_lib()


class Tmp:
    """a DeviceBuffer<uint8_t> scratch of the probe"""

    def __init__(self):
        self.h = L().probe_tmp_new()

    def size(self):
        return int(L().probe_tmp_size(self.h))

    def __del__(self):
        try:
            L().probe_tmp_free(self.h)
        except Exception:
            pass


def ptr(a):
    return a.ctypes.data


def filled(n, dtype, width=1):
    """an output of n (+ GUARD) elements pre-filled with a pattern"""
    a = np.full((n + GUARD) * width, FILL[np.dtype(dtype)], dtype)
    return a


def ok(rc):
    assert rc == PA_OK, (rc, L().probe_last_error().decode())


# ---- bits_for / grid_for: host code, no GPU ----
def test_probe_compiles_and_bits_for(built):
    lib = L()
    assert lib.probe_guard() == GUARD
    values = [0, 1, 2, 3, 2 ** 64 - 1] + [v for k in range(1, 64) for v in (2 ** k - 1, 2 ** k, 2 ** k + 1)]
    for v in values:
        assert lib.probe_bits_for(v) == int(v).bit_length(), v
    assert lib.probe_bits_for(0) == 0 and lib.probe_bits_for(2 ** 63) == 64


def test_grid_for(built):
    """blocks that cover n items: the ceiling of n / block while it fits the 32-bit return type. 2^32 * 256 - 255 items need 2^32 blocks
    of 256, the first count that does not fit: there, and beyond, the answer is 0 (a launch that fails), never the count's low 32 bits
    (a small grid that would silently cover the first few items), and n + block - 1 must not wrap at 2^64 either."""
    lib = L()
    edge = 2 ** 32 * 256 - 255
    for block in (256, 64):
        for n in (0, 1, 255, 256, 257, block - 1, block, block + 1, 2 ** 32 - 1, 2 ** 32, (2 ** 32 - 1) * block, (2 ** 32 - 1) * block + 1, edge, edge - 1,
                  edge + 256, 2 ** 32 * 256 + 1, 2 ** 64 - 1):
            want = (n + block - 1) // block
            assert lib.probe_grid_for(n, block) == (want if want < 2 ** 32 else 0), (n, block)
    assert lib.probe_grid_for(edge - 1, 256) == 2 ** 32 - 1 and lib.probe_grid_for(edge, 256) == 0 and lib.probe_grid_for(2 ** 32 * 256 + 1, 256) == 0
    for n in (0, 1, 255, 256, 257, edge):
        assert lib.probe_grid_for_default(n) == lib.probe_grid_for(n, 256)


# ---- sorts ----
# name -> (probe entry, key bits, has values, descending)
SORTS = {
    "keys_ull_int": ("probe_sort_keys_ull_int", 64, False, False),
    "keys_ull_size": ("probe_sort_keys_ull_size", 64, False, False),
    "pairs_ull_u32_int": ("probe_sort_pairs_ull_u32_int", 64, True, False),
    "pairs_u32_u32_size": ("probe_sort_pairs_u32_u32_size", 32, True, False),
    "pairs_u64_u32_size": ("probe_sort_pairs_u64_u32_size", 64, True, False),
    "pairs_ull_u32_size": ("probe_sort_pairs_ull_u32_size", 64, True, False),
    "pairs_u128_u32_size": ("probe_sort_pairs_u128_u32_size", 128, True, False),
    "pairs_desc_u32_u32_size": ("probe_sort_pairs_desc_u32_u32_size", 32, True, True),
    "pairs_desc_u32_u32_int": ("probe_sort_pairs_desc_u32_u32_int", 32, True, True),
}
BIT_RANGES = [(0, 1), (0, 48), (0, 62), (0, 32), (0, 33), (0, 64), (7, 19)]   # [0, 2k) for k = 24, 31
WIDE_RANGES = [(0, 96), (0, 128), (60, 70), (64, 65)]                          # 128-bit keys only (k > 32: up to [0, 128))


def ranges_of(bits):
    return [r for r in BIT_RANGES + (WIDE_RANGES if bits == 128 else []) if r[1] <= bits]


def random_words(rng, n, bits):
    """n keys of `bits` bits as little-endian 64-bit (or 32-bit) words: shape (n,) or, for 128 bits, (n, 2) = (low, high)"""
    if bits == 32:
        return rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    w = rng.integers(0, 2 ** 64, (n, bits // 64), dtype=np.uint64)
    return w[:, 0].copy() if bits == 64 else w


def field(keys, bits, b0, b1):
    """the bits [b0, b1) of every key as (low, high) uint64 words"""
    if bits <= 64:
        lo, hi = keys.astype(np.uint64), np.zeros(len(keys), np.uint64)
    else:
        lo, hi = keys[:, 0].copy(), keys[:, 1].copy()
    if b0 >= 64:
        lo, hi = hi >> np.uint64(b0 - 64), np.zeros_like(hi)
    elif b0:
        lo, hi = (lo >> np.uint64(b0)) | (hi << np.uint64(64 - b0)), hi >> np.uint64(b0)
    w = b1 - b0
    if w < 64:
        lo, hi = lo & np.uint64((1 << w) - 1), np.zeros_like(hi)
    elif w < 128:
        hi = hi & np.uint64((1 << (w - 64)) - 1)
    return lo, hi


def set_field(keys, bits, b0, b1, values):
    """keys with the bits [b0, b1) replaced by values (small integers), everything else kept: garbage above and below stays"""
    ints = [int(k) for k in keys] if bits <= 64 else [int(k[0]) | (int(k[1]) << 64) for k in keys]
    mask = ((1 << (b1 - b0)) - 1) << b0
    ints = [(k & ~mask) | ((int(v) << b0) & mask) for k, v in zip(ints, values)]
    if bits == 128:
        return np.array([[k & (2 ** 64 - 1), k >> 64] for k in ints], np.uint64).reshape(len(ints), 2)
    return np.array(ints, np.uint64).astype(keys.dtype)


def expected_order(keys, bits, b0, b1, desc):
    lo, hi = field(keys, bits, b0, b1)
    if desc:   # stable under the complemented masked key
        w = b1 - b0
        lo = ~lo & np.uint64((1 << min(w, 64)) - 1)
    return np.lexsort((lo, hi))   # (a stable sort by the last key first: high word, then low word)


def run_sort(name, tmp, keys, vals, b0, b1):
    entry, bits, has_vals, desc = SORTS[name]
    n = len(keys)
    width = 2 if bits == 128 else 1
    kdt = np.uint32 if bits == 32 else np.uint64
    kout = filled(n, kdt, width)
    keys = np.ascontiguousarray(keys)
    if has_vals:
        vout = filled(n, np.uint32)
        ok(getattr(L(), entry)(tmp.h, ptr(keys), ptr(kout), ptr(vals), ptr(vout), n, b0, b1))
    else:
        vout = None
        ok(getattr(L(), entry)(tmp.h, ptr(keys), ptr(kout), n, b0, b1))
    order = expected_order(keys, bits, b0, b1, desc)
    what = (name, n, b0, b1)
    assert np.array_equal(kout[: n * width].reshape(keys.shape), keys[order]), what
    assert (kout[n * width:] == FILL[np.dtype(kdt)]).all(), what       # nothing behind the end
    if has_vals:
        assert np.array_equal(vout[:n], vals[order]), what
        assert (vout[n:] == FILL[np.dtype(np.uint32)]).all(), what


@gpu
@pytest.mark.parametrize("name", list(SORTS))
def test_sort_sizes(name):
    """every size, the bit ranges in turn, random keys with garbage above end_bit and below begin_bit, values = positions"""
    bits = SORTS[name][1]
    rng = np.random.default_rng(len(name))
    tmp = Tmp()
    rs = ranges_of(bits)
    for j, n in enumerate(SIZES):
        keys = random_words(rng, n, bits)
        vals = np.arange(n, dtype=np.uint32)
        b0, b1 = rs[j % len(rs)]
        run_sort(name, tmp, keys, vals, b0, b1)
        if n == SIZES[-1]:
            run_sort(name, tmp, keys, vals, 0, bits)
    # n = 0: a no-op
    run_sort(name, tmp, random_words(rng, 0, bits), np.zeros(0, np.uint32), 0, bits)
    run_sort(name, Tmp(), random_words(rng, 0, bits), np.zeros(0, np.uint32), 0, 1)    # ... on a scratch that was never allocated, too


@gpu
@pytest.mark.parametrize("name", list(SORTS))
def test_sort_bit_ranges_and_stability(name):
    bits = SORTS[name][1]
    rng = np.random.default_rng(100 + len(name))
    tmp = Tmp()
    for n in (4097, 100003):
        keys = random_words(rng, n, bits)
        vals = rng.permutation(n).astype(np.uint32)
        for b0, b1 in ranges_of(bits):
            run_sort(name, tmp, keys, vals, b0, b1)
    n = 20011
    keys = random_words(rng, n, bits)
    vals = np.arange(n, dtype=np.uint32)
    for b0, b1 in ((7, 19), (0, bits), (0, 2)):
        # three distinct masked keys: stability alone decides the order inside each
        three = set_field(keys, bits, b0, b1, [(0, 1, (1 << (b1 - b0)) - 1)[j] for j in rng.integers(0, 3, n)])
        lo, hi = field(three, bits, b0, b1)
        assert len(set(zip(lo.tolist(), hi.tolist()))) == 3
        run_sort(name, tmp, three, vals, b0, b1)
        # all masked keys equal (the garbage differs): the output is the input
        same = set_field(keys, bits, b0, b1, [5 % (1 << (b1 - b0))] * n)
        run_sort(name, tmp, same, vals, b0, b1)
        assert np.array_equal(expected_order(same, bits, b0, b1, SORTS[name][3]), np.arange(n))
    run_sort(name, tmp, np.ascontiguousarray(np.broadcast_to(keys[:1], keys.shape)), vals, 0, bits)   # every key the same


# ---- scans ----
SCANS = {   # name: (entry, in type, out type, inclusive)
    "inclusive_u32_u32": ("probe_scan_inclusive_u32_u32", np.uint32, np.uint32, True),
    "exclusive_u32_u32": ("probe_scan_exclusive_u32_u32", np.uint32, np.uint32, False),
    "exclusive_ull_ull": ("probe_scan_exclusive_ull_ull", np.uint64, np.uint64, False),
    "inclusive_u32_ull": ("probe_scan_inclusive_u32_ull", np.uint32, np.uint64, True),
    "exclusive_u32_ull": ("probe_scan_exclusive_u32_ull", np.uint32, np.uint64, False),
}


def scan_reference(x, out_dtype, inclusive):
    """cumulative sums in Python-exact 64-bit arithmetic (no input here sums past 2^64), cast to the output type"""
    c = np.cumsum(x.astype(np.uint64), dtype=np.uint64)
    if not inclusive:
        c = np.concatenate([np.zeros(1, np.uint64), c[:-1]]) if len(x) else c
    return c.astype(out_dtype)   # (uint32: modulo 2^32, which is what a sum in uint32 is)


@gpu
@pytest.mark.parametrize("name", list(SCANS))
def test_scan_sizes(name):
    entry, it, ot, inclusive = SCANS[name]
    rng = np.random.default_rng(7)
    tmp = Tmp()
    for n in [0] + SIZES:
        x = rng.integers(0, 4000 if it == np.uint32 else 2 ** 40, n, dtype=np.uint64).astype(it)   # 1 000 003 * 4000 < 2^32: no wrap
        out = filled(n, ot)
        ok(getattr(L(), entry)(tmp.h, ptr(x), ptr(out), n))
        assert np.array_equal(out[:n], scan_reference(x, ot, inclusive)), (name, n)
        assert (out[n:] == FILL[np.dtype(ot)]).all(), (name, n)
    if it == np.uint32:   # sums in uint32 wrap modulo 2^32 like uint32 arithmetic; into uint64 they are carried past 2^32
        x = rng.integers(0, 2 ** 32, 4097, dtype=np.uint64).astype(np.uint32)
        out = filled(len(x), ot)
        ok(getattr(L(), entry)(tmp.h, ptr(x), ptr(out), len(x)))
        assert np.array_equal(out[:len(x)], scan_reference(x, ot, inclusive))


def scan_on(entry, x, ot, offset=512, tail=256):
    """the caller-carved form: the scratch is exactly prim_bytes(...) bytes at `offset` of a larger block -> (out, block, need)"""
    lib = L()
    n = len(x)
    need = C.c_uint64()
    out = filled(n, ot)
    probe = np.full(8, 0xA5, np.uint8)
    rc = getattr(lib, entry)(ptr(x), ptr(out), n, ptr(probe), 0, 0, C.byref(need))   # a block of no bytes: only the size comes back
    assert rc != PA_OK and need.value > 0 and (out == FILL[np.dtype(ot)]).all()
    block = np.full(offset + need.value + tail, 0xA5, np.uint8)
    need2 = C.c_uint64()
    ok(getattr(lib, entry)(ptr(x), ptr(out), n, ptr(block), len(block), offset, C.byref(need2)))
    assert need2.value == need.value
    return out, block, int(need.value)


@gpu
@pytest.mark.parametrize("entry,ot", [("probe_scan_exclusive_on_u32_u32", np.uint32), ("probe_scan_exclusive_on_u32_u64", np.uint64)])
def test_scan_exclusive_on_a_carved_scratch(entry, ot):
    rng = np.random.default_rng(8)
    for n in [0] + SIZES:
        x = rng.integers(0, 4000, n, dtype=np.uint64).astype(np.uint32)
        out, block, need = scan_on(entry, x, ot)
        assert np.array_equal(out[:n], scan_reference(x, ot, False)), (entry, n)
        assert (out[n:] == FILL[np.dtype(ot)]).all(), (entry, n)
        assert (block[:512] == 0xA5).all() and (block[512 + need:] == 0xA5).all(), (entry, n)   # the bytes on either side of the carve


@gpu
def test_scan_u32_into_u64_is_summed_as_u64():
    """lengths in uint32, offsets in uint64 that pass 4 GiB (compact.hip, render.hip): the sum must be carried in the OUTPUT type"""
    rng = np.random.default_rng(9)
    x = np.concatenate([np.full(3, 0x80000000, np.uint32), (0xFFFFFFF0 - rng.integers(0, 16, 100003)).astype(np.uint32)])
    want = scan_reference(x, np.uint64, False)
    assert int(want[3]) == 3 << 31 and int(want[-1]) > 2 ** 48 and int(x.astype(np.uint64).sum()) > 2 ** 32
    out, block, need = scan_on("probe_scan_exclusive_on_u32_u64", x, np.uint64)
    assert np.array_equal(out[:len(x)], want)
    assert (out[len(x):] == FILL[np.dtype(np.uint64)]).all() and (block[:512] == 0xA5).all() and (block[512 + need:] == 0xA5).all()
    # the same input summed as uint32 wraps: the two instantiations differ exactly there
    out32, _, _ = scan_on("probe_scan_exclusive_on_u32_u32", x, np.uint32)
    assert np.array_equal(out32[:len(x)], want.astype(np.uint32)) and not np.array_equal(out32[:len(x)].astype(np.uint64), want)


SCAN_TOTALS = {   # name: (entry, in type, out type)
    "u32_u32": ("probe_scan_inclusive_total_u32_u32", np.uint32, np.uint32),
    "ull_ull": ("probe_scan_inclusive_total_ull_ull", np.uint64, np.uint64),
    "u32_ull": ("probe_scan_inclusive_total_u32_ull", np.uint32, np.uint64),
}


@gpu
@pytest.mark.parametrize("name", list(SCAN_TOTALS))
def test_scan_inclusive_total(name):
    """the scan, and its last element on the host: every size from 1 up; a total wider than the input is carried past 2^32"""
    entry, it, ot = SCAN_TOTALS[name]
    rng = np.random.default_rng(13)
    tmp = Tmp()
    cases = [rng.integers(0, 4000 if it == np.uint32 else 2 ** 40, n, dtype=np.uint64).astype(it) for n in SIZES]
    if it == np.uint32:
        cases.append(rng.integers(2 ** 31, 2 ** 32, 4097, dtype=np.uint64).astype(np.uint32))
        assert int(cases[-1].astype(np.uint64).sum()) > 2 ** 32
    for x in cases:
        n = len(x)
        out, total = filled(n, ot), np.full(1, FILL[np.dtype(ot)], ot)
        ok(getattr(L(), entry)(tmp.h, ptr(x), ptr(out), n, ptr(total)))
        want = scan_reference(x, ot, True)
        assert np.array_equal(out[:n], want) and (out[n:] == FILL[np.dtype(ot)]).all(), (name, n)
        assert int(total[0]) == int(want[-1]) == int(out[n - 1]), (name, n)
    if name == "u32_ull":
        assert int(total[0]) == int(cases[-1].astype(np.uint64).sum()) > 2 ** 32


# ---- run-length encode, reduce by key ----
def run_shapes(n):
    """lists of run lengths that sum to n"""
    shapes = [[1] * n, [n]]
    if n > 1:
        shapes.append([n - 1, 1])                      # a last run of one
    if n >= 5000:   # boundaries on 255 / 256 / 257 and on 4 096 (tiles of the usual sizes), a last run of one
        head = [255, 1, 1, 3839, 1, 255, 2, 256, 3]
        shapes.append(head + [n - sum(head) - 1, 1])
        assert np.cumsum(head).tolist()[:4] == [255, 256, 257, 4096]
    return shapes


def keys_of_runs(rng, runs, dtype=np.uint64):
    """one random key per run (64 bits, or 32), neighbours different, repeated to the run's length (a key may come again in a later run)"""
    k = rng.integers(0, 2 ** (8 * np.dtype(dtype).itemsize), len(runs), dtype=np.uint64).astype(dtype)
    k[1:][k[1:] == k[:-1]] ^= dtype(1)
    if len(runs) > 4:
        k[4] = k[0]   # a key that comes again later is a run of its own
        if k[4] == k[3] or (len(runs) > 5 and k[4] == k[5]):
            k[4] ^= dtype(2)
    return np.repeat(k, runs), k


@gpu
def test_run_length_encode_and_reduce_by_key():
    lib = L()
    rng = np.random.default_rng(10)
    tmp = Tmp()
    for n in SIZES:
        for runs in run_shapes(n) if n <= 100003 else run_shapes(n)[1:]:
            keys, uniq = keys_of_runs(rng, runs)
            r = len(runs)
            cap = r + 8
            # run lengths
            u, c, cnt = np.full(cap, FILL[np.dtype(np.uint64)], np.uint64), np.full(cap, 0xDEADBEEF, np.uint32), np.full(1, 0xDEADBEEF, np.uint32)
            ok(lib.probe_run_length_encode_ull(tmp.h, ptr(keys), n, ptr(u), ptr(c), cap, ptr(cnt)))
            what = (n, r)
            assert int(cnt[0]) == r, what
            assert np.array_equal(u[:r], uniq) and np.array_equal(c[:r], np.array(runs, np.uint32)), what
            assert (u[r:] == FILL[np.dtype(np.uint64)]).all() and (c[r:] == 0xDEADBEEF).all(), what      # nothing behind the runs
            # ... of 32-bit keys
            keys32, uniq32 = keys_of_runs(rng, runs, np.uint32)
            u, c, cnt = np.full(cap, 0xDEADBEEF, np.uint32), np.full(cap, 0xDEADBEEF, np.uint32), np.full(1, 0xDEADBEEF, np.uint32)
            ok(lib.probe_run_length_encode_u32(tmp.h, ptr(keys32), n, ptr(u), ptr(c), cap, ptr(cnt)))
            assert int(cnt[0]) == r and np.array_equal(u[:r], uniq32) and np.array_equal(c[:r], np.array(runs, np.uint32)), what
            assert (u[r:] == 0xDEADBEEF).all() and (c[r:] == 0xDEADBEEF).all(), what
            # sums of values per run. Values below 1000 and at most 1 000 003 of them: every uint32 sum stays below 2^32.
            vals = rng.integers(0, 1000, n, dtype=np.uint64).astype(np.uint32)
            sums = Counter()
            for run, v in zip(np.repeat(np.arange(r), runs).tolist(), vals.tolist()):
                sums[run] += v
            assert max(sums.values()) < 2 ** 32
            u, s, cnt = np.full(cap, FILL[np.dtype(np.uint64)], np.uint64), np.full(cap, 0xDEADBEEF, np.uint32), np.full(1, 0xDEADBEEF, np.uint32)
            ok(lib.probe_reduce_by_key_sum_ull_u32(tmp.h, ptr(keys), ptr(vals), n, ptr(u), ptr(s), cap, ptr(cnt)))
            assert int(cnt[0]) == r, what
            assert np.array_equal(u[:r], uniq) and s[:r].tolist() == [sums[j] for j in range(r)], what
            assert (u[r:] == FILL[np.dtype(np.uint64)]).all() and (s[r:] == 0xDEADBEEF).all(), what
    # n = 0: no runs, outputs untouched
    for entry in ("rle", "rle32", "rbk"):
        u, c, cnt = np.full(8, 7, np.uint32 if entry == "rle32" else np.uint64), np.full(8, 7, np.uint32), np.full(1, 0xDEADBEEF, np.uint32)
        k0, v0 = np.zeros(1, np.uint64), np.zeros(1, np.uint32)
        if entry == "rle":
            ok(lib.probe_run_length_encode_ull(tmp.h, ptr(k0), 0, ptr(u), ptr(c), 8, ptr(cnt)))
        elif entry == "rle32":
            ok(lib.probe_run_length_encode_u32(tmp.h, ptr(v0), 0, ptr(u), ptr(c), 8, ptr(cnt)))
        else:
            ok(lib.probe_reduce_by_key_sum_ull_u32(tmp.h, ptr(k0), ptr(v0), 0, ptr(u), ptr(c), 8, ptr(cnt)))
        assert int(cnt[0]) == 0 and (u == 7).all() and (c == 7).all(), entry


# ---- the collapse of sorted items ----
BUS_RECORD = np.dtype([("barcode", "<u8"), ("umi", "<u8"), ("ec", "<i4"), ("count", "<u4"), ("flags", "<u4"), ("pad", "<u4")])
COLLAPSE_SIZES = [1, 2, 255, 256, 257, 4097]


def collapse_shapes(n):
    """lists of run lengths that sum to n: all equal, all distinct, a boundary exactly at item 255, 256, 257 (the seam of two blocks), a last run of one"""
    shapes = [[n], [1] * n] + [[b, n - b] for b in (255, 256, 257) if b < n]
    if n > 1:
        shapes.append([n - 1, 1])
    if n > 257:
        shapes.append([255, 1, 1, n - 258, 1])
    return shapes


def collapse_items(kind, rng, runs):
    """-> (the items as the probe takes them, the key of every run as `unique` holds it: shape (runs,), or (runs, 2) = (low, high) for 128 bits)"""
    if kind == "u128":
        k = rng.integers(0, 2 ** 64, (len(runs), 2), dtype=np.uint64)
        k[:, 1] = k[0, 1]                  # equal high words: the low word decides ...
        k[1::2, 0] = k[0::2, 0][:len(k[1::2])]
        k[1::2, 1] ^= np.uint64(1)         # ... and equal low words, where the high word does
        assert all((k[j] != k[j - 1]).any() for j in range(1, len(k)))
        return np.ascontiguousarray(np.repeat(k, runs, axis=0)), k
    items, k = keys_of_runs(rng, runs)
    if kind == "ull":
        return items, k
    rec = np.zeros(len(items), BUS_RECORD)   # equal barcodes with different UMIs and ecs: a run is a run of the barcode field alone
    rec["barcode"] = items
    rec["umi"] = rng.integers(0, 2 ** 62, len(items), dtype=np.uint64)
    rec["ec"] = np.arange(len(items)) % 7
    rec["count"], rec["flags"], rec["pad"] = 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF   # (nothing but the barcode may be read as a key)
    return rec, k


@gpu
@pytest.mark.parametrize("kind", ["ull", "u128", "record"])
def test_collapse_runs(kind):
    """sorted items -> unique[runs], start[runs + 1] with start[runs] = n, heads and pos = the flags and their scan; nothing behind what is written;
    the null-start form writes the same unique and leaves start alone"""
    entry = getattr(L(), "probe_collapse_runs_" + kind)
    rng = np.random.default_rng(14)
    tmp = Tmp()
    width = 2 if kind == "u128" else 1
    for n in COLLAPSE_SIZES:
        for runs in collapse_shapes(n):
            items, uniq = collapse_items(kind, rng, runs)
            r, cap = len(runs), len(runs) + 8
            want_start = np.concatenate([[0], np.cumsum(runs)]).astype(np.uint32)
            want_heads = np.zeros(n, np.uint32)
            want_heads[want_start[:-1]] = 1
            for with_start in (1, 0):
                heads, pos = filled(n, np.uint32), filled(n, np.uint32)
                unique, start, cnt = np.full(cap * width, FILL[np.dtype(np.uint64)], np.uint64), np.full(cap + 1, 0xDEADBEEF, np.uint32), np.full(1, 0xDEADBEEF, np.uint32)
                ok(entry(tmp.h, ptr(items), n, ptr(heads), ptr(pos), ptr(unique), ptr(start), cap, with_start, ptr(cnt)))
                what = (kind, n, r, with_start)
                assert int(cnt[0]) == r, what
                assert np.array_equal(heads[:n], want_heads) and np.array_equal(pos[:n], np.cumsum(want_heads, dtype=np.uint32)), what
                assert (heads[n:] == 0xDEADBEEF).all() and (pos[n:] == 0xDEADBEEF).all(), what
                assert np.array_equal(unique[: r * width].reshape(uniq.shape), uniq) and (unique[r * width:] == FILL[np.dtype(np.uint64)]).all(), what
                if with_start:
                    assert np.array_equal(start[: r + 1], want_start) and int(start[r]) == n and (start[r + 1:] == 0xDEADBEEF).all(), what
                else:
                    assert (start == 0xDEADBEEF).all(), what


# ---- selection ----
@gpu
def test_select_flagged_indices():
    lib = L()
    rng = np.random.default_rng(11)
    tmp = Tmp()
    for n in [0] + SIZES:
        cases = {"none": np.zeros(n, np.uint32), "all": np.ones(n, np.uint32), "random": (rng.random(n) < 0.3).astype(np.uint32)}
        if n:
            first, last = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
            first[0], last[-1] = 1, 1
            odd = np.where(rng.random(n) < 0.5, rng.choice(np.array([0x80000000, 2, 0xFFFFFFFF, 256], np.uint32), n), 0).astype(np.uint32)
            odd[-1] = 0x80000000
            cases.update(first=first, last=last, not_one=odd)   # a flag is "not zero", whatever its bits
        for what, flags in cases.items():
            want = np.flatnonzero(flags).astype(np.uint32)
            cap = n + 4
            out, cnt = np.full(cap, 0xDEADBEEF, np.uint32), np.full(1, 0xDEADBEEF, np.uint32)
            ok(lib.probe_select_flagged_indices_u32(tmp.h, ptr(flags) if n else ptr(np.zeros(1, np.uint32)), n, ptr(out), cap, ptr(cnt)))
            assert int(cnt[0]) == len(want), (what, n)
            assert np.array_equal(out[:len(want)], want) and (out[len(want):] == 0xDEADBEEF).all(), (what, n)


# ---- the scratch of a chain of operations ----
@gpu
def test_scratch_chain_never_shrinks():
    lib = L()
    rng = np.random.default_rng(12)
    tmp = Tmp()
    assert tmp.size() == 0
    small = rng.integers(0, 1000, 100, dtype=np.uint64).astype(np.uint32)
    n = 1000003
    low = rng.integers(0, 5000, n, dtype=np.uint64)
    keys = low | ((low * np.uint64(2654435761) & np.uint64(0xFFFFF)) << np.uint64(40))   # bits above the sorted 13: a function of the low ones,
    assert len(np.unique(keys)) == len(np.unique(low)) <= 5000                         # so the sorted keys have at most 5 000 runs (cap 5 008)
    s1, s2, sorted_ = filled(100, np.uint32), filled(100, np.uint32), filled(n, np.uint64)
    cap = 5008
    u, c, cnt = np.full(cap, FILL[np.dtype(np.uint64)], np.uint64), np.full(cap, 0xDEADBEEF, np.uint32), np.full(1, 0xDEADBEEF, np.uint32)
    sizes = np.zeros(4, np.uint64)
    ok(lib.probe_chain(tmp.h, ptr(small), 100, ptr(s1), ptr(s2), ptr(keys), ptr(sorted_), n, 13, ptr(u), ptr(c), cap, ptr(cnt), ptr(sizes)))
    sizes = sizes.tolist()
    assert sizes[0] > 0 and sizes[1] > sizes[0] and sizes[2] == sizes[1] and sizes[3] >= sizes[2] and tmp.size() == sizes[3], sizes
    want_scan = scan_reference(small, np.uint32, False)
    assert np.array_equal(s1[:100], want_scan) and np.array_equal(s2[:100], want_scan) and (s1[100:] == 0xDEADBEEF).all()
    order = np.argsort(keys & np.uint64(0x1FFF), kind="stable")
    assert np.array_equal(sorted_[:n], keys[order]) and (sorted_[n:] == FILL[np.dtype(np.uint64)]).all()
    full = keys[order]
    starts = np.flatnonzero(np.concatenate([[True], full[1:] != full[:-1]]))
    r = len(starts)
    assert int(cnt[0]) == r <= 5000
    assert np.array_equal(u[:r], full[starts]) and np.array_equal(c[:r], np.diff(np.concatenate([starts, [n]])).astype(np.uint32))
    assert (u[r:] == FILL[np.dtype(np.uint64)]).all() and (c[r:] == 0xDEADBEEF).all()
    # a second chain on the same scratch: smaller requests leave it as it is
    before = tmp.size()
    out = filled(100, np.uint32)
    ok(lib.probe_scan_exclusive_u32_u32(tmp.h, ptr(small), ptr(out), 100))
    assert tmp.size() == before and np.array_equal(out[:100], want_scan)
