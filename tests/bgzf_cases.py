"""BGZF test vectors, pure Python (zlib and struct only; no product code): a BGZF writer over zlib.compressobj, a bit writer for
hand-assembled DEFLATE payloads, the valid / corrupt / not-BGZF case lists of tests/test_bgzf_cases.py and tests/test_gpu_inflate.py, a
Python walk of the member headers, and zlib's verdict on a member (the yardstick: a member is good exactly when zlib.decompressobj(-15)
inflates its payload with eof true, no unused data, ISIZE bytes and the trailer's CRC-32)."""
import functools
import random
import struct
import zlib

EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


# ------------------------------------------------------------------ writer ----
def member(payload: bytes, isize: int, crc: int, extra_before: bytes = b"", flg_extra: int = 0, name: bytes = b"") -> bytes:
    """one BGZF member around a raw DEFLATE payload; extra_before: other subfields in front of BC; name: FNAME (flg_extra |= 8)"""
    xlen = len(extra_before) + 6
    tail = name
    total = 12 + xlen + len(tail) + len(payload) + 8
    assert total <= 65536, total
    head = struct.pack("<BBBBIBBH", 0x1f, 0x8b, 8, 4 | flg_extra, 0, 0, 0xff, xlen) + extra_before + b"BC" + struct.pack("<HH", 2, total - 1)
    return head + tail + payload + struct.pack("<II", crc & 0xFFFFFFFF, isize & 0xFFFFFFFF)


def deflate(text: bytes, level: int = 6, strategy: int = zlib.Z_DEFAULT_STRATEGY) -> bytes:
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    return c.compress(text) + c.flush()


def good_member(text: bytes, level: int = 6, strategy: int = zlib.Z_DEFAULT_STRATEGY, **kw) -> bytes:
    return member(deflate(text, level, strategy), len(text), zlib.crc32(text), **kw)


def raw_member(payload: bytes, text: bytes, **kw) -> bytes:
    """a hand-assembled payload with the header and trailer of the text it is meant to give"""
    return member(payload, len(text), zlib.crc32(text), **kw)


def bgzf(text: bytes, chunk: int = 65280, level: int = 6, strategy: int = zlib.Z_DEFAULT_STRATEGY, eof: bool = True) -> bytes:
    out = b"".join(good_member(text[i:i + chunk], level, strategy) for i in range(0, len(text), chunk))
    return out + (EOF_BLOCK if eof else b"")


def bgzf_chunks(chunks, level: int = 6, eof: bool = True) -> bytes:
    """members of the given texts (sizes chosen by hand)"""
    return b"".join(good_member(c, level) for c in chunks) + (EOF_BLOCK if eof else b"")


# -------------------------------------------------------------- bit writer ----
class Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def bits(self, value: int, n: int):
        """n bits of value, least significant first (how DEFLATE packs everything but Huffman codes)"""
        assert 0 <= value < (1 << n) or n == 0
        self.acc |= value << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8
        return self

    def code(self, code: int, n: int):
        """a Huffman code: most significant bit first"""
        for i in range(n - 1, -1, -1):
            self.bits((code >> i) & 1, 1)
        return self

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)
        return self

    def raw(self, data: bytes):
        assert self.n == 0
        self.out += data
        return self

    def done(self) -> bytes:
        return bytes(self.align().out)


def canon(lens):
    """canonical codes (RFC 1951 3.2.2): {symbol: (code, length)}"""
    count = [0] * 16
    for l in lens:
        count[l] += 1
    count[0] = 0
    code, nxt = 0, [0] * 16
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = {}
    for s, l in enumerate(lens):
        if l:
            out[s] = (nxt[l], l)
            nxt[l] += 1
    return out


LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
FIXED_LIT = canon([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
FIXED_DIST = canon([5] * 32)


def len_sym(length):
    for s in range(28, -1, -1):
        if LEN_BASE[s] <= length and (s == 28 or length < LEN_BASE[s] + (1 << LEN_EXTRA[s])):
            if s == 28 and length != 258:
                continue
            return 257 + s, LEN_EXTRA[s], length - LEN_BASE[s]
    raise ValueError(length)


def dist_sym(d):
    for s in range(29, -1, -1):
        if DIST_BASE[s] <= d:
            return s, DIST_EXTRA[s], d - DIST_BASE[s]
    raise ValueError(d)


class Block:
    """symbols of one Huffman block written through code tables {symbol: (code, length)}"""

    def __init__(self, w: Bits, lit, dist):
        self.w, self.lit, self.dist = w, lit, dist

    def sym(self, s):
        self.w.code(*self.lit[s])
        return self

    def lits(self, data: bytes):
        for b in data:
            self.sym(b)
        return self

    def match(self, length, d, via284=False):
        if via284:
            assert length == 258
            s, eb, ev = 284, 5, 31
        else:
            s, eb, ev = len_sym(length)
        self.sym(s)
        self.w.bits(ev, eb)
        ds, deb, dev = dist_sym(d)
        self.w.code(*self.dist[ds])
        self.w.bits(dev, deb)
        return self

    def dsym_raw(self, ds):
        self.w.code(*self.dist[ds])
        return self

    def eob(self):
        return self.sym(256)


def fixed(w: Bits, final=1) -> Block:
    w.bits(final, 1).bits(1, 2)
    return Block(w, FIXED_LIT, FIXED_DIST)


def stored(w: Bits, data: bytes, final=1, nlen=None):
    w.bits(final, 1).bits(0, 2).align()
    w.raw(struct.pack("<HH", len(data), (len(data) ^ 0xFFFF) if nlen is None else nlen) + data)
    return w


# the code-length code every hand-made dynamic block uses: complete (13 codes of 4 bits, 6 of 5), all 19 lengths sent
CL_LENS = [4] * 13 + [5] * 6
CL_CODE = canon(CL_LENS)
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
CL_EXTRA = {16: 2, 17: 3, 18: 7}


def dynamic(w: Bits, nlen, ndist, seq, final=1, lit_lens=None, dist_lens=None) -> Block:
    """header of a dynamic block: seq = the code-length symbols as written, (symbol, extra value) for 16 / 17 / 18, plain ints otherwise.
    lit_lens / dist_lens: what seq expands to (for the codes of the symbols that follow)"""
    w.bits(final, 1).bits(2, 2).bits(nlen - 257, 5).bits(ndist - 1, 5).bits(19 - 4, 4)
    for s in CL_ORDER:
        w.bits(CL_LENS[s], 3)
    for item in seq:
        s, ev = item if isinstance(item, tuple) else (item, None)
        w.code(*CL_CODE[s])
        if s >= 16:
            w.bits(ev, CL_EXTRA[s])
    return Block(w, canon(lit_lens) if lit_lens else {}, canon(dist_lens) if dist_lens else {})


def expand(seq):
    out = []
    for item in seq:
        s, ev = item if isinstance(item, tuple) else (item, None)
        if s < 16:
            out.append(s)
        elif s == 16:
            out += [out[-1]] * (3 + ev)
        elif s == 17:
            out += [0] * (3 + ev)
        else:
            out += [0] * (11 + ev)
    return out


def zeros(n):
    """n zero lengths as 18 / 17 runs and single zeros"""
    out = []
    while n >= 11:
        r = min(n, 138)
        out.append((18, r - 11))
        n -= r
    if n >= 3:
        out.append((17, n - 3))
        n = 0
    return out + [0] * n


def simple_dynamic(w: Bits, lit: dict, dist_lens, final=1, nlen=None) -> Block:
    """dynamic block whose literal/length lengths are given as {symbol: length} and sent as plainly as possible"""
    nlen = nlen or max(257, max(lit) + 1)
    seq, at = [], 0
    for s in sorted(lit):
        seq += zeros(s - at) + [lit[s]]
        at = s + 1
    seq += zeros(nlen - at) + list(dist_lens)
    lens = expand(seq)
    assert len(lens) == nlen + len(dist_lens)
    return dynamic(w, nlen, len(dist_lens), seq, final, lens[:nlen], lens[nlen:])


# ------------------------------------------------------------------- texts ----
def fastq_like(n_bytes: int, seed: int = 1) -> bytes:
    rng = random.Random(seed)
    out = bytearray()
    i = 0
    while len(out) < n_bytes:
        seq = "".join(rng.choice("ACGT") for _ in range(rng.randint(90, 151)))
        qual = "".join(rng.choice("#5AF") * rng.randint(1, 12) for _ in range(40))[:len(seq)]
        out += ("@SIM:%d:%d extra\n%s\n+\n%s\n" % (seed, i, seq, qual)).encode()
        i += 1
    return bytes(out[:n_bytes])


def fibonacci_text() -> bytes:
    """symbol weights 1, 1, 2, 3, 5, ...: the Huffman code of Z_HUFFMAN_ONLY reaches zlib's 15-bit limit"""
    a, b, out = 1, 1, bytearray()
    for s in range(21):
        out += bytes([65 + s]) * a
        a, b = b, a + b
    rng = random.Random(5)
    lst = list(out)
    rng.shuffle(lst)
    return bytes(lst)


# ------------------------------------------------------------- valid cases ----
def _hand_valid():
    """(name, payload, text) of the hand-assembled members"""
    cases = []
    w = Bits(); simple_dynamic(w, {65: 1, 256: 1}, [1]).eob()
    cases.append(("dynamic block that is only end-of-block", w.done(), b""))
    w = Bits(); simple_dynamic(w, {256: 1}, [0]).eob()
    cases.append(("single literal/length code of one bit, no distance code", w.done(), b""))
    w = Bits(); simple_dynamic(w, {97: 2, 98: 2, 256: 2, 257: 2}, [1]).lits(b"ab").match(3, 1).eob()
    cases.append(("one distance code of one bit", w.done(), b"abbbb"))
    w = Bits(); simple_dynamic(w, {120: 1, 256: 1}, [0]).lits(b"xxx").eob()
    cases.append(("HDIST = 1 with length 0", w.done(), b"xxx"))
    # 16 across the literal/distance seam: ... 256: 2, 257: 2, then 16 x 4 gives the four distance lengths
    seq = zeros(97) + [2, 2] + zeros(157) + [2, 2, (16, 1)]
    lens = expand(seq)
    assert len(lens) == 262 and lens[258:] == [2, 2, 2, 2]
    w = Bits(); dynamic(w, 258, 4, seq, 1, lens[:258], lens[258:]).lits(b"ab").match(3, 2).eob()
    cases.append(("repeat 16 across the literal/distance seam", w.done(), b"ababa"))
    seq = [(17, 7), (18, 127), 1, (18, 96), 1, 0]
    lens = expand(seq)
    assert len(lens) == 258 and lens[148] == 1 and lens[256] == 1
    w = Bits(); dynamic(w, 257, 1, seq, 1, lens[:257], lens[257:]).lits(bytes([148]) * 3).eob()
    cases.append(("17 and 18 at maximum run", w.done(), bytes([148]) * 3))
    w = Bits(); fixed(w).lits(b"abc").match(3, 3).eob()
    cases.append(("match length 3", w.done(), b"abcabc"))
    w = Bits(); fixed(w).lits(b"xy").match(258, 2).eob()
    cases.append(("length 258 via symbol 285", w.done(), b"xy" * 130))
    w = Bits(); fixed(w).lits(b"xy").match(258, 2, via284=True).eob()
    cases.append(("length 258 via 284 + 31", w.done(), b"xy" * 130))
    w = Bits(); fixed(w).lits(b"a").match(258, 1).match(258, 1).lits(b"b").match(7, 1).eob()
    cases.append(("distance 1 with length 258", w.done(), b"a" * 517 + b"b" * 8))
    rnd = random.Random(11).randbytes(32768)
    w = Bits(); stored(w, rnd, 0); fixed(w).match(10, 32768).lits(b"!").match(258, 32768).eob()
    t = bytearray(rnd)
    for ln in (10, 1, 258):
        if ln == 1:
            t += b"!"
        else:
            for _ in range(ln):
                t.append(t[-32768])
    cases.append(("distance 32768 exactly, back into a stored block", w.done(), bytes(t)))
    w = Bits(); fixed(w).lits(b"abcd").match(4, 4).eob()
    cases.append(("distance equal to the bytes produced so far", w.done(), b"abcdabcd"))
    w = Bits(); fixed(w, 0).lits(b"hello").eob(); fixed(w).match(5, 5).match(9, 3).eob()
    cases.append(("match across a block boundary", w.done(), b"hellohello" + b"llollollo"))
    w = Bits(); fixed(w, 0).lits(b"Q").eob(); stored(w, b"stored bytes", 0); fixed(w).match(6, 12).eob()
    cases.append(("stored after a block that ended mid-byte", w.done(), b"Qstored bytes" + b"stored"))
    return cases


def _flush_payload(parts, mode):
    c = zlib.compressobj(6, zlib.DEFLATED, -15, 9)
    out = b""
    for p in parts[:-1]:
        out += c.compress(p) + c.flush(mode)
    return out + c.compress(parts[-1]) + c.flush()


@functools.lru_cache(None)
def valid_cases():
    """[(name, file bytes, text)]"""
    fq = fastq_like(200000, 3)
    rnd = random.Random(21).randbytes(65000)   # (os.urandom's kind of bytes, the same ones every run)
    cases = []
    add = lambda name, data, text: cases.append((name, data, text))
    add("empty member first, middle and last", EOF_BLOCK + good_member(b"abc") + EOF_BLOCK + good_member(b"defg") + EOF_BLOCK, b"abcdefg")
    add("no EOF block", bgzf(fq[:3000], 1000, eof=False), fq[:3000])
    sizes = [1, 2, 3, 5, 63, 64, 65, 65280, 65536, 1, 65, 3]
    chunks, at = [], 0
    big = fq + b"A" * 65536
    for s in sizes:
        chunks.append(b"A" * 65536 if s == 65536 else big[at:at + s])
        at += s
    add("ISIZE 1 .. 65536 interleaved", bgzf_chunks(chunks), b"".join(chunks))
    add("level 0 (stored)", member(deflate(rnd, 0), len(rnd), zlib.crc32(rnd)) + good_member(fq[:100], 0) + EOF_BLOCK, rnd + fq[:100])
    for mode, nm in ((zlib.Z_SYNC_FLUSH, "Z_SYNC_FLUSH"), (zlib.Z_FULL_FLUSH, "Z_FULL_FLUSH")):
        parts = [fq[:700], fq[700:1500], fq[500:2500]]
        t = b"".join(parts)
        add("empty stored block between compressed ones (%s)" % nm, raw_member(_flush_payload(parts, mode), t) + EOF_BLOCK, t)
    hi = bytes((i * 7 + 3) % 256 for i in range(3000)) + bytes(range(144, 256)) * 3
    add("Z_FIXED with literals >= 144", bgzf(hi, 2000, 6, zlib.Z_FIXED), hi)
    fib = fibonacci_text()
    add("Z_HUFFMAN_ONLY, 15-bit codes", bgzf(fib, 65280, 6, zlib.Z_HUFFMAN_ONLY), fib)
    rle = b"".join(bytes([65 + i % 7]) * (1 + (i * 37) % 300) for i in range(200))
    add("Z_RLE", bgzf(rle, 65280, 6, zlib.Z_RLE), rle)
    for lvl in (1, 9):
        add("level %d, FASTQ-like" % lvl, bgzf(fq, 65280, lvl), fq)
        add("level %d, random bytes" % lvl, bgzf(rnd, 30000, lvl), rnd)
    hand = _hand_valid()
    add("hand-assembled members", b"".join(raw_member(p, t) for _, p, t in hand) + EOF_BLOCK, b"".join(t for _, _, t in hand))
    for n in (1, 63, 64, 65):
        add("%d members" % n, bgzf(fq[:n * 50], 50, eof=False), fq[:n * 50])
    add("more members than the grid", bgzf(fq[:2100 * 9], 9, 1, eof=False), fq[:2100 * 9])
    other = b"XY" + struct.pack("<H", 5) + b"hello"
    add("BC behind another subfield", good_member(fq[:500], extra_before=other) + good_member(fq[500:900], extra_before=other + other) + EOF_BLOCK, fq[:900])
    return cases


def hand_valid_names():
    return [n for n, _, _ in _hand_valid()]


# ----------------------------------------------------------- corrupt cases ----
@functools.lru_cache(None)
def corrupt_cases():
    """[(name, file bytes, index of the corrupt member, [text of member 0, None, text of member 2])]: one corrupt member between two good neighbours
    of awkward sizes"""
    left, right = fastq_like(777, 8), fastq_like(1301, 9)
    good = deflate(b"some text that is good, some text that is good\n" * 5)
    good_text = b"some text that is good, some text that is good\n" * 5
    out = []

    def add(name, bad_member):
        out.append((name, good_member(left) + bad_member + good_member(right) + EOF_BLOCK, 1, [left, None, right]))

    def claim(payload, text=b"abcabc"):
        return raw_member(payload, text)

    add("block type 3", claim(Bits().bits(1, 1).bits(3, 2).done()))
    add("stored NLEN wrong", claim(stored(Bits(), b"abcabc", 1, nlen=0x1234).done()))
    w = Bits(); simple_dynamic(w, {97: 1, 98: 1, 256: 1}, [1]).lits(b"ab").eob()
    add("over-subscribed code lengths", claim(w.done(), b"ab"))
    w = Bits(); simple_dynamic(w, {97: 2, 256: 2}, [1]).lits(b"a").eob()
    add("incomplete code with maximum length > 1", claim(w.done(), b"a"))
    w = Bits(); b = simple_dynamic(w, {97: 1, 98: 1}, [1]); b.lits(b"ab"); w.bits(0, 16)
    add("EOB code missing", claim(w.done(), b"ab"))
    seq = [(16, 0)] + [0] * 253 + [1] + [1, 1]
    w = Bits(); dynamic(w, 257, 1, seq); w.bits(0, 16)
    add("code 16 first", claim(w.done(), b""))
    seq = zeros(97) + [1] + zeros(158) + [1, (18, 127)]
    w = Bits(); dynamic(w, 257, 1, seq); w.bits(0, 16)
    add("repeat running past HLIT + HDIST", claim(w.done(), b"a"))
    w = Bits(); fixed(w).lits(b"abc").sym(286).eob()
    add("fixed-block symbol 286", claim(w.done(), b"abc"))
    w = Bits(); b = fixed(w).lits(b"abc").sym(257); b.dsym_raw(30); w.bits(0, 13); b.eob()
    add("distance symbol 30", claim(w.done()))
    w = Bits(); fixed(w).lits(b"abc").match(3, 4).eob()
    add("distance one beyond the produced bytes", claim(w.done()))
    add("payload cut one byte short", raw_member(good[:-1], good_text))
    add("payload with one byte too many", raw_member(good + b"\x00", good_text))
    add("ISIZE one too large", member(good, len(good_text) + 1, zlib.crc32(good_text)))
    add("ISIZE one too small", member(good, len(good_text) - 1, zlib.crc32(good_text)))
    add("one flipped bit in the CRC", member(good, len(good_text), zlib.crc32(good_text) ^ 0x00400000))
    st = bytearray(stored(Bits(), good_text).done())
    st[40] ^= 0x20
    add("one flipped literal", raw_member(bytes(st), good_text))
    return out


# the status (a PA_INFLATE_* name of include/pseudoaligner_amd.h without its prefix) each corrupt member must end with
EXPECTED_STATUS = {"block type 3": "BAD_BLOCK_TYPE", "stored NLEN wrong": "STORED_LEN", "over-subscribed code lengths": "BAD_CODE_LENGTHS",
                   "incomplete code with maximum length > 1": "BAD_CODE_LENGTHS", "EOB code missing": "NO_END_OF_BLOCK", "code 16 first": "BAD_REPEAT",
                   "repeat running past HLIT + HDIST": "BAD_REPEAT", "fixed-block symbol 286": "BAD_SYMBOL", "distance symbol 30": "BAD_SYMBOL",
                   "distance one beyond the produced bytes": "DISTANCE_TOO_FAR", "payload cut one byte short": "INPUT_EXHAUSTED",
                   "payload with one byte too many": "TRAILING_INPUT", "ISIZE one too large": "OUTPUT_TOO_SHORT", "ISIZE one too small": "OUTPUT_TOO_LONG",
                   "one flipped bit in the CRC": "CRC_MISMATCH", "one flipped literal": "CRC_MISMATCH"}


# ---------------------------------------------------------- not-BGZF files ----
@functools.lru_cache(None)
def not_bgzf_cases():
    import gzip
    import io
    fq = fastq_like(5000, 4)
    plain = gzip.compress(fq)
    buf = io.BytesIO()
    with gzip.GzipFile(filename="reads.fq", mode="wb", fileobj=buf) as g:
        g.write(fq)
    named = buf.getvalue()
    ok = bgzf(fq, 2000)
    m = good_member(fq[:100])
    beyond = bytearray(m + EOF_BLOCK)
    struct.pack_into("<H", beyond, 16, len(beyond) + 5)   # BSIZE of the first member points past the end
    bc3 = struct.pack("<BBBBIBBH", 0x1f, 0x8b, 8, 4, 0, 0, 0xff, 7) + b"BC" + struct.pack("<H", 3) + b"\x00\x00\x00" + deflate(b"x") + struct.pack("<II", zlib.crc32(b"x"), 1)
    return [("ordinary gzip", plain), ("gzip with FNAME only", named), ("last member truncated", ok[:-40]), ("BSIZE beyond the end", bytes(beyond)),
            ("BC length != 2", bc3 + EOF_BLOCK), ("first member BGZF, second ordinary", m + plain), ("no bytes", b"")]


# ------------------------------------------------- Python walk and verdict ----
def walk(data: bytes):
    """the member table as a list of dicts (in_off, out_off, file_off, in_len, out_len, crc32), or None when the bytes are not BGZF"""
    rows, at, text = [], 0, 0
    if not data:
        return None
    while at < len(data):
        if len(data) - at < 26 or data[at:at + 3] != b"\x1f\x8b\x08":
            return None
        flg = data[at + 3]
        if not flg & 4 or flg & 0xE0:
            return None
        xlen = struct.unpack_from("<H", data, at + 10)[0]
        ex = data[at + 12:at + 12 + xlen]
        if len(ex) != xlen:
            return None
        bsize, x = None, 0
        while x < xlen:
            if xlen - x < 4:
                return None
            slen = struct.unpack_from("<H", ex, x + 2)[0]
            if x + 4 + slen > xlen:
                return None
            if ex[x:x + 2] == b"BC":
                if slen != 2:
                    return None
                if bsize is None:
                    bsize = struct.unpack_from("<H", ex, x + 4)[0]
            x += 4 + slen
        if bsize is None or at + bsize + 1 > len(data):
            return None
        blk = data[at:at + bsize + 1]
        p = 12 + xlen
        for bit in (8, 16):
            if flg & bit:
                z = blk.find(b"\0", p)
                if z < 0:
                    return None
                p = z + 1
        if flg & 2:
            p += 2
        if p + 8 > len(blk):
            return None
        crc, isize = struct.unpack_from("<II", blk, len(blk) - 8)
        if isize > 65536:
            return None
        rows.append(dict(in_off=at + p, out_off=text, file_off=at, in_len=len(blk) - 8 - p, out_len=isize, crc32=crc))
        text += isize
        at += len(blk)
    return rows


def zlib_verdict(payload: bytes, isize: int, crc: int):
    """(accepted, text or None) by the rule in the module docstring"""
    d = zlib.decompressobj(-15)
    try:
        text = d.decompress(payload)
    except zlib.error:
        return False, None
    ok = d.eof and not d.unused_data and len(text) == isize and zlib.crc32(text) == crc
    return ok, text if ok else None
