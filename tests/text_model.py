"""Independent model of the text kernels of process_reads (csrc/fastq_scan.hip, csrc/render.hip): pure Python / numpy, no product code and
none of the kernels' arithmetic. Written from what the reference does with a record (src/pseudoaligner.rs:430-461, :490, bio 1.5's
fastq::Record) and from the buffers' contracts in csrc/kernels.hpp:

  scan    the lines of text[begin, end) by bytes.split; four lines to a record; record.id() = header[1..].trim_end().splitn(2, ' ').next():
          drop the first byte, strip trailing White_Space (its ASCII members: 0x09-0x0D and 0x20), cut at the first 0x20; record.seq() = the
          second line without one trailing CR
  encode  DnaString::from_dna_string (:450): 2 bits per base, A=0 C=1 G=2 T=3 in either case, anything else 0, in tiles of 64 reads
  render  println!("{:?}", (flag, id, class, coverage)) (:455-461, :490) with `impl Debug for str` restated for bytes < 0x80

tests/test_text_model.py pins the model itself; tests/test_gpu_text_kernels.py compares the kernels with it."""
import numpy as np

WHITE_SPACE = bytes([0x09, 0x0A, 0x0B, 0x0C, 0x0D, 0x20])   # the ASCII members of Unicode's White_Space: what str::trim_end strips
RESULT_DTYPE = np.dtype([("coverage", "<u4"), ("mismatches", "<u4"), ("class_off", "<u4"), ("class_len", "<u4")])   # pa_read_result
MAPPED_BIT = 0x80000000     # PA_MAPPED_BIT (mismatches)
CLASS_REF = 0x80000000      # PA_CLASS_REF (class_off)
COVERAGE_THRESHOLD = 32     # PA_READ_COVERAGE_THRESHOLD (src/config.rs:16)
FLAG_BUCKETS = 64           # PA_RENDER_FLAG_BUCKETS
FLAG_BUCKET_READS = 1000000


def record_id(header: bytes) -> bytes:
    """bio 1.5's Record::id() of a header line (without its line break): header[1..].trim_end().splitn(2, ' ').next()"""
    return header[1:].rstrip(WHITE_SPACE).split(b" ", 1)[0]


def record_seq(line: bytes) -> bytes:
    return line[:-1] if line.endswith(b"\r") else line


def scan(text, begin, end, cap_lines=None, cap_recs=None):
    """The records of text[begin, end). -> dict(lines, n, consumed, line_start, recs, max_seq, odd, overflow): line_start[l] = where line l
    starts, counted from `begin` (lines + 1 entries: the last is the position behind the last line break); recs[r] = (id_off, id_len,
    seq_off, seq_len) with offsets into `text`; consumed = the position behind the last whole record, from `begin` (0 without a record);
    overflow: a line table of cap_lines entries does not hold lines + 1 starts, or n records do not fit cap_recs."""
    win = bytes(text[begin:end])
    parts = win.split(b"\n")
    lines = len(parts) - 1
    line_start = [0]
    for p in parts[:-1]:
        line_start.append(line_start[-1] + len(p) + 1)
    n = lines // 4
    recs, odd, max_seq = [], False, 0
    for r in range(n):
        header, seq_line, plus = parts[4 * r], parts[4 * r + 1], parts[4 * r + 2]
        rid, seq = record_id(header), record_seq(seq_line)
        recs.append((begin + line_start[4 * r] + 1, len(rid), begin + line_start[4 * r + 1], len(seq)))
        odd = odd or not header.startswith(b"@") or not plus.startswith(b"+")
        max_seq = max(max_seq, len(seq))
    overflow = (cap_lines is not None and lines + 1 > cap_lines) or (cap_recs is not None and n > cap_recs)
    return dict(lines=lines, n=n, consumed=line_start[4 * n] if n else 0, line_start=np.array(line_start, np.uint32),
                recs=np.array(recs, np.uint32).reshape(n, 4), max_seq=max_seq, odd=int(odd), overflow=int(overflow))


_CODE = {ord("C"): 1, ord("c"): 1, ord("G"): 2, ord("g"): 2, ord("T"): 3, ord("t"): 3}


def encode(seqs, wpr):
    """-> (tiles, lens): tiles[(tile * wpr + w) * 64 + r] = word w of read 64 * tile + r, base j of a read in bits [2 (j % 32), 2 (j % 32) + 2)
    of word j // 32; a read longer than 32 * wpr bases is cut there (lens holds the cut length); lanes beyond the last read are zero"""
    n = len(seqs)
    tiles = [0] * (((n + 63) // 64) * wpr * 64)
    lens = np.zeros(n, np.uint32)
    for i, s in enumerate(seqs):
        s = bytes(s)[: 32 * wpr]
        lens[i] = len(s)
        for j, c in enumerate(s):
            tiles[((i // 64) * wpr + j // 32) * 64 + i % 64] |= _CODE.get(c, 0) << (2 * (j % 32))
    return np.array(tiles, np.uint64), lens


def escape_debug(rid: bytes) -> bytes:
    """what `impl Debug for str` prints between the quotes, for bytes < 0x80: \\t \\r \\n \\\\ \\" \\0 by name, the other control bytes (< 0x20 and
    0x7f) as \\u{hex} without leading zeros, everything else — the apostrophe too — as it is. Bytes >= 0x80 are copied (a
    documented limitation, pinned as documented)."""
    named = {0x09: b"\\t", 0x0D: b"\\r", 0x0A: b"\\n", 0x5C: b"\\\\", 0x22: b'\\"', 0x00: b"\\0"}
    out = bytearray()
    for c in bytes(rid):
        if c in named:
            out += named[c]
        elif c < 0x20 or c == 0x7F:
            out += b"\\u{%x}" % c
        else:
            out.append(c)
    return bytes(out)


def render(results, arena, arena_cap, ids, cls_text, flag_mark):
    """-> (lines, flagged): lines[i] = the bytes of read i's tuple with its line break, flagged[j] = the flagged reads of bucket j (bucket 0:
    the reads before flag_mark, bucket j: the j-th million behind them, the last bucket: everything beyond). results: RESULT_DTYPE;
    cls_text[c] = index class c as "1, 5, 9"; a class in the arena that does not lie inside arena_cap entries is printed empty."""
    lines, flagged = [], [0] * FLAG_BUCKETS
    for i in range(len(results)):
        cov, mm, off, cl = (int(results[i][f]) for f in ("coverage", "mismatches", "class_off", "class_len"))
        mapped = bool(mm & MAPPED_BIT)
        flag = mapped and cov >= COVERAGE_THRESHOLD and cl == 0
        if off & CLASS_REF:
            cls = bytes(cls_text[off & ~CLASS_REF])
        elif off + cl <= arena_cap:
            cls = b", ".join(b"%d" % int(x) for x in arena[off:off + cl])
        else:
            cls = b""
        lines.append(b'(%s, "%s", [%s], %d)\n' % (b"true" if flag else b"false", escape_debug(ids[i]), cls, cov if mapped else 0))
        if flag:
            flagged[0 if i < flag_mark else min(FLAG_BUCKETS - 1, 1 + (i - flag_mark) // FLAG_BUCKET_READS)] += 1
    return lines, flagged
