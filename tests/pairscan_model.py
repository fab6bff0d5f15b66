"""A pure-Python model of the pair scan (csrc/pair_scan.hip, pa_pairs_gather_device): record i of an R1 text against record i of an R2
text. The rules are the ones the host's pair reader applies per pair (csrc/pair_reader.cpp: HostPairReader::gather, with pair_id_len of csrc/fastq_text.hpp):

  id          record.id() with a trailing "/1" or "/2" cut, when the id has at least two bytes ("/1" alone becomes empty, "/3" stays)
  first bad   the smallest batch position whose two cut ids differ in length or in a byte
  lengths     len2 = the R2 sequence's length, len1 = min(the R1 sequence's length, prefix); prefix 0xFFFFFFFF keeps all of R1
  bytes       the pieces back to back, offsets[i] = the bytes of the pieces before i, offsets[n] = all of them, continued across the
              segments of a batch
  maxima      the longest piece of each mate

and two rules that only the device entry point has: a record row that points outside its text gives two empty pieces (first outside = its
batch position), and a piece that would end beyond the capacity of its output is not written while the byte counts still include it.

The id rule is the inline function pair_id_len (csrc/fastq_text.hpp): tests/pairplan/pairplan_check.cpp runs the product's own function over the id
cases that tests/test_pairscan_model.py pins this model on. The gather sits in an unnamed namespace of the library and cannot be called from a test:
agreement with it is established on the GPU tier, in two steps: the kernels equal this model bit for bit (tests/test_gpu_pairscan_edges.py), and the
drivers on the device path equal the same call on the host path, which is HostPairReader::gather (tests/test_gpu_pairs_ingest.py)."""

WHOLE_READ = 0xFFFFFFFF
NONE = 0xFFFFFFFFFFFFFFFF
CTL_NAMES = ("first_bad", "max_len1", "max_len2", "bytes1", "bytes2", "first_outside")


def cut_id(ident: bytes) -> bytes:
    if len(ident) >= 2 and ident[-2:] in (b"/1", b"/2"):
        return ident[:-2]
    return ident


class Batch:
    """the outputs of a batch as pa_pairs_gather_device leaves them: bytes (pre-filled with `canary`), offsets, the control block"""

    def __init__(self, cap1: int, cap2: int, n_off: int, canary: int = 0xEE):
        self.bytes1, self.bytes2 = bytearray([canary]) * cap1, bytearray([canary]) * cap2
        self.off1, self.off2 = [None] * n_off, [None] * n_off
        self.ctl = dict(first_bad=NONE, max_len1=0, max_len2=0, bytes1=0, bytes2=0, first_outside=NONE)

    def add_segment(self, text1: bytes, rec1, text2: bytes, rec2, prefix: int, base: int) -> None:
        """rec1 / rec2: rows (id offset, id length, sequence offset, sequence length) of the segment's pairs, offsets into their own text"""
        assert len(rec1) == len(rec2)
        c = self.ctl
        if base == 0:
            c.update(first_bad=NONE, max_len1=0, max_len2=0, bytes1=0, bytes2=0, first_outside=NONE)
        for i, (q1, q2) in enumerate(zip(rec1, rec2)):
            pos = base + i
            inside = all(q[0] + q[1] <= len(t) and q[2] + q[3] <= len(t) for q, t in ((q1, text1), (q2, text2)))
            p1 = p2 = b""
            if inside:
                if cut_id(text1[q1[0]:q1[0] + q1[1]]) != cut_id(text2[q2[0]:q2[0] + q2[1]]):
                    c["first_bad"] = min(c["first_bad"], pos)
                p1 = text1[q1[2]:q1[2] + min(q1[3], prefix)]
                p2 = text2[q2[2]:q2[2] + q2[3]]
            else:
                c["first_outside"] = min(c["first_outside"], pos)
            for piece, out, off, key, mx in ((p1, self.bytes1, self.off1, "bytes1", "max_len1"), (p2, self.bytes2, self.off2, "bytes2", "max_len2")):
                off[pos] = c[key]
                if c[key] + len(piece) <= len(out):
                    out[c[key]:c[key] + len(piece)] = piece
                c[key] += len(piece)
                c[mx] = max(c[mx], len(piece))
        self.off1[base + len(rec1)] = c["bytes1"]
        self.off2[base + len(rec2)] = c["bytes2"]

    def ctl_words(self):
        return [self.ctl[k] for k in CTL_NAMES]


def layout(records, lead: bytes = b"", gap: bytes = b"\n"):
    """(id, sequence) byte pairs laid out as a text: lead, then per record '@' id gap sequence gap -> (text, rows). Nothing here has to look
    like FASTQ: the pair scan only follows the rows."""
    text, rows = bytearray(lead), []
    for ident, seq in records:
        text += b"@"
        id_off = len(text)
        text += ident + gap
        seq_off = len(text)
        text += seq + gap
        rows.append((id_off, len(ident), seq_off, len(seq)))
    return bytes(text), rows
