"""What tools/bench_cells.py, bench_bus.py and bench_pairs.py share for their file-level legs: the input form (--input plain|bgzf), the switch
to the host path (--host-scan sets PA_PAIRS_HOST_SCAN=1 for the whole process), several timed calls (--calls) and what the library says about
the input afterwards. BGZF is written with Python's zlib, member by member, as tests/bgzf_cases.py does: no bgzip binary is needed."""
import os
import statistics
import struct
import time
import zlib

BGZF_CHUNK = 65280
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def add_args(ap):
    ap.add_argument("--input", choices=["plain", "bgzf"], default="plain", help="form of the FASTQ files of the file-level leg")
    ap.add_argument("--host-scan", action="store_true", help="PA_PAIRS_HOST_SCAN=1: scan, id compare and gather on the host, as before the device path")
    ap.add_argument("--calls", type=int, default=1, help="timed file-level calls (median, min and max are reported)")


def apply(args):
    if args.host_scan:
        os.environ["PA_PAIRS_HOST_SCAN"] = "1"
    else:
        os.environ.setdefault("PA_PAIRS_DEVICE_PLAIN", "1")   # plain files take the device path too: what the tools compare with --host-scan


def suffix(args):
    return ".gz" if args.input == "bgzf" else ""


class Writer:
    """a FASTQ file written piece by piece: as it is, or as BGZF members of BGZF_CHUNK bytes of text each"""

    def __init__(self, path, kind):
        self.f, self.kind, self.pending = open(path, "wb"), kind, b""

    def _member(self, text):
        c = zlib.compressobj(1, zlib.DEFLATED, -15)
        payload = c.compress(text) + c.flush()
        total = 12 + 6 + len(payload) + 8
        assert total <= 65536
        self.f.write(struct.pack("<BBBBIBBH", 0x1f, 0x8b, 8, 4, 0, 0, 0xff, 6) + b"BC" + struct.pack("<HH", 2, total - 1) + payload +
                     struct.pack("<II", zlib.crc32(text), len(text)))

    def write(self, data):
        if self.kind == "plain":
            self.f.write(data)
            return
        data = self.pending + data
        n = len(data) // BGZF_CHUNK * BGZF_CHUNK
        for i in range(0, n, BGZF_CHUNK):
            self._member(data[i:i + BGZF_CHUNK])
        self.pending = data[n:]

    def close(self):
        if self.kind == "bgzf":
            if self.pending:
                self._member(self.pending)
            self.f.write(EOF_BLOCK)
        self.f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def timed_calls(fn, calls):
    """fn() `calls` times -> (seconds of each call, the last call's answer)"""
    secs, out = [], None
    for _ in range(max(1, calls)):
        t = time.perf_counter()
        out = fn()
        secs.append(time.perf_counter() - t)
    return secs, out


def report(pa, args, pairs, secs):
    """the entries every tool adds to its JSON line"""
    rates = sorted(pairs / s for s in secs)
    out = {"input": args.input, "host_scan": bool(args.host_scan), "calls": len(secs), "file_seconds_all": [round(s, 4) for s in secs],
           "file_pairs_per_s_median": round(statistics.median(rates)), "file_pairs_per_s_min": round(rates[0]), "file_pairs_per_s_max": round(rates[-1])}
    if hasattr(pa, "pairs_input_stats") and hasattr(pa.lib(), "pa_pairs_input_stats"):   # (an older library under PA_PRODUCT_SO has no such entry point)
        out["pairs_input_stats"] = pa.pairs_input_stats()
    return out
