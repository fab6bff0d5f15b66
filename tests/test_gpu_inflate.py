"""pa_bgzf_inflate_device (csrc/inflate.hip) on the vectors of tests/bgzf_cases.py: torch uint8 tensors as d_comp and d_text, 256 sentinel
bytes in front of and behind the text, the text pre-filled with a pattern. Valid members give Python's text and status 0; a corrupt member
gives its status, leaves its neighbours' text exact and writes nothing outside its own bytes. Every vector has been through the same decoder
on the CPU under sanitizers first (tests/test_bgzf_cases.py). Every comparison is exact. A HIP error ends the session: nothing more is
started on a GPU that may have faulted."""
import numpy as np
import pytest

import bgzf_cases as bc
import helpers

pytestmark = pytest.mark.gpu

GUARD = 256
SENTINEL, PATTERN = 0x5A, 0xC3
MEMBER = np.dtype([("in_off", "<u8"), ("out_off", "<u8"), ("file_off", "<u8"), ("in_len", "<u4"), ("out_len", "<u4"), ("crc32", "<u4"), ("reserved", "<u4")])


@pytest.fixture(scope="module")
def torch_gpu():
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("the gpu tier needs a GPU")
    try:
        helpers.pa.lib()
    except ImportError:   # a tree that was never built
        helpers.build_all()
    return torch


def table(rows):
    t = np.zeros(len(rows), MEMBER)
    for f in ("in_off", "out_off", "file_off", "in_len", "out_len", "crc32"):
        t[f] = [r[f] for r in rows]
    return t


def inflate(torch, data, rows, text_cap=None):
    """-> (the whole text buffer with its guards as numpy, statuses): one launch over `rows` of the file `data`"""
    pa = helpers.pa
    n_text = sum(r["out_len"] for r in rows) if text_cap is None else text_cap
    comp = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    members = torch.from_numpy(table(rows).view(np.uint8).copy()).cuda()
    buf = torch.full((GUARD + n_text + GUARD,), PATTERN, dtype=torch.uint8, device="cuda")
    buf[:GUARD] = SENTINEL
    buf[GUARD + n_text:] = SENTINEL
    status = torch.full((len(rows) + 2,), 0x7EADBEEF, dtype=torch.int32, device="cuda")
    try:
        pa.bgzf_inflate_device(0, comp.data_ptr(), comp.numel(), members.data_ptr(), len(rows), buf.data_ptr() + GUARD, n_text, status.data_ptr(),
                               torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    except (pa.PaError, RuntimeError) as e:
        pytest.exit("inflate kernel: %s" % e, returncode=3)
    out, st = buf.cpu().numpy(), status.cpu().numpy()
    assert (out[:GUARD] == SENTINEL).all() and (out[GUARD + n_text:] == SENTINEL).all(), "sentinels"
    assert (st[len(rows):] == 0x7EADBEEF).all(), "status words behind the last member"
    return out, st[:len(rows)]


VALID = bc.valid_cases()
CORRUPT = bc.corrupt_cases()


@pytest.mark.parametrize("k", range(len(VALID)), ids=[n for n, _, _ in VALID])
def test_valid(torch_gpu, k):
    name, data, text = VALID[k]
    out, st = inflate(torch_gpu, data, bc.walk(data))
    assert not st.any(), (name, np.flatnonzero(st)[:5], st[np.flatnonzero(st)[:5]])
    got = out[GUARD:GUARD + len(text)].tobytes()
    if got != text:
        bad = np.flatnonzero(np.frombuffer(got, np.uint8) != np.frombuffer(text, np.uint8))
        raise AssertionError("%s: %d bytes differ, first at %d" % (name, len(bad), bad[0]))


@pytest.mark.parametrize("k", range(len(CORRUPT)), ids=[n for n, _, _, _ in CORRUPT])
def test_corrupt(torch_gpu, k):
    name, data, bad, texts = CORRUPT[k]
    rows = bc.walk(data)
    out, st = inflate(torch_gpu, data, rows)
    names = helpers.pa._ffi.INFLATE_STATUS_NAMES
    assert st[bad] != 0 and names[st[bad]] == bc.EXPECTED_STATUS[name], (name, st)
    assert [int(s) for i, s in enumerate(st) if i != bad] == [0] * (len(rows) - 1), (name, st)
    for i in (0, 2):   # the neighbours' text is exact: nothing of the corrupt member reached it
        r = rows[i]
        assert out[GUARD + r["out_off"]:GUARD + r["out_off"] + r["out_len"]].tobytes() == texts[i], (name, i)
    # nothing at or beyond the corrupt member's end differs from what the neighbours own: behind it lie only the right neighbour's text (exact, above)
    # and the rear guard (checked by inflate()); its own out_len bytes are unspecified by the header's contract


def test_repeat_run_and_a_run_from_the_middle(torch_gpu):
    text = bc.fastq_like(200 * 4000, 17)
    data = bc.bgzf(text, 4000, eof=False)
    rows = bc.walk(data)
    assert len(rows) == 200
    a, sa = inflate(torch_gpu, data, rows)
    b, sb = inflate(torch_gpu, data, rows)
    assert a.tobytes() == b.tobytes() and not sa.any() and not sb.any()
    assert a[GUARD:-GUARD].tobytes() == text
    c, sc = inflate(torch_gpu, data, rows[101:])   # out_off is rebased on the first row passed
    assert not sc.any() and c[GUARD:-GUARD].tobytes() == text[101 * 4000:]


def test_rows_that_do_not_fit_are_refused_untouched(torch_gpu):
    """a table row is checked before its member is touched: text beyond text_cap, payload beyond the compressed bytes, ISIZE beyond 64 KiB"""
    text = bc.fastq_like(3000, 23)
    data = bc.bgzf(text, 1000, eof=False)
    rows = bc.walk(data)
    out, st = inflate(torch_gpu, data, rows, text_cap=2999)
    assert st.tolist() == [0, 0, 1] and out[GUARD:GUARD + 2000].tobytes() == text[:2000] and (out[GUARD + 2000:GUARD + 2999] == PATTERN).all()
    long_row = dict(rows[2], in_len=len(data) - rows[2]["in_off"] + 1)   # one byte beyond the compressed bytes
    out, st = inflate(torch_gpu, data, rows[:2] + [long_row])
    assert st.tolist() == [0, 0, 1] and (out[GUARD + 2000:GUARD + 3000] == PATTERN).all()
    huge = dict(rows[1], out_len=65537)
    out, st = inflate(torch_gpu, data, [rows[0], huge], text_cap=70000)
    assert st.tolist() == [0, 1] and (out[GUARD + 1000:GUARD + 70000] == PATTERN).all()


def test_convenience_wrapper(torch_gpu):
    name, data, text = VALID[2]
    got, st = helpers.pa.bgzf_inflate(data)
    assert got == text and not st.any()
    with pytest.raises(helpers.pa.PaError):
        helpers.pa.bgzf_inflate(bc.not_bgzf_cases()[0][1])
