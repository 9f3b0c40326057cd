"""k_hash_operand alone (kernels/hash_operand.hip through the production
launch_hash_operand, via libcapjwt_tk.so's tk_hash_operand): every operand byte
and every span the kernel writes, against hashlib + base64.

* Every source length at which SHA-256 or SHA-512 takes one block more, the
  block sizes +- 1 and the cap of 8192 x three families x source offsets 0..3
  mod 4, with family 0 ("no value") mixed into the same waves.
* 1 / 63 / 64 / 65 / 257 jobs with one and two hash columns, behind 0, 1 and 2
  plain string columns whose spans the kernel must leave alone, at several
  operand bases.
* The last source ends at the last byte of the source bytes.
* A slot is 44 bytes: the characters, then zeros; family 0 gives the one byte
  0x00.  Nothing outside the slots and the hashed columns' spans is written.
"""
import ctypes
import os

import pytest

from cap_amd import _lib
from tests import claims_match_hash_cases as HC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOT = 44


@pytest.fixture(scope="module")
def tk():
    L = ctypes.CDLL(os.path.join(ROOT, "cap_amd", "libcapjwt_tk.so"))
    L.tk_hash_operand.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint32,
                                  ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
    return L


def run(tk, cols, nstr=0, op_base=0, lead=0):
    """cols: hash columns as pack_hargs takes them -> (operand buffer, span rows)"""
    h = _lib.pack_hargs(cols, lead=lead)
    njobs, nhash = len(h["src"]), h["nhash"]
    flat = [x for row in h["src"] for x in row]
    src = (_lib.JgHSrc * len(flat))()
    for t, (off, ln, fam) in zip(src, flat):
        t.off, t.len, t.fam = off, ln, fam
    op = ctypes.create_string_buffer(op_base + SLOT * njobs * nhash)
    spans = (_lib.JgSArg * (njobs * (nstr + nhash)))()
    rc = tk.tk_hash_operand(h["bytes"], len(h["bytes"]), src, njobs, nhash, nstr, op_base, op, spans)
    assert rc == 0
    return h, op.raw, [[(spans[i * (nstr + nhash) + c].off, spans[i * (nstr + nhash) + c].len) for c in range(nstr + nhash)]
                       for i in range(njobs)]


def check(cols, nstr, op_base, h, op, rows):
    nhash = len(cols)
    assert op[:op_base] == b"\xa5" * op_base                                     # the caller's operand bytes
    seen = []
    for i, row in enumerate(rows):
        assert row[:nstr] == [(0xa5a5a5a5, 0xa5a5a5a5)] * nstr, i                 # the caller's spans
        for c in range(nhash):
            want = HC.hash_value(*cols[c][i]) if cols[c][i] is not None else b"\0"
            off = op_base + SLOT * (i * nhash + c)
            assert row[nstr + c] == (off, len(want)), (i, c, row)
            assert op[off:off + SLOT] == want + bytes(SLOT - len(want)), (i, c, cols[c][i] and len(cols[c][i][0]))
            seen.append(want)
    return seen


def test_every_length_family_and_offset(tk):
    # every (family, length) with its source at every alignment: fillers in front of a source move it there
    want_at = [(fam, n, a) for fam in HC.FAMS for n in HC.LENGTHS for a in range(4)]
    blob, srcs = bytearray(), []
    for k, (fam, n, a) in enumerate(want_at):
        while len(blob) % 4 != a:
            blob += b"#"
        srcs.append((len(blob), n, 0 if k % 13 == 7 else fam))             # family 0 in every wave
        blob += HC.source(k, n)
    assert len(srcs) == 3 * 19 * 4 and all(off % 4 == a for (off, _, _), (_, _, a) in zip(srcs, want_at))
    assert srcs[-1][1] > 0 and srcs[-1][0] + srcs[-1][1] == len(blob)       # the last source ends at the last byte
    njobs = len(srcs)
    src = (_lib.JgHSrc * njobs)()
    for t, (off, ln, fam) in zip(src, srcs):
        t.off, t.len, t.fam = off, ln, fam
    op = ctypes.create_string_buffer(SLOT * njobs)
    spans = (_lib.JgSArg * njobs)()
    assert tk.tk_hash_operand(bytes(blob), len(blob), src, njobs, 1, 0, 0, op, spans) == 0
    got, seen = op.raw, []
    for k, (off, n, fam) in enumerate(srcs):
        want = HC.hash_value(bytes(blob[off:off + n]), fam) if fam else b"\0"
        assert (spans[k].off, spans[k].len) == (SLOT * k, len(want)), k
        assert got[SLOT * k:SLOT * (k + 1)] == want + bytes(SLOT - len(want)), (k, fam, n, off % 4)
        seen.append(want)
    text = b"".join(seen)
    assert b"-" in text and b"_" in text and {len(v) for v in seen} == {1, 22, 32, 43}


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_job_counts_columns_and_bases(tk, n):
    for nhash, nstr, op_base in ((1, 0, 0), (2, 0, 4), (1, 1, 64), (2, 2, 132), (1, 3, 8), (2, 1, 0)):
        cols = [[None if (k + c) % 7 == 3 else (HC.source(k + 31 * c, (53 * k + 17 * c) % 300), HC.FAMS[(k + c) % 3])
                 for k in range(n)] for c in range(nhash)]
        if cols[-1][-1] is None or not cols[-1][-1][0]:
            cols[-1][-1] = (b"the last source", HC.SHA384)
        h, op, rows = run(tk, cols, nstr=nstr, op_base=op_base, lead=n % 4)
        off, ln, _ = h["src"][-1][-1]
        assert ln > 0 and off + ln == len(h["bytes"])                            # ends at the last byte of the buffer
        seen = check(cols, nstr, op_base, h, op, rows)
        if n >= 63:
            assert {len(v) for v in seen} == {1, 22, 32, 43}


def test_refused_arguments_do_not_launch(tk):
    src = (_lib.JgHSrc * 1)()
    op, spans = ctypes.create_string_buffer(SLOT), (_lib.JgSArg * 4)()
    for off, ln, fam, nhash, nstr, base in ((0, 4, 1, 1, 0, 0), (2, 2, 1, 1, 0, 0), (0, 1, 4, 1, 0, 0), (0, 1, 1, 3, 0, 0),
                                            (0, 1, 1, 1, 4, 0), (0, 1, 1, 1, 0, 2)):
        src[0].off, src[0].len, src[0].fam = off, ln, fam
        assert tk.tk_hash_operand(b"abc", 3, src, 1, nhash, nstr, base, op, spans) == -1
    assert op.raw == bytes(SLOT)
