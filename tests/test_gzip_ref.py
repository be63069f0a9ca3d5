"""gzip_ref, the pure-Python reader the GPU inflate is compared with, against zlib and gzip, and
gzip_cases against gzip_ref: every valid case decodes to what zlib gives and really reaches the
edge it is named for; every invalid case is rejected, by Python's own readers too where they can
read it.  No GPU."""
import gzip
import zlib

import pytest

import gzip_cases as K
import gzip_ref as G

REFS = K.refs()


def cpython(data):
    """gzip.decompress, or the exception's class name."""
    try:
        return gzip.decompress(data)
    except (OSError, EOFError, zlib.error) as e:
        return type(e).__name__


def test_case_names_are_unique():
    names = [c.name for c in K.VALID + K.INVALID]
    assert len(set(names)) == len(names)


@pytest.mark.parametrize("case", K.VALID, ids=[c.name for c in K.VALID])
def test_valid_cases_agree_with_zlib_and_reach_their_edge(case):
    text, tr = REFS[case.name]
    assert tr.status == G.OK == case.status
    assert cpython(case.data) == text
    # member by member through zlib's own gzip wrapper
    # (zlib refuses reserved flag bits, which Go and section 5j ignore)
    rest, parts = case.data, []
    while rest and not any(f & 0xE0 for f in tr.flags):
        d = zlib.decompressobj(31)
        parts.append(d.decompress(rest))
        assert d.eof
        rest = d.unused_data
    assert not parts or (b"".join(parts) == text and len(parts) == tr.members)
    assert tr.in_used == len(case.data) and tr.crc32 == zlib.crc32(text)
    assert case.edge(tr, text)


@pytest.mark.parametrize("case", K.INVALID, ids=[c.name for c in K.INVALID])
def test_invalid_cases_are_rejected(case):
    _, tr = REFS[case.name]
    assert tr.status == case.status != G.OK
    got = cpython(case.data)
    if case.cpython_rejects:
        assert isinstance(got, str), "Python's gzip reads this file"
    else:
        assert isinstance(got, bytes), "Python's gzip is no longer lenient here: drop the exemption"


def test_the_cases_cover_every_block_type_and_the_named_edges():
    traces = [REFS[c.name][1] for c in K.VALID]
    assert {t for tr in traces for t in tr.block_types} == {0, 1, 2}
    assert max(tr.max_code_len for tr in traces) == 15
    assert max(tr.max_dist for tr in traces) == 32768 and max(tr.max_len for tr in traces) == 258
    assert any(tr.cross_boundary_repeat for tr in traces)
    assert max(tr.stored_lens[0] for tr in traces if tr.stored_lens) == 65535
    assert {c.status for c in K.INVALID} == {G.EOF, G.HEADER, G.DATA, G.CHECKSUM}


def test_writer_round_trips_through_zlib():
    syms = list(b"hello ") + [(5, 6), (258, 1), 0, 255, (3, 11), (200, 100)]
    w = G.BitWriter()
    w.stored(b"abc")
    w.fixed(syms, final=True)
    want = b"abc" + G.expand(syms, b"abc")
    assert zlib.decompress(w.done(), -15) == want
    assert G.gunzip(G.member(w.done(), want))[0] == want


def test_the_multi_member_file_lies_about_its_size():
    data = K.lying_isize(K.filler(5000, 1), 5)
    text, tr = G.gunzip(data)
    assert tr.status == G.OK and tr.members == 2 and len(text) == 5005
    assert int.from_bytes(data[-4:], "little") == 5
