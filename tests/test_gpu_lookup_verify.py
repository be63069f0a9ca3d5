"""MPHF.LookupWithVerify on the GPU (s3imph_index_lookup_verify_device; mphf.go:306-320), against
Lookup masked by byte equality with the stored prefix (run on an MI355X, -m gpu).

Lookup compares a 64-bit fingerprint, so it cannot tell a stored prefix that was changed after the
build from the key it was built with; LookupWithVerify reads the stored bytes and can.  The handle
is attached (Index.from_arrays) and its prefix blob is a tampered copy: the MPHF still answers for
the original keys, the stored bytes differ at chosen places."""
import numpy as np
import pytest

import keysets
import names_cases as NC
import oracle as O

pytestmark = pytest.mark.gpu

NOT_FOUND = NC.NOT_FOUND
LENGTHS = (1, 7, 8, 9, 16, 17, 1024)


@pytest.fixture(scope="module")
def s3():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import s3imph
    return s3imph


ROLES = ("first", "last", "ninth")


def _tampered(keys, at, role):
    """(stored keys, the set of tampered indices): the key of every length in LENGTHS changed in
    its first, last or ninth byte (`role`; the ninth where the key has one); one key stored minus
    its last byte (caught by length, the bytes agree); the root "" stored as "x"."""
    stored = list(keys)
    bad = set()
    for ln in LENGTHS:
        byte = {"first": 0, "last": ln - 1, "ninth": 8}[role]
        if byte >= ln:
            continue
        i = at[ln]
        k = bytearray(stored[i])
        k[byte] ^= 0x01
        stored[i] = bytes(k)
        bad.add(i)
    short = at[15]
    stored[short] = stored[short][:-1]
    bad.add(short)
    stored[at[0]] = b"x"
    bad.add(at[0])
    return stored, bad


@pytest.fixture(scope="module")
def built(oracle_lib):
    keys = NC.edge_keys()
    blob, offs = O.keys_to_blob(keys)
    st, fp, pos, mph = oracle_lib.build(blob, offs)
    assert st == 0
    return keys, NC.by_length(keys), mph, fp, pos


@pytest.fixture(scope="module", params=ROLES)
def rig(s3, built, request):
    keys, at, mph, fp, pos = built
    stored, bad = _tampered(keys, at, request.param)
    assert len(bad) == 2 + sum(1 for ln in LENGTHS if {"first": 0, "last": ln - 1, "ninth": 8}[request.param] < ln)
    idx = NC.attached(s3, mph, fp, pos, *O.keys_to_blob(stored))
    yield keys, stored, bad, idx
    idx.close()


def _want(keys, stored):
    return np.array([i if stored[i] == k else NOT_FOUND for i, k in enumerate(keys)], np.uint64)


def test_tampered_prefixes_are_caught(rig):
    keys, stored, bad, idx = rig
    n = len(keys)
    plain = idx.lookup(keys)
    assert np.array_equal(plain, np.arange(n, dtype=np.uint64))  # Lookup still finds every one of them
    got = idx.lookup_verify(keys)
    want = _want(keys, stored)
    assert set(np.flatnonzero(want == NOT_FOUND).tolist()) == bad
    assert np.array_equal(got, want)


@pytest.mark.parametrize("shift", range(8))
def test_queries_at_every_byte_offset(rig, shift):
    """The query blob starts `shift` bytes into its buffer: both blobs go through load8 at any
    alignment, and the tampered keys sit next to clean ones of every length."""
    keys, stored, bad, idx = rig
    sel = sorted(bad) + [i for i in range(0, len(keys), 37)]
    q = [keys[i] for i in sel]
    blob, offs = O.keys_to_blob(q)
    buf = np.zeros(shift + (len(blob) + 7) // 8 * 8 + 16, np.uint8)
    buf[shift:shift + len(blob)] = blob
    d_buf = NC.dev(buf)
    d_offs = NC.dev(offs + np.uint64(shift))  # offsets[0] = shift: the keys start there
    got = idx.lookup_verify_device(d_buf, d_offs, len(q)).cpu().numpy().view(np.uint64)
    plain = idx.lookup_device(d_buf, d_offs, len(q)).cpu().numpy().view(np.uint64)
    assert np.array_equal(plain, np.array(sel, np.uint64))
    want = _want(keys, stored)[sel]
    assert np.array_equal(got, want)
    # the same through a tensor sliced at +shift (an unaligned base pointer, offsets from 0)
    got2 = idx.lookup_verify_device(d_buf[shift:], NC.dev(offs), len(q)).cpu().numpy().view(np.uint64)
    assert np.array_equal(got2, want)


def test_non_members_stay_not_found(s3):
    """TestMPHFNoFalsePositives' strings (mphf_test.go:182-218) against its own set."""
    keys, idx = NC.golden_index(s3, "mphf_no_false_pos")
    q = [k.encode() for k in keysets.NON_MEMBERS]
    assert np.all(idx.lookup_verify(q) == np.uint64(NOT_FOUND))
    assert np.array_equal(idx.lookup_verify(keys), np.arange(len(keys), dtype=np.uint64))
    assert len(idx.lookup_verify([])) == 0
    idx.close()


def forged_fingerprint(oracle_lib, keys, mph, fp, pos):
    """(non-member k, fingerprints with one slot forged) such that the oracle's Lookup finds k."""
    st, m = oracle_lib.unmarshal(mph)
    assert st == 0
    for k in (b"zz-%d/" % i for i in range(256)):
        for slot in range(len(keys)):
            fp2 = fp.copy()
            fp2[slot] = np.uint64(O.py_fnv1_64(k))
            if oracle_lib.lookup(m, fp2, pos, k) is not None:
                return k, fp2
    raise AssertionError("no probe key lands in an occupied slot")


def test_false_positive_of_the_fingerprint_is_refused(s3, oracle_lib):
    """A non-member that Lookup does return: the stored fingerprint at its slot is overwritten
    with the non-member's own FNV-1, which is what a fingerprint collision looks like."""
    keys = [b"", b"a/", b"a/b/", b"b/", b"c/"]
    blob, offs = O.keys_to_blob(keys)
    st, fp, pos, mph = oracle_lib.build(blob, offs)
    assert st == 0
    k, fp2 = forged_fingerprint(oracle_lib, keys, mph, fp, pos)
    idx = NC.attached(s3, mph, fp2, pos, blob, offs)
    assert idx.lookup([k])[0] != NOT_FOUND        # the false positive
    assert idx.lookup_verify([k])[0] == NOT_FOUND  # refused by the bytes
    idx.close()
