"""VerifyMPHF on the GPU (s3imph_index_verify_device, Index.verify; mphf.go:372-393): every stored
prefix is looked up and the mismatches are reduced on the device to their count, the first of them
and what the lookup gave there (run on an MI355X, -m gpu).  Attached handles of ~5000 keys; the
expected triple is the numpy comparison of the oracle's Lookup with arange."""
import numpy as np
import pytest

import names_cases as NC
import oracle as O

pytestmark = pytest.mark.gpu

NOT_FOUND = NC.NOT_FOUND


@pytest.fixture(scope="module")
def s3():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import s3imph
    return s3imph


@pytest.fixture(scope="module")
def built(oracle_lib):
    keys = NC.edge_keys()
    blob, offs = O.keys_to_blob(keys)
    st, fp, pos, mph = oracle_lib.build(blob, offs)
    assert st == 0
    return keys, blob, offs, mph, fp, pos


def _swapped(pos):
    """mph_pos with the entries that hold 0 and n - 1 exchanged: stored prefix 0 looks up to n - 1
    and the other way round."""
    n = len(pos)
    p = pos.copy()
    i0, i1 = int(np.flatnonzero(pos == 0)[0]), int(np.flatnonzero(pos == n - 1)[0])
    p[i0], p[i1] = n - 1, 0
    return p


def _last_replaced(keys):
    stored = list(keys)
    stored[-1] = b"zzzz/not-a-member/"
    return stored


def test_clean(s3, built):
    keys, blob, offs, mph, fp, pos = built
    idx = NC.attached(s3, mph, fp, pos, blob, offs)
    assert idx.verify_device() == (0, NOT_FOUND, NOT_FOUND)
    idx.verify()
    idx.close()


def test_swapped_positions(s3, built):
    keys, blob, offs, mph, fp, pos = built
    n = len(keys)
    idx = NC.attached(s3, mph, fp, _swapped(pos), blob, offs)
    assert idx.verify_device() == (2, 0, n - 1)
    with pytest.raises(s3.MPHFError) as e:
        idx.verify()
    assert e.value.status == s3.ERR_INTERNAL
    assert str(e.value) == f'lookup returned wrong pos for "": got {n - 1}, want 0'
    idx.close()


def test_non_member_stored(s3, oracle_lib, built):
    keys, blob, offs, mph, fp, pos = built
    n = len(keys)
    stored = _last_replaced(keys)
    st, m = oracle_lib.unmarshal(mph)
    assert st == 0 and oracle_lib.lookup(m, fp, pos, stored[-1]) is None  # the oracle agrees it is none
    idx = NC.attached(s3, mph, fp, pos, *O.keys_to_blob(stored))
    assert idx.verify_device() == (1, n - 1, NOT_FOUND)
    with pytest.raises(s3.MPHFError) as e:
        idx.verify()
    assert e.value.status == s3.ERR_INTERNAL
    assert str(e.value) == f'lookup failed for prefix "zzzz/not-a-member/" at pos {n - 1}'
    idx.close()


def test_many_bad_across_workgroups(s3, built):
    """Every 7th position rotated by one: the count and the minimum come from many waves."""
    keys, blob, offs, mph, fp, pos = built
    n = len(keys)
    sel = np.arange(3, n, 7)
    perm = np.arange(n, dtype=np.uint64)
    perm[sel] = np.roll(sel, 1)
    idx = NC.attached(s3, mph, fp, perm[pos.astype(np.int64)], blob, offs)
    assert idx.verify_device() == (len(sel), 3, int(sel[-1]))
    idx.close()


def test_empty_index(s3):
    idx = NC.attached(s3, b"", np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.uint8),
                      np.zeros(1, np.uint64))
    assert idx.count == 0 and idx.has_prefixes()
    assert idx.verify_device() == (0, NOT_FOUND, NOT_FOUND)
    idx.verify()
    idx.close()


def test_second_attach_replaces_the_first(s3, built):
    keys, blob, offs, mph, fp, pos = built
    n = len(keys)
    idx = NC.attached(s3, mph, fp, pos, *O.keys_to_blob(_last_replaced(keys)))
    assert idx.verify_device()[0] == 1
    idx.attach_prefixes(NC.dev(NC.padded(blob)), NC.dev(offs))
    assert idx.verify_device() == (0, NOT_FOUND, NOT_FOUND)
    assert idx.prefix_strings([n - 1]) == [keys[-1]]
    with pytest.raises(s3.MPHFError) as e:
        idx.attach_prefixes(None, NC.dev(offs))
    assert e.value.status == s3.ERR_INVALID
    idx.close()
