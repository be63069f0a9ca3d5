"""The index built from .csv.gz inventory files (s3imph_index_from_csv_gz_host,
s3imph_rowset_add_csv_gz): the directory equals, file for file, the one the CSV call writes for
the inflated texts, whatever the group size; a file whose trailer does not tell its size is
inflated twice; a corrupt file fails the call with its index and leaves the directory empty."""
import gzip
import os

import numpy as np
import pytest

import gzip_cases as K
import s3imph
from test_gpu_csv import LISTINGS, files_of, render

pytestmark = pytest.mark.gpu

SCHEMA = (1, 2, 3, 4)


def same_dirs(got, want, with_tiers, some_keys):
    names = files_of(want)
    assert files_of(got) == names and "manifest.json" in names
    assert any(n.startswith("tier_stats") for n in names) == (with_tiers and some_keys)
    for n in names:
        if n != "manifest.json":
            assert (got / n).read_bytes() == (want / n).read_bytes(), n
    # manifest.json carries the time of the build; everything else in it must agree
    a, b = s3imph.read_manifest(str(got)), s3imph.read_manifest(str(want))
    a.pop("created_at")
    b.pop("created_at")
    assert a == b
    s3imph.verify_manifest(str(got))


def four_files(case):
    """The listing as CSV rows in four files; the second one gzipped as two members, so that its
    last four bytes tell only the second member's size."""
    name, keys, sizes, tiers, max_depth = case
    sel = [i for i, k in enumerate(keys) if k and b"\r\n" not in k and not k.endswith(b"\r")]
    perm = np.random.default_rng(12).permutation(len(sel))
    keys = [keys[sel[i]] for i in perm]
    sizes = [sizes[sel[i]] for i in perm]
    tiers = None if tiers is None else [tiers[sel[i]] for i in perm]
    rows = render(keys, sizes, tiers, b"\n")
    q = [len(rows) * k // 4 for k in range(5)]
    texts = [b"".join(rows[q[k]:q[k + 1]]) for k in range(4)]
    gz = [gzip.compress(t, 6) for t in texts]
    half = len(texts[1]) * 3 // 4
    gz[1] = gzip.compress(texts[1][:half]) + gzip.compress(texts[1][half:], 1)
    return texts, gz, tiers is not None, max_depth, len(keys)


@pytest.mark.parametrize("case", LISTINGS, ids=[c[0] for c in LISTINGS])
def test_directory_from_csv_gz_equals_the_one_from_the_texts(tmp_path, case):
    texts, gz, with_tiers, max_depth, n_keys = four_files(case)
    want = tmp_path / "want"
    want.mkdir()
    total = s3imph.build_index_from_inventory_csv(texts, SCHEMA, str(want), with_tiers=with_tiers, max_depth=max_depth)
    cost = [len(f) + s3imph.gunzip_room_hint(f) for f in gz]
    once = max(cost[0] + cost[1], cost[2] + cost[3])  # two groups: the list is split once
    assert once < sum(cost)
    for group_bytes in (1, once, 1 << 62, 0):
        got = tmp_path / ("got_%d" % group_bytes)
        got.mkdir()
        assert s3imph.build_index_from_inventory_csv_gz(gz, SCHEMA, str(got), with_tiers=with_tiers,
                                                        max_depth=max_depth, group_bytes=group_bytes) == total
        same_dirs(got, want, with_tiers, n_keys > 0)


def test_a_file_that_needs_more_room_than_its_trailer_says(tmp_path):
    text = K.filler(300000, 21)
    cut = text.index(b"\n", 290000) + 1
    lying = gzip.compress(text[:cut]) + gzip.compress(text[cut:])
    assert s3imph.gunzip_room_hint(lying) == len(text) - cut < len(text) // 20
    files = [gzip.compress(K.filler(5000, 22)), lying, gzip.compress(b""), gzip.compress(K.filler(7000, 23))]
    texts = [gzip.decompress(f) for f in files]
    got, want = tmp_path / "got", tmp_path / "want"
    got.mkdir()
    want.mkdir()
    total = s3imph.build_index_from_inventory_csv(texts, (0, 1, 2, 3), str(want), with_tiers=True)
    assert total["n_objects"] > 4000
    assert s3imph.build_index_from_inventory_csv_gz(files, (0, 1, 2, 3), str(got), with_tiers=True) == total
    same_dirs(got, want, True, True)


@pytest.mark.parametrize("group_bytes", [1, 0])
def test_a_corrupt_file_fails_the_build_and_writes_nothing(tmp_path, group_bytes):
    good = gzip.compress(K.filler(3000, 24))
    by_name = {c.name: c for c in K.INVALID}
    for name, text in (("crc_bit", "invalid checksum"), ("cut_at_21", "unexpected EOF"),
                       ("trailing_zeros", "invalid header"), ("len_nlen_mismatch", "corrupt input"),
                       ("zero_length", "unexpected EOF")):
        files = [good, good, good, by_name[name].data, by_name["bad_magic_1"].data, good]
        with pytest.raises(s3imph.MPHFError) as e:
            s3imph.build_index_from_inventory_csv_gz(files, (0, 1, 2, 3), str(tmp_path), group_bytes=group_bytes)
        assert e.value.status == s3imph.ERR_FORMAT and str(e.value) == "gzip: file 3: " + text
        assert os.listdir(tmp_path) == []
    with s3imph.RowSet() as rs:
        with pytest.raises(s3imph.MPHFError) as e:
            rs.add_csv_gz([good, by_name["isize_bit"].data], (0, 1, 2, 3), group_bytes=group_bytes)
        assert e.value.status == s3imph.ERR_FORMAT and str(e.value) == "gzip: file 1: invalid checksum"
        assert rs.runs == 0


@pytest.mark.parametrize("with_tiers", [False, True], ids=["plain", "tiers"])
def test_rowset_add_csv_gz_equals_add_csv_on_the_texts(tmp_path, with_tiers):
    chunks = [[K.filler(20000, 31), K.filler(300, 32)], [K.filler(9000, 33)], [b"", K.filler(4000, 34)]]
    got, want = tmp_path / "got", tmp_path / "want"
    got.mkdir()
    want.mkdir()
    with s3imph.RowSet(with_tiers=with_tiers) as a, s3imph.RowSet(with_tiers=with_tiers) as b:
        for k, texts in enumerate(chunks):
            a.add_csv_gz([gzip.compress(t, 1 + 4 * k) for t in texts], (0, 1, 2, 3), group_bytes=k)
            b.add_csv(texts, (0, 1, 2, 3))
        assert a.runs == b.runs == 3 and a.rows == b.rows
        a.build(str(got))
        b.build(str(want))
    same_dirs(got, want, with_tiers, True)
