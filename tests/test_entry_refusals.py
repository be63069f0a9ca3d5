"""The host entry points refused before any device work: a device index of 64 or more is turned
down by the default-context lookup without a HIP call, so every host entry point's "no context"
branch gives the same status and wording with and without a GPU.  Pinned here: the stage each
message names (the stage whose entry point was called first, not the one that made the call), what
the array-returning calls leave in their out-pointers after the refusal, and that empty input needs
no device at all."""
import ctypes

import numpy as np
import pytest

import s3imph

BAD_DEVICE = 64
SCHEMA = (0, 1, -1, -1)
CSV = b"a/b,1\na/c,2\n"


def _listing():
    blob, offs = s3imph.keys_to_blob([b"a/b", b"a/c"])
    return blob, offs, np.array([1, 2], np.uint64), np.array([0, 1], np.uint8)


def _run():
    blob, offs = s3imph.keys_to_blob([b"a/", b"a/b/"])
    return (blob, offs, np.array([1, 2], np.uint32), np.array([2, 1], np.uint64), np.array([3, 1], np.uint64))


def _aggregate(tmp):
    blob, offs, sizes, _ = _listing()
    s3imph.aggregate(blob, offs, sizes, device=BAD_DEVICE)


def _aggregate_tiers(tmp):
    blob, offs, sizes, tiers = _listing()
    s3imph.aggregate(blob, offs, sizes, device=BAD_DEVICE, tiers=tiers)


def _index_from_objects(tmp):
    blob, offs, sizes, _ = _listing()
    s3imph.build_index_from_objects(blob, offs, sizes, tmp, device=BAD_DEVICE)


def _index_from_unsorted(tmp):
    blob, offs, sizes, tiers = _listing()
    s3imph.build_index_from_unsorted_objects(blob, offs, sizes, tmp, tiers=tiers, device=BAD_DEVICE)


def _rowset_add_objects(tmp):
    blob, offs, sizes, _ = _listing()
    with s3imph.RowSet(device=BAD_DEVICE) as rs:
        rs.add_objects(blob, offs, sizes)


def _sort(tmp):
    blob, offs, _, _ = _listing()
    s3imph.sort_objects(blob, offs, device=BAD_DEVICE)


def _csv_parse(tmp):
    s3imph.parse_inventory_csv(CSV, SCHEMA, device=BAD_DEVICE)


def _index_from_csv(tmp):
    s3imph.build_index_from_inventory_csv([CSV], SCHEMA, tmp, device=BAD_DEVICE)


def _rowset_add_csv(tmp):
    with s3imph.RowSet(device=BAD_DEVICE) as rs:
        rs.add_csv([CSV], SCHEMA)


def _merge(tmp):
    s3imph.merge_rows([_run()], device=BAD_DEVICE)


def _index_from_rows(tmp):
    s3imph.build_index_from_rows([_run()], tmp, device=BAD_DEVICE)


def _rowset_build(tmp):
    with s3imph.RowSet(device=BAD_DEVICE) as rs:
        rs.add_rows(_run())
        assert rs.runs == 1 and rs.rows == 2
        rs.build(tmp)


def _finalize(tmp):
    blob, offs = s3imph.keys_to_blob([b"a/", b"a/b/"])
    s3imph.finalize_index_host(blob, offs, tmp, device=BAD_DEVICE)


def _build_host(tmp):
    blob, offs = s3imph.keys_to_blob([b"a/", b"a/b/"])
    s3imph.build_host(blob, offs, device=BAD_DEVICE)


REFUSALS = [
    (_aggregate, "aggregate: invalid device"),
    (_aggregate_tiers, "aggregate: invalid device"),
    (_index_from_objects, "aggregate: invalid device"),
    (_index_from_unsorted, "aggregate: invalid device"),
    (_rowset_add_objects, "aggregate: invalid device"),
    (_sort, "sort: invalid device"),
    (_csv_parse, "csv: invalid device"),
    (_index_from_csv, "csv: invalid device"),
    (_rowset_add_csv, "csv: invalid device"),
    (_merge, "merge: invalid device"),
    (_index_from_rows, "merge: invalid device"),
    (_rowset_build, "merge: invalid device"),
    (_finalize, "invalid device"),
    (_build_host, "invalid device"),
]


@pytest.mark.parametrize("call,message", REFUSALS, ids=[c.__name__.lstrip("_") for c, _ in REFUSALS])
def test_invalid_device_wording(call, message, tmp_path):
    with pytest.raises(s3imph.MPHFError) as e:
        call(str(tmp_path))
    assert e.value.status == s3imph.ERR_HIP
    assert str(e.value) == message


# ---- the four array-returning calls through ctypes: what the out-pointers hold afterwards ----

POISON = 0xDEAD0  # never dereferenced: the calls null their out-pointers before anything else


def _outs(k):
    return [ctypes.c_void_p(POISON) for _ in range(k)]


def _refs(ps):
    return [ctypes.byref(p) for p in ps]


def _call_aggregate_tiers(device, m):
    blob, offs, sizes, tiers = _listing()
    out, n, mask = _outs(7), ctypes.c_uint64(7), ctypes.c_uint64(7)
    err = ctypes.create_string_buffer(1024)
    p = s3imph._np_ptr
    rc = s3imph.LIB.s3imph_aggregate_tiers_host(device, p(blob), p(offs), p(sizes), p(tiers), m, 0, *_refs(out),
                                                ctypes.byref(mask), ctypes.byref(n), err, 1024)
    return rc, out, n.value, mask.value, err.value.decode()


def _call_merge(device, k):
    arr, _, keep = s3imph._row_runs([_run()])
    out, n, mask, info = _outs(7), ctypes.c_uint64(7), ctypes.c_uint64(7), s3imph.MergeInfo()
    err = ctypes.create_string_buffer(1024)
    rc = s3imph.LIB.s3imph_merge_rows_host(device, arr, k, *_refs(out), ctypes.byref(mask), ctypes.byref(n),
                                           ctypes.byref(info), err, 1024)
    del keep
    return rc, out, n.value, mask.value, err.value.decode()


def _call_csv(device, length):
    buf = np.frombuffer(CSV, np.uint8)
    out, info = _outs(4), s3imph.CsvInfo()
    err = ctypes.create_string_buffer(1024)
    rc = s3imph.LIB.s3imph_csv_parse_host(device, s3imph._np_ptr(buf), length, ctypes.byref(s3imph._csv_schema(SCHEMA)),
                                          *_refs(out), ctypes.byref(info), err, 1024)
    return rc, out, err.value.decode()


def _call_sort(device, m):
    blob, offs, _, _ = _listing()
    order, info = ctypes.c_void_p(POISON), s3imph.SortInfo()
    err = ctypes.create_string_buffer(1024)
    rc = s3imph.LIB.s3imph_sort_objects_host(device, s3imph._np_ptr(blob), s3imph._np_ptr(offs), m,
                                             ctypes.byref(order), ctypes.byref(info), err, 1024)
    return rc, order, err.value.decode()


def _one_zero_offset(p):
    """p is a one-entry offsets array holding 0; frees it."""
    assert p.value
    assert ctypes.cast(p, ctypes.POINTER(ctypes.c_uint64))[0] == 0
    s3imph.LIB.s3imph_free(p)


@pytest.mark.parametrize("call,units,message", [(_call_aggregate_tiers, 2, "aggregate: invalid device"),
                                                (_call_merge, 1, "merge: invalid device")],
                         ids=["aggregate_tiers", "merge_rows"])
def test_refused_rows_leave_nothing(call, units, message):
    rc, out, n, mask, err = call(BAD_DEVICE, units)
    assert rc == s3imph.ERR_HIP and err == message
    assert [p.value for p in out] == [None] * 7
    assert n == 0 and mask == 0


def test_refused_csv_parse_leaves_nothing():
    rc, out, err = _call_csv(BAD_DEVICE, len(CSV))
    assert rc == s3imph.ERR_HIP and err == "csv: invalid device"
    assert [p.value for p in out] == [None] * 4


def test_refused_sort_leaves_nothing():
    rc, order, err = _call_sort(BAD_DEVICE, 2)
    assert rc == s3imph.ERR_HIP and err == "sort: invalid device"
    assert order.value is None


@pytest.mark.parametrize("call", [_call_aggregate_tiers, _call_merge], ids=["aggregate_tiers", "merge_rows"])
def test_empty_rows_need_no_device(call):
    rc, out, n, mask, err = call(BAD_DEVICE, 0)
    assert rc == s3imph.OK and err == ""
    assert n == 0 and mask == 0
    assert [p.value for i, p in enumerate(out) if i != 1] == [None] * 6
    _one_zero_offset(out[1])


def test_empty_csv_needs_no_device():
    rc, out, err = _call_csv(BAD_DEVICE, 0)
    assert rc == s3imph.OK and err == ""
    assert [p.value for i, p in enumerate(out) if i != 1] == [None] * 3
    _one_zero_offset(out[1])


def test_empty_sort_needs_no_device():
    rc, order, err = _call_sort(BAD_DEVICE, 0)
    assert rc == s3imph.OK and err == ""
    assert order.value is None
