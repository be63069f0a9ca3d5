"""tests/stream_cases.py on its own (no GPU): every case's decoy and real input have the same
names, dtypes and shapes and the same offsets arrays, their indices are in range, and the
restatements give the two different answers — without which tests/test_gpu_streams.py could not
tell a stale read from a fresh one."""
import numpy as np
import pytest

import stream_cases as SC


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle_lib):
    return oracle_lib


@pytest.mark.parametrize("name", SC.NAMES)
def test_decoy_and_real_share_their_shape_and_differ_in_their_answer(name):
    c = SC.case(name)
    assert c.name == name and c.family in SC.FAMILIES
    assert c.decoy.keys() == c.real.keys() and c.want_decoy.keys() == c.want_real.keys()
    changed = 0
    for k, d in c.decoy.items():
        r = c.real[k]
        assert d.dtype == r.dtype and d.shape == r.shape, k
        assert not d.flags.writeable and not r.flags.writeable, k
        changed += d.tobytes() != r.tobytes()
        if k == "offsets":
            assert np.array_equal(d, r), "the offsets arrays must be identical"
            assert d[0] == 0 and (np.diff(d.astype(np.int64)) >= 0).all()
            blob = c.decoy.get("blob", c.decoy.get("keys"))
            assert int(d[-1]) <= len(blob) - 8, "readable up to the length rounded up to 8 bytes"
    assert changed, "the inputs are the same bytes"
    assert SC.differ(c.want_decoy, c.want_real), "a stale read would pass"
    # every array of the answers differs somewhere or is an info field; at least one array does
    assert any(isinstance(w, np.ndarray) and w.tobytes() != np.asarray(c.want_real[k]).tobytes()
               for k, w in c.want_decoy.items())
    SC.same(c.want_real, c.want_real)


def test_indices_are_in_range_or_checked_values():
    m = SC.M_OBJ
    for side in (SC.case("gather_objects").decoy, SC.case("gather_objects").real):
        assert sorted(side["order"].tolist()) == list(range(m))
    for name in ("nodes_device", "tiers_device", "cost_device", "descendants_at", "descendants_filtered",
                 "descendants_upto", "top_rows", "top_one"):
        for side in (SC.case(name).decoy, SC.case(name).real):
            p = side["pos"]
            assert ((p < SC.N) | (p == SC.N) | (p == SC.NONE)).all(), name
    for side in (SC.case("merge_rows").decoy, SC.case("merge_rows").real):
        assert side["tier_count"].shape == (12, SC.case("merge_rows").static["n"])


def test_shapes_reach_what_the_kernels_split_on():
    import s3imph
    S = s3imph.merge_geometry()
    starts = SC.case("merge_rows").static["run_starts"]
    assert len(starts) == 4 and (np.diff(starts.astype(np.int64)) > S).all()
    _, tile = s3imph.csv_geometry()
    assert 3 * tile < SC.case("csv").static["length"] < 8 * tile
    for name in ("descendants_at", "descendants_filtered", "descendants_upto"):
        for w in (SC.case(name).want_decoy, SC.case(name).want_real):
            assert w["total"] > 2048 and w["row_ptr"][-1] == w["total"] == len(w["out"]), name
    assert SC.case("top_rows").want_real["n_rows"] == SC.NQ and SC.case("top_one").want_real["n_rows"] == 1
    assert SC.case("top_one").want_real["top_n"].tolist() == [SC.K]


def test_same_reports_the_first_difference():
    a = {"x": np.arange(4, dtype=np.uint64), "n": 3}
    SC.same(dict(a), a)
    with pytest.raises(AssertionError, match=r"x\[2\] = 9, want 2"):
        SC.same({"x": np.array([0, 1, 9, 3], np.uint64), "n": 3}, a)
    with pytest.raises(AssertionError):
        SC.same({"x": a["x"].astype(np.int64), "n": 3}, a)
    with pytest.raises(AssertionError):
        SC.same({"x": a["x"], "n": 4}, a)
