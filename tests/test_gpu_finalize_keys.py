"""Finalize's key pass where keys cut, fill or exceed the 32 KiB staging window of
k_fin_keys_lds, where an lcp off by one byte or a '/' count leaking past a key's end changes
an answer, at depths beyond the first depth_offsets offer, and at the block pass's edges.

Every case runs the device form at a 16-byte aligned blob (the LDS-staged pass) and at views
shifted by 1, 8 and 15 bytes (the per-lane pass k_fin_keys); where noted also
finalize_index_host with a non-zero offsets[0].  All five arrays and max_depth are compared,
exactly, with oracle_lib.finalize (oracle/finalize_oracle.c).  The key sets and the window
regime each one reaches are stated on the CPU in tests/test_finalize_regimes.py.
"""
import functools

import numpy as np
import pytest

import finalize_keysets as K
import oracle as O
from conftest import to_dev

pytestmark = pytest.mark.gpu

ARRAYS = ("depth", "subtree_end", "max_depth_in_subtree", "depth_offsets", "depth_positions")
FILES = {"depth.u32": ("depth", 4), "subtree_end.u64": ("subtree_end", 8),
         "max_depth_in_subtree.u32": ("max_depth_in_subtree", 4), "depth_offsets.u64": ("depth_offsets", 8),
         "depth_positions.u64": ("depth_positions", 8)}
SHIFTS = (0, 1, 8, 15)


@pytest.fixture(scope="module")
def s3():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import s3imph
    return s3imph


@pytest.fixture(scope="module")
def ctx(s3):
    c = s3.DeviceBuilder(0)
    yield c
    c.close()


def _dev_view(a, shift):
    """`a` (u8) at `shift` bytes into a zeroed, 16-byte aligned device allocation: a view whose
    data pointer is `shift` mod 16, readable to round_up(len(a), 8) and 8 bytes on (the blob
    contract asks for round_up(len(a), 8) only)."""
    import torch
    a = np.ascontiguousarray(a, np.uint8)
    n = len(a)
    buf = torch.zeros(shift + (n + 7) // 8 * 8 + 8, dtype=torch.uint8, device="cuda")
    if n:
        buf[shift:shift + n] = torch.from_numpy(a.copy()).to("cuda")
    view = buf[shift:]
    assert buf.data_ptr() % 16 == 0
    assert view.data_ptr() % 16 == shift
    return view


def _unwrap(r):
    out = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in r.items()}
    for k in ("depth", "max_depth_in_subtree"):
        out[k] = out[k].view(np.uint32)
    for k in ("subtree_end", "depth_positions", "depth_offsets"):
        out[k] = out[k].view(np.uint64)
    return out


def _same(got, want, what):
    # lcp and depth go wrong before the hierarchy does: depth is compared first
    for k in ARRAYS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, (what, k, "first at", int(bad[0]), "got", int(g[bad[0]]), "want", int(w[bad[0]]),
                               "wrong", int(bad.size))
    assert got["max_depth"] == want["max_depth"], what


def _device_all_shifts(ctx, blob, offs, depths, want, what, depths_view=None):
    """The device form at each shift of the blob; `depths_view` replaces the depths tensor."""
    import torch
    n = len(offs) - 1
    d_offs = to_dev(offs)
    d_depths = depths_view
    if d_depths is None and depths is not None:
        d_depths = torch.from_numpy(np.array(depths, np.uint32).view(np.int32)).cuda()
    for shift in SHIFTS:
        r = ctx.finalize_index(_dev_view(blob, shift), d_offs, n, d_depths)
        torch.cuda.synchronize()
        _same(_unwrap(r), want, (what, "shift", shift))


def _host_form(s3, blob, offs, depths, want, tmp_path, what):
    """finalize_index_host behind 13 junk bytes (offsets[0] == 13); the files read back."""
    junk = np.frombuffer(b"/junk/bytes//", np.uint8)
    assert len(junk) == 13
    s3.finalize_index_host(np.concatenate([junk, blob]), offs + np.uint64(13), str(tmp_path),
                           None if depths is None else np.array(depths, np.uint32))
    for name, (k, w) in FILES.items():
        data = s3.read_array(str(tmp_path / name), w)
        assert np.array_equal(data, want[k]), (what, "host", name)


@functools.lru_cache(maxsize=None)
def _case(name, depths):
    """(blob, offsets, caller depths or None, the oracle's arrays) of a named set: computed
    once, shared, read-only."""
    keys = K.keyset(name)
    blob, offs = K.blob_of(keys)
    d = {"slashes": None, "hashed": K.hashed_depths(len(keys)), "true": K.true_depths(keys)}[depths]
    want = O.lib().finalize(blob, offs, d)
    for a in (blob, offs) + tuple(v for v in want.values() if hasattr(v, "setflags")) + (() if d is None else (d,)):
        a.setflags(write=False)
    return blob, offs, d, want


# ------------------------------------------------------------------------ a. comb ----
@pytest.mark.parametrize("depths", ["slashes", "hashed", "true"])
@pytest.mark.parametrize("name", ["comb", "comb_flip"])
def test_comb(s3, ctx, oracle_lib, tmp_path, name, depths):
    """Rounds cut by the window; one subtree_end per prefix of the spine, so an lcp wrong by
    one byte at any byte phase shows."""
    blob, offs, d, want = _case(name, depths)
    assert len(set(want["subtree_end"].tolist())) == 601
    _device_all_shifts(ctx, blob, offs, d, want, (name, depths))
    _host_form(s3, blob, offs, d, want, tmp_path, (name, depths))


# ------------------------------------------------------------------- b. mask leak ----
@pytest.mark.parametrize("name", ["mask_leak", "slash_sweep"])
def test_slash_count_stops_at_the_key_end(ctx, oracle_lib, name):
    blob, offs, d, want = _case(name, "slashes")
    if name == "mask_leak":
        keys = K.keyset(name)
        assert want["depth"].tolist() == [len(k) if k[0] == 0x2F else 0 for k in keys]
    else:
        assert set(want["depth"].tolist()) == {1}
    _device_all_shifts(ctx, blob, offs, d, want, name)


# ---------------------------------------------------------------------- c. ragged ----
def test_ragged_lengths_1_to_1024(s3, ctx, oracle_lib, tmp_path):
    """Most rounds cut; max_depth beyond the 64 depth_offsets entries offered first, so
    finalize_index and finalize_from_host both take their capacity retry."""
    blob, offs, d, want = _case("ragged", "slashes")
    assert want["max_depth"] >= 63
    _device_all_shifts(ctx, blob, offs, d, want, "ragged")
    _host_form(s3, blob, offs, d, want, tmp_path, "ragged")


# ------------------------------------------------------------------- d. exact fit ----
@pytest.mark.parametrize("name", ["exact_fit", "exact_fit_plus1", "exact_fit_slash", "exact_fit_slash_plus1"])
def test_key_ending_at_the_window_end(ctx, oracle_lib, name):
    """The 32nd 1024-byte key ends at the window's last byte, or one byte past it; in the
    _slash sets that byte is a '/', so it counts only if it is read from where it lies."""
    blob, offs, d, want = _case(name, "slashes")
    _device_all_shifts(ctx, blob, offs, d, want, name)


# -------------------------------------------------------------------- e. oversize ----
@pytest.mark.parametrize("depths", ["slashes", "hashed"])
@pytest.mark.parametrize("name", ["oversize_first", "oversize_last", "oversize_nested"])
def test_keys_longer_than_the_window(s3, ctx, oracle_lib, tmp_path, name, depths):
    blob, offs, d, want = _case(name, depths)
    if name == "oversize_nested":
        assert want["subtree_end"][300:305].tolist() == [304] * 5
    _device_all_shifts(ctx, blob, offs, d, want, (name, depths))
    _host_form(s3, blob, offs, d, want, tmp_path, (name, depths))


# ----------------------------------------------------------- f. depth-index edges ----
PLACED = [[(1234, v)] for v in K.EDGE_DEPTHS] + [
    [(2999, 64)],                                       # the deep key is the last key
    [(0, 70_000)],                                      # ... the first key
    [(5, 62), (1234, 70_000), (2000, 255), (2999, 3)],  # gaps of 1, 58, 192 and tens of thousands
]


@pytest.mark.parametrize("placed", PLACED, ids=["+".join("%d@%d" % (v, p) for p, v in pl) for pl in PLACED])
def test_depth_index_edges(s3, ctx, oracle_lib, tmp_path, placed):
    """Caller depths on both sides of the 64-entry first offer, at the radix sort's 8/9 and
    16/17 key bits, with wide gaps between occupied depths (k_fin_doff)."""
    import torch
    keys = K.short_tree()
    blob, offs = K.blob_of(keys)
    depths = K.edge_depths(len(keys), placed)
    want = oracle_lib.finalize(blob, offs, depths)
    assert want["max_depth"] == max(v for _, v in placed)
    assert len(want["depth_offsets"]) == want["max_depth"] + 2
    d_depths = torch.from_numpy(depths.view(np.int32)).cuda()
    r = ctx.finalize_index(to_dev(blob, pad8=True), to_dev(offs), len(keys), d_depths)
    torch.cuda.synchronize()
    _same(_unwrap(r), want, ("aligned", placed))
    r = ctx.finalize_index(_dev_view(blob, 8), to_dev(offs), len(keys), d_depths)
    torch.cuda.synchronize()
    _same(_unwrap(r), want, ("shift 8", placed))
    _host_form(s3, blob, offs, depths, want, tmp_path, placed)


# ------------------------------------------------------------ g. block-pass edges ----
@pytest.mark.parametrize("n", K.BLOCK_EDGE_N)
def test_block_pass_edges_with_unaligned_caller_depths(ctx, oracle_lib, n):
    """Caller depths as a view 4 bytes into an allocation: k_fin_blocks takes its per-lane
    branch for every lane, at n % 4 in 0..3 and n on both sides of the 1024-key block."""
    import torch
    keys = K.comb_cut(n)
    blob, offs = K.blob_of(keys)
    depths = K.hashed_depths(n)
    want = oracle_lib.finalize(blob, offs, depths)
    buf = torch.zeros(n + 4, dtype=torch.int32, device="cuda")
    buf[1:n + 1] = torch.from_numpy(depths.view(np.int32)).cuda()
    view = buf[1:n + 1]
    assert view.data_ptr() % 16 == 4
    _device_all_shifts(ctx, blob, offs, None, want, ("comb_cut", n), depths_view=view)
    # and the '/' count at the same sizes, into the library's own (aligned) depth array
    _device_all_shifts(ctx, blob, offs, None, oracle_lib.finalize(blob, offs), ("comb_cut slashes", n))
