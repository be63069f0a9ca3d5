"""Inputs and expected answers for tests/test_gpu_streams.py (no GPU here).

Every case holds two inputs of identical shape for one device entry point, a decoy and the real
one, and the answer the existing restatements give for each (sort_ref, aggregate_ref, tiers_ref,
csv_ref, merge_ref, pricing_ref, finalize_queries, the oracle).  The two share their offsets arrays
(fixed-width keys, monotone byte substitutions) and their record structure, so whatever mixture of
the two a misordered kernel reads stays in bounds; indices (the gather's order, query positions) are
in range in both, or are the values the kernels check (n, 2^64 - 1).  Their answers differ, which is
what lets the GPU test tell which of the two the library read; tests/test_stream_cases.py asserts
both properties for every case.

A case's inputs are numpy arrays by name (u64 / u32 kept unsigned here); `want` maps the names of
the outputs the GPU test reads back to arrays, ints or bytes, compared exactly by `same`."""
import functools
from dataclasses import dataclass, field

import numpy as np

import aggregate_ref as A
import csv_ref
import finalize_queries as Q
import merge_ref as M
import oracle as O
import pricing_cases as C
import pricing_ref as P
import s3imph
import sort_ref
import tiers_ref as T
from test_gpu_pricing import K, N, SLOTS, key_columns, tree_prefixes

NONE = (1 << 64) - 1
TIER_IDS = SLOTS[5]
FAMILIES = ("build", "listing", "merge", "reader")


@dataclass
class Case:
    name: str
    family: str
    decoy: dict
    real: dict
    want_decoy: dict
    want_real: dict
    static: dict = field(default_factory=dict)  # what both inputs share besides the shapes


def same(got: dict, want: dict, what: str = "") -> None:
    """Every entry of `want` against `got`, exactly: arrays by dtype, shape and value."""
    for name, w in want.items():
        g = got[name]
        if isinstance(w, np.ndarray):
            g = np.asarray(g)
            assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.dtype, w.shape)
            if g.tobytes() != w.tobytes():
                flat = np.flatnonzero(np.frombuffer(g.tobytes(), np.uint8) != np.frombuffer(w.tobytes(), np.uint8))
                at = int(flat[0]) // max(w.dtype.itemsize, 1)
                raise AssertionError(f"{what}: {name}[{at}] = {g.reshape(-1)[at]}, want {w.reshape(-1)[at]} "
                                     f"({len(flat)} bytes differ)")
        else:
            assert g == w, (what, name, g, w)


def differ(a: dict, b: dict) -> bool:
    try:
        same(a, b)
    except AssertionError:
        return True
    return False


def padded(blob) -> np.ndarray:
    """A key blob readable up to its length rounded up to 8 bytes, and a word beyond."""
    blob = np.frombuffer(bytes(blob), np.uint8) if not isinstance(blob, np.ndarray) else blob
    out = np.zeros((len(blob) + 7) // 8 * 8 + 8, np.uint8)
    out[:len(blob)] = blob
    return out


def _blob(keys):
    blob, offs = O.keys_to_blob(keys)
    return padded(blob), offs


# ---- the MPHF build, its lookup and the finalize: a sorted prefix set ----------------------------
def prefix_sets():
    """3180 byte-sorted prefixes of three fixed widths.  The real set substitutes d -> e, s -> t,
    o -> p (monotone, so it stays sorted) and ends every seventh leaf in '0' instead of '/', which
    changes that leaf's depth and with it every finalize array."""
    dec, real = [], []
    for d in range(30):
        dec.append(b"d%02d/" % d)
        real.append(b"e%02d/" % d)
        for s in range(5):
            dec.append(b"d%02d/s%d/" % (d, s))
            real.append(b"e%02d/t%d/" % (d, s))
            for o in range(20):
                dec.append(b"d%02d/s%d/o%04d/" % (d, s, o))
                real.append(b"e%02d/t%d/p%04d" % (d, s, o) + (b"0" if o % 7 == 3 else b"/"))
    assert dec == sorted(set(dec)) and real == sorted(set(real))
    return dec, real


def _build_want(keys):
    blob, offs = O.keys_to_blob(keys)
    st, fp, po, mph = O.lib().build(blob, offs)
    assert st == 0
    n = len(keys)
    return {"fp": fp, "pos": po, "mph": mph, "lookup": np.arange(n, dtype=np.uint64),
            "n_keys": n, "mph_bin_len": len(mph), "status": 0}


def build_case():
    dec, real = prefix_sets()
    (db, do), (rb, ro) = _blob(dec), _blob(real)
    return Case("build", "build", {"blob": db, "offsets": do}, {"blob": rb, "offsets": ro},
                _build_want(dec), _build_want(real), {"n": len(dec)})


def _oracle_lookup(mph_bin, fp, po, queries):
    st, mph = O.lib().unmarshal(mph_bin)
    assert st == 0
    hits = [O.lib().lookup(mph, fp, po, q) for q in queries]
    return np.array([NONE if h is None else h for h in hits], np.uint64)


def lookup_case():
    """Lookups against the decoy set's MPHF (loaded before the run, static): the decoy queries are
    its members in order, the real ones its leaves in reverse with every fifth a non-member."""
    dec, _ = prefix_sets()
    w = _build_want(dec)
    leaves = [i for i, k in enumerate(dec) if len(k) == 13]
    real = list(dec)
    for j, i in enumerate(leaves):
        real[i] = dec[leaves[-1 - j]] if j % 5 else b"x" + dec[i][1:]
    (db, do), (rb, ro) = _blob(dec), _blob(real)
    static = {"mph": w["mph"], "fp": w["fp"], "pos": w["pos"], "n": len(dec), "nq": len(dec)}
    return Case("lookup", "build", {"blob": db, "offsets": do}, {"blob": rb, "offsets": ro},
                {"result": _oracle_lookup(w["mph"], w["fp"], w["pos"], dec)},
                {"result": _oracle_lookup(w["mph"], w["fp"], w["pos"], real)}, static)


def _finalize_want(keys):
    arr = O.lib().finalize(*O.keys_to_blob(keys))
    return {"depth": arr["depth"], "subtree_end": arr["subtree_end"],
            "max_depth_in_subtree": arr["max_depth_in_subtree"], "depth_positions": arr["depth_positions"],
            "depth_offsets": arr["depth_offsets"], "max_depth": int(arr["max_depth"])}


def finalize_case():
    dec, real = prefix_sets()
    (db, do), (rb, ro) = _blob(dec), _blob(real)
    return Case("finalize_index", "build", {"blob": db, "offsets": do}, {"blob": rb, "offsets": ro},
                _finalize_want(dec), _finalize_want(real), {"n": len(dec)})


# ---- the listing stages: object keys of one width ------------------------------------------------
M_OBJ = 3000


def listing(real: bool):
    """3000 byte-sorted object keys of 15 bytes, one u64 size and one tier id each."""
    a, b = (b"e", b"t") if real else (b"d", b"s")
    keys = [a + b"%02d/" % (i // 100) + b + b"%d/obj-%04d" % ((i // 20) % 5, i % 20) for i in range(M_OBJ)]
    assert keys == sorted(set(keys)) and all(len(k) == 15 for k in keys)
    rng = np.random.default_rng(11 + real)
    sizes = rng.integers(0, 1 << 40, M_OBJ, dtype=np.uint64)
    sizes[7] = NONE - 5  # the sums wrap
    return keys, sizes, rng.integers(0, 12, M_OBJ).astype(np.uint8)


def shuffled(real: bool):
    keys, sizes, tiers = listing(real)
    perm = np.random.default_rng(21 + real).permutation(M_OBJ)
    keys = [keys[i] for i in perm]
    if real:  # equal keys: the sort is stable, n_equal counts them
        keys[10], keys[2000] = keys[20], keys[30]
    return keys, sizes[perm], tiers[perm]


def sort_case():
    ins, wants = [], []
    for real in (False, True):
        keys, _, _ = shuffled(real)
        blob, offs = _blob(keys)
        ins.append({"keys": blob, "offsets": offs})
        wants.append(dict(sort_ref.info(keys), order=sort_ref.sort_order(keys)))
    return Case("sort_objects", "listing", ins[0], ins[1], wants[0], wants[1], {"m": M_OBJ})


def gather_case():
    ins, wants = [], []
    for real in (False, True):
        keys, sizes, tiers = shuffled(real)
        order = sort_ref.sort_order(keys)
        blob, offs = _blob(keys)
        ins.append({"keys": blob, "offsets": offs, "sizes": sizes, "tiers": tiers, "order": order})
        out = b"".join(keys[i] for i in order)
        assert out == b"".join(sorted(keys))
        wants.append({"keys": np.frombuffer(out + b"\0" * (-len(out) % 8), np.uint8), "offsets": offs.copy(),
                      "sizes": sizes[order], "tiers": tiers[order], "key_bytes": len(out)})
    return Case("gather_objects", "listing", ins[0], ins[1], wants[0], wants[1], {"m": M_OBJ})


def aggregate_case():
    ins, wants = [], []
    for real in (False, True):
        keys, sizes, tiers = listing(real)
        blob, offs = _blob(keys)
        ins.append({"keys": blob, "offsets": offs, "sizes": sizes, "tiers": tiers})
        rows = T.aggregate_dict_tiers(keys, sizes, tiers)
        assert [r[:4] for r in rows] == A.aggregate_dict(keys, sizes)
        pb, po, depth, cnt, tot = A.rows_to_arrays([r[:4] for r in rows])
        tc, tb = T.tier_arrays(rows)
        wants.append({"blob": np.concatenate([pb, np.zeros(-len(pb) % 8, np.uint8)]), "offsets": po, "depth": depth,
                      "object_count": cnt, "total_bytes": tot, "tier_count": tc, "tier_bytes": tb,
                      "n_prefixes": len(rows), "blob_bytes": len(pb), "n_objects": M_OBJ,
                      "total_bytes_sum": int(sum(int(z) for z in sizes) & NONE), "first_unsorted": NONE,
                      "max_depth_seen": 2, "present_mask": T.present_mask(tiers), "first_bad_tier": NONE})
    return Case("aggregate", "listing", ins[0], ins[1], wants[0], wants[1], {"m": M_OBJ})


CSV_ROWS = 1000
CSV_SCHEMA = (0, 1, 2, 3)


def csv_text(real: bool) -> bytes:
    """1000 records of 36 bytes (a few 8 KiB tiles), the fields at the same offsets in both texts:
    keys of one width, sizes of seven digits, two storage classes of ten letters."""
    keys, sizes, _ = listing(real)
    rows = []
    for i in range(CSV_ROWS):
        cls = (b"GLACIER_IR", b"ONEZONE_IA")[(i % 3 == 0) if real else i % 2]
        rows.append(keys[i] + b",%07d," % (int(sizes[i]) % 10_000_000) + cls + b",\n")
    text = b"".join(rows)
    assert len(text) == 36 * CSV_ROWS
    return text


def csv_case():
    ins, wants = [], []
    for real in (False, True):
        text = csv_text(real)
        rec = csv_ref.records(text, CSV_SCHEMA)
        assert rec["keys"] == csv_ref.records(text, CSV_SCHEMA, csv_ref.parse_automaton)["keys"]
        blob, offs = csv_ref.listing(rec)
        ins.append({"csv": padded(np.frombuffer(text, np.uint8))})
        wants.append(dict(rec["info"], keys=np.frombuffer(blob, np.uint8), offsets=offs, sizes=rec["sizes"],
                          tiers=rec["tiers"]))
    return Case("csv", "listing", ins[0], ins[1], wants[0], wants[1], {"length": 36 * CSV_ROWS, "schema": CSV_SCHEMA})


# ---- the row merge: three sorted runs past the sample step ---------------------------------------
def merge_runs(real: bool):
    S = s3imph.merge_geometry()
    lead = b"m/%06d/" if real else b"k/%06d/"
    runs = []
    for r, (lo, n, step) in enumerate(((0, 2 * S + 1, 3), (1, S + 1, 2), (2, 2 * S + 2, 5))):
        run = []
        for i in range(n):
            c = (7 if real else 1) + 100 * r + i
            run.append(M.row(lead % (lo + i * step), 1 + (i + real) % 2, c, c * 1000 + 7,
                             {(i + real) % 12: (c, c * 1000 + 7), (i + 5) % 12: (1, 0)}))
        runs.append(run)
    return runs


def merge_case():
    ins, wants, starts = [], [], None
    for real in (False, True):
        runs = merge_runs(real)
        flat = [r for run in runs for r in run]
        blob, offs, depth, cnt, nbytes, tc, tb = M.to_arrays(flat)
        starts = np.concatenate([[0], np.cumsum([len(run) for run in runs])]).astype(np.uint64)
        ins.append({"blob": padded(blob), "offsets": offs, "depth": depth, "count": cnt, "bytes": nbytes,
                    "tier_count": tc, "tier_bytes": tb})
        rows = M.merge_heap(runs)
        assert rows == M.merge_dict(runs) and M.first_unsorted(runs) is None
        ob, oo, od, oc, on, otc, otb = M.to_arrays(rows)
        wants.append({"blob": np.concatenate([ob, np.zeros(-len(ob) % 8, np.uint8)]), "offsets": oo, "depth": od,
                      "object_count": oc, "total_bytes": on, "tier_count": otc, "tier_bytes": otb,
                      "consumed": (oc + on), "n_in": len(flat), "n_out": len(rows), "blob_bytes": len(ob),
                      "first_unsorted": NONE, "present_mask": M.present_mask(rows),
                      "max_depth_seen": max(r[1] for r in rows), "n_runs": len(runs)})
    return Case("merge_rows", "merge", ins[0], ins[1], wants[0], wants[1],
                {"run_starts": starts, "n": int(starts[-1])})


# ---- the reader: one index (static), late query arrays -------------------------------------------
@functools.lru_cache(maxsize=None)
def reader_tree():
    """The tree of tests/test_gpu_pricing.py (4096 nodes, one parent with 2100 children) with its
    stats and the fixture's columns for five tiers: everything the reader cases are answered from."""
    prefixes = tree_prefixes()
    blob, offs = O.keys_to_blob(prefixes)
    st, fp, po, mph = O.lib().build(blob, offs)
    assert st == 0
    arr = O.lib().finalize(blob, offs)
    tc, tb = np.zeros((12, N), np.uint64), np.zeros((12, N), np.uint64)
    for t in TIER_IDS:
        tc[t], tb[t] = C.COUNT[:, t], C.BYTES[:, t]
    return {"prefixes": prefixes, "arr": arr, "stats": key_columns(), "tc": tc, "tb": tb, "mph": mph, "fp": fp,
            "pos": po, "at": {p: i for i, p in enumerate(prefixes)}}


NQ = 600


def reader_positions(real: bool) -> np.ndarray:
    """600 query positions: big/ (2100 children, so the rows pass a 2048-position chunk), the root,
    parents of few children, nodes all over the tree, and the two checked values n and 2^64 - 1."""
    t = reader_tree()
    rng = np.random.default_rng(31 + real)
    pos = rng.integers(0, N, NQ).astype(np.uint64)
    named = [t["at"][p] for p in (b"big/", b"p00/", b"p01/", b"p09/", b"p10/", b"p11/", b"")]
    if real:
        named = named[::-1]
    pos[:len(named)] = named
    pos[NQ // 2], pos[NQ - 1 - real] = N, NONE
    return pos


def reader_lookup_case():
    t = reader_tree()
    ins, wants = [], []
    for real in (False, True):
        lo = 1500 if real else 0
        keys = [b"big/c%04d/" % (lo + j) for j in range(NQ)]
        if real:
            keys = keys[::-1]
            keys[3::7] = [b"big/x%04d/" % j for j in range(len(keys[3::7]))]  # not members
        blob, offs = _blob(keys)
        ins.append({"blob": blob, "offsets": offs})
        wants.append({"pos": _oracle_lookup(t["mph"], t["fp"], t["pos"], keys)})
        assert (wants[-1]["pos"] == NONE).sum() == (len(keys[3::7]) if real else 0)
    return Case("lookup_device", "reader", ins[0], ins[1], wants[0], wants[1], {"nq": NQ})


def _nodes_want(pos):
    t = reader_tree()
    arr, (oc, tb) = t["arr"], t["stats"]
    out = np.zeros(len(pos), s3imph.NODE_DTYPE)
    for q, p in enumerate(int(v) for v in pos):
        if p < N:
            out[q] = (p, arr["subtree_end"][p], oc[p], tb[p], arr["depth"][p], arr["max_depth_in_subtree"][p], 1, 0)
    return {"nodes": out}


def _tiers_want(pos):
    t = reader_tree()
    out = np.zeros((len(pos), len(TIER_IDS), 2), np.uint64)
    mask = np.zeros(len(pos), np.uint32)
    for q, p in enumerate(int(v) for v in pos):
        for s, (_, _, nbytes, count) in enumerate(T.get_breakdown_all(TIER_IDS, t["tc"], t["tb"], p)):
            out[q, s] = (count, nbytes)
            mask[q] |= np.uint32((1 << s) if (count | nbytes) else 0)
    return {"tiers": out, "mask": mask}


def _cost_want(pos):
    ref = C.ref_records("default", TIER_IDS)
    out = np.zeros(len(pos), s3imph.COST_DTYPE)
    for q, p in enumerate(int(v) for v in pos):
        r = ref[p] if p < N else P.ZERO_COST
        out[q] = (r["total"], r["monitoring"], r["min_object_size"], r["glacier_overhead"], r["per_tier"],
                  r["tier_mask"], r["found"])
    return {"cost": out}


def _position_case(name, want_of):
    d, r = reader_positions(False), reader_positions(True)
    return Case(name, "reader", {"pos": d}, {"pos": r}, want_of(d), want_of(r), {"nq": NQ})


def _csr(rows, levels):
    """The CSR the reader returns for `rows` (lists of positions) and the queries' levels."""
    lens = [len(r) for r in rows]
    flat = [p for r in rows for p in r]
    return {"levels": np.array(levels, np.int32), "row_ptr": np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64),
            "out": np.array(flat, np.uint64), "n_rows": len(rows), "total": len(flat)}, rows


def _kept(row, min_count, min_bytes):
    oc, tb = reader_tree()["stats"]
    if not (min_count or min_bytes):
        return row
    return [p for p in row if int(oc[p]) >= min_count and int(tb[p]) >= min_bytes]


def _at_rows(pos, rel, min_count=0, min_bytes=0):
    arr = reader_tree()["arr"]
    rows, levels = [], []
    for p, r in zip((int(v) for v in pos), (int(v) for v in rel)):
        got = Q.descendants_at_depth(arr, p, r) if p < N else None
        levels.append(0 if got is None else 1)
        rows.append(_kept(got or [], min_count, min_bytes))
    return _csr(rows, levels)


def _upto_rows(pos, max_rel):
    arr = reader_tree()["arr"]
    R = min(max(max_rel, 0), int(arr["max_depth"]))
    rows, levels = [], []
    for p in (int(v) for v in pos):
        got = (Q.descendants_up_to_depth(arr, p, max_rel) if p < N else None) or []
        levels.append(len(got))
        rows += got + [[]] * (R - len(got))
    return _csr(rows, levels)


def reader_rels(real: bool) -> np.ndarray:
    rel = np.random.default_rng(41 + real).integers(-1, 4, NQ).astype(np.int32)
    rel[:8] = 1
    return rel


def descendants_at_case(min_count=0):
    ins, wants = [], []
    for real in (False, True):
        pos, rel = reader_positions(real), reader_rels(real)
        ins.append({"pos": pos, "rel": rel})
        wants.append(_at_rows(pos, rel, min_count)[0])
        assert wants[-1]["total"] > 2048
    name = "descendants_filtered" if min_count else "descendants_at"
    return Case(name, "reader", ins[0], ins[1], wants[0], wants[1], {"nq": NQ, "min_count": min_count})


def descendants_upto_case():
    d, r = reader_positions(False), reader_positions(True)
    return Case("descendants_upto", "reader", {"pos": d}, {"pos": r}, _upto_rows(d, 2)[0], _upto_rows(r, 2)[0],
                {"nq": NQ, "max_rel": 2})


def _top_want(csr_rows, key_of, k):
    want, rows = csr_rows
    top_n = np.zeros(len(rows), np.int32)
    top_pos = np.full((len(rows), k), NONE, np.uint64)
    top_key = np.zeros((len(rows), k), np.uint64)
    for r, row in enumerate(rows):
        best = P.top_of_row(row, key_of, k)
        top_n[r] = len(best)
        top_pos[r, :len(best)] = best
        top_key[r, :len(best)] = [key_of[p] for p in best]
    return {"top_n": top_n, "top_pos": top_pos, "top_key": top_key, "n_rows": want["n_rows"]}


def top_rows_case():
    """Many rows (the segmented sort), ranked by cost."""
    ref = C.ref_records("default", TIER_IDS)
    key_of = [r["total"] for r in ref]
    ins, wants = [], []
    for real in (False, True):
        pos, rel = reader_positions(real), reader_rels(real)
        ins.append({"pos": pos, "rel": rel})
        wants.append(_top_want(_at_rows(pos, rel), key_of, K))
    return Case("top_rows", "reader", ins[0], ins[1], wants[0], wants[1], {"nq": NQ, "key": "cost", "k": K})


def top_one_case():
    """One row (sorted device-wide), ranked by object count: big/'s children against the root's."""
    t = reader_tree()
    key_of = [int(v) for v in t["stats"][0]]
    ins, wants = [], []
    for name in (b"big/", b""):
        pos, rel = np.array([t["at"][name]], np.uint64), np.array([1], np.int32)
        ins.append({"pos": pos, "rel": rel})
        wants.append(_top_want(_at_rows(pos, rel), key_of, K))
    return Case("top_one", "reader", ins[0], ins[1], wants[0], wants[1], {"nq": 1, "key": "count", "k": K})


BUILDERS = {
    "build": build_case, "lookup": lookup_case, "finalize_index": finalize_case,
    "sort_objects": sort_case, "gather_objects": gather_case, "aggregate": aggregate_case, "csv": csv_case,
    "merge_rows": merge_case,
    "lookup_device": reader_lookup_case,
    "nodes_device": lambda: _position_case("nodes_device", _nodes_want),
    "tiers_device": lambda: _position_case("tiers_device", _tiers_want),
    "cost_device": lambda: _position_case("cost_device", _cost_want),
    "descendants_at": descendants_at_case, "descendants_filtered": lambda: descendants_at_case(5),
    "descendants_upto": descendants_upto_case, "top_rows": top_rows_case, "top_one": top_one_case,
}
NAMES = tuple(BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name: str) -> Case:
    """The case, built once and shared; nothing may change its arrays."""
    c = BUILDERS[name]()
    for d in (c.decoy, c.real, c.want_decoy, c.want_real):
        for a in d.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return c
