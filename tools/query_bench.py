#!/usr/bin/env python3
"""Batched reader queries on one GPU (s3imph.Index), each figure beside what it is to be
read against.  One process; every timed section runs under its own time limit (SIGALRM with
its default action: a section that hangs ends the process, nothing more is started).

Index: C2's 10M synthetic prefixes (gen_keys(0, 42, 32, 0, 10_000_000)), MPHF and finalize
arrays built on the GPU, random object_count / total_bytes, attached with Index.from_arrays.

  (a) lookup + nodes (StatsForPrefix) for 1M member prefixes, queries/s
        against MPHF.Lookup alone (s3imph_lookup_device, what the library had before)
  (a, tiers) the batched tier breakdown (TierBreakdownAll + TierBreakdown's mask, 12 tiers) for the
        same 1M positions, queries/s and GB/s of table read + result written,
        against nodes_device on those positions, and against the same answer gathered from
        column-major columns ([12][n] counts and bytes, torch.index_select: 24 scattered 8-byte
        loads per query) — the layout the interleaved [n][2T] table replaces
  (b) DescendantsAtDepth at rel = 1 for 1M random positions, queries/s, plan and fill apart
        against the numpy searchsorted restatement on the host (on --host-queries of them);
        C2's nodes below the root are leaves, so these rows are empty: the same positions at
        rel = 0 (one position per row), plain and filtered, are timed beside them
  (c) the root at every rel, GB/s of the fill at 16 B per position (8 read + 8 written)
        against a device-to-device copy of the same bytes

All calls wait for their stream, so the host clock around a call times the device work plus
its launch; each figure is the median of --reps calls after --warmup.  Prints one JSON line.

    python tools/query_bench.py [--keys 10000000] [--queries 1000000] [--reps 20]
"""
import argparse
import json
import os
import signal
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "s3-inv-db_amd"))

import numpy as np  # noqa: E402


class section:
    """A timed section with a hard limit: past it the process is terminated."""

    def __init__(self, name, limit):
        self.name, self.limit = name, limit

    def __enter__(self):
        signal.signal(signal.SIGALRM, signal.SIG_DFL)
        signal.alarm(self.limit)
        print(f"[query_bench] {self.name} (limit {self.limit} s)", file=sys.stderr, flush=True)

    def __exit__(self, *exc):
        signal.alarm(0)


def median_s(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts), max(ts)


def host_at(arr, pos, rel):
    """DescendantsAtDepth through numpy.searchsorted (index.go:206-228, depthindex.go:193-259)."""
    t = int(arr["depth"][pos]) + rel
    if rel < 0 or t > arr["max_depth"]:
        return None
    o = arr["depth_offsets"]
    sl = arr["depth_positions"][int(o[t]):int(o[t + 1])]
    lo = np.searchsorted(sl, np.uint64(pos), "left")
    hi = np.searchsorted(sl, arr["subtree_end"][pos], "right")
    return sl[lo:max(lo, hi)]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--keys", type=int, default=10_000_000)
    ap.add_argument("--queries", type=int, default=1_000_000)
    ap.add_argument("--host-queries", type=int, default=50_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=120, help="seconds per section")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()

    import torch
    import s3imph
    if not torch.cuda.is_available():
        sys.exit("query_bench: no GPU (there is no CPU fallback)")
    dev = f"cuda:{a.device}"
    n, nq = a.keys, min(a.queries, a.keys)
    rng = np.random.default_rng(7)
    res = {"bench": "query", "keys": n, "queries": nq, "reps": a.reps, "device": torch.cuda.get_device_name(a.device)}

    with section("build the index on the GPU", a.limit):
        blob, offs = s3imph.gen_keys(0, 42, 32, 0, n)
        d_blob = torch.from_numpy(blob).to(dev)
        d_offs = torch.from_numpy(offs.view(np.int64)).to(dev)
        d_fp = torch.empty(n, dtype=torch.int64, device=dev)
        d_po = torch.empty(n, dtype=torch.int64, device=dev)
        ctx = s3imph.DeviceBuilder(a.device)
        ctx.build(d_blob, d_offs, n, d_fp, d_po)
        f = ctx.finalize_index(d_blob, d_offs, n)
        oc = rng.integers(0, 2**64, n, dtype=np.uint64)
        tb = rng.integers(0, 2**64, n, dtype=np.uint64)
        d_oc = torch.from_numpy(oc.view(np.int64)).to(dev)
        d_tb = torch.from_numpy(tb.view(np.int64)).to(dev)
        idx = s3imph.Index.from_arrays(ctx.mph_bin(), d_fp, d_po, f["depth"], f["subtree_end"],
                                       f["max_depth_in_subtree"], f["depth_offsets"], f["depth_positions"],
                                       f["max_depth"], d_oc, d_tb)
        arr = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in f.items()}
        for k in ("subtree_end", "depth_positions", "depth_offsets"):
            arr[k] = arr[k].view(np.uint64)
        for k in ("depth", "max_depth_in_subtree"):
            arr[k] = arr[k].view(np.uint32)
        res["max_depth"] = int(idx.max_depth)

    with section("(a) lookup + nodes, 1M member prefixes", a.limit):
        members = rng.choice(n, nq, replace=False).astype(np.int64)
        lens = (offs[members + 1] - offs[members]).astype(np.int64)
        qoffs = np.zeros(nq + 1, np.uint64)
        qoffs[1:] = np.cumsum(lens)
        src = np.repeat(offs[members].astype(np.int64) - qoffs[:-1].astype(np.int64), lens) + \
            np.arange(int(qoffs[-1]), dtype=np.int64)
        qblob = np.zeros((int(qoffs[-1]) + 7) // 8 * 8 + 8, np.uint8)
        qblob[: int(qoffs[-1])] = blob[src]
        d_qblob = torch.from_numpy(qblob).to(dev)
        d_qoffs = torch.from_numpy(qoffs.view(np.int64)).to(dev)
        d_res = torch.empty(nq, dtype=torch.int64, device=dev)

        def stats_for_prefix():
            return idx.nodes_device(idx.lookup_device(d_qblob, d_qoffs, nq))

        def mphf_lookup():  # the lookup the library had before the reader
            ctx.lookup(d_qblob, d_qoffs, nq, d_fp, d_po, n, d_res)

        got = stats_for_prefix().cpu().numpy().reshape(-1).view(s3imph.NODE_DTYPE)
        assert np.array_equal(got["pos"], members.astype(np.uint64)) and got["found"].all()
        assert np.array_equal(got["object_count"], oc[members])
        mphf_lookup()
        assert np.array_equal(d_res.cpu().numpy().view(np.uint64), members.astype(np.uint64))
        t, lo, hi = median_s(stats_for_prefix, a.warmup, a.reps)
        tb_, blo, bhi = median_s(mphf_lookup, a.warmup, a.reps)
        res["a_lookup_nodes_qps"] = nq / t
        res["a_lookup_nodes_ms"] = [1e3 * t, 1e3 * lo, 1e3 * hi]
        res["a_baseline_mphf_lookup_qps"] = nq / tb_
        res["a_baseline_mphf_lookup_ms"] = [1e3 * tb_, 1e3 * blo, 1e3 * bhi]

    with section("(a, tiers) tier breakdown of the same 1M positions", a.limit):
        g = torch.Generator(device=dev)
        g.manual_seed(11)
        d_tc = torch.randint(0, 1 << 40, (12, n), dtype=torch.int64, device=dev, generator=g)
        d_tbt = torch.randint(0, 1 << 50, (12, n), dtype=torch.int64, device=dev, generator=g)
        d_tc[:, ::3] = 0
        d_tbt[:, ::3] = 0
        idx.attach_tiers(list(range(12)), d_tc, d_tbt)
        d_mpos = torch.from_numpy(members.astype(np.uint64).view(np.int64)).to(dev)
        out, mask = idx.tiers_device(d_mpos)
        assert torch.equal(out[:, :, 0], d_tc[:, d_mpos].T) and torch.equal(out[:, :, 1], d_tbt[:, d_mpos].T)
        assert torch.equal(mask.cpu() != 0, torch.from_numpy(members % 3 != 0))
        del out, mask

        def tiers():
            return idx.tiers_device(d_mpos)

        def nodes():
            return idx.nodes_device(d_mpos)

        def column_major():
            r = torch.index_select(d_tc, 1, d_mpos), torch.index_select(d_tbt, 1, d_mpos)
            torch.cuda.synchronize()
            return r

        tt, tlo, thi = median_s(tiers, a.warmup, a.reps)
        tn, nlo, nhi = median_s(nodes, a.warmup, a.reps)
        tcm, clo, chi = median_s(column_major, a.warmup, a.reps)
        res["a_tiers_qps"] = nq / tt
        res["a_tiers_ms"] = [1e3 * tt, 1e3 * tlo, 1e3 * thi]
        res["a_tiers_gbps"] = 1e-9 * nq * (2 * 192 + 8 + 4) / tt
        res["a_tiers_baseline_nodes_ms"] = [1e3 * tn, 1e3 * nlo, 1e3 * nhi]
        res["a_tiers_ratio_to_nodes"] = tt / tn
        res["a_tiers_column_major_gather_ms"] = [1e3 * tcm, 1e3 * clo, 1e3 * chi]
        res["a_tiers_ratio_to_column_major"] = tt / tcm
        del d_tc, d_tbt

    with section("(b) DescendantsAtDepth rel = 1, 1M random positions", a.limit):
        qpos = rng.integers(0, n, nq).astype(np.uint64)
        d_qpos = torch.from_numpy(qpos.view(np.int64)).to(dev)
        d_rel = torch.ones(nq, dtype=torch.int32, device=dev)
        levels, row_ptr, out = idx.descendants_csr(d_qpos, d_rel)
        lv, rp, o = levels.cpu().numpy(), row_ptr.cpu().numpy(), out.cpu().numpy().view(np.uint64)
        hq = min(a.host_queries, nq)
        t0 = time.perf_counter()
        want = [host_at(arr, int(p), 1) for p in qpos[:hq]]
        t_host = time.perf_counter() - t0
        for q, w in enumerate(want):
            assert (w is None) == (lv[q] == 0) and (w is None or np.array_equal(w, o[rp[q]:rp[q + 1]])), q
        total = int(rp[-1])
        tp, plo, phi = median_s(lambda: idx.descendants_plan(d_qpos, d_rel), a.warmup, a.reps)
        tf, flo, fhi = median_s(lambda: idx.descendants_fill(total), a.warmup, a.reps)
        res["b_total_positions"] = total
        res["b_plan_qps"] = nq / tp
        res["b_fill_qps"] = nq / tf
        res["b_plan_fill_qps"] = nq / (tp + tf)
        res["b_plan_ms"] = [1e3 * tp, 1e3 * plo, 1e3 * phi]
        res["b_fill_ms"] = [1e3 * tf, 1e3 * flo, 1e3 * fhi]
        res["b_baseline_host_searchsorted_qps"] = hq / t_host
        res["b_baseline_host_queries"] = hq
        # C2's prefixes are not ancestor-closed: below the root every node is a leaf, so the rows
        # above are all empty.  The same positions at rel = 0 (every row holds the node itself,
        # one row per output slot: the fill's per-slot row search at its worst), plain and
        # filtered (a quarter passes both columns)
        d_rel0 = torch.zeros(nq, dtype=torch.int32, device=dev)
        total0 = idx.descendants_plan(d_qpos, d_rel0)[3]
        assert total0 == nq
        assert np.array_equal(idx.descendants_fill(total0).cpu().numpy().view(np.uint64), qpos)
        tp0, _, _ = median_s(lambda: idx.descendants_plan(d_qpos, d_rel0), a.warmup, a.reps)
        tf0, _, _ = median_s(lambda: idx.descendants_fill(total0), a.warmup, a.reps)
        res["b0_rel0_plan_ms"], res["b0_rel0_fill_ms"] = 1e3 * tp0, 1e3 * tf0
        res["b0_rel0_plan_fill_qps"] = nq / (tp0 + tf0)
        tfp, _, _ = median_s(lambda: idx.descendants_plan(d_qpos, d_rel0, 0, 2**63, 2**63), a.warmup, a.reps)
        kept = idx.descendants_plan(d_qpos, d_rel0, 0, 2**63, 2**63)[3]
        assert kept == int(((oc[qpos.astype(np.int64)] >= np.uint64(2**63)) & (tb[qpos.astype(np.int64)] >= np.uint64(2**63))).sum())
        tff, _, _ = median_s(lambda: idx.descendants_fill(kept), a.warmup, a.reps)
        res["b0_filtered_kept"] = kept
        res["b0_filtered_plan_ms"], res["b0_filtered_fill_ms"] = 1e3 * tfp, 1e3 * tff

    with section("(c) the root at every rel", a.limit):
        rels = np.arange(0, idx.max_depth + 1, dtype=np.int32)
        root = np.zeros(len(rels), np.uint64)
        _, row_ptr, _, total = idx.descendants_plan(root, rels)
        out = idx.descendants_fill(total)
        want = np.concatenate([host_at(arr, 0, int(r)) for r in rels])
        assert np.array_equal(out.cpu().numpy().view(np.uint64), want)
        tf, flo, fhi = median_s(lambda: idx.descendants_fill(total), a.warmup, a.reps)
        src, dst = torch.empty(total, dtype=torch.int64, device=dev), torch.empty(total, dtype=torch.int64, device=dev)

        def d2d():
            dst.copy_(src)
            torch.cuda.synchronize()

        tc, clo, chi = median_s(d2d, a.warmup, a.reps)
        res["c_total_positions"] = total
        res["c_row_lengths"] = np.diff(row_ptr.cpu().numpy()).tolist()
        res["c_fill_gbps"] = 16e-9 * total / tf
        res["c_fill_ms"] = [1e3 * tf, 1e3 * flo, 1e3 * fhi]
        res["c_baseline_d2d_gbps"] = 16e-9 * total / tc
        res["c_baseline_d2d_ms"] = [1e3 * tc, 1e3 * clo, 1e3 * chi]

    idx.close()
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
