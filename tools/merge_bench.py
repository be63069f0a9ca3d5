#!/usr/bin/env python3
"""The row merge on one GPU (s3imph.DeviceBuilder.merge_rows_plan / merge_rows_fill; DESIGN.md
section 4.5e), each figure beside what it is to be read against.  One process; every section runs
under its own time limit (SIGALRM with its default action: a section that hangs or fails ends the
process, nothing more is started).

Input: the listing of tools/aggregate_bench.py (gen_keys(0, 42, 32, 1, P) prefixes with --per
objects each, random sizes, one random tier id per object), put into a seeded random order on the
device and cut into --chunks chunks; each chunk is sorted, gathered and aggregated (with tiers) into
one run, as RowSet.add_objects does, and the runs are concatenated into the merge's single row set.
Before anything is timed the merged rows must equal, in all seven arrays, the rows of the whole
listing aggregated at once.

  plan      merge_rows_plan with tier columns: check, splitters, rank, heads, two scans, the
            heads' places, the pass over the tier columns for present_mask
  fill      merge_rows_fill with tier columns: the rows' sums and the byte emit
  plan/fill (no tiers)  the same without tier columns; this plan is check + splitters + rank +
            heads + scans, an upper bound on the ordering alone
  (i)       a device-to-device copy of every input row byte (blob, offsets, depth, count, bytes and
            the 24 tier columns): the floor; plan + fill over it is the ratio reported
  (ii)      DeviceBuilder.sort_objects on the concatenated row keys: the ordering with no new
            kernel (48 B/row of scratch, rounds that grow with the shared prefix length); to be read
            against the tier-less plan, and kernel by kernel against check + splitters + rank in
            the trace below
  (iii)     for scale only: a Python heapq.merge + fold over --cpu-rows of the same rows, one
            thread — Python, not the Go heap merge

All device calls wait for their stream, so the host clock around a call times the device work plus
its launches and its D2H of the totals; each figure is the median of --reps calls after --warmup.
The kernels apart come from a run of their own:
    rocprofv3 --kernel-trace --stats -- python tools/merge_bench.py --objects 10000000 --reps 1
Prints one JSON line per listing size.

    python tools/merge_bench.py [--objects 10000000,100000000] [--per 4] [--chunks 8] [--reps 5]
"""
import argparse
import heapq
import json
import os
import signal
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "s3-inv-db_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402


class section:
    """A timed section with a hard limit: past it the process is terminated."""

    def __init__(self, name, limit):
        self.name, self.limit = name, limit

    def __enter__(self):
        signal.signal(signal.SIGALRM, signal.SIG_DFL)
        signal.alarm(self.limit)
        print(f"[merge_bench] {self.name} (limit {self.limit} s)", file=sys.stderr, flush=True)

    def __exit__(self, *exc):
        signal.alarm(0)


def median_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return [statistics.median(ts), min(ts), max(ts)]


def rows_of(ctx, torch, keys, offs, sizes, tiers, m):
    """aggregate plan + fill + fill_tiers of a sorted listing: the row arrays, trimmed."""
    info = ctx.aggregate_plan(keys, offs, m, sizes, tiers=tiers)
    out = ctx.aggregate_fill()
    t = ctx.aggregate_fill_tiers()
    n = info["n_prefixes"]
    return {"blob": out["blob"][: info["blob_bytes"]].clone(), "offsets": out["offsets"].clone(),
            "depth": out["depth"].clone(), "count": out["object_count"].clone(), "bytes": out["total_bytes"].clone(),
            "tc": t["tier_count"][:, :n].clone(), "tb": t["tier_bytes"][:, :n].clone(), "n": n,
            "mask": info["present_mask"]}


def run(a, s3imph, torch, m):
    from aggregate_bench import device_listing
    dev = f"cuda:{a.device}"
    m = m // a.per * a.per
    res = {"bench": "merge", "objects": m, "per_prefix": a.per, "chunks": a.chunks, "reps": a.reps,
           "sample_step": s3imph.merge_geometry(), "device": torch.cuda.get_device_name(a.device)}
    ctx = s3imph.DeviceBuilder(a.device)

    with section(f"listing of {m} objects, its rows at once, then shuffled", a.limit):
        s_keys, s_offs, s_sizes, nbytes = device_listing(s3imph, torch, dev, m, a.per)
        g = torch.Generator(device=dev)
        g.manual_seed(11)
        s_tiers = torch.randint(0, 12, (m,), dtype=torch.uint8, device=dev, generator=g)
        whole = rows_of(ctx, torch, s_keys, s_offs, s_sizes, s_tiers, m)
        perm = torch.randperm(m, device=dev, generator=g).to(torch.int32)
        sh = ctx.gather_objects(s_keys, s_offs, m, perm, d_sizes=s_sizes, d_tiers=s_tiers)
        u_keys, u_offs, u_sizes, u_tiers = sh["keys"], sh["offsets"], sh["sizes"], sh["tiers"]
        del perm, sh, s_keys, s_offs, s_sizes, s_tiers
        res["rows_whole"] = whole["n"]

    with section(f"{a.chunks} chunks, each sorted, gathered and aggregated into a run", a.limit):
        runs = []
        t0 = time.perf_counter()
        for c in range(a.chunks):
            lo, hi = m * c // a.chunks, m * (c + 1) // a.chunks
            offs_c = u_offs[lo:hi + 1]
            order, _ = ctx.sort_objects(u_keys, offs_c, hi - lo)
            gl = ctx.gather_objects(u_keys, offs_c, hi - lo, order, d_sizes=u_sizes[lo:hi], d_tiers=u_tiers[lo:hi])
            runs.append(rows_of(ctx, torch, gl["keys"], gl["offsets"], gl["sizes"], gl["tiers"], hi - lo))
            del order, gl
        torch.cuda.synchronize()
        res["runs_ms"] = 1e3 * (time.perf_counter() - t0)
        del u_keys, u_offs, u_sizes, u_tiers
        starts = np.concatenate([[0], np.cumsum([r["n"] for r in runs])]).astype(np.uint64)
        n_in = int(starts[-1])
        blob_len = sum(int(r["blob"].numel()) for r in runs)
        d_blob = torch.zeros((blob_len + 7) // 8 * 8 + 8, dtype=torch.uint8, device=dev)
        d_blob[:blob_len] = torch.cat([r["blob"] for r in runs])
        bases = np.concatenate([[0], np.cumsum([int(r["blob"].numel()) for r in runs])])
        d_offs = torch.cat([runs[0]["offsets"][:1]] + [r["offsets"][1:] + int(bases[i]) for i, r in enumerate(runs)])
        d_depth = torch.cat([r["depth"] for r in runs])
        d_cnt = torch.cat([r["count"] for r in runs])
        d_bytes = torch.cat([r["bytes"] for r in runs])
        d_tc = torch.cat([r["tc"] for r in runs], dim=1).contiguous()
        d_tb = torch.cat([r["tb"] for r in runs], dim=1).contiguous()
        del runs
        res["rows_in"], res["row_key_bytes"] = n_in, blob_len
        res["run_rows"] = [int(x) for x in np.diff(starts)]

    def plan(tiers=True):
        return ctx.merge_rows_plan(d_blob, d_offs, d_depth, d_cnt, d_bytes, starts,
                                   d_tier_count=d_tc if tiers else None, d_tier_bytes=d_tb if tiers else None,
                                   tier_stride=n_in if tiers else 0)

    with section("check: the merged rows equal the rows of the whole listing", a.limit):
        info = plan()
        out = ctx.merge_rows_fill()
        n = whole["n"]
        assert info["n_out"] == n and info["blob_bytes"] == whole["blob"].numel(), info
        assert info["present_mask"] == whole["mask"]
        assert torch.equal(out["blob"][: info["blob_bytes"]], whole["blob"])
        for name, key in (("offsets", "offsets"), ("depth", "depth"), ("object_count", "count"),
                          ("total_bytes", "bytes")):
            assert torch.equal(out[name], whole[key]), name
        assert torch.equal(out["tier_count"][:, :n], whole["tc"]) and torch.equal(out["tier_bytes"][:, :n], whole["tb"])
        res["rows_out"] = n
        del out, whole

    with section("plan and fill, with tier columns", a.limit):
        res["plan_ms"] = median_ms(plan, a.warmup, a.reps)
        res["fill_ms"] = median_ms(ctx.merge_rows_fill, a.warmup, a.reps)
        total = res["plan_ms"][0] + res["fill_ms"][0]
        res["rows_in_per_s"] = n_in / (1e-3 * total)

    with section("plan and fill, without tier columns", a.limit):
        res["plan_notiers_ms"] = median_ms(lambda: plan(False), a.warmup, a.reps)
        res["fill_notiers_ms"] = median_ms(ctx.merge_rows_fill, a.warmup, a.reps)

    with section("(i) device-to-device copy of every input row byte", a.limit):
        srcs = [d_blob, d_offs, d_depth, d_cnt, d_bytes, d_tc, d_tb]
        dsts = [torch.empty_like(t) for t in srcs]
        row_bytes = sum(t.numel() * t.element_size() for t in srcs)

        def d2d():
            for d, s in zip(dsts, srcs):
                d.copy_(s)
            torch.cuda.synchronize()

        res["i_copy_ms"] = median_ms(d2d, a.warmup, a.reps)
        res["input_bytes"] = row_bytes
        res["i_copy_gbps"] = 1e-9 * row_bytes / (1e-3 * res["i_copy_ms"][0])
        res["merge_over_copy"] = total / res["i_copy_ms"][0]
        del dsts

    with section("(ii) sort_objects on the concatenated row keys", a.limit):
        order, sinfo = ctx.sort_objects(d_blob, d_offs, n_in)
        res["ii_sort_rounds"] = sinfo["rounds"]
        res["ii_sort_ms"] = median_ms(lambda: ctx.sort_objects(d_blob, d_offs, n_in), a.warmup, a.reps)
        res["ii_sort_over_plan_notiers"] = res["ii_sort_ms"][0] / res["plan_notiers_ms"][0]
        del order

    if a.cpu_rows:
        with section("(iii) Python heapq.merge + fold, one thread", a.limit):
            per = max(1, a.cpu_rows // a.chunks)
            host = []
            for c in range(a.chunks):
                lo = int(starts[c])
                hi = min(int(starts[c + 1]), lo + per)
                o = d_offs[lo:hi + 1].cpu().numpy()
                raw = d_blob[int(o[0]):int(o[-1])].cpu().numpy().tobytes()
                cnt = d_cnt[lo:hi].cpu().numpy()
                host.append([(raw[int(o[i] - o[0]):int(o[i + 1] - o[0])], int(cnt[i])) for i in range(hi - lo)])
            rows = sum(len(h) for h in host)
            t0 = time.perf_counter()
            out_rows, last, acc = 0, None, 0
            for key, cnt in heapq.merge(*host):
                if key != last:
                    out_rows += 1
                    last, acc = key, 0
                acc += cnt
            t = time.perf_counter() - t0
            res["iii_python_heap_merge"] = {"what": "Python heapq.merge + fold of (key, count), one thread; not Go",
                                            "rows": rows, "rows_out": out_rows, "seconds": t, "rows_per_s": rows / t}
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--objects", default="10000000,100000000", help="listing sizes, comma-separated")
    ap.add_argument("--per", type=int, default=4, help="objects per prefix")
    ap.add_argument("--chunks", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cpu-rows", type=int, default=1_000_000)
    ap.add_argument("--limit", type=int, default=240, help="seconds per section")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()

    import torch
    import s3imph
    if not torch.cuda.is_available():
        sys.exit("merge_bench: no GPU (there is no CPU fallback)")
    for m in (int(x) for x in a.objects.split(",") if x):
        print(json.dumps(run(a, s3imph, torch, m)), flush=True)


if __name__ == "__main__":
    main()
