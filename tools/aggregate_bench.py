#!/usr/bin/env python3
"""Prefix aggregation on one GPU (s3imph.DeviceBuilder.aggregate_plan / aggregate_fill,
s3imph.build_index_from_objects), each figure beside what it is to be read against.  One
process; every section runs under its own time limit (SIGALRM with its default action: a
section that hangs ends the process, nothing more is started).

Listing: gen_keys(0, 42, 32, 1, P) prefixes, each with --per objects "<prefix>part-<j>", so the
keys are byte-sorted by construction; sizes are random u64 below 2^40.  Built on the device in
chunks, then copied to the host for (c).

  (a) plan + fill, device-resident: objects/s, and key bytes/s
        against a device-to-device copy of the key blob (bytes/s; the pass reads every key
        twice, so half the copy's rate is its bound)
  (a, --tiers) plan + fill + fill_tiers with one tier id per object, hash(index) % 12 (every tile
        of the tier pass holds all 12 tiers: the worst case for its reductions), beside the plain
        plan + fill of the same run and beside a bound from (a)'s copy: the tier pass reads 9 bytes
        per object, the emit writes 192 bytes per row, at the rate the copy moves bytes (it reads
        and writes the blob, so twice its key bytes/s)
  (b) DeviceBuilder.finalize_index on the same key blob: its key pass does the same per-byte
        work (count '/', lcp with the neighbour) and is the yardstick; the call also runs the
        subtree pass and the depth radix sort, so it is an upper bound on the key pass
        (the kernels apart: rocprofv3 --kernel-trace --stats -- python tools/aggregate_bench.py)
  (c) build_index_from_objects from host memory into a directory, end to end
        beside the sum of its device parts: (a) + the MPHF build + finalize of the produced rows;
        the rest is PCIe and file writing
  (d) for scale only: the Python dict restatement (tests/aggregate_ref.py) on --cpu-objects
        objects, one thread — Python, not the Go aggregator

All device calls wait for their stream, so the host clock around a call times the device work
plus its launches; each figure is the median of --reps calls after --warmup.  Prints one JSON
line per listing size.

    python tools/aggregate_bench.py [--objects 10000000,100000000] [--per 4] [--reps 10] [--tiers]
"""
import argparse
import json
import os
import shutil
import signal
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "s3-inv-db_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402


class section:
    """A timed section with a hard limit: past it the process is terminated."""

    def __init__(self, name, limit):
        self.name, self.limit = name, limit

    def __enter__(self):
        signal.signal(signal.SIGALRM, signal.SIG_DFL)
        signal.alarm(self.limit)
        print(f"[aggregate_bench] {self.name} (limit {self.limit} s)", file=sys.stderr, flush=True)

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


def device_listing(s3imph, torch, dev, m, per, chunk=1_000_000):
    """(d_keys u8 padded, d_offs int64[m + 1], d_sizes int64[m]) for m = P * per objects."""
    P = m // per
    suffix = torch.tensor([list(b"part-%d" % j) for j in range(per)], dtype=torch.uint8, device=dev)
    S = suffix.shape[1]
    blobs, lens = [], []
    for a in range(0, P, chunk):
        cnt = min(chunk, P - a)
        pb, po = s3imph.gen_keys(0, 42, 32, 1 + a, cnt)
        d_pb = torch.from_numpy(pb).to(dev)
        d_po = torch.from_numpy(po.view(np.int64)).to(dev)
        L = d_po[1:] - d_po[:-1]
        obj_len = (L + S).repeat_interleave(per)
        ooff = torch.cumsum(obj_len, 0) - obj_len
        obj = torch.repeat_interleave(torch.arange(cnt * per, device=dev), obj_len)
        within = torch.arange(obj.shape[0], device=dev) - ooff[obj]
        pidx = obj // per
        in_suffix = within >= L[pidx]
        src = torch.where(in_suffix, torch.zeros_like(within), d_po[:-1][pidx] + within)
        out = d_pb[src]
        sfx = suffix[obj % per, torch.clamp(within - L[pidx], 0, S - 1)]
        blobs.append(torch.where(in_suffix, sfx, out))
        lens.append(obj_len)
        del obj, within, pidx, in_suffix, src, out, sfx
    lens = torch.cat(lens)
    d_offs = torch.zeros(lens.shape[0] + 1, dtype=torch.int64, device=dev)
    torch.cumsum(lens, 0, out=d_offs[1:])
    nbytes = int(d_offs[-1])
    d_keys = torch.zeros((nbytes + 7) // 8 * 8 + 8, dtype=torch.uint8, device=dev)
    d_keys[:nbytes] = torch.cat(blobs)
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    d_sizes = torch.randint(0, 1 << 40, (lens.shape[0],), dtype=torch.int64, device=dev, generator=g)
    return d_keys, d_offs, d_sizes, nbytes


def run(a, s3imph, torch, m):
    dev = f"cuda:{a.device}"
    m = m // a.per * a.per
    res = {"bench": "aggregate", "objects": m, "per_prefix": a.per, "reps": a.reps,
           "device": torch.cuda.get_device_name(a.device)}
    ctx = s3imph.DeviceBuilder(a.device)

    with section(f"listing of {m} objects", a.limit):
        d_keys, d_offs, d_sizes, nbytes = device_listing(s3imph, torch, dev, m, a.per)
        torch.cuda.synchronize()
        res["key_bytes"] = nbytes

    with section("(a) plan + fill, device-resident", a.limit):
        info = ctx.aggregate_plan(d_keys, d_offs, m, d_sizes)
        rows = ctx.aggregate_fill()
        n, pbytes = info["n_prefixes"], info["blob_bytes"]
        assert n > 0
        res["rows"], res["row_bytes"], res["max_depth"] = n, pbytes, info["max_depth_seen"]
        tp, plo, phi = median_s(lambda: ctx.aggregate_plan(d_keys, d_offs, m, d_sizes), a.warmup, a.reps)
        tf, flo, fhi = median_s(lambda: ctx.aggregate_fill(), a.warmup, a.reps)
        res["a_plan_ms"] = [1e3 * tp, 1e3 * plo, 1e3 * phi]
        res["a_fill_ms"] = [1e3 * tf, 1e3 * flo, 1e3 * fhi]
        res["a_objects_per_s"] = m / (tp + tf)
        res["a_key_gbps"] = 1e-9 * nbytes / (tp + tf)
        res["a_plan_key_gbps"] = 1e-9 * nbytes / tp
        dst = torch.empty_like(d_keys)

        def d2d():
            dst.copy_(d_keys)
            torch.cuda.synchronize()

        tc, clo, chi = median_s(d2d, a.warmup, a.reps)
        res["a_baseline_copy_key_gbps"] = 1e-9 * nbytes / tc
        res["a_baseline_copy_ms"] = [1e3 * tc, 1e3 * clo, 1e3 * chi]
        del dst

    if a.tiers:
        with section("(a, --tiers) plan + fill + fill_tiers", a.limit):
            idx = torch.arange(m, dtype=torch.int64, device=dev)
            d_tiers = (((idx * 2654435761) >> 11) % 12).to(torch.uint8)  # hash(index) % 12
            del idx
            tinfo = ctx.aggregate_plan(d_keys, d_offs, m, d_sizes, tiers=d_tiers)
            ctx.aggregate_fill()
            ctx.aggregate_fill_tiers()
            assert tinfo["n_prefixes"] == n and tinfo["present_mask"] == 0xfff
            ttp, _, _ = median_s(lambda: ctx.aggregate_plan(d_keys, d_offs, m, d_sizes, tiers=d_tiers), a.warmup, a.reps)
            ttf, _, _ = median_s(lambda: ctx.aggregate_fill(), a.warmup, a.reps)
            ttt, tlo, thi = median_s(lambda: ctx.aggregate_fill_tiers(), a.warmup, a.reps)
            moved = 9 * m + 192 * n                  # the tier pass's reads + the emit's writes
            bound = moved / (2 * nbytes / tc)        # at the bytes/s the copy moves (read + write)
            extra = ttp + ttf + ttt - (tp + tf)
            res["t_plan_ms"], res["t_fill_ms"] = 1e3 * ttp, 1e3 * ttf
            res["t_fill_tiers_ms"] = [1e3 * ttt, 1e3 * tlo, 1e3 * thi]
            res["t_total_ms"] = 1e3 * (ttp + ttf + ttt)
            res["t_plain_total_ms"] = 1e3 * (tp + tf)
            res["t_ratio_to_plain"] = (ttp + ttf + ttt) / (tp + tf)
            res["t_extra_ms"] = 1e3 * extra
            res["t_bound_bytes"] = moved
            res["t_bound_ms"] = 1e3 * bound
            res["t_extra_ratio_to_bound"] = extra / bound
            res["t_objects_per_s"] = m / (ttp + ttf + ttt)
            # the plain path after a tiers plan: what section (a) measured, measured again
            tp2, p2lo, p2hi = median_s(lambda: ctx.aggregate_plan(d_keys, d_offs, m, d_sizes), a.warmup, a.reps)
            tf2, f2lo, f2hi = median_s(lambda: ctx.aggregate_fill(), a.warmup, a.reps)
            res["t_plain_again_ms"] = {"plan": [1e3 * tp2, 1e3 * p2lo, 1e3 * p2hi],
                                       "fill": [1e3 * tf2, 1e3 * f2lo, 1e3 * f2hi]}
            del d_tiers
        rows = ctx.aggregate_fill()

    if a.only_a:
        ctx.close()
        return res, None

    with section("(b) finalize_index on the same key blob", a.limit):
        tz, zlo, zhi = median_s(lambda: ctx.finalize_index(d_keys, d_offs, m), a.warmup, a.reps)
        res["b_finalize_index_ms"] = [1e3 * tz, 1e3 * zlo, 1e3 * zhi]
        res["b_finalize_index_objects_per_s"] = m / tz
        res["b_finalize_index_key_gbps"] = 1e-9 * nbytes / tz

    with section("(c) parts: MPHF build + finalize of the produced rows", a.limit):
        d_fp = torch.empty(n, dtype=torch.int64, device=dev)
        d_po = torch.empty(n, dtype=torch.int64, device=dev)
        tb, _, _ = median_s(lambda: ctx.build(rows["blob"], rows["offsets"], n, d_fp, d_po), 1, 3)
        tz2, _, _ = median_s(lambda: ctx.finalize_index(rows["blob"], rows["offsets"], n, rows["depth"]), 1, 3)
        res["c_parts_ms"] = {"aggregate": 1e3 * (tp + tf), "build": 1e3 * tb, "finalize": 1e3 * tz2}
        res["c_parts_sum_ms"] = 1e3 * (tp + tf + tb + tz2)
        del d_fp, d_po, rows

    with section("(c) build_index_from_objects, host memory to directory", a.limit):
        keys = d_keys[:nbytes].cpu().numpy()
        offs = d_offs.cpu().numpy().view(np.uint64)
        sizes = d_sizes.cpu().numpy().view(np.uint64)
        out = tempfile.mkdtemp(prefix="agg_bench_", dir=a.tmp)
        try:
            te, elo, ehi = median_s(lambda: s3imph.build_index_from_objects(keys, offs, sizes, out), a.e2e_warmup,
                                       a.e2e_reps)
            res["c_end_to_end_ms"] = [1e3 * te, 1e3 * elo, 1e3 * ehi]
            res["c_end_to_end_objects_per_s"] = m / te
            res["c_dir_bytes"] = sum(os.path.getsize(os.path.join(out, f)) for f in os.listdir(out))
        finally:
            shutil.rmtree(out, ignore_errors=True)

    ctx.close()
    return res, (keys, offs, sizes)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--objects", default="10000000,100000000")
    ap.add_argument("--per", type=int, default=4, help="objects per prefix (at most 10)")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--e2e-reps", type=int, default=3)
    ap.add_argument("--e2e-warmup", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cpu-objects", type=int, default=1_000_000)
    ap.add_argument("--limit", type=int, default=240, help="seconds per section")
    ap.add_argument("--tmp", default=None, help="where (c) writes its directory")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--tiers", action="store_true", help="also time the per-tier columns (a, --tiers)")
    ap.add_argument("--only-a", action="store_true", help="stop after section (a) (and --tiers)")
    a = ap.parse_args()
    assert 1 <= a.per <= 10

    import torch
    import s3imph
    if not torch.cuda.is_available():
        sys.exit("aggregate_bench: no GPU (there is no CPU fallback)")
    host = None
    for m in [int(x) for x in a.objects.split(",")]:
        res, listing = run(a, s3imph, torch, m)
        print(json.dumps(res), flush=True)
        host = host or listing
    if host is None:
        return

    with section("(d) the Python dict restatement, one thread", a.limit):
        import aggregate_ref as R
        keys, offs, sizes = host
        k = min(a.cpu_objects, len(offs) - 1)
        ks = R.keys_of(keys, offs[:k + 1])
        t0 = time.perf_counter()
        rows = R.aggregate_dict(ks, sizes[:k])
        t = time.perf_counter() - t0
        print(json.dumps({"bench": "aggregate_cpu_scale", "what": "Python restatement, not the Go aggregator",
                          "objects": k, "rows": len(rows), "seconds": t, "objects_per_s": k / t}), flush=True)


if __name__ == "__main__":
    main()
