#!/usr/bin/env python3
"""The inventory CSV parse on one GPU (s3imph.DeviceBuilder.csv_plan / csv_fill; DESIGN.md section
4.5d), each figure beside what it is to be read against.  One process; every section runs under
its own time limit (SIGALRM with its default action: a section that hangs ends the process).

Input: an inventory-shaped, headerless CSV synthesised from gen_keys(0, 42, 32, 0, --rows) in a
seeded random order — bucket, key, size, last-modified date, storage class — with --quoted-pct of
the keys quoted and holding a "" escape (the re-walked kind).  Before anything is timed the
listing the GPU returns for the first --check-rows rows is compared with tests/csv_ref.py's.

  plan      DeviceBuilder.csv_plan: the automaton passes, the record table, the field pass, the scans
  fill      DeviceBuilder.csv_fill: offsets, sizes, tiers and the key bytes
  (i)       a device-to-device copy of the same number of bytes: the memory floor of one pass over
            the text (the passes read it about three times, and the record walk once more)
  (ii)      the host-to-device copy of the same buffer, from pageable and from pinned memory: what
            any path that starts from host memory is bound by
  (iii)     csv_ref.records on the first --check-rows rows, one CPU thread: Python standing in for the
            per-row loop being replaced (not Go's encoding/csv)

Times are device events on the stream the calls run on, each the median of --reps calls after
--warmup, with the min-max spread.  Prints a table and one JSON line.

    python tools/csv_bench.py [--rows 10000000] [--reps 7] [--out profiles/csv_bench.txt]
"""
import argparse
import json
import os
import signal
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "s3-inv-db_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402

SCHEMA = (1, 2, 4, -1)
CLASSES = (b"STANDARD", b"GLACIER", b"STANDARD_IA", b"DEEP_ARCHIVE")
DATE = b"2024-01-01T00:00:00.000Z"


class section:
    def __init__(self, name, limit):
        self.name, self.limit = name, limit

    def __enter__(self):
        signal.signal(signal.SIGALRM, signal.SIG_DFL)
        signal.alarm(self.limit)
        print(f"[csv_bench] {self.name} (limit {self.limit} s)", file=sys.stderr, flush=True)

    def __exit__(self, *exc):
        signal.alarm(0)


def synthesise(rows: int, quoted_pct: float, seed: int = 7):
    """The CSV text as a uint8 array and the offset of every row's start (rows + 1 entries)."""
    import s3imph
    rng = np.random.default_rng(seed)
    blob, offs = s3imph.gen_keys(0, 42, 32, 0, rows + 1)
    offs = offs.astype(np.int64)[1:]  # key 0 is "", which the reader drops: rows use keys 1..rows
    perm = rng.permutation(rows)
    kstart, klen = offs[:-1][perm], np.diff(offs)[perm]
    quoted = rng.random(rows) < quoted_pct / 100.0
    size = rng.integers(1_000_000, 10_000_000, rows)  # seven digits
    cls = rng.integers(0, len(CLASSES), rows)
    clen = np.array([len(c) for c in CLASSES])[cls]
    head, mid = b"bucket,", b"," + b"0000000" + b"," + DATE + b","
    q = quoted.astype(np.int64)
    rlen = len(head) + klen + 5 * q + len(mid) + clen + 1
    start = np.zeros(rows + 1, np.int64)
    np.cumsum(rlen, out=start[1:])
    out = np.empty(int(start[-1]), np.uint8)

    def put(at, text):
        out[at[:, None] + np.arange(len(text))] = np.frombuffer(text, np.uint8)

    for lo in range(0, rows, 1 << 19):  # piece by piece, in slices that keep the index arrays small
        sl = slice(lo, min(rows, lo + (1 << 19)))
        st, kl, ks, qs = start[:-1][sl], klen[sl], kstart[sl], q[sl]
        put(st, head)
        out[st[quoted[sl]] + len(head)] = ord('"')
        kat = st + len(head) + qs  # after the opening quote
        j = np.arange(int(kl.sum())) - np.repeat(np.cumsum(kl) - kl, kl)  # byte index within its key
        out[np.repeat(kat, kl) + j] = blob[np.repeat(ks, kl) + j]
        put((kat + kl)[quoted[sl]], b'""q"')
        mat = kat + kl + 4 * qs
        put(mat, mid)
        for d in range(7):
            out[mat + 1 + d] = 48 + (size[sl] // 10 ** (6 - d)) % 10
        cat = mat + len(mid)
        for c, name in enumerate(CLASSES):
            put(cat[cls[sl] == c], name)
    out[start[1:] - 1] = 10
    return out, start


def timed(fn, stream, warmup, reps):
    import torch
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--quoted-pct", type=float, default=1.0)
    ap.add_argument("--check-rows", type=int, default=100_000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import csv_ref
    import s3imph
    if not torch.cuda.is_available():
        sys.exit("csv_bench needs a GPU: nothing is measured without one")

    with section("synthesise", 300):
        text, start = synthesise(args.rows, args.quoted_pct)
    nbytes = len(text)
    res = {"rows": args.rows, "bytes": nbytes, "quoted_pct": args.quoted_pct, "reps": args.reps}

    with section("reference on the first rows", 300):
        k = min(args.check_rows, args.rows)
        head = text[:start[k]].tobytes()
        t0 = time.perf_counter()
        want = csv_ref.records(head, SCHEMA)
        cpu_s = time.perf_counter() - t0
        assert want["info"]["n_objects"] == k
        res["cpu_ref"] = {"rows": k, "seconds": cpu_s, "rows_per_s": k / cpu_s}

    stream = torch.cuda.current_stream()
    ctx = s3imph.DeviceBuilder(0)
    with section("H2D", 300):
        d_text = torch.empty((nbytes + 7) // 8 * 8, dtype=torch.uint8, device="cuda")
        src = torch.from_numpy(text)
        res["h2d_pageable"] = timed(lambda: d_text[:nbytes].copy_(src), stream, 1, 3)
        pinned = src.pin_memory()
        res["h2d_pinned"] = timed(lambda: d_text[:nbytes].copy_(pinned, non_blocking=True), stream, 1, args.reps)
        del pinned

    with section("check against the reference", 120):
        info = ctx.csv_plan(d_text, len(head), SCHEMA, stream=stream)
        assert info == want["info"], (info, want["info"])
        out = ctx.csv_fill(stream=stream)
        blob, offs = csv_ref.listing(want)
        assert out["keys"].cpu().numpy().tobytes() == blob
        assert out["offsets"].cpu().numpy().view(np.uint64).tolist() == offs.tolist()
        assert out["sizes"].cpu().numpy().view(np.uint64).tolist() == want["sizes"].tolist()
        assert out["tiers"].cpu().numpy().tolist() == want["tiers"].tolist()
        del out

    with section("plan and fill", 600):
        info = ctx.csv_plan(d_text, nbytes, SCHEMA, stream=stream)
        assert info["n_objects"] == args.rows and info["n_records"] == args.rows
        n, kb = info["n_objects"], info["key_bytes"]
        d_keys = torch.empty((kb + 7) // 8 * 8 + 8, dtype=torch.uint8, device="cuda")
        d_offs = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        d_sizes = torch.empty(n, dtype=torch.int64, device="cuda")
        d_tiers = torch.empty(n, dtype=torch.uint8, device="cuda")
        res["info"] = info
        res["plan"] = timed(lambda: ctx.csv_plan(d_text, nbytes, SCHEMA, stream=stream), stream, args.warmup, args.reps)
        res["fill"] = timed(lambda: ctx.csv_fill(d_keys, d_offs, d_sizes, d_tiers, stream=stream), stream, args.warmup,
                            args.reps)

    with section("D2D copy", 120):
        d_copy = torch.empty_like(d_text)
        res["d2d_copy"] = timed(lambda: d_copy.copy_(d_text), stream, args.warmup, args.reps)

    parse = res["plan"]["median_ms"] + res["fill"]["median_ms"]
    res["parse_ms"] = parse
    res["gb_per_s"] = nbytes / parse / 1e6
    res["rows_per_s"] = args.rows / parse * 1e3
    res["parse_over_d2d_copy"] = parse / res["d2d_copy"]["median_ms"]
    res["parse_over_h2d_pinned"] = parse / res["h2d_pinned"]["median_ms"]
    res["parse_over_h2d_pageable"] = parse / res["h2d_pageable"]["median_ms"]
    res["speedup_over_cpu_ref_rows_per_s"] = res["rows_per_s"] / res["cpu_ref"]["rows_per_s"]
    res["parse_below_h2d_pinned"] = parse < res["h2d_pinned"]["median_ms"]

    lines = [f"csv_bench: {args.rows} rows, {nbytes} bytes ({nbytes / args.rows:.1f} B/row), "
             f"{args.quoted_pct}% quoted keys, median of {args.reps} (min-max)"]
    for name in ("plan", "fill", "d2d_copy", "h2d_pinned", "h2d_pageable"):
        r = res[name]
        lines.append(f"  {name:13s} {r['median_ms']:9.3f} ms  ({r['min_ms']:.3f} - {r['max_ms']:.3f})  "
                     f"{nbytes / r['median_ms'] / 1e6:8.1f} GB/s of text")
    lines.append(f"  plan + fill   {parse:9.3f} ms = {res['parse_over_d2d_copy']:.1f} x the D2D copy, "
                 f"{res['parse_over_h2d_pinned']:.2f} x the pinned H2D, {res['parse_over_h2d_pageable']:.2f} x the pageable H2D")
    lines.append(f"  rows/s        {res['rows_per_s']:.3e} on the GPU; {res['cpu_ref']['rows_per_s']:.3e} for csv_ref on "
                 f"{res['cpu_ref']['rows']} rows (one CPU thread, Python)")
    lines.append(json.dumps(res))
    text_out = "\n".join(lines) + "\n"
    sys.stdout.write(text_out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text_out)
    ctx.close()


if __name__ == "__main__":
    main()
