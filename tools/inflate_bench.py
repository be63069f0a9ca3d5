#!/usr/bin/env python3
"""The gzip inflate on one GPU (s3imph.DeviceBuilder.gunzip), each figure
beside what it is to be read against.  One process; every section runs under its own time limit
(SIGALRM with its default action: a section that hangs ends the process).

Input: inventory-like text (the `filler` rows of tests/gzip_cases.py), --distinct different texts of
--file-mib MiB each, compressed with zlib level 6 into single-member gzip files and used in turn
for 1, 64 and 1024 files; and one file of --big-mib MiB, the same texts back to back in one member.
Before anything is timed the first call's output is compared with zlib's, byte for byte.

  gunzip    DeviceBuilder.gunzip: k_inflate (a wave per file), k_crc32_chunks, k_crc32_fold
  (i)       zlib.decompress of the same files on one host thread
  (ii)      the host-to-device copy of the inflated text from pinned memory: what this stage takes
            off PCIe (the compressed bytes still cross it)
  (iii)     a device-to-device copy of the output: the memory floor of writing it once

Times of the GPU rows are device events on the stream the calls run on, the median of --reps calls
after one warm-up (the single large file: one call), with the min-max spread.  Prints a table and
one JSON line.

    python tools/inflate_bench.py [--reps 3] [--out profiles/inflate_bench.txt]
"""
import argparse
import json
import os
import signal
import statistics
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "s3-inv-db_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402


class section:
    def __init__(self, name, limit):
        self.name, self.limit = name, limit

    def __enter__(self):
        signal.signal(signal.SIGALRM, signal.SIG_DFL)
        signal.alarm(self.limit)
        print(f"[inflate_bench] {self.name} (limit {self.limit} s)", file=sys.stderr, flush=True)

    def __exit__(self, *exc):
        signal.alarm(0)


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


def gzip_file(text: bytes) -> bytes:
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    return c.compress(text) + c.flush()


def run(ctx, torch, stream, name, files, texts, reps):
    """One row of the table: `files` (gzip) whose texts are `texts`, all in one call."""
    n = len(files)
    gz_offs = np.concatenate([[0], np.cumsum([len(f) for f in files])]).tolist()
    out_offs = np.concatenate([[0], np.cumsum([(len(t) + 7) // 8 * 8 for t in texts])]).tolist()
    d_gz = torch.from_numpy(np.frombuffer(b"".join(files), np.uint8).copy()).to("cuda")
    d_out = torch.zeros(out_offs[-1], dtype=torch.uint8, device="cuda")
    infos = ctx.gunzip(d_gz, gz_offs, d_out, out_offs, stream=stream)
    assert all(i["status"] == 0 for i in infos), [i for i in infos if i["status"]][:3]
    for k in sorted({0, n // 2, n - 1}):
        assert d_out[out_offs[k]:out_offs[k] + len(texts[k])].cpu().numpy().tobytes() == texts[k], k
    text_bytes, gz_bytes = sum(len(t) for t in texts), gz_offs[-1]
    r = {"files": n, "text_bytes": text_bytes, "gz_bytes": gz_bytes, "ratio": text_bytes / gz_bytes}
    r["gunzip"] = timed(lambda: ctx.gunzip(d_gz, gz_offs, d_out, out_offs, stream=stream), stream, 0, reps)
    t0 = time.perf_counter()
    for f in files:
        zlib.decompress(f, 31)
    r["zlib_one_thread_ms"] = (time.perf_counter() - t0) * 1e3
    d_copy = torch.empty_like(d_out)
    r["d2d_copy"] = timed(lambda: d_copy.copy_(d_out), stream, 1, 5)
    del d_copy
    pinned = torch.empty(min(text_bytes, 1 << 30), dtype=torch.uint8).pin_memory()
    h2d = timed(lambda: d_out[:len(pinned)].copy_(pinned, non_blocking=True), stream, 1, 5)
    r["h2d_pinned_text_ms"] = h2d["median_ms"] * text_bytes / len(pinned)  # scaled where the text exceeds 1 GiB
    g = r["gunzip"]["median_ms"]
    r["text_gb_per_s"] = text_bytes / g / 1e6
    r["gunzip_over_zlib"] = g / r["zlib_one_thread_ms"]
    r["gunzip_over_h2d_text"] = g / r["h2d_pinned_text_ms"]
    line = (f"  {name:12s} {n:5d} files {text_bytes / 2**20:8.1f} MiB text ({r['ratio']:.1f}:1)  gunzip {g:10.2f} ms "
            f"({r['gunzip']['min_ms']:.2f} - {r['gunzip']['max_ms']:.2f}) = {r['text_gb_per_s']:7.3f} GB/s of text | "
            f"zlib 1 thread {r['zlib_one_thread_ms']:9.1f} ms | H2D of the text {r['h2d_pinned_text_ms']:8.2f} ms | "
            f"D2D copy {r['d2d_copy']['median_ms']:7.3f} ms")
    return r, line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--file-mib", type=int, default=4)
    ap.add_argument("--big-mib", type=int, default=256)
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--counts", default="1,64,1024")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import gzip_cases
    import s3imph
    if not torch.cuda.is_available():
        sys.exit("inflate_bench needs a GPU: nothing is measured without one")

    with section("synthesise and compress", 600):
        texts = [gzip_cases.filler(args.file_mib << 20, 100 + k) for k in range(args.distinct)]
        files = [gzip_file(t) for t in texts]
        big_text = b"".join(texts[k % args.distinct] for k in range(args.big_mib // args.file_mib))
        big = gzip_file(big_text)

    stream = torch.cuda.current_stream()
    ctx = s3imph.DeviceBuilder(0)
    res = {"geometry": s3imph.gunzip_geometry(), "rows": {}}
    lines = [f"inflate_bench: filler text, zlib level 6, {args.file_mib} MiB of text per file; in_chunk_bytes, "
             f"batch_symbols, waves_per_cu = {res['geometry']}; median of {args.reps} (min-max)"]
    for n in [int(c) for c in args.counts.split(",")]:
        with section(f"{n} files", 900):
            r, line = run(ctx, torch, stream, f"{n} x {args.file_mib} MiB", [files[k % args.distinct] for k in range(n)],
                          [texts[k % args.distinct] for k in range(n)], args.reps)
        res["rows"][str(n)] = r
        lines.append(line)
    with section("one large file", 900):
        r, line = run(ctx, torch, stream, f"1 x {args.big_mib} MiB", [big], [big_text], 1)
    res["rows"]["big"] = r
    lines.append(line)
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
