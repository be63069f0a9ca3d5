#!/usr/bin/env python3
"""The listing sort on one GPU (s3imph.DeviceBuilder.sort_objects / gather_objects; DESIGN.md
section 4.5c), each figure beside what it is to be read against.  One process; every section
runs under its own time limit (SIGALRM with its default action: a section that hangs or fails
ends the process, nothing more is started).

Listings: gen_keys(0, 42, 32, 0, --objects) (s3-like, avg 32 B) and gen_keys(1, 42, 0, 0,
--skew-objects) (lengths log-uniform up to 1024 B), each put into a seeded random order on the
device — by gather_objects itself with a torch.randperm order; the sort + gather of the result
must give back the generator's listing byte for byte, which the tool checks before it times.

  sort      DeviceBuilder.sort_objects of the shuffled listing (the order only)
  gather    DeviceBuilder.gather_objects into that order (keys, offsets, sizes, tiers)
  all       sort + gather + aggregate_plan + aggregate_fill: shuffled listing to prefix rows
  (i)       aggregate_plan + aggregate_fill alone on the sorted listing: what `all` adds to
  (ii)      a device-to-device copy of the same key bytes: the gather's floor
  (iii)     a single-thread host sort of --cpu-objects of the same keys (Python's sorted over
            bytes: memcmp order, the same order; not Go's sort.Strings) — the cost being replaced
  rounds    refinement rounds and the active keys / segments entering each (the library's
            S3IMPH_DEBUG lines of one extra sort, captured from stderr)

All device calls wait for their stream, so the host clock around a call times the device work
plus its launches and the one D2H per round; each figure is the median of --reps calls after
--warmup.  Prints one JSON line per listing.

    python tools/sort_bench.py [--objects 10000000] [--skew-objects 2000000] [--reps 5]
"""
import argparse
import json
import os
import re
import signal
import statistics
import sys
import tempfile
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
        print(f"[sort_bench] {self.name} (limit {self.limit} s)", file=sys.stderr, flush=True)

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


def debug_rounds(s3imph, device, d_keys, d_offs, m):
    """One sort on a context made with S3IMPH_DEBUG set, its stderr lines parsed:
    [(round, active, segments)]."""
    os.environ["S3IMPH_DEBUG"] = "1"
    try:
        ctx = s3imph.DeviceBuilder(device)
    finally:
        del os.environ["S3IMPH_DEBUG"]
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as f:
        os.dup2(f.fileno(), 2)
        try:
            ctx.sort_objects(d_keys, d_offs, m)
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        ctx.close()
        f.seek(0)
        text = f.read().decode(errors="replace")
    return [[int(x) for x in g] for g in re.findall(r"sort round (\d+): (\d+) active in (\d+) segments", text)]


def run(a, s3imph, torch, kind, avg, m):
    dev = f"cuda:{a.device}"
    res = {"bench": "sort", "kind": kind, "objects": m, "reps": a.reps, "device": torch.cuda.get_device_name(a.device)}
    ctx = s3imph.DeviceBuilder(a.device)

    with section(f"listing: gen_keys({kind}, 42, {avg}, 0, {m}), shuffled on the device", a.limit):
        blob, offs = s3imph.gen_keys(kind, 42, avg, 0, m)
        nbytes = int(offs[-1])
        s_keys = torch.from_numpy(blob[: (nbytes + 7) // 8 * 8]).to(dev)
        s_offs = torch.from_numpy(offs.view(np.int64)).to(dev)
        g = torch.Generator(device=dev)
        g.manual_seed(7)
        s_sizes = torch.randint(0, 1 << 40, (m,), dtype=torch.int64, device=dev, generator=g)
        s_tiers = torch.randint(0, 12, (m,), dtype=torch.uint8, device=dev, generator=g)
        perm = torch.randperm(m, device=dev, generator=g).to(torch.int32)
        sh = ctx.gather_objects(s_keys, s_offs, m, perm, d_sizes=s_sizes, d_tiers=s_tiers)
        u_keys, u_offs, u_sizes, u_tiers = sh["keys"], sh["offsets"], sh["sizes"], sh["tiers"]
        del perm, sh
        res["key_bytes"], res["avg_key_bytes"] = nbytes, nbytes / m
        if a.cpu_objects:
            host_keys = [blob[int(offs[i]):int(offs[i + 1])].tobytes() for i in
                         np.random.default_rng(7).permutation(m)[: a.cpu_objects]]
        del blob, offs

    with section("check: sort + gather gives back the generator's listing", a.limit):
        order, info = ctx.sort_objects(u_keys, u_offs, m)
        out = ctx.gather_objects(u_keys, u_offs, m, order, d_sizes=u_sizes, d_tiers=u_tiers)
        assert info["first_unsorted"] != 2**64 - 1 and info["n_equal"] == 0 and info["key_bytes"] == nbytes
        assert torch.equal(out["keys"][:nbytes], s_keys[:nbytes]) and torch.equal(out["offsets"], s_offs)
        assert torch.equal(out["sizes"], s_sizes) and torch.equal(out["tiers"], s_tiers)
        res["rounds"] = info["rounds"]
        del out

    with section("sort", a.limit):
        res["sort_ms"] = median_ms(lambda: ctx.sort_objects(u_keys, u_offs, m), a.warmup, a.reps)
        res["sort_objects_per_s"] = m / (1e-3 * res["sort_ms"][0])

    with section("gather", a.limit):
        res["gather_ms"] = median_ms(
            lambda: ctx.gather_objects(u_keys, u_offs, m, order, d_sizes=u_sizes, d_tiers=u_tiers), a.warmup, a.reps)
        res["gather_key_gbps"] = 1e-9 * nbytes / (1e-3 * res["gather_ms"][0])

    def everything():
        o, _ = ctx.sort_objects(u_keys, u_offs, m)
        gl = ctx.gather_objects(u_keys, u_offs, m, o, d_sizes=u_sizes, d_tiers=u_tiers)
        ctx.aggregate_plan(gl["keys"], gl["offsets"], m, gl["sizes"])
        ctx.aggregate_fill()

    with section("all: sort + gather + aggregate plan + fill", a.limit):
        res["all_ms"] = median_ms(everything, a.warmup, a.reps)
        res["all_objects_per_s"] = m / (1e-3 * res["all_ms"][0])

    def plan_fill():
        ctx.aggregate_plan(s_keys, s_offs, m, s_sizes)
        ctx.aggregate_fill()

    with section("(i) aggregate plan + fill alone on the sorted listing", a.limit):
        res["i_plan_fill_ms"] = median_ms(plan_fill, a.warmup, a.reps)

    with section("(ii) device-to-device copy of the key bytes", a.limit):
        dst = torch.empty_like(s_keys)

        def d2d():
            dst.copy_(s_keys)
            torch.cuda.synchronize()

        res["ii_copy_ms"] = median_ms(d2d, a.warmup, a.reps)
        res["ii_copy_key_gbps"] = 1e-9 * nbytes / (1e-3 * res["ii_copy_ms"][0])
        del dst

    with section("rounds: active keys and segments entering each", a.limit):
        res["per_round"] = debug_rounds(s3imph, a.device, u_keys, u_offs, m)

    if a.cpu_objects:
        with section("(iii) single-thread host sort (Python sorted over bytes)", a.limit):
            t0 = time.perf_counter()
            sorted(range(len(host_keys)), key=host_keys.__getitem__)
            t = time.perf_counter() - t0
            res["iii_host_sort"] = {"what": "Python sorted, one thread; not Go's sort.Strings",
                                    "objects": len(host_keys), "seconds": t, "objects_per_s": len(host_keys) / t}
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--objects", type=int, default=10_000_000, help="kind 0 listing (0: skip)")
    ap.add_argument("--skew-objects", type=int, default=2_000_000, help="kind 1 listing (0: skip)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cpu-objects", type=int, default=1_000_000)
    ap.add_argument("--limit", type=int, default=120, help="seconds per section")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()

    import torch
    import s3imph
    if not torch.cuda.is_available():
        sys.exit("sort_bench: no GPU (there is no CPU fallback)")
    for kind, avg, m in ((0, 32, a.objects), (1, 0, a.skew_objects)):
        if m:
            print(json.dumps(run(a, s3imph, torch, kind, avg, m)), flush=True)


if __name__ == "__main__":
    main()
