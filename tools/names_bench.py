#!/usr/bin/env python3
"""The prefix-blob queries of the GPU reader (s3imph.Index: prefixes_plan / prefixes_fill,
lookup_verify_device, verify_device), each figure beside what it is to be read against.  One
process; every timed section runs under its own time limit (SIGALRM with its default action: a
section that hangs ends the process, nothing more is started).

Index: C2's 10M synthetic prefixes (gen_keys(0, 42, 32, 0, 10_000_000)), MPHF and finalize arrays
built on the GPU, attached with Index.from_arrays, the key blob attached as its stored prefixes.

  (a) PrefixString for 1M positions, sequential (one run of the index) and random: plan and fill
        apart, names/s, and GB/s of the fill at 2 bytes moved per name byte (read + written)
        against a device-to-device copy of the same byte count
        and against the Python prefix_string loop over the host mmap (on --host-queries of them)
  (b) lookup_verify over the names (a) returned for the random positions (1M member keys)
        against lookup over the same blob
  (c) verify (VerifyMPHF: every stored prefix looked up, reduced on the device)
        against one lookup over the stored blob

All calls wait for their stream, so the host clock around a call times the device work plus its
launch; each figure is the median of --reps calls after --warmup.  Prints one JSON line.

    python tools/names_bench.py [--keys 10000000] [--queries 1000000] [--reps 20]
"""
import argparse
import json
import os
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
        print(f"[names_bench] {self.name} (limit {self.limit} s)", file=sys.stderr, flush=True)

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


def ms(t):
    return [round(1e3 * v, 4) for v in t]


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
        sys.exit("names_bench: no GPU (there is no CPU fallback)")
    dev = f"cuda:{a.device}"
    n, nq = a.keys, min(a.queries, a.keys)
    rng = np.random.default_rng(7)
    res = {"bench": "names", "keys": n, "queries": nq, "reps": a.reps, "device": torch.cuda.get_device_name(a.device)}

    with section("build the index on the GPU", a.limit):
        blob, offs = s3imph.gen_keys(0, 42, 32, 0, n)
        d_blob = torch.from_numpy(blob).to(dev)
        d_offs = torch.from_numpy(offs.view(np.int64)).to(dev)
        d_fp = torch.empty(n, dtype=torch.int64, device=dev)
        d_po = torch.empty(n, dtype=torch.int64, device=dev)
        ctx = s3imph.DeviceBuilder(a.device)
        ctx.build(d_blob, d_offs, n, d_fp, d_po)
        f = ctx.finalize_index(d_blob, d_offs, n)
        mph = ctx.mph_bin()
        idx = s3imph.Index.from_arrays(mph, d_fp, d_po, f["depth"], f["subtree_end"], f["max_depth_in_subtree"],
                                       f["depth_offsets"], f["depth_positions"], f["max_depth"])
        idx.attach_prefixes(d_blob, d_offs)
        res["blob_bytes"] = int(offs[-1])

    with section("(a) PrefixString for a batch", 2 * a.limit):
        tmp = tempfile.TemporaryDirectory()
        s3imph.write_index_files(tmp.name, mph, d_fp.cpu().numpy().view(np.uint64), d_po.cpu().numpy().view(np.uint64),
                                 blob[: int(offs[-1])], offs)
        idx.dir = tmp.name  # the two prefix files are all prefix_string reads
        start = int(rng.integers(0, n - nq + 1))
        batches = {"sequential": np.arange(start, start + nq, dtype=np.uint64),
                   "random": rng.integers(0, n, nq).astype(np.uint64)}
        names = None
        for name, pos in batches.items():
            d_pos = torch.from_numpy(pos.view(np.int64)).to(dev)
            o, fnd, out = idx.prefixes_device(d_pos)
            p = pos.astype(np.int64)
            want_offs = np.zeros(nq + 1, np.uint64)
            want_offs[1:] = np.cumsum(offs[p + 1] - offs[p])
            total = int(want_offs[-1])
            assert np.array_equal(o.cpu().numpy().view(np.uint64), want_offs) and bool(fnd.all())
            got, oh = out.cpu().numpy(), want_offs.astype(np.int64)
            for q in rng.integers(0, nq, 2000):
                assert got[oh[q]:oh[q + 1]].tobytes() == blob[int(offs[p[q]]):int(offs[p[q] + 1])].tobytes(), (name, q)
            if name == "sequential":
                assert got[:total].tobytes() == blob[int(offs[start]):int(offs[start + nq])].tobytes()
            buf = torch.empty((total + 7) // 8 * 8, dtype=torch.uint8, device=dev)
            tp = median_s(lambda: idx.prefixes_plan(d_pos), a.warmup, a.reps)
            idx.prefixes_plan(d_pos)
            tf = median_s(lambda: idx.prefixes_fill(total, out=buf), a.warmup, a.reps)
            src = torch.empty_like(buf)

            def d2d():
                buf.copy_(src)
                torch.cuda.synchronize()

            tc = median_s(d2d, a.warmup, a.reps)
            hq = min(a.host_queries, nq)
            idx.prefix_string(int(pos[0]))
            t0 = time.perf_counter()
            for v in pos[:hq]:
                idx.prefix_string(int(v))
            t_host = time.perf_counter() - t0
            res[f"a_{name}_bytes"] = total
            res[f"a_{name}_plan_ms"], res[f"a_{name}_fill_ms"] = ms(tp), ms(tf)
            res[f"a_{name}_plan_fill_names_per_s"] = nq / (tp[0] + tf[0])
            res[f"a_{name}_fill_gbps"] = 2e-9 * total / tf[0]
            res[f"a_{name}_baseline_d2d_ms"] = ms(tc)
            res[f"a_{name}_baseline_d2d_gbps"] = 2e-9 * total / tc[0]
            res[f"a_{name}_fill_ratio_to_d2d"] = tf[0] / tc[0]
            res[f"a_{name}_baseline_python_loop_names_per_s"] = hq / t_host
            res[f"a_{name}_baseline_python_loop_queries"] = hq
            if name == "random":
                names = (out, o, pos)
            del buf, src
        tmp.cleanup()

    with section("(b) lookup_verify beside lookup, 1M member keys", a.limit):
        q_blob, q_offs, pos = names
        want = torch.from_numpy(pos.view(np.int64)).to(dev)
        assert torch.equal(idx.lookup_device(q_blob, q_offs, nq), want)
        assert torch.equal(idx.lookup_verify_device(q_blob, q_offs, nq), want)
        tv = median_s(lambda: idx.lookup_verify_device(q_blob, q_offs, nq), a.warmup, a.reps)
        tl = median_s(lambda: idx.lookup_device(q_blob, q_offs, nq), a.warmup, a.reps)
        res["b_lookup_verify_ms"], res["b_baseline_lookup_ms"] = ms(tv), ms(tl)
        res["b_lookup_verify_qps"], res["b_baseline_lookup_qps"] = nq / tv[0], nq / tl[0]
        res["b_ratio_to_lookup"] = tv[0] / tl[0]

    with section("(c) verify beside one lookup over the stored blob", a.limit):
        assert idx.verify_device() == (0, 2**64 - 1, 2**64 - 1)
        tv = median_s(idx.verify_device, a.warmup, a.reps)
        tl = median_s(lambda: idx.lookup_device(d_blob, d_offs, n), a.warmup, a.reps)
        res["c_verify_ms"], res["c_baseline_lookup_ms"] = ms(tv), ms(tl)
        res["c_verify_keys_per_s"] = n / tv[0]
        res["c_ratio_to_lookup"] = tv[0] / tl[0]

    idx.close()
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
