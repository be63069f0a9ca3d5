#!/usr/bin/env python3
"""The monthly cost per position and the ranked descendant rows on one GPU (s3imph.Index, include/
s3imph.h section 5h), each figure beside what it is to be read against.  One process; every timed
section runs under its own time limit (SIGALRM with its default action: a section that hangs ends
the process, nothing more is started).

Index: a root, --parents directories below it and 10 directories below each (1.1M nodes by
default), MPHF and finalize arrays built on the GPU, 12 tiers of random counts and bytes attached
with Index.attach_tiers.

  (cost) cost_device on 1M and 10M random positions and on the sequential positions, queries/s and
        GB/s (16 T read + 136 written per query),
        against the unchanged tiers_device on the same positions (the same gather: 16 T read,
        16 T + 4 written) and against a device-to-device copy of the output bytes
  (top a) descendants_top (cost, k = 10) of one row holding every depth-2 node (1M positions)
  (top b) descendants_top (cost, k = 10) of --parents rows of 10
        each against the plan + fill it extends

All calls wait for their stream, so the host clock around a call times the device work plus its
launch; each figure is the median of --reps calls after --warmup.  Prints one JSON line.

    python tools/cost_bench.py [--parents 100000] [--reps 7]
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
        print(f"[cost_bench] {self.name} (limit {self.limit} s)", file=sys.stderr, flush=True)

    def __exit__(self, *exc):
        signal.alarm(0)


def median_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return [1e3 * statistics.median(ts), 1e3 * min(ts), 1e3 * max(ts)]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parents", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=120, help="seconds per section")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()

    import torch
    import s3imph
    if not torch.cuda.is_available():
        sys.exit("cost_bench: no GPU (there is no CPU fallback)")
    dev = f"cuda:{a.device}"
    T, K = 12, 10
    res = {"bench": "cost", "reps": a.reps, "tiers": T, "k": K, "device": torch.cuda.get_device_name(a.device)}

    with section("build the index on the GPU", a.limit):
        keys = [b""]
        for p in range(a.parents):
            keys.append(b"p%06d/" % p)
            keys += [b"p%06d/c%d/" % (p, c) for c in range(10)]
        blob, offs = s3imph.keys_to_blob(keys)
        n = len(keys)
        pad = np.zeros((len(blob) + 7) // 8 * 8 + 8, np.uint8)
        pad[:len(blob)] = blob
        d_blob = torch.from_numpy(pad).to(dev)
        d_offs = torch.from_numpy(offs.view(np.int64)).to(dev)
        d_fp = torch.empty(n, dtype=torch.int64, device=dev)
        d_po = torch.empty(n, dtype=torch.int64, device=dev)
        ctx = s3imph.DeviceBuilder(a.device)
        ctx.build(d_blob, d_offs, n, d_fp, d_po)
        f = ctx.finalize_index(d_blob, d_offs, n)
        g = torch.Generator(device=dev)
        g.manual_seed(11)
        d_oc = torch.randint(0, 1 << 40, (n,), dtype=torch.int64, device=dev, generator=g)
        d_tb = torch.randint(0, 1 << 50, (n,), dtype=torch.int64, device=dev, generator=g)
        idx = s3imph.Index.from_arrays(ctx.mph_bin(), d_fp, d_po, f["depth"], f["subtree_end"],
                                       f["max_depth_in_subtree"], f["depth_offsets"], f["depth_positions"],
                                       f["max_depth"], d_oc, d_tb)
        d_tc = torch.randint(0, 1 << 30, (T, n), dtype=torch.int64, device=dev, generator=g)
        d_tbt = torch.randint(0, 1 << 46, (T, n), dtype=torch.int64, device=dev, generator=g)
        idx.attach_tiers(list(range(T)), d_tc, d_tbt)
        del d_tc, d_tbt
        pt = s3imph.PriceTable.default_us_east_1()._c()
        res["nodes"], res["max_depth"] = n, int(idx.max_depth)

    with section("(cost) cost_device beside tiers_device and a copy", 2 * a.limit):
        for name, d_pos in (("1m_random", torch.randint(0, n, (1_000_000,), dtype=torch.int64, device=dev, generator=g)),
                            ("10m_random", torch.randint(0, n, (10_000_000,), dtype=torch.int64, device=dev, generator=g)),
                            ("sequential", torch.arange(n, dtype=torch.int64, device=dev))):
            nq = int(d_pos.shape[0])
            got = idx.cost_device(d_pos[:1000], pt).cpu().numpy().reshape(-1).view(s3imph.COST_DTYPE)
            bd = idx.tier_breakdown_all(d_pos[:1000])
            for q in range(0, 1000, 97):  # the kernel against the host entry point
                assert got[q].tobytes() == s3imph.compute_monthly_cost_record(bd[q], pt).tobytes()
            src = torch.empty(nq * 17, dtype=torch.int64, device=dev)
            dst = torch.empty(nq * 17, dtype=torch.int64, device=dev)

            def d2d():
                dst.copy_(src)
                torch.cuda.synchronize()

            tc = median_ms(lambda: idx.cost_device(d_pos, pt), a.warmup, a.reps)
            tt = median_ms(lambda: idx.tiers_device(d_pos), a.warmup, a.reps)
            td = median_ms(d2d, a.warmup, a.reps)
            del src, dst
            res[f"cost_{name}_queries"] = nq
            res[f"cost_{name}_ms"] = tc
            res[f"cost_{name}_qps"] = nq / (1e-3 * tc[0])
            res[f"cost_{name}_gbps"] = 1e-9 * nq * (16 * T + 136) / (1e-3 * tc[0])
            res[f"cost_{name}_baseline_tiers_ms"] = tt
            res[f"cost_{name}_baseline_tiers_gbps"] = 1e-9 * nq * (32 * T + 4) / (1e-3 * tt[0])
            res[f"cost_{name}_ratio_to_tiers"] = tc[0] / tt[0]
            res[f"cost_{name}_baseline_d2d_of_output_ms"] = td

    with section("(top) descendants_top beside plan + fill", 2 * a.limit):
        parents = torch.arange(a.parents, dtype=torch.int64, device=dev) * 11 + 1
        for name, d_q, rel in (("a_one_row", torch.zeros(1, dtype=torch.int64, device=dev), 2), ("b_rows_of_10", parents, 1)):
            _, row_ptr, n_rows, total = idx.descendants_plan(d_q, rel)
            assert total == 10 * a.parents and n_rows == int(d_q.shape[0])
            top_n, top_pos, top_key = idx.top_of_plan(n_rows, "cost", K, pt)
            # the keys are the positions' totals, in descending order
            flat = top_pos.reshape(-1)
            costs = idx.cost_device(flat, pt)[:, 0].reshape(n_rows, K)
            assert torch.equal(costs, top_key) and bool((top_n == K).all())
            u = top_key.cpu().numpy().view(np.uint64)
            assert bool((u[:, :-1] >= u[:, 1:]).all())

            def plan_fill():
                idx.descendants_fill(idx.descendants_plan(d_q, rel)[3])

            def plan_top():
                idx.top_of_plan(idx.descendants_plan(d_q, rel)[2], "cost", K, pt)

            tpf = median_ms(plan_fill, a.warmup, a.reps)
            tpt = median_ms(plan_top, a.warmup, a.reps)
            tp = median_ms(lambda: idx.descendants_plan(d_q, rel), a.warmup, a.reps)
            res[f"top_{name}_rows"], res[f"top_{name}_positions"] = n_rows, total
            res[f"top_{name}_plan_top_ms"] = tpt
            res[f"top_{name}_baseline_plan_fill_ms"] = tpf
            res[f"top_{name}_baseline_plan_ms"] = tp
            res[f"top_{name}_ratio_to_plan_fill"] = tpt[0] / tpf[0]

    idx.close()
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
