"""Where and when the device entry points run (include/s3imph.h: "Synchronous on `stream`"; NULL =
the context's own blocking stream): every wrapper with a ``stream=`` parameter, DistBuilder apart,
called while the stream that produces its inputs is still busy.

Method (one harness, `drive`, for every case of tests/stream_cases.py).  The device tensors hold a
decoy; one undelayed warm-up call is checked against the decoy's answer (after one on the real
input, so that the scratch fits both); then a delay
(torch.cuda._sleep) is queued on the producing stream, an event `ev` recorded behind it and the real
input copied in behind that (pinned host memory, non_blocking); `ev` must still be pending when the
call is made, and the call must answer for the real input, exactly, info fields included.  A kernel
on the wrong stream, a null-stream copy or an early read-back answers for the decoy instead.  Three
modes: `current` (torch's current stream is the side stream, stream=None), `explicit` (stream=s while
the default stream sits behind a second, three times longer delay whose event must still be pending
after the call: whatever the wrapper itself queues with torch lags behind the library; the outputs are
read on s and again after the device drained), `null` (default stream throughout, the library on its
own blocking stream).  The negative control calls with another non-blocking stream than the one that
produces: it must return with `ev` pending and answer for the decoy, or the run shows nothing.

Calibration (MI355X, this suite's shapes).  torch.cuda._sleep ran at 2397 cycles per microsecond
(measured per session with events, never assumed).  The warm-up calls took 0.07 to 0.5 ms for the
reader queries, the lookups, the gather and the aggregation, 2.4 to 5.5 ms for the MPHF build, the
finalize, the CSV parse, the merge and the ranked rows, 8.9 ms for the sort, and 10 ms for the first
call of a session (the kernels' load).  The delay is max(50 ms, 10 x the case's own warm-up time),
so 50 to 105 ms; the default stream's in explicit mode is three times that.  A delay that proves too
short fails one of the "still pending" assertions; it never passes silently.  The streams are picked
per session by a probe: a pair on which a short operation completes while the other stream sleeps
(two torch streams can share a hardware queue)."""
import time

import numpy as np
import pytest

import s3imph
import stream_cases as SC
from index_dirs import write_index_dir
from test_gpu_pricing import key_columns, lib_table, with_tiers

pytestmark = pytest.mark.gpu

MODES = ("current", "explicit", "null")
FLOOR_MS = 50.0
MARGIN = 10.0
LONG = 3.0


def _t(a):
    """numpy -> torch on the host (unsigned 64 / 32 as their signed bits)."""
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a.copy())


class Rig:
    """The session's streams and the sleep kernel's measured rate."""

    def __init__(self):
        import torch
        assert torch.cuda.is_available(), "GPU tests need a GPU"
        self.torch = torch
        self.default = torch.cuda.default_stream()
        self.cycles_per_ms = self._calibrate()
        pool = [torch.cuda.Stream() for _ in range(8)]
        self.s = next((x for x in pool if self._independent(self.default, x) and self._independent(x, self.default)),
                      None)
        assert self.s is not None, "no side stream runs while the default stream is busy"
        self.s2 = next((x for x in pool if x is not self.s and self._independent(self.s, x)), None)
        assert self.s2 is not None, "no second side stream runs while the first is busy"
        print(f"[streams] sleep rate {self.cycles_per_ms / 1000:.1f} cycles/us")

    def _calibrate(self) -> float:
        torch = self.torch
        rate = 0.0
        for _ in range(2):  # the first run pays the kernel's load
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            torch.cuda._sleep(20_000_000)
            b.record()
            b.synchronize()
            rate = 20_000_000 / a.elapsed_time(b)
        assert rate > 0
        return rate

    def sleep(self, ms: float) -> None:
        self.torch.cuda._sleep(int(ms * self.cycles_per_ms))

    def _independent(self, busy, other) -> bool:
        """A small fill on `other` completes while `busy` sleeps."""
        torch = self.torch
        held, done = torch.cuda.Event(), torch.cuda.Event()
        with torch.cuda.stream(busy):
            self.sleep(FLOOR_MS)
            held.record()
        with torch.cuda.stream(other):
            torch.zeros(64, device="cuda").add_(1)
            done.record()
        done.synchronize()
        ok = not held.query()
        torch.cuda.synchronize()
        return ok


@pytest.fixture(scope="module")
def rig():
    return Rig()


@pytest.fixture(scope="module")
def ctx():
    c = s3imph.DeviceBuilder(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def lookup_ctx(oracle_lib):
    """A context answering against the lookup case's MPHF, with its fp / pos arrays on the device."""
    st = SC.case("lookup").static
    c = s3imph.DeviceBuilder(0)
    c.load_mph_bin(st["mph"])
    yield c, _t(st["fp"]).cuda(), _t(st["pos"]).cuda()
    c.close()


@pytest.fixture(scope="module")
def idx(tmp_path_factory, oracle_lib):
    """The reader cases' index: stats and five tiers (as test_gpu_pricing.with_tiers builds one)."""
    t = SC.reader_tree()
    d = tmp_path_factory.mktemp("stream_tree")
    write_index_dir(str(d), oracle_lib, t["prefixes"], stats=key_columns())
    i = with_tiers((d, t["prefixes"]), tmp_path_factory.mktemp("stream_idx"), SC.TIER_IDS)
    assert i.count == SC.N and i.present_tiers() == list(SC.TIER_IDS)
    yield i
    i.close()


def _read(out: dict, want: dict, torch, stream) -> dict:
    """The outputs on the host, read on `stream`, in the dtypes and shapes of `want`."""
    got = {}
    with torch.cuda.stream(stream):
        for k, w in want.items():
            v = out[k]
            if callable(v):
                v = v()
            if torch.is_tensor(v):
                v = v.cpu().numpy()
                if isinstance(w, np.ndarray) and v.nbytes == w.nbytes:
                    v = np.ascontiguousarray(v).reshape(-1).view(w.dtype).reshape(w.shape)
            got[k] = v
    return got


def drive(rig, case, call, mode):
    """Warm-up on the decoy, then the call behind a busy producing stream (module docstring).
    call(dev, stream) makes the library call(s) on the tensors `dev` and returns the outputs by the
    names of the case's answer (tensors, values, or callables evaluated when the outputs are read)."""
    torch = rig.torch
    s, s2, default = rig.s, rig.s2, rig.default
    arg = {"current": None, "explicit": s, "null": None, "control": s2}[mode]
    cur = s if mode == "current" else default
    producer = default if mode == "null" else s
    consumer = {"current": s, "explicit": s, "null": default, "control": s2}[mode]
    dev = {k: _t(a).cuda() for k, a in case.real.items()}
    host = {k: _t(a).pin_memory() for k, a in case.real.items()}
    torch.cuda.synchronize()

    def once():
        with torch.cuda.stream(cur):
            return call(dev, arg)

    # Two undelayed calls first, on the real input and then on the decoy.  They grow the library's
    # scratch to what either input needs (dalloc / grow free and reallocate, and hipFree waits for
    # the whole device, which would drain the delay and hide a misordering; the two inputs have
    # one shape but not always one result size) and fill torch's caching allocator on the streams
    # used: with the same context, handle and shapes the measured call below allocates nothing.
    SC.same(_read(once(), case.want_real, torch, consumer), case.want_real, f"{case.name} {mode} priming")
    for k, a in case.decoy.items():
        dev[k].copy_(_t(a))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = once()
    warm_ms = (time.perf_counter() - t0) * 1e3
    SC.same(_read(out, case.want_decoy, torch, consumer), case.want_decoy, f"{case.name} {mode} warm-up")
    del out
    torch.cuda.synchronize()

    delay_ms = max(FLOOR_MS, MARGIN * warm_ms)
    print(f"[streams] {case.name} {mode}: warm-up {warm_ms:.2f} ms, delay {delay_ms:.0f} ms")
    ev, ev_long = torch.cuda.Event(), torch.cuda.Event()
    if mode == "explicit":  # the default stream, torch's current one, stays busy past the call
        rig.sleep(LONG * delay_ms)
        ev_long.record()
    with torch.cuda.stream(producer):
        rig.sleep(delay_ms)
        ev.record()
        for k, t in dev.items():
            t.copy_(host[k], non_blocking=True)
    assert not ev.query(), "the delay ended before the call was made: inconclusive"
    out = once()
    try:
        if mode == "control":
            assert not ev.query(), "the call did not return while the producing stream was busy: inconclusive"
            # the call is synchronous, so the outputs were complete at the assertion above; reading
            # them back may itself queue behind the producer's pending host-to-device copies
            SC.same(_read(out, case.want_decoy, torch, consumer), case.want_decoy,
                    f"{case.name} control (a stale read must see the decoy)")
            return
        if mode == "explicit":
            assert not ev_long.query(), "the call waited for the default stream"
        SC.same(_read(out, case.want_real, torch, consumer), case.want_real, f"{case.name} {mode}")
        if mode == "explicit":  # whatever the wrapper queued on the default stream has now run
            torch.cuda.synchronize()
            SC.same(_read(out, case.want_real, torch, consumer), case.want_real,
                    f"{case.name} explicit, after the default stream drained")
    finally:
        torch.cuda.synchronize()


# ---- the calls -------------------------------------------------------------------------------
def _calls(ctx, lookup_ctx, idx, torch):
    i64 = dict(dtype=torch.int64, device="cuda")
    pt = lib_table("default")

    def build(dev, stream):
        n = SC.case("build").static["n"]
        fp, po, res = torch.empty(n, **i64), torch.empty(n, **i64), torch.empty(n, **i64)
        info = ctx.build(dev["blob"], dev["offsets"], n, fp, po, stream=stream)
        ctx.lookup(dev["blob"], dev["offsets"], n, fp, po, n, res, stream=stream)
        # mph_bin has no stream argument (a null-stream D2H): taken when the outputs are read
        return {"fp": fp, "pos": po, "lookup": res, "mph": ctx.mph_bin, "n_keys": info["n_keys"],
                "mph_bin_len": info["mph_bin_len"], "status": info["status"]}

    def lookup(dev, stream):
        c, d_fp, d_po = lookup_ctx
        st = SC.case("lookup").static
        res = torch.empty(st["nq"], **i64)
        c.lookup(dev["blob"], dev["offsets"], st["nq"], d_fp, d_po, st["n"], res, stream=stream)
        return {"result": res}

    def finalize_index(dev, stream):
        return ctx.finalize_index(dev["blob"], dev["offsets"], SC.case("finalize_index").static["n"], stream=stream)

    def sort_objects(dev, stream):
        order, info = ctx.sort_objects(dev["keys"], dev["offsets"], SC.M_OBJ, stream=stream)
        return dict(info, order=order)

    def gather_objects(dev, stream):
        return ctx.gather_objects(dev["keys"], dev["offsets"], SC.M_OBJ, dev["order"], dev["sizes"], dev["tiers"],
                                  stream=stream)

    def aggregate(dev, stream):
        info = ctx.aggregate_plan(dev["keys"], dev["offsets"], SC.M_OBJ, dev["sizes"], 0, stream=stream,
                                  tiers=dev["tiers"])
        out = ctx.aggregate_fill(stream=stream)
        t = ctx.aggregate_fill_tiers(stream=stream)
        n = info["n_prefixes"]
        out.update(info, total_bytes_sum=info["total_bytes"], total_bytes=out["total_bytes"],
                   tier_count=t["tier_count"][:, :n], tier_bytes=t["tier_bytes"][:, :n])
        return out

    def csv(dev, stream):
        st = SC.case("csv").static
        info = ctx.csv_plan(dev["csv"], st["length"], st["schema"], stream=stream)
        return dict(info, **ctx.csv_fill(stream=stream))

    def merge_rows(dev, stream):
        st = SC.case("merge_rows").static
        info = ctx.merge_rows_plan(dev["blob"], dev["offsets"], dev["depth"], dev["count"], dev["bytes"],
                                   st["run_starts"], d_tier_count=dev["tier_count"], d_tier_bytes=dev["tier_bytes"],
                                   tier_stride=st["n"], stream=stream)
        out = ctx.merge_rows_fill(stream=stream)
        n = info["n_out"]
        # a torch op queued on the call's stream right behind the fill consumes its outputs
        with torch.cuda.stream(torch.cuda.current_stream() if stream is None else stream):
            consumed = out["object_count"] + out["total_bytes"]
        out.update(info, consumed=consumed, tier_count=out["tier_count"][:, :n], tier_bytes=out["tier_bytes"][:, :n])
        return out

    def lookup_device(dev, stream):
        return {"pos": idx.lookup_device(dev["blob"], dev["offsets"], SC.NQ, stream=stream)}

    def nodes_device(dev, stream):
        return {"nodes": idx.nodes_device(dev["pos"], stream=stream)}

    def tiers_device(dev, stream):
        out, mask = idx.tiers_device(dev["pos"], stream=stream)
        return {"tiers": out, "mask": mask}

    def cost_device(dev, stream):
        return {"cost": idx.cost_device(dev["pos"], pt, stream=stream)}

    def descendants(name):
        def call(dev, stream):
            mc = SC.case(name).static["min_count"]
            levels, row_ptr, n_rows, total = idx.descendants_plan(dev["pos"], dev["rel"], min_count=mc, stream=stream)
            out = idx.descendants_fill(total, stream=stream)
            return {"levels": levels, "row_ptr": row_ptr, "out": out, "n_rows": n_rows, "total": total}
        return call

    def descendants_upto(dev, stream):
        levels, row_ptr, out = idx.descendants_csr(dev["pos"], None, SC.case("descendants_upto").static["max_rel"],
                                                   stream=stream)
        return {"levels": levels, "row_ptr": row_ptr, "out": out, "n_rows": int(row_ptr.shape[0]) - 1,
                "total": int(out.shape[0])}

    def top_rows(dev, stream):
        top_n, top_pos, top_key = idx.descendants_top(dev["pos"], dev["rel"], key="cost", k=SC.K, pt=pt, stream=stream)
        return {"top_n": top_n, "top_pos": top_pos, "top_key": top_key, "n_rows": int(top_n.shape[0])}

    def top_one(dev, stream):
        _, _, n_rows, _ = idx.descendants_plan(dev["pos"], dev["rel"], stream=stream)
        top_n, top_pos, top_key = idx.top_of_plan(n_rows, "count", SC.K, stream=stream)
        return {"top_n": top_n, "top_pos": top_pos, "top_key": top_key, "n_rows": n_rows}

    return {"build": build, "lookup": lookup, "finalize_index": finalize_index, "sort_objects": sort_objects,
            "gather_objects": gather_objects, "aggregate": aggregate, "csv": csv, "merge_rows": merge_rows,
            "lookup_device": lookup_device, "nodes_device": nodes_device, "tiers_device": tiers_device,
            "cost_device": cost_device, "descendants_at": descendants("descendants_at"),
            "descendants_filtered": descendants("descendants_filtered"), "descendants_upto": descendants_upto,
            "top_rows": top_rows, "top_one": top_one}


@pytest.fixture(scope="module")
def calls(rig, ctx, lookup_ctx, idx):
    c = _calls(ctx, lookup_ctx, idx, rig.torch)
    assert set(c) == set(SC.NAMES)
    return c


# ---- the tests -------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", SC.NAMES)
def test_the_call_is_ordered_on_its_stream(rig, calls, name, mode):
    drive(rig, SC.case(name), calls[name], mode)


# one of every family and the wrappers that fill their outputs with torch
CONTROLS = ("lookup", "aggregate", "merge_rows", "descendants_at", "tiers_device")


@pytest.mark.parametrize("name", CONTROLS)
def test_another_stream_sees_the_decoy(rig, calls, name):
    """The negative control: called with a stream that does not produce the inputs, the library
    returns while the producer is still delayed and answers for the decoy."""
    assert {SC.case(n).family for n in CONTROLS} == set(SC.FAMILIES)
    drive(rig, SC.case(name), calls[name], "control")


def test_host_arguments_are_converted_on_the_given_stream(rig, idx):
    """Positions and rel given as host values: the wrapper's own upload and its zero fills go to
    the stream it passes on, so the call neither waits for a busy default stream nor races it."""
    torch = rig.torch
    c = SC.case("descendants_at")
    pos = c.real["pos"]
    want = SC._at_rows(pos, np.ones(len(pos), np.int32))[0]
    tiers_want = SC.case("tiers_device").want_real

    def call():
        levels, row_ptr, n_rows, total = idx.descendants_plan(pos, 1, stream=rig.s)
        out = idx.descendants_fill(total, stream=rig.s)
        t, mask = idx.tiers_device(pos, stream=rig.s)
        return {"levels": levels, "row_ptr": row_ptr, "out": out, "n_rows": n_rows, "total": total, "tiers": t,
                "mask": mask}

    both = dict(want, **tiers_want)
    t0 = time.perf_counter()
    SC.same(_read(call(), both, torch, rig.s), both, "warm-up")
    delay_ms = max(FLOOR_MS, MARGIN * (time.perf_counter() - t0) * 1e3) * LONG
    torch.cuda.synchronize()
    ev = torch.cuda.Event()
    rig.sleep(delay_ms)
    ev.record()
    out = call()
    try:
        assert not ev.query(), "the call waited for the default stream"
        SC.same(_read(out, both, torch, rig.s), both, "on the stream")
        torch.cuda.synchronize()
        SC.same(_read(out, both, torch, rig.s), both, "after the default stream drained")
    finally:
        torch.cuda.synchronize()
