"""The prefix-blob entry points on a caller's busy stream (include/s3imph.h: every query call waits
for its stream before it returns): prefixes_plan + prefixes_fill, lookup_verify_device and
verify_device, called while the stream that produces their inputs is still busy (run on an MI355X,
-m gpu).  The decoy / real form of tests/test_gpu_streams.py, with helpers of its own.

Method.  The device tensors a call reads hold a decoy.  Two undelayed calls come first, on the real
input and on the decoy, each checked (they also grow the handle's scratch to what either needs, so
the measured call allocates nothing: hipFree would drain the device and hide a misordering).  Then a
delay (torch.cuda._sleep, its rate measured per session) is queued on the producing stream, an event
recorded behind it and the real input copied in behind that from pinned memory; the event must still
be pending when the call is made, and the call must answer for the real input, exactly, by the time
it returns.  Modes: `current` (torch's current stream is the side stream), `explicit` (stream=s
while the default stream sits behind a three times longer delay that must still be pending after
the call), `null` (the default stream throughout, the library on its own blocking stream).  The
control calls on another non-blocking stream than the one that produces: it must return while the
event is pending and answer for the decoy, or the run shows nothing.

The two inputs of a case have one shape and both are in bounds for the kernels in any mixture:
positions are below n or one of the values the kernels check (n, 2^64 - 1); the query and the stored
blobs are fixed-width keys over one offsets array that is never rewritten."""
import time

import numpy as np
import pytest

import names_cases as NC
import oracle as O

pytestmark = pytest.mark.gpu

NOT_FOUND = NC.NOT_FOUND
MODES = ("current", "explicit", "null")
FLOOR_MS, MARGIN, LONG = 50.0, 10.0, 3.0
N = 3000
NQ = 2500


def _keys(real: bool):
    """3000 byte-sorted keys of 11 bytes; the real set substitutes d -> e, s -> t (monotone)."""
    a, b = (b"e", b"t") if real else (b"d", b"s")
    keys = [a + b"%03d/" % (i // 10) + b + b"%04d/" % i for i in range(N)]
    assert keys == sorted(set(keys)) and all(len(k) == 11 for k in keys)
    return keys


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


class World:
    pass


@pytest.fixture(scope="module")
def world(rig, oracle_lib):
    """An attached handle over the decoy key set's MPHF.  Its stored-prefix blob is a device tensor
    the test owns (w.d_stored): the verify case rewrites it, the others leave the decoy keys there."""
    import s3imph
    w = World()
    w.keys, w.other = _keys(False), _keys(True)
    w.blob, w.offs = O.keys_to_blob(w.keys)
    st, fp, pos, mph = oracle_lib.build(w.blob, w.offs)
    assert st == 0
    w.idx = NC.attached(s3imph, mph, fp, pos)
    w.d_stored = NC.dev(NC.padded(w.blob))
    w.d_offs = NC.dev(w.offs)
    w.idx.attach_prefixes(w.d_stored, w.d_offs)
    st, w.m = oracle_lib.unmarshal(mph)
    assert st == 0
    w.lookup = lambda k: oracle_lib.lookup(w.m, fp, pos, k)
    yield w
    w.idx.close()


def _host(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a.copy())


def _same(got: dict, want: dict, what: str) -> None:
    for name, w in want.items():
        g = got[name]
        if isinstance(w, np.ndarray):
            g = np.asarray(g)
            assert g.shape == w.shape and g.tobytes() == w.tobytes(), (what, name)
        else:
            assert g == w, (what, name, g, w)


def _read(out: dict, want: dict, torch, stream) -> dict:
    got = {}
    with torch.cuda.stream(stream):
        for k, w in want.items():
            v = out[k]
            if torch.is_tensor(v):
                v = v.cpu().numpy()
                if isinstance(w, np.ndarray):
                    v = np.ascontiguousarray(v).reshape(-1).view(w.dtype)[:w.size].reshape(w.shape)
            got[k] = v
    return got


def drive(rig, dev, real, decoy, want_real, want_decoy, call, mode, what):
    """dev: the device tensors the call reads, by name; real / decoy: their two contents (numpy);
    call(stream) makes the library call(s) and returns the outputs by the names of `want_*`."""
    torch = rig.torch
    s, s2, default = rig.s, rig.s2, rig.default
    arg = {"current": None, "explicit": s, "null": None, "control": s2}[mode]
    cur = s if mode == "current" else default
    producer = default if mode == "null" else s
    consumer = {"current": s, "explicit": s, "null": default, "control": s2}[mode]
    host = {k: _host(a).pin_memory() for k, a in real.items()}

    def once():
        with torch.cuda.stream(cur):
            return call(arg)

    for k, a in real.items():
        dev[k].copy_(_host(a))
    torch.cuda.synchronize()
    _same(_read(once(), want_real, torch, consumer), want_real, f"{what} {mode} priming")
    for k, a in decoy.items():
        dev[k].copy_(_host(a))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = once()
    warm_ms = (time.perf_counter() - t0) * 1e3
    _same(_read(out, want_decoy, torch, consumer), want_decoy, f"{what} {mode} warm-up")
    del out
    torch.cuda.synchronize()

    delay_ms = max(FLOOR_MS, MARGIN * warm_ms)
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
            _same(_read(out, want_decoy, torch, consumer), want_decoy, f"{what} control (a stale read sees the decoy)")
            return
        if mode == "explicit":
            assert not ev_long.query(), "the call waited for the default stream"
        _same(_read(out, want_real, torch, consumer), want_real, f"{what} {mode}")
        if mode == "explicit":
            torch.cuda.synchronize()
            _same(_read(out, want_real, torch, consumer), want_real, f"{what} explicit, after the default stream drained")
    finally:
        torch.cuda.synchronize()


# ---- prefixes_plan + prefixes_fill ---------------------------------------------------------------
def _names_case(w):
    rng = np.random.default_rng(41)
    decoy = rng.integers(0, N, NQ).astype(np.uint64)
    real = rng.integers(0, N, NQ).astype(np.uint64)
    real[::9] = N            # not found: the real answer is shorter
    real[4::31] = NOT_FOUND
    wants = []
    for pos in (decoy, real):
        offs, found, raw = NC.want_names(w.blob, w.offs, pos)
        wants.append({"offsets": offs, "found": found, "bytes": raw, "total": int(offs[-1])})
    assert wants[0]["total"] != wants[1]["total"]
    return decoy, real, wants[0], wants[1]


def _names_call(w, d_pos):
    def call(stream):
        offs, found, out = w.idx.prefixes_device(d_pos, stream=stream)
        return {"offsets": offs, "found": found, "bytes": out, "total": int(out.numel())}
    return call


def _names_want(want):
    # the fill returns round_up(total, 8) bytes: compared as that size
    return dict(want, total=len(want["bytes"]))


@pytest.mark.parametrize("mode", MODES + ("control",))
def test_prefixes_on_a_busy_stream(rig, world, mode):
    decoy, real, want_decoy, want_real = _names_case(world)
    d_pos = NC.dev(decoy)
    drive(rig, {"pos": d_pos}, {"pos": real}, {"pos": decoy}, _names_want(want_real), _names_want(want_decoy),
          _names_call(world, d_pos), mode, "prefixes")


# ---- lookup_verify_device ------------------------------------------------------------------------
def _verify_lookup_case(w):
    """Queries of one width over one offsets array: the decoy asks for members in order, the real
    one for members in reverse with every fifth a non-member (the other set's key)."""
    decoy = w.keys[:NQ]
    real = [w.other[i] if i % 5 == 0 else w.keys[NQ - 1 - i] for i in range(NQ)]
    at = {k: i for i, k in enumerate(w.keys)}
    wants = []
    for q in (decoy, real):
        wants.append({"pos": np.array([at.get(k, NOT_FOUND) for k in q], np.uint64)})
        # the oracle's Lookup agrees wherever it finds the key's own bytes
        for k, p in list(zip(q, wants[-1]["pos"]))[::97]:
            if p != NOT_FOUND:
                assert w.lookup(k) == int(p)
    (db, offs), (rb, offs2) = O.keys_to_blob(decoy), O.keys_to_blob(real)
    assert np.array_equal(offs, offs2)
    return NC.padded(db), NC.padded(rb), offs, wants[0], wants[1]


@pytest.mark.parametrize("mode", MODES + ("control",))
def test_lookup_verify_on_a_busy_stream(rig, world, mode):
    db, rb, offs, want_decoy, want_real = _verify_lookup_case(world)
    d_blob, d_offs = NC.dev(db), NC.dev(offs)

    def call(stream):
        return {"pos": world.idx.lookup_verify_device(d_blob, d_offs, NQ, stream=stream)}

    drive(rig, {"blob": d_blob}, {"blob": rb}, {"blob": db}, want_real, want_decoy, call, mode, "lookup_verify")


# ---- verify_device -------------------------------------------------------------------------------
def _stored_case(w):
    """The handle's stored-prefix blob itself is the input: the decoy is the clean blob, the real
    one stores the other set's key at 40 places, none of which the MPHF finds."""
    real = list(w.keys)
    bad = list(range(17, N, 75))
    for i in bad:
        real[i] = w.other[i]
        assert w.lookup(real[i]) is None
    rb, offs = O.keys_to_blob(real)
    assert np.array_equal(offs, w.offs)
    clean = {"n_bad": 0, "first_bad": NOT_FOUND, "first_got": NOT_FOUND}
    return NC.padded(w.blob), NC.padded(rb), clean, {"n_bad": len(bad), "first_bad": bad[0], "first_got": NOT_FOUND}


@pytest.mark.parametrize("mode", MODES + ("control",))
def test_verify_on_a_busy_stream(rig, world, mode):
    db, rb, want_decoy, want_real = _stored_case(world)

    def call(stream):
        n_bad, first_bad, first_got = world.idx.verify_device(stream=stream)
        return {"n_bad": n_bad, "first_bad": first_bad, "first_got": first_got}

    try:
        drive(rig, {"stored": world.d_stored}, {"stored": rb}, {"stored": db}, want_real, want_decoy, call, mode,
              "verify")
    finally:
        world.d_stored.copy_(_host(db))
        rig.torch.cuda.synchronize()
