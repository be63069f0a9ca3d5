"""bench.py --dump-outputs and the plain / --full split.

CPU: dump_outputs() stores every value exactly (u64 as two 32-bit halves in float64), keeps
the same seeded sample from run to run, stays under 64 MB, and its digests cover the whole
arrays.  GPU: a plain C2 run prints only the headline's line and dumps the build's outputs,
which equal the oracle's at every sampled entry; --full adds the lines that ride beside it."""
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402

M64 = (1 << 64) - 1
NAMES = ["sample_index", "mph_fp_hi32", "mph_fp_lo32", "mph_pos", "mph_bin_index", "mph_bin_words", "digest"]


def _load(d):
    out = {}
    for name in NAMES:
        a = np.load(os.path.join(str(d), name + ".npy"))
        assert a.dtype == np.float64
        out[name] = a
    return out


def _from_limbs(limbs) -> int:
    return sum(int(x) << (16 * i) for i, x in enumerate(limbs))


def _check_dump(d, fp, po, mph):
    """The dump in directory d against the whole outputs (u64 fp, u64 po, mph.bin bytes)."""
    a = _load(d)
    n = len(fp)
    idx = a["sample_index"].astype(np.int64)
    assert len(idx) == min(n, bench.DUMP_SAMPLE) and idx.min() >= 0 and idx.max() < n
    assert np.all(np.diff(idx) >= 0)
    got_fp = (a["mph_fp_hi32"].astype(np.uint64) << np.uint64(32)) | a["mph_fp_lo32"].astype(np.uint64)
    assert np.array_equal(got_fp, fp[idx])
    assert np.array_equal(a["mph_pos"].astype(np.uint64), po[idx])
    words = np.frombuffer(mph + b"\0" * (-len(mph) % 4), dtype="<u4")
    widx = a["mph_bin_index"].astype(np.int64)
    assert len(widx) == min(len(words), bench.DUMP_SAMPLE)
    assert np.array_equal(a["mph_bin_words"].astype(np.uint32), words[widx])
    dg = a["digest"]
    assert len(dg) == 18
    assert _from_limbs(dg[0:4]) == int(fp.sum(dtype=np.uint64))
    assert _from_limbs(dg[4:8]) == int(po.sum(dtype=np.uint64))
    assert _from_limbs(dg[8:10]) == zlib.crc32(mph)
    assert _from_limbs(dg[10:14]) == len(mph)
    assert _from_limbs(dg[14:18]) == n
    total = sum(os.path.getsize(os.path.join(str(d), f)) for f in os.listdir(str(d)))
    assert total <= 64 * 10**6
    return a


@pytest.mark.parametrize("n", [1000, bench.DUMP_SAMPLE + 12345])
def test_dump_outputs_exact_repeatable_and_bounded(tmp_path, n):
    import torch
    rng = np.random.default_rng(7)
    fp = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    po = rng.permutation(n).astype(np.uint64)
    mph = rng.bytes(4 * n + 3)
    # the device arrays may be longer than the build's output count: the tail is not output
    t_fp = torch.from_numpy(np.concatenate([fp, fp[:5]]).view(np.int64))
    t_po = torch.from_numpy(np.concatenate([po, po[:5]]).view(np.int64))
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), t_fp, t_po, n, mph)
    a = _check_dump(tmp_path / "a", fp, po, mph)
    b = _load(tmp_path / "b")
    for name in NAMES:
        assert np.array_equal(a[name], b[name]), name


def _run_bench(*argv):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *argv], capture_output=True,
                       text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1
    return lines[0]


HEADLINE_KEYS = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus"}
FULL_ONLY_KEYS = {"stages_ms", "roofline", "lookup", "finalize", "host_e2e", "bitmap_n1", "secondary", "cpu_baseline"}


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_builds_outputs(tmp_path, oracle_lib):
    import s3imph
    res = _run_bench("--config", "c2", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "out"))
    assert HEADLINE_KEYS <= set(res)
    assert not FULL_ONLY_KEYS & set(res), sorted(FULL_ONLY_KEYS & set(res))
    assert res["steps"] == 3 and res["warmup"] == 1 and res["unit"] == "keys/s" and res["dtype"] == "u64"
    cfg = bench.CONFIGS["c2"]
    n = cfg["keys_per_gpu"]
    assert res["value"] == pytest.approx(n / (res["ms_per_step"] / 1e3))
    blob, offs = s3imph.gen_keys(cfg["kind"], 42, cfg["avg"], 0, n)
    st, fp, po, mph = oracle_lib.build(blob[: offs[-1]], offs)
    assert st == 0
    _check_dump(tmp_path / "out", fp, po, mph)


@pytest.mark.gpu
def test_full_run_adds_the_lines_beside_the_headline():
    res = _run_bench("--full", "--config", "c2", "--steps", "2", "--warmup", "1", "--no-cpu-baseline",
                     "--no-secondary")
    assert HEADLINE_KEYS <= set(res)
    assert {"stages_ms", "roofline", "lookup", "finalize", "host_e2e"} <= set(res)
    assert res["lookup"]["all_members_found"] is True
    assert res["steps"] == 2
