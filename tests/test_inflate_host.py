"""The decode functions the GPU inflate shares with the host (s3imph_inflate.h: the bit reader, the
table builder, the header walk, step()) on the CPU: tools/inflate_host.cpp drives them as lane 0 of
k_inflate does, built here with AddressSanitizer and UndefinedBehaviorSanitizer, over every case
of gzip_cases at four window sizes, and every field and every byte is compared with gzip_ref.  The
driver's window is a buffer of exactly the window's size, so a read outside it is reported, and it
counts steps, so a broken termination argument fails here and hangs no GPU.  No GPU."""
import os
import re
import shutil
import subprocess

import pytest

import gzip_cases as K
import gzip_ref as G
from conftest import ROOT

CXX = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
WINDOWS = (64, 80, K.IN_CHUNK, 0)  # 64 is the smallest a refill may leave a step's bytes in; 0: the whole file
CASES = K.VALID + K.INVALID
LINE = re.compile(rb"window=(\d+) status=(\d+) out_bytes=(\d+) in_used=(\d+) members=(\d+) crc32=(\d+) steps=(\d+) "
                  rb"text=(\d+)\n")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if CXX is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path_factory.mktemp("inflate_host") / "inflate_host")
    # the sanitizers' runtimes are linked into the program (GCC's flags, then Clang's), so that
    # it starts whatever else the process environment loads in front of it
    for static in (["-static-libasan", "-static-libubsan"], ["-static-libsan"]):
        p = subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror"] + static +
                           ["-I", os.path.join(ROOT, "s3-inv-db_amd", "csrc"),
                            os.path.join(ROOT, "tools", "inflate_host.cpp"), "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        if p.returncode == 0:
            return exe
    raise AssertionError(p.stdout.decode(errors="replace")[-3000:])


def run(exe, path, data):
    """[(window, fields, steps, text)] of one driver process, a plain child of this one."""
    with open(path, "wb") as f:
        f.write(data)
    p = subprocess.run([exe, path, str(K.BATCH)] + [str(w) for w in WINDOWS], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE)
    assert p.returncode == 0 and p.stderr == b"", (p.returncode, p.stderr.decode(errors="replace")[-2000:])
    runs, at = [], 0
    for _ in WINDOWS:
        m = LINE.match(p.stdout, at)
        assert m, p.stdout[at:at + 200]
        window, status, out_bytes, in_used, members, crc32, steps, n = (int(g) for g in m.groups())
        text = p.stdout[m.end():m.end() + n]
        assert len(text) == n and p.stdout[m.end() + n:m.end() + n + 1] == b"\n"
        at = m.end() + n + 1
        runs.append((window, dict(status=status, out_bytes=out_bytes, in_used=in_used, members=members, crc32=crc32),
                     steps, text))
    assert at == len(p.stdout) and [r[0] for r in runs] == list(WINDOWS)
    return runs


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_host_driver_agrees_with_gzip_ref(driver, tmp_path, case):
    text, tr = K.refs()[case.name]
    assert tr.status == case.status
    want = dict(status=tr.status, out_bytes=len(text), in_used=tr.in_used, members=tr.members, crc32=tr.crc32)
    skip = ()
    if tr.status in (G.EOF, G.HEADER):
        # section 5j defines in_used for a file that was read to its end only; the two readers
        # agree on it behind corrupt data as well, but not on where a cut or a bad header byte
        # lies: step() has taken the byte that gzip_ref refuses to take
        skip = ("in_used",)
    elif tr.status == G.CHECKSUM:
        # the text's CRC is compared after the decode (k_crc32_fold on the GPU), so a member
        # with a wrong one has been counted and its promised CRC folded in; gzip_ref stops at it
        skip = ("members", "crc32")
    for window, got, steps, got_text in run(driver, str(tmp_path / "case.gz"), case.data):
        for k in skip:
            got[k] = want[k]
        assert got == want, (case.name, window)
        assert got_text == text, (case.name, window)
        assert steps <= 64 + 16 * 8 * len(case.data)
