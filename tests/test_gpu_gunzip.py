"""gzip files inflated on the GPU (include/s3imph.h section 5j) against gzip_ref and zlib, byte for
byte and info field for info field.  Every input lies at an odd offset inside an allocation
poisoned with 0xA5, every output range in a buffer poisoned with 0x5A, and every byte a file may
not write must still be poison afterwards: beyond its out_bytes, beyond its room, around the
ranges.  The corrupt files are ordinary data for a decoder that checks its bounds: each must end
with its status, leave the poison alone and let the call return."""
import gzip
import zlib

import numpy as np
import pytest

import gzip_cases as K
import gzip_ref as G
import s3imph

pytestmark = pytest.mark.gpu

IN_POISON, OUT_POISON = 0xA5, 0x5A
CRC_ONLY = ("crc_bit", "stored_payload_bit")  # ISIZE is right and every bit decodes: only the CRC-32 tells
NAMED = [c for c in K.VALID if not c.name.startswith("filler_")]
FILLERS = [c for c in K.VALID if c.name.startswith("filler_")]


@pytest.fixture(scope="module")
def ctx():
    c = s3imph.DeviceBuilder(0)
    yield c
    c.close()


def pack(files):
    """The files back to back from byte 1 of a poisoned allocation, and their offsets."""
    import torch
    offs = np.cumsum([1] + [len(f) for f in files]).tolist()
    raw = np.full(offs[-1] + 9, IN_POISON, np.uint8)
    for f, o in zip(files, offs):
        raw[o:o + len(f)] = np.frombuffer(f, np.uint8)
    return torch.from_numpy(raw).to("cuda"), offs


def inflate(ctx, cases, rooms=None, stream=None):
    """One call over `cases`; rooms default to the text's length (exact).  Checks every file
    against the reference and every byte outside what it may write; returns the infos."""
    import torch
    refs = K.refs()
    texts = [refs[c.name][0] for c in cases]
    if rooms is None:
        rooms = [len(t) for t in texts]
    d_gz, gz_offs = pack([c.data for c in cases])
    out_offs = np.cumsum([3] + list(rooms)).tolist()
    d_out = torch.full((out_offs[-1] + 11,), OUT_POISON, dtype=torch.uint8, device="cuda")
    infos = ctx.gunzip(d_gz, gz_offs, d_out, out_offs, stream=stream)
    out = d_out.cpu().numpy()
    assert (out[:3] == OUT_POISON).all() and (out[out_offs[-1]:] == OUT_POISON).all()
    assert len(infos) == len(cases)
    for c, text, room, o, info in zip(cases, texts, rooms, out_offs, infos):
        tr = refs[c.name][1]
        got = out[o:o + room].tobytes()
        if c.status != G.OK:
            # a wrong CRC shows only on a text that was written whole: short of room the file needs more
            unseen = c.name in CRC_ONLY and info["out_bytes"] > room
            assert info["status"] == (s3imph.GZ_MORE if unseen else c.status), (c.name, info)
            continue
        want = dict(out_bytes=len(text), in_used=len(c.data), members=tr.members,
                    status=s3imph.GZ_OK if len(text) <= room else s3imph.GZ_MORE, crc32=zlib.crc32(text), reserved=0)
        assert info == want, c.name
        fit = min(len(text), room)
        assert got[:fit] == text[:fit], c.name
        assert got[fit:] == bytes([OUT_POISON]) * (room - fit), c.name
    return infos


@pytest.mark.parametrize("case", NAMED, ids=[c.name for c in NAMED])
def test_valid_streams_alone(ctx, case):
    inflate(ctx, [case])


def test_filler_at_every_length_in_one_call(ctx):
    inflate(ctx, FILLERS)


def test_every_valid_stream_in_one_call(ctx):
    inflate(ctx, K.VALID)


ROOMY = [c for c in NAMED if c.name in ("dynamic_level_6", "stored_65535", "fixed_258_at_32768", "rle", "two_members",
                                        "dependent_matches_over_a_batch_edge", "match_into_previous_stored_block",
                                        "huffman_only_15_bits", "empty_member", "every_length_and_distance_symbol",
                                        "sync_flush_every_50_bytes", "single_distance_code",
                                        "stored_then_matches_then_stored")]


@pytest.mark.parametrize("short", ["one_byte", "half", "all"])
def test_too_little_room_reports_the_size_and_keeps_what_fits(ctx, short):
    refs = K.refs()
    sizes = [len(refs[c.name][0]) for c in ROOMY]
    rooms = [max(n - 1, 0) if short == "one_byte" else n // 2 if short == "half" else 0 for n in sizes]
    infos = inflate(ctx, ROOMY, rooms)
    # the empty member needs no room at all
    assert [i["status"] for i in infos] == [s3imph.GZ_MORE if n else s3imph.GZ_OK for n in sizes]


def test_room_of_three_crc_chunks_beyond_the_text(ctx):
    """Every room exceeds its text by 3 x 8192 + 5 bytes: k_crc32_chunks has lanes whose chunk lies
    wholly behind the text, and k_crc32_fold ends on whole chunks for the texts that are a
    multiple of 8192 and on a short one for the others."""
    refs = K.refs()
    sizes = [len(refs[c.name][0]) for c in NAMED]
    assert {8191, 8192, 8193, 16384} <= set(sizes)
    infos = inflate(ctx, NAMED, [n + 3 * 8192 + 5 for n in sizes])
    assert [i["status"] for i in infos] == [s3imph.GZ_OK] * len(NAMED)


def test_more_files_than_the_grid_has_waves(ctx):
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = cus * K.WAVES_PER_CU + 3
    inflate(ctx, [FILLERS[(7 * i) % len(FILLERS)] for i in range(n)])


def test_invalid_streams_end_with_their_status(ctx):
    inflate(ctx, K.INVALID, rooms=[517] * len(K.INVALID))
    # and without any room
    inflate(ctx, K.INVALID, rooms=[0] * len(K.INVALID))


BAD_NAMES = ("cut_at_33", "bad_magic_0", "wrong_fhcrc", "trailing_zeros", "zero_length", "block_type_3",
             "len_nlen_mismatch", "distance_past_the_member_start", "second_member_reaches_into_the_first",
             "over_subscribed_code_lengths", "crc_bit", "isize_bit", "stored_payload_bit",
             "unused_bit_of_the_single_distance_code", "fixed_symbol_286_then_the_end",
             "one_stage_cut_at_%d" % K.IN_CHUNK)


@pytest.mark.parametrize("name", BAD_NAMES)
def test_one_bad_file_between_two_good_ones(ctx, name):
    bad = next(c for c in K.INVALID if c.name == name)
    good = {c.name: c for c in NAMED}
    cases = [good["dynamic_level_6"], bad, good["two_members"]]
    refs = K.refs()
    infos = inflate(ctx, cases, rooms=[len(refs[cases[0].name][0]), 700, len(refs[cases[2].name][0])])
    assert [i["status"] for i in infos] == [s3imph.GZ_OK, bad.status, s3imph.GZ_OK]


def test_host_gunzip_of_a_mixed_list():
    names = ("empty_member", "stored_65535", "dynamic_level_9", "three_members", "fixed_258_at_32768", "filler_17",
             "all_flags", "huffman_only_15_bits")
    files = [next(c.data for c in K.VALID if c.name == n) for n in names]
    files.insert(3, K.lying_isize(K.filler(40000, 2), 5))  # the hint says 5 bytes: inflated twice
    texts, infos = s3imph.gunzip(files, with_info=True)
    assert texts == [gzip.decompress(f) for f in files]
    assert [i["status"] for i in infos] == [s3imph.GZ_OK] * len(files)
    assert [i["crc32"] for i in infos] == [zlib.crc32(t) for t in texts]
    assert infos[3]["members"] == 2 and infos[3]["out_bytes"] == 40005


def test_host_gunzip_names_the_first_bad_file():
    good = next(c.data for c in K.VALID if c.name == "dynamic_level_1")
    by_name = {c.name: c for c in K.INVALID}
    for name, text in (("cut_at_40", "unexpected EOF"), ("cm_7", "invalid header"),
                       ("block_type_3", "corrupt input"), ("crc_bit", "invalid checksum")):
        files = [good, good, by_name[name].data, good, by_name["zero_length"].data]
        with pytest.raises(s3imph.MPHFError) as e:
            s3imph.gunzip(files)
        assert e.value.status == s3imph.ERR_FORMAT and str(e.value) == "gzip: file 2: " + text


def test_gunzip_on_a_busy_stream(ctx):
    """DeviceBuilder.gunzip on a caller's stream that is still busy producing its input: behind a
    delay the stream copies the real file over a decoy of the same size; the call is made while
    the delay is pending and must answer for the real file (test_gpu_streams.py's method)."""
    import torch
    from test_gpu_streams import FLOOR_MS, Rig
    rig = Rig()
    decoy, real = K.with_size(1500, 71), K.with_size(1500, 72)
    t_decoy, t_real = gzip.decompress(decoy), gzip.decompress(real)
    assert len(decoy) == len(real) == 1500 and t_decoy != t_real
    room = max(len(t_decoy), len(t_real))
    d_gz, offs = pack([decoy])
    pinned = torch.from_numpy(np.frombuffer(real, np.uint8).copy()).pin_memory()
    d_out = torch.full((room + 16,), OUT_POISON, dtype=torch.uint8, device="cuda")
    # the warm-up answers for the decoy
    info = ctx.gunzip(d_gz, offs, d_out, [5, 5 + room])[0]
    assert info["crc32"] == zlib.crc32(t_decoy) and info["status"] == s3imph.GZ_OK
    ev = torch.cuda.Event()
    with torch.cuda.stream(rig.s):
        rig.sleep(FLOOR_MS)
        ev.record()
        d_gz[1:1501].copy_(pinned, non_blocking=True)
    assert not ev.query(), "the delay ended before the call"
    info = ctx.gunzip(d_gz, offs, d_out, [5, 5 + room], stream=rig.s)[0]
    assert info["status"] == s3imph.GZ_OK and info["out_bytes"] == len(t_real) and info["crc32"] == zlib.crc32(t_real)
    with torch.cuda.stream(rig.s):
        out = d_out.cpu().numpy()
    assert out[5:5 + len(t_real)].tobytes() == t_real
    torch.cuda.synchronize()
