"""Index directories for the reader tests, written from the oracle alone (no GPU): the MPHF
files through s3imph.write_index_files, the finalize arrays of oracle_lib.finalize in the
reference's S3ID framing, and optionally object_count.u64 / total_bytes.u64."""
import os

import numpy as np

import oracle as O
import s3imph

FINALIZE_FILES = (("subtree_end.u64", "subtree_end", 8), ("depth.u32", "depth", 4),
                  ("max_depth_in_subtree.u32", "max_depth_in_subtree", 4), ("depth_offsets.u64", "depth_offsets", 8),
                  ("depth_positions.u64", "depth_positions", 8))


def s3id_array(vals, width):
    """O.s3id_u64_array / O.s3id_u32_array (the latter packs value by value: large u32 arrays
    take the same bytes from numpy)."""
    if width == 8:
        return O.s3id_u64_array(vals)
    if len(vals) <= 4096:
        return O.s3id_u32_array(vals)
    return O.s3id_header(len(vals), 4) + np.ascontiguousarray(vals, dtype="<u4").tobytes()


def write_stats(path, object_count, total_bytes):
    for name, vals in (("object_count.u64", object_count), ("total_bytes.u64", total_bytes)):
        with open(os.path.join(path, name), "wb") as f:
            f.write(s3id_array(vals, 8))


def write_index_dir(path, oracle_lib, keys, stats=None, depths=None):
    """Writes the directory for the byte-sorted `keys`; returns oracle_lib.finalize's arrays."""
    blob, offs = O.keys_to_blob(keys)
    st, fp, pos, mph = oracle_lib.build(blob, offs)
    assert st == 0
    os.makedirs(path, exist_ok=True)
    s3imph.write_index_files(str(path), mph, fp, pos, blob, offs)
    arr = oracle_lib.finalize(blob, offs, None if depths is None else np.asarray(depths, np.uint32))
    for name, key, width in FINALIZE_FILES:
        with open(os.path.join(path, name), "wb") as f:
            f.write(s3id_array(arr[key], width))
    if stats is not None:
        write_stats(path, *stats)
    return arr
