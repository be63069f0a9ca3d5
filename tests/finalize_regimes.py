"""Which keys each round of k_fin_keys_lds (s3imph_finalize.hip) takes, from the offsets alone.

No GPU and no library: a restatement of the kernel's round walk, so that a test can say on
the CPU whether a key set reaches the window paths of that kernel before a GPU sees it.

The three constants below are copied from the kernel ON PURPOSE.  The coverage conditions
of tests/test_finalize_regimes.py are stated on the inputs through this walk; if someone
changes the kernel's geometry (workgroup size, window bytes, grid), the key sets no longer
cut / fill / exceed the window where the tests say they do.  Update the constants with the
kernel and the conditions fail, naming the set that lost its regime: that failure is the
intended alarm, not a nuisance.  Re-shape the set, do not relax the condition.

The walk (one workgroup per contiguous key range, rounds of up to 2 * kFinT keys):
  grid = min(kFinGrid, ceil(n / (2 * kFinT)));  per = ceil(n / grid)
  range of workgroup b: [b * per, min(n, (b + 1) * per))
  round at r0:  last = min(range end, r0 + 2 * kFinT)
                wlo  = offsets[r0] & ~15
                wend = min(round_up16(offsets[last]), wlo + kFinBB)
                key i of [r0, last) fits when offsets[i + 1] <= wend   (a prefix of the round)
                m = number of fitting keys; m == 0 -> the first key is taken from global memory
                the next round starts at r0 + max(m, 1)
Offsets are taken relative to offsets[0]: the staged pass runs on 16-byte aligned blobs whose
first key starts at the allocation (the host form rebases its offsets the same way).
"""
import numpy as np

kFinT = 256
kFinBB = 32 << 10
kFinGrid = 4096


def walk(offsets) -> dict:
    """rounds / cut / oversize / exact / fit of the staged key pass for these offsets.

    cut       rounds in which the fitting keys are a non-empty, proper prefix of the round
    oversize  rounds whose first key does not fit (it falls back to global memory)
    exact     rounds whose last fitting key ends exactly at wlo + kFinBB
    fit       keys taken from the window (n - fit keys were read from global memory)"""
    offs = np.asarray(offsets, np.uint64).astype(np.int64)
    offs = offs - offs[0]
    n = len(offs) - 1
    out = {"rounds": 0, "cut": 0, "oversize": 0, "exact": 0, "fit": 0}
    if n <= 0:
        return out
    G = 2 * kFinT
    grid = min(kFinGrid, (n + G - 1) // G)
    per = (n + grid - 1) // grid
    for b in range(grid):
        g, gend = b * per, min(n, (b + 1) * per)
        while g < gend:
            last = min(gend, g + G)
            wlo = int(offs[g]) & ~15
            wend = min((int(offs[last]) + 15) & ~15, wlo + kFinBB)
            # ends of the round's keys ascend: the fitting keys are a prefix of the round
            m = int(np.searchsorted(offs[g + 1:last + 1], wend, side="right"))
            out["rounds"] += 1
            if m == 0:
                out["oversize"] += 1
                m = 1
            else:
                out["fit"] += m
                if m < last - g:
                    out["cut"] += 1
                if int(offs[g + m]) == wlo + kFinBB:
                    out["exact"] += 1
            g += m
    return out
