#!/usr/bin/env python3
"""Share of SHORT waves of the staged routed pass 1 (csrc/dvq_pass1.h, SEL == 2) at the headline's inputs, on the CPU: the entropy
maps of bench.py's WeakDual.inputs_np for the three stream slots (B = 256, rank 0), gated at the benchmark's threshold.
A wave is one image row of 32 positions; with f fine cells of 16 in its cell row the even row has 16 + f real columns, the odd
row 2 f; a wave is short when it has at most 16.  Also the MFMA column groups a workgroup scores under the per-wave rule, packed
per row pair and packed per workgroup (the D = 256 form), with the histogram of the last.  Prints one JSON line.
  python tools/short_wave_share.py [-o file.json]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def column_groups(f):
    """MFMA column groups (16 columns; a workgroup of four waves has 8) per workgroup under the three packing rules, from the fine
    cells per cell row f [B, 16] of a dual grid: a workgroup is two cell rows = four image rows, even rows with 16 + f real columns,
    odd rows with 2 f.
    -> {"per_wave": a wave scores one group when it has at most 16 real columns, else two (the rule of every D below 256),
        "per_row_pair": the real columns of a cell row's two image rows packed together,
        "per_workgroup": ceil(nreal_wg / 16), the workgroup-packed form (D = 256),
        "histogram": {G: workgroups} of the last, "workgroups": their number}"""
    f = np.asarray(f).reshape(-1, 2)                                                 # [workgroup][cell row]
    even, odd = 16 + f, 2 * f
    per_wave = ((even > 16).astype(int) + 1 + (odd > 16).astype(int) + 1).sum(-1)
    per_pair = (-(-(even + odd) // 16)).sum(-1)
    g = -(-(even + odd).sum(-1) // 16)
    return {"workgroups": int(g.size), "per_wave": float(per_wave.mean()), "per_row_pair": float(per_pair.mean()),
            "per_workgroup": float(g.mean()), "histogram": {str(int(k)): int((g == k).sum()) for k in np.unique(g)}}


def headline_fine_cells():
    """fine cells per cell row [3 slots][B = 256][16] of the headline's inputs (bench.py's WeakDual.inputs_np, rank 0)"""
    import bench
    from dynamicvectorquantization_amd import synth
    B, b0 = 256, 128
    out = []
    for k in range(3):
        base = synth.entropy_map(5903 + 100 * k, b0, 16, 16, image_offset=0)
        ent = np.concatenate([np.roll(base, 5 * j, axis=-1) for j in range(B // b0)], 0)
        out.append((ent > np.float32(bench.THR_R05)).sum(-1))
    return out


def main():
    import bench
    per_slot, tot_short, tot_waves, fine_cells, cells = [], 0, 0, 0, 0
    fs = headline_fine_cells()
    for k in range(3):
        f = fs[k]                                                                    # fine cells per cell row [B, 16]
        even, odd = 16 + f, 2 * f
        short = int((even <= 16).sum() + (odd <= 16).sum())
        waves = 2 * f.size
        per_slot.append({"slot": k, "waves": waves, "short": short, "share": short / waves,
                         "short_odd_rows": int((odd <= 16).sum()), "short_even_rows": int((even <= 16).sum()),
                         "fine_ratio": float(f.sum()) / (f.size * 16)})
        tot_short += short
        tot_waves += waves
        fine_cells += int(f.sum())
        cells += f.size * 16
    # MFMAs and top-2 updates a short wave leaves out: half of its own
    rec = {"what": "short waves (at most 16 real columns) of pass 1 at the headline's inputs", "threshold": bench.THR_R05,
           "slots": per_slot, "share_of_waves": tot_short / tot_waves, "share_of_mfma_removed": 0.5 * tot_short / tot_waves,
           "fine_ratio": fine_cells / cells,
           "column_groups_per_workgroup": column_groups(np.concatenate(fs, 0))}
    line = json.dumps(rec)
    print(line)
    if "-o" in sys.argv:
        open(sys.argv[sys.argv.index("-o") + 1], "w").write(line + "\n")


if __name__ == "__main__":
    main()
