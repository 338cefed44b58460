"""Time the hopping stage (include/trxsig_l1hop.h) on the production plan (128 ARFCNs; C0: combination V on TN 0, VII on TN 1, I
elsewhere; I on every other carrier) over 104 frames with every combination-I and -VII slot hopping, in allocations of 64 rows
where the plan allows (per TN: the first 64 eligible rows, then the rest; the lone combination-VII slot is an allocation of one):
trxsig_l1hop_bits on a burst grid and its map, trxsig_l1hop_result on a pull-shaped result, and trxsig_l1hop_cells on sample
cells at sps 4 -- each beside the time one read and one write of the bytes it touches would take at the sustained HBM rate
tools/hbm_bench.hip reports on the same box (--hbm-bench: the compiled binary, run first in a process of its own; or --hbm-tbps:
a figure measured elsewhere).  The calls rotate through copies of their buffers whose total is past twice the 256 MiB
memory-side cache, so nothing is served from it.  Medians over repeated HIP-event windows of --calls calls each, per call.
A side measurement: no threshold anywhere.  Results go to profiles/l1hop_bench.json (or --out) and to stdout.

    hipcc --offload-arch=gfx950 -O3 tools/hbm_bench.hip -o hbm_bench
    python tools/l1hop_bench.py --hbm-bench ./hbm_bench [--arfcns 128] [--frames 104] [--reps 30] [--calls 10] [--out profiles/l1hop_bench.json]"""
import argparse
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]


def hbm_rate(path):
    """the read-only line of tools/hbm_bench.hip: TB/s"""
    out = subprocess.run([path], check=True, capture_output=True, text=True, timeout=300).stdout
    m = re.search(r"write 0 B .*= ([0-9.]+) TB/s", out)
    if not m:
        raise SystemExit("no read-only line in the output of %s:\n%s" % (path, out))
    return float(m.group(1)), m.group(0)


def production_plan(A):
    comb = np.ones((A, 8), np.uint8)
    comb[0, 0], comb[0, 1] = 5, 7
    group = np.full((A, 8), -1, np.int8)
    for tn in range(8):
        rows = [a for a in range(A) if comb[a, tn] == 1]
        group[rows[:64], tn] = 0
        group[rows[64:128], tn] = 1                          # (rows past 128 would not hop)
    group[0, 1] = 2
    return comb, group, np.array([1, 17, 5], np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arfcns", type=int, default=128)
    ap.add_argument("--frames", type=int, default=104)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--calls", type=int, default=10, help="calls per HIP-event window")
    ap.add_argument("--hbm-bench", default=None, help="compiled tools/hbm_bench.hip, run before anything else")
    ap.add_argument("--hbm-tbps", type=float, default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "l1hop_bench.json"))
    a = ap.parse_args()
    if (a.hbm_bench is None) == (a.hbm_tbps is None):
        raise SystemExit("give --hbm-bench or --hbm-tbps")
    tbps, line = hbm_rate(a.hbm_bench) if a.hbm_bench else (a.hbm_tbps, "given on the command line")

    import torch
    import _pkg
    import l1_hop_model as lhm
    m = _pkg.load()
    sps = 4
    ctx = m.TrxSig(sps, 0)
    ctx.use_torch_stream()
    A, F = a.arfcns, a.frames
    T = 8 * F
    fn = 51 * 26 * 5
    comb, group, hsn = production_plan(A)
    hp = m.L1Hop(ctx, comb, group, hsn, max_frames=F)
    sizes = sorted({len(hp.members(g, tn)) for g in range(hp.groups()) for tn in range(8)} - {0})
    # the slots that change rows in this call (the model's map: host work, once)
    radio = lhm.HopModel(comb, group, hsn).map(fn, F)
    moved = int((radio != np.arange(A)).sum())
    hopping = int((group >= 0).sum()) * F
    cache = 256 << 20
    cell = 157 * sps + 4                                     # 632 samples: even, so every cell start is 16-byte aligned
    cells_bytes = sum(lhm.cell_len(t, sps) for t in range(T)) * A * 8
    n_bits = 2 * cache // (A * T * 149) + 1
    n_cells = max(2, 2 * cache // (2 * T * A * cell * 8) + 1)
    grids = [torch.zeros(A, T, 148, dtype=torch.uint8, device="cuda") for _ in range(n_bits)]
    whats = [torch.zeros(A, T, dtype=torch.uint8, device="cuda") for _ in range(n_bits)]
    src = [torch.zeros(T, A, cell, 2, dtype=torch.float32, device="cuda") for _ in range(n_cells)]
    dst = [torch.zeros(T, A, cell, 2, dtype=torch.float32, device="cuda") for _ in range(n_cells)]
    row = torch.arange(T * A, dtype=torch.int32, device="cuda").reshape(T, A)
    res = m.TrxGroupResult(n_slots=T, n_arfcn=A, n_rows=T * A, d_row=row.data_ptr(), d_valid=None, d_flags=None, d_amp=None,
                           d_toa=None, d_avgpwr=None, d_threshold=None, d_soft=None, soft_stride=148)
    turn = [0]

    def bits_call():
        k = turn[0] % n_bits
        turn[0] += 1
        hp.bits(1, fn, F, grids[k], whats[k])

    def cells_call():
        k = turn[0] % n_cells
        turn[0] += 1
        hp.cells(1, fn, F, src[k], A * cell, cell, dst[k], A * cell, cell)

    def result_call():
        hp.result(res, fn)

    def window(fnc):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ts = []
        for _ in range(a.reps):
            ev[0].record()
            for _ in range(a.calls):
                fnc()
            ev[1].record(); torch.cuda.synchronize()
            ts.append(ev[0].elapsed_time(ev[1]) * 1000.0 / a.calls)
        return float(np.median(ts))

    out = dict(arfcns=A, frames=F, slots=A * T, sps=sps, allocation_sizes=sizes, hopping_slots=hopping, moved_slots=moved,
               copies_bits=n_bits, copies_cells=n_cells, hbm_read_tbps=tbps, hbm_bench_line=line, calls_per_window=a.calls,
               windows=a.reps)
    for fnc, key, touched in ((bits_call, "bits", 2 * moved * 149), (result_call, "result", 2 * T * A * 4),
                              (cells_call, "cells", 2 * cells_bytes)):
        for _ in range(3):
            fnc()
        us = window(fnc)
        floor = touched / (tbps * 1e12) * 1e6
        out[key + "_us"] = round(us, 1)
        out[key + "_bytes_at_hbm_rate_us"] = round(floor, 2)
        out[key + "_over_floor"] = round(us / floor, 2)
    out["cells_tbps"] = round(2 * cells_bytes / out["cells_us"] / 1e6, 2)
    out["note"] = ("*_bytes_at_hbm_rate_us: one read and one write of the bytes the call touches over hbm_read_tbps -- bits: the 148 "
                   "+ 1 bytes of every slot that changes rows; result: the [8 F][A] index array; cells: every sample of every cell; "
                   "*_over_floor: the measured median over that; cells_tbps: samples read plus written per second")
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    hp.destroy()
    ctx.close()


if __name__ == "__main__":
    main()
