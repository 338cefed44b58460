"""Time the tracking receiver (include/trxsig_l1trk.h) at sps 4: trxsig_l1trk_slice on 128 columns x 104 frames (one phone per
column, every column a C0 column, so the AFC sums run on ten or eleven frames of each), beside the time one read and one write
of every sample would take at the sustained HBM rate tools/hbm_bench.hip reports on the same box (--hbm-bench: the compiled
binary, run first in a process of its own; or --hbm-tbps: a figure measured elsewhere), and trxsig_l1trk_update on a pull-shaped
result with every row valid beside it.  The calls rotate through --copies copies of the streams and of the cells, so that
nothing is served from the memory-side cache (one copy of the streams alone is twice its size).  Medians of repeated HIP-event
windows.  A side measurement: no threshold anywhere.  Results go to profiles/l1trk_bench.json (or --out) and to stdout.

    hipcc --offload-arch=gfx950 -O3 tools/hbm_bench.hip -o hbm_bench
    python tools/l1trk_bench.py --hbm-bench ./hbm_bench [--cols 128] [--frames 104] [--reps 30] [--out profiles/l1trk_bench.json]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cols", type=int, default=128)
    ap.add_argument("--frames", type=int, default=104)
    ap.add_argument("--copies", type=int, default=2)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--hbm-bench", default=None, help="compiled tools/hbm_bench.hip, run before anything else")
    ap.add_argument("--hbm-tbps", type=float, default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "l1trk_bench.json"))
    a = ap.parse_args()
    if (a.hbm_bench is None) == (a.hbm_tbps is None):
        raise SystemExit("give --hbm-bench or --hbm-tbps")
    tbps, line = hbm_rate(a.hbm_bench) if a.hbm_bench else (a.hbm_tbps, "given on the command line")

    import torch
    import _pkg
    m = _pkg.load()
    sps = 4
    ctx = m.TrxSig(sps, 0)
    ctx.use_torch_stream()
    rng = np.random.default_rng(1)
    A, F = a.cols, a.frames
    T, cell, frame = 8 * F, 160 * sps, 1250 * sps
    n = F * frame + 64
    fn = 51 * 26 * 5
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    streams = [torch.randn(A, n, 2, dtype=torch.float32, device="cuda") for _ in range(a.copies)]
    cells = [torch.zeros(T, A, cell, 2, dtype=torch.float32, device="cuda") for _ in range(a.copies)]
    trk = m.L1Trk(ctx, np.arange(A), np.arange(A), F)
    for p in range(A):
        trk.set(p, 1, fn, int(rng.integers(16, 48)), int(rng.integers(0, 1 << 26)), int(rng.integers(0, 1 << 32)))
    # a pull-shaped result: every cell has a row, every row is valid, TOAs inside the gate
    row = dev(np.arange(T * A, dtype=np.int32).reshape(T, A))
    valid = dev(np.full(T * A, m.F_DETECT, np.uint8))
    toa = dev(rng.uniform(-1.0, 1.0, T * A).astype(np.float32))
    res = m.TrxGroupResult(n_slots=T, n_arfcn=A, n_rows=T * A, d_row=row.data_ptr(), d_valid=valid.data_ptr(), d_flags=None, d_amp=None,
                           d_toa=toa.data_ptr(), d_avgpwr=None, d_threshold=None, d_soft=None, soft_stride=148)
    turn = [0]

    def slice_call():
        k = turn[0] % a.copies
        turn[0] += 1
        trk.slice(streams[k], n, 0, n, fn, F, cells[k], A * cell, cell)      # the anchor is F frames ahead again: the same span

    def both():
        slice_call()
        trk.update(res, fn)

    def window(fnc):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ts = []
        for _ in range(a.reps):
            ev[0].record(); fnc(); ev[1].record(); torch.cuda.synchronize()
            ts.append(ev[0].elapsed_time(ev[1]) * 1000.0)
        return float(np.median(ts))

    for _ in range(3):
        slice_call()
    traffic = A * F * frame * 8 * 2
    out = dict(cols=A, frames=F, sps=sps, copies=a.copies, samples=A * F * frame, hbm_read_tbps=tbps, hbm_bench_line=line,
               traffic_at_hbm_rate_us=round(traffic / (tbps * 1e12) * 1e6, 1))
    us = window(slice_call)
    out["slice_us"] = round(us, 1)
    out["slice_gbytes_per_s"] = round(traffic / us / 1e3, 1)
    both()
    both_us = window(both)
    out["slice_update_us"] = round(both_us, 1)
    out["update_us"] = round(both_us - us, 1)
    st = trk.collect()
    out["fcch_frames_per_call"] = int(st["n_fcch"])
    out["status_clear"] = bool((st["status"] == 0).all())
    out["note"] = ("traffic_at_hbm_rate_us: one read and one write of every sample over hbm_read_tbps; update_us: the difference of the "
                   "two medians (a result with a valid row in every cell: %d rows per phone)" % T)
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    trk.destroy()
    ctx.close()


if __name__ == "__main__":
    main()
