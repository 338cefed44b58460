"""Time the ciphering stage (include/trxsig_l1ciph.h) on the production plan (128 ARFCNs; C0: combination V on TN 0, VII on
TN 1, I elsewhere; I on every other carrier) over 104 frames with every dedicated channel ciphered: trxsig_l1ciph_bits on a burst
grid and trxsig_l1ciph_soft on a pull-shaped result with a valid row in every slot, downlink (114 output clocks a slot) and uplink
(228), each beside the time one read and one write of the rows it touches (148 bytes, or 148 floats, per ciphered slot) would
take at the sustained HBM rate tools/hbm_bench.hip reports on the same box (--hbm-bench: the compiled binary, run first in a
process of its own; or --hbm-tbps: a figure measured elsewhere).  The calls rotate through copies of the grid and of the rows
whose total is past twice the 256 MiB memory-side cache, so nothing is served from it.  Medians over repeated HIP-event windows
of --calls calls each, per call.
A side measurement: no threshold anywhere.  Results go to profiles/l1ciph_bench.json (or --out) and to stdout.

    hipcc --offload-arch=gfx950 -O3 tools/hbm_bench.hip -o hbm_bench
    python tools/l1ciph_bench.py --hbm-bench ./hbm_bench [--arfcns 128] [--frames 104] [--reps 30] [--calls 10] [--out profiles/l1ciph_bench.json]"""
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
    ap.add_argument("--arfcns", type=int, default=128)
    ap.add_argument("--frames", type=int, default=104)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--calls", type=int, default=10, help="calls per HIP-event window")
    ap.add_argument("--hbm-bench", default=None, help="compiled tools/hbm_bench.hip, run before anything else")
    ap.add_argument("--hbm-tbps", type=float, default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "l1ciph_bench.json"))
    a = ap.parse_args()
    if (a.hbm_bench is None) == (a.hbm_tbps is None):
        raise SystemExit("give --hbm-bench or --hbm-tbps")
    tbps, line = hbm_rate(a.hbm_bench) if a.hbm_bench else (a.hbm_tbps, "given on the command line")

    import torch
    import _pkg
    m = _pkg.load()
    ctx = m.TrxSig(4, 0)
    ctx.use_torch_stream()
    rng = np.random.default_rng(1)
    A, F = a.arfcns, a.frames
    T = 8 * F
    fn = 51 * 26 * 5
    comb = np.ones((A, 8), np.uint8)
    comb[0, 0], comb[0, 1] = 5, 7
    ci = m.L1Ciph(ctx, comb)
    for cls in (m.L1_TCH, m.L1_XCCH):
        for i in range(ci.channels(cls)):
            ci.set(cls, i, m.A5_1, rng.integers(1, 256, 8))
    cache = 256 << 20
    n_bits = 2 * cache // (A * T * 148) + 1
    n_soft = 2 * cache // (A * T * 148 * 4) + 1
    grids = [torch.zeros(A, T, 148, dtype=torch.uint8, device="cuda") for _ in range(n_bits)]
    rows = [torch.zeros(T * A, 148, dtype=torch.float32, device="cuda") for _ in range(n_soft)]
    row = torch.arange(T * A, dtype=torch.int32, device="cuda").reshape(T, A)
    valid = torch.full((T * A,), m.F_DETECT, dtype=torch.uint8, device="cuda")
    results = [m.TrxGroupResult(n_slots=T, n_arfcn=A, n_rows=T * A, d_row=row.data_ptr(), d_valid=valid.data_ptr(), d_flags=None,
                                d_amp=None, d_toa=None, d_avgpwr=None, d_threshold=None, d_soft=r.data_ptr(), soft_stride=148)
               for r in rows]
    # the slots each direction ciphers: the rows one call changes from zero (a keystream of 114 zeros does not happen)
    n_on = []
    for up in (0, 1):
        ci.bits(up, fn, F, grids[0])
        ctx.synchronize()
        n_on.append(int(grids[0].any(dim=2).sum()))
        ci.bits(up, fn, F, grids[0])
    turn = [0]

    def bits_call(up):
        k = turn[0] % n_bits
        turn[0] += 1
        ci.bits(up, fn, F, grids[k])

    def soft_call(up):
        k = turn[0] % n_soft
        turn[0] += 1
        ci.soft(up, results[k], fn)

    def window(fnc, up):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ts = []
        for _ in range(a.reps):
            ev[0].record()
            for _ in range(a.calls):
                fnc(up)
            ev[1].record(); torch.cuda.synchronize()
            ts.append(ev[0].elapsed_time(ev[1]) * 1000.0 / a.calls)
        return float(np.median(ts))

    out = dict(arfcns=A, frames=F, slots=A * T, copies_bits=n_bits, copies_soft=n_soft, hbm_read_tbps=tbps, hbm_bench_line=line,
               calls_per_window=a.calls, windows=a.reps)
    for up, name in ((0, "downlink"), (1, "uplink")):
        out["ciphered_slots_" + name] = n_on[up]
        for fnc, key, width in ((bits_call, "bits", 148), (soft_call, "soft", 148 * 4)):
            for _ in range(3):
                fnc(up)
            us = window(fnc, up)
            floor = 2 * n_on[up] * width / (tbps * 1e12) * 1e6
            out["%s_%s_us" % (key, name)] = round(us, 1)
            out["%s_%s_rows_at_hbm_rate_us" % (key, name)] = round(floor, 1)
            out["%s_%s_over_floor" % (key, name)] = round(us / floor, 2)
    out["bits_uplink_over_downlink"] = round(out["bits_uplink_us"] / out["bits_downlink_us"], 2)
    out["soft_uplink_over_downlink"] = round(out["soft_uplink_us"] / out["soft_downlink_us"], 2)
    out["note"] = ("*_rows_at_hbm_rate_us: one read and one write of the ciphered slots' rows (148 bytes of bits, 148 floats of soft "
                   "values) over hbm_read_tbps; *_over_floor: the measured median over that")
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    ci.destroy()
    ctx.close()


if __name__ == "__main__":
    main()
