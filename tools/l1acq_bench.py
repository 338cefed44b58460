"""Time mobile-side acquisition (include/trxsig_l1acq.h): trxsig_l1acq_search over 128 streams x 13 frames at sps 4 -- one C0
carrier's downlink (tests/l1_acq_model.py's builder: FCCH / SCH on TN 0, random, dummy and alternating-bit bursts elsewhere) cut in
at 128 different points, each stream with its own frequency offset (|f| <= 0.1 cycle / symbol), gain and noise at 20 dB.

Reported: the per-call median over repeated HIP-event windows of --calls searches each, the calls rotating through --sets copies
of the samples (together larger than the 256 MB memory-side cache, so that every call reads its streams from HBM); the bytes a
call reads (the samples, once) and that figure divided by the sustained HBM read rate tools/hbm_bench.hip reports on the same box
(--hbm-bench: the compiled binary, run first, in a process of its own; or --hbm-tbps: a figure measured elsewhere) -- the time the
search would take if reading the samples once at that rate were all it did.  There is no earlier code to compare with: no
threshold anywhere, the file is the record.  Results go to profiles/l1acq_bench.json (or --out) and to stdout.

    hipcc --offload-arch=gfx950 -O3 tools/hbm_bench.hip -o hbm_bench
    python tools/l1acq_bench.py --hbm-bench ./hbm_bench [--streams 128] [--frames 13] [--sets 6] [--reps 20] [--calls 10]"""
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
    ap.add_argument("--streams", type=int, default=128)
    ap.add_argument("--frames", type=int, default=13)
    ap.add_argument("--sets", type=int, default=6, help="copies of the samples the calls rotate through")
    ap.add_argument("--reps", type=int, default=20, help="timed windows")
    ap.add_argument("--calls", type=int, default=10, help="searches per window (one event pair)")
    ap.add_argument("--hbm-bench", default=None, help="compiled tools/hbm_bench.hip, run before anything else")
    ap.add_argument("--hbm-tbps", type=float, default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "l1acq_bench.json"))
    a = ap.parse_args()
    if (a.hbm_bench is None) == (a.hbm_tbps is None):
        raise SystemExit("give --hbm-bench or --hbm-tbps")
    tbps, line = hbm_rate(a.hbm_bench) if a.hbm_bench else (a.hbm_tbps, "given on the command line")

    import torch
    import _pkg
    import fectxbind
    import l1_acq_model as am
    import oraclebind
    m = _pkg.load()
    sps, S, F, bsic = 4, a.streams, a.frames, 33
    ctx = m.TrxSig(sps, 0)
    ctx.use_torch_stream()
    rng = np.random.default_rng(1)
    o, tx = oraclebind.Oracle(sps), fectxbind.FecTxOracle()
    clean, _ = am.build_stream(o, tx, rng, 51 * 26 * 9, 2 * F, bsic, extra_slots=0)
    N = F * 1250 * sps
    cuts = rng.integers(0, len(clean) - N, S)
    host = np.stack([clean[c:c + N] for c in cuts]).astype(np.complex64)
    gen = torch.Generator(device="cuda").manual_seed(1)
    x = torch.view_as_complex(torch.from_numpy(host.view(np.float32).reshape(S, N, 2)).cuda())
    f = (torch.rand(S, 1, device="cuda", generator=gen) - 0.5) * 0.2
    gain = torch.polar(0.3 + 2.7 * torch.rand(S, 1, device="cuda", generator=gen), 6.2831853 * torch.rand(S, 1, device="cuda", generator=gen))
    n = torch.arange(N, device="cuda", dtype=torch.float64)[None, :]
    x = x * torch.polar(torch.ones(S, N, device="cuda"), (2 * np.pi * f.double() * n / sps).float()) * gain
    sets = []
    for _ in range(a.sets):
        noise = torch.view_as_complex(torch.randn(S, N, 2, device="cuda", generator=gen)) * (gain.abs() * 10 ** (-20 / 20.0) * np.sqrt(0.5))
        sets.append(torch.view_as_real((x + noise).to(torch.complex64)).contiguous())
    acq = m.L1Acq(ctx, S, N)
    for d in sets:                                           # warm up every buffer
        acq.search(d, N, N, S)
    g = acq.collect()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ts, k = [], 0
    for _ in range(a.reps):
        ev[0].record()
        for _ in range(a.calls):
            acq.search(sets[k % a.sets], N, N, S)
            k += 1
        ev[1].record(); torch.cuda.synchronize()
        ts.append(ev[0].elapsed_time(ev[1]) * 1000.0 / a.calls)
    us = float(np.median(ts))
    read = S * N * 8
    out = dict(sps=sps, streams=S, frames=F, samples_per_stream=N, sets=a.sets, set_bytes=read, reps=a.reps, calls_per_window=a.calls,
               l1acq_search_us=round(us, 1), l1acq_search_us_p10_p90=[round(float(np.percentile(ts, 10)), 1), round(float(np.percentile(ts, 90)), 1)],
               bytes_read_per_call=read, hbm_read_tbps=tbps, hbm_bench_line=line,
               read_once_at_hbm_rate_us=round(read / (tbps * 1e12) * 1e6, 1),
               search_over_read_once=round(us / (read / (tbps * 1e12) * 1e6), 2),
               streams_fcch_found=int((g["state"] & 1).astype(bool).sum()), streams_window_inside=int((g["state"] & 2).astype(bool).sum()),
               streams_decoded=int((g["state"] == 15).sum()), streams_bsic_right=int(((g["state"] == 15) & (g["bsic"] == bsic)).sum()),
               note="l1acq_search_us: one trxsig_l1acq_search (FCCH search, pick, SCH detect + demodulate + decode of one window per "
                    "stream); read_once_at_hbm_rate_us: bytes_read_per_call over hbm_read_tbps; a stream whose strongest frequency "
                    "burst has its SCH beyond the 13 frames counts in streams_fcch_found only")
    print(json.dumps(out))
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
