"""Time the synchronisation-burst sequence equaliser (trxsig_mlse_sch_batch, include/trxsig.h) at sps 4 on 65,536 SCH bursts, beside
trxsig_demodulate_batch, trxsig_mlse_batch (the normal-burst equaliser: 2 x 61 trellis steps a burst where this one has 2 x 42) and
trxsig_mlse_access_batch (1 x 39 steps, four bursts a wave where this one has two) on the same buffers with the same amplitudes and
TOAs, and all of them beside the time ONE read of the batch's samples would take at the sustained HBM rate tools/hbm_bench.hip
reports on the same box (--hbm-bench: the compiled binary, run first in a process of its own; or --hbm-tbps: a figure measured
elsewhere).  Medians of repeated HIP-event windows; the sample buffers rotate, together larger than the memory-side cache, so that
every timed call reads its samples from HBM.  Side measurements: nothing is asserted.  Results go to profiles/mlse_sch_bench.json
(or --out) and to stdout.

    hipcc --offload-arch=gfx950 -O3 tools/hbm_bench.hip -o hbm_bench
    python tools/mlse_sch_bench.py --hbm-bench ./hbm_bench [--bursts 65536] [--reps 30] [--out profiles/mlse_sch_bench.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
CODED = np.r_[3:42, 106:145]


def sch_batch_torch(synth, sps, B, seed, max_delay_sym=5, chunk=8192):
    """B SCH-shaped bursts on the device (tail, 39 random bits, the extended training sequence, 39 random bits, tail; the library's
    synthetic channel: a gain, a delay of 0..max_delay_sym symbols and a fraction, noise sigma 0 / 0.1 / 0.3 in turn) with an echo
    one symbol late: (x, off, length, bits).  The equaliser does not look at the code, so the coded bits are random."""
    import torch
    from fectxbind import XTS_BITS
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    xts = torch.tensor([int(c) for c in XTS_BITS], dtype=torch.uint8, device=dev)
    sig = torch.tensor((0.0, 0.1, 0.3), dtype=torch.float32, device=dev)
    xs, bits_all = [], []
    for s in range(0, B, chunk):
        n = min(chunk, B - s)
        bits = torch.zeros(n, 148, dtype=torch.uint8, device=dev)
        bits[:, 42:106] = xts
        bits[:, 3:42] = torch.randint(0, 2, (n, 39), device=dev, generator=gen, dtype=torch.uint8)
        bits[:, 106:145] = torch.randint(0, 2, (n, 39), device=dev, generator=gen, dtype=torch.uint8)
        amp = torch.polar(300 + 2700 * torch.rand(n, device=dev, generator=gen), 2 * np.pi * torch.rand(n, device=dev, generator=gen))
        delay = (torch.randint(0, max_delay_sym + 1, (n,), device=dev, generator=gen) * sps).to(torch.float32) + \
            torch.rand(n, device=dev, generator=gen)
        x, _, _ = synth._torch_batch(bits, sps, delay, amp, sig[(torch.arange(n, device=dev) + s) % 3], dev, gen)
        xs.append(x); bits_all.append(bits)
    _, length, off = synth.burst_lengths(B, sps)
    x = torch.cat(xs)
    echo = torch.zeros_like(x)
    echo[sps:] = x[:-sps] * complex(0.45, -0.3)
    return (x + echo).contiguous(), torch.from_numpy(off.astype(np.int32)).to(dev), torch.from_numpy(length).to(dev), torch.cat(bits_all)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bursts", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--hbm-bench", default=None, help="compiled tools/hbm_bench.hip, run before anything else")
    ap.add_argument("--hbm-tbps", type=float, default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mlse_sch_bench.json"))
    a = ap.parse_args()
    if (a.hbm_bench is None) == (a.hbm_tbps is None):
        raise SystemExit("give --hbm-bench or --hbm-tbps")
    from air_bench import hbm_rate
    tbps, line = hbm_rate(a.hbm_bench) if a.hbm_bench else (a.hbm_tbps, "given on the command line")

    import torch
    import _pkg
    m = _pkg.load()
    from openbts_ttsou_amd import synth
    sps, B = 4, a.bursts
    ctx = m.TrxSig(sps, 0)
    ctx.use_torch_stream()
    x, off, length, bits = sch_batch_torch(synth, sps, B, seed=3)
    sample_bytes = x.numel() * 8
    n_copies = max(2, (512 << 20) // sample_bytes + 1)
    xs = [x] + [x.clone() for _ in range(n_copies - 1)]
    flags = torch.zeros(B, dtype=torch.uint8, device="cuda"); amp = torch.zeros(B, 2, device="cuda"); toa = torch.zeros(B, device="cuda")
    soft = [torch.zeros(B, 148, device="cuda") for _ in range(4)]
    chan = [torch.zeros(B, 5, 2, device="cuda") for _ in range(3)]; win = [torch.zeros(B, dtype=torch.int32, device="cuda") for _ in range(3)]
    # amplitude and TOA from acquisition's own SCH detector on the burst's slot (its TOA is relative to the slot's start, which is
    # the offset the demodulator and the equalisers are given); a call takes at most 65,535 windows
    acq = m.L1Acq(ctx, 1, 1024)
    step = 16384
    for s in range(0, B, step):
        e = min(B, s + step)
        acq.detect_sch(x, off[s:e], length[s:e], flags[s:e], amp[s:e], toa[s:e], soft[0][s:e], soft_stride=148)
    torch.cuda.synchronize()
    acq.destroy()
    det = (flags & m.F_DETECT) != 0
    turn = [0]

    def window(fnc):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ts = []
        for _ in range(a.reps):
            turn[0] += 1
            ev[0].record(); fnc(xs[turn[0] % n_copies]); ev[1].record(); torch.cuda.synchronize()
            ts.append(ev[0].elapsed_time(ev[1]) * 1000.0)
        return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))

    en = det.to(torch.uint8)
    demod = lambda buf: ctx.demodulate(buf, off, length, amp, toa, soft[0], enable=en)
    sch = lambda buf: ctx.mlse_sch(buf, off, length, amp, toa, soft[1], enable=en, chan=chan[0], win=win[0])
    normal = lambda buf: ctx.mlse(buf, off, length, 2, amp, toa, soft[2], enable=en, chan=chan[1], win=win[1])      # (the cost alone: its soft bits mean nothing here)
    access = lambda buf: ctx.mlse_access(buf, off, length, amp, toa, soft[3], enable=en, chan=chan[2], win=win[2])  # (likewise)
    for _ in range(3):
        demod(xs[0]); sch(xs[0]); normal(xs[0]); access(xs[0])
    torch.cuda.synchronize()
    d_us, q_us, n_us, c_us = window(demod), window(sch), window(normal), window(access)
    w = win[0].cpu().numpy()
    d = det.cpu().numpy()
    hb = bits.cpu().numpy()
    err = lambda s: int((((s.cpu().numpy() > 0.5) != hb)[d][:, CODED]).sum())
    floor = sample_bytes / (tbps * 1e12) * 1e6
    r1 = lambda v: round(v, 1)
    out = dict(bursts=B, sps=sps, detected=int(d.sum()), sample_bytes=sample_bytes, sample_buffers_in_rotation=n_copies,
               hbm_read_tbps=tbps, hbm_bench_line=line, one_read_of_the_samples_us=r1(floor),
               demodulate_us=r1(d_us[0]), demodulate_min_max_us=[r1(d_us[1]), r1(d_us[2])],
               mlse_sch_us=r1(q_us[0]), mlse_sch_min_max_us=[r1(q_us[1]), r1(q_us[2])],
               mlse_normal_us=r1(n_us[0]), mlse_normal_min_max_us=[r1(n_us[1]), r1(n_us[2])],
               mlse_access_us=r1(c_us[0]), mlse_access_min_max_us=[r1(c_us[1]), r1(c_us[2])],
               demodulate_over_one_read=round(d_us[0] / floor, 2), mlse_sch_over_one_read=round(q_us[0] / floor, 2),
               mlse_normal_over_one_read=round(n_us[0] / floor, 2), mlse_access_over_one_read=round(c_us[0] / floor, 2),
               mlse_sch_over_demodulate=round(q_us[0] / d_us[0], 2), mlse_sch_over_mlse_normal=round(q_us[0] / n_us[0], 2),
               mlse_sch_over_mlse_access=round(q_us[0] / c_us[0], 2), mlse_sch_ns_per_burst=round(q_us[0] * 1e3 / B, 2),
               windows=dict((str(k), int((w == k).sum())) for k in (-4, -3, -2, -1, 0, 1, 2)),
               coded_bit_errors=dict(demodulate=err(soft[0]), mlse_sch=err(soft[1]), of=int(d.sum()) * len(CODED)),
               note="the batch: synthetic SCH-shaped bursts (GSM 05.02 5.2.5 map, random coded bits; a delay of 0..5 symbols and a fraction; "
                    "sigma 0 / 0.1 / 0.3 in turn) plus an echo one symbol late at 0.54 of the amplitude; amplitude and TOA from "
                    "trxsig_l1acq_detect_sch_batch on the burst's slot, detected bursts only; trxsig_mlse_batch (tsc 2) and "
                    "trxsig_mlse_access_batch run on the same buffers for their cost alone; medians of --reps HIP-event windows, one call "
                    "each, the samples read from a buffer not touched since the rotation came round")
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
