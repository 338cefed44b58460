"""Time the access-burst sequence equaliser (trxsig_mlse_access_batch, include/trxsig.h) at sps 4 on 65,536 access bursts, beside
trxsig_demodulate_batch and trxsig_mlse_batch (the normal-burst equaliser: 2 x 61 trellis steps a burst where this one has 39,
two bursts a wave where this one has four) on the same buffers with the same amplitudes and TOAs, and all three beside the time
ONE read of the batch's samples would take at the sustained HBM rate tools/hbm_bench.hip reports on the same box (--hbm-bench: the
compiled binary, run first in a process of its own; or --hbm-tbps: a figure measured elsewhere).  Medians of repeated HIP-event
windows; the sample buffers rotate, together larger than the memory-side cache, so that every timed call reads its samples from
HBM.  Side measurements: nothing is asserted.  Results go to profiles/mlse_access_bench.json (or --out) and to stdout.

    hipcc --offload-arch=gfx950 -O3 tools/hbm_bench.hip -o hbm_bench
    python tools/mlse_access_bench.py --hbm-bench ./hbm_bench [--bursts 65536] [--reps 30] [--out profiles/mlse_access_bench.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
HEAD = "00111010" "01001011011111111001100110101010001111000"      # GSM 05.02 5.2.7: extended tail and synchronisation sequence


def access_batch_torch(synth, sps, B, seed, max_delay_sym=20, chunk=8192):
    """B access bursts on the device (the library's synthetic channel: a gain, a delay of 0..max_delay_sym symbols and a fraction,
    noise sigma 0 / 0.1 / 0.3 in turn) with an echo one symbol late: (x, off, length, bits)."""
    import torch
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    head = torch.tensor([int(c) for c in HEAD], dtype=torch.uint8, device=dev)
    sig = torch.tensor((0.0, 0.1, 0.3), dtype=torch.float32, device=dev)
    xs, bits_all = [], []
    for s in range(0, B, chunk):
        n = min(chunk, B - s)
        bits = torch.zeros(n, 148, dtype=torch.uint8, device=dev)
        bits[:, :49] = head
        bits[:, 49:85] = torch.randint(0, 2, (n, 36), device=dev, generator=gen, dtype=torch.uint8)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mlse_access_bench.json"))
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
    x, off, length, bits = access_batch_torch(synth, sps, B, seed=3)
    sample_bytes = x.numel() * 8
    n_copies = max(2, (512 << 20) // sample_bytes + 1)
    xs = [x] + [x.clone() for _ in range(n_copies - 1)]
    flags = torch.zeros(B, dtype=torch.uint8, device="cuda"); amp = torch.zeros(B, 2, device="cuda"); toa = torch.zeros(B, device="cuda")
    soft = torch.zeros(B, 148, device="cuda"); soft2 = torch.zeros(B, 148, device="cuda"); soft3 = torch.zeros(B, 148, device="cuda")
    chan = torch.zeros(B, 5, 2, device="cuda"); win = torch.zeros(B, dtype=torch.int32, device="cuda")
    chan3 = torch.zeros(B, 5, 2, device="cuda"); win3 = torch.zeros(B, dtype=torch.int32, device="cuda")
    ctx.detect_demod_rach(x, off, length, flags, amp, toa, soft, energy_thresh=-1.0)
    torch.cuda.synchronize()
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
    demod = lambda buf: ctx.demodulate(buf, off, length, amp, toa, soft, enable=en)
    access = lambda buf: ctx.mlse_access(buf, off, length, amp, toa, soft2, enable=en, chan=chan, win=win)
    normal = lambda buf: ctx.mlse(buf, off, length, 2, amp, toa, soft3, enable=en, chan=chan3, win=win3)      # (the cost alone: its soft bits mean nothing here)
    for _ in range(3):
        demod(xs[0]); access(xs[0]); normal(xs[0])
    torch.cuda.synchronize()
    d_us, q_us, n_us = window(demod), window(access), window(normal)
    w = win.cpu().numpy()
    pay = np.arange(49, 85)
    d = det.cpu().numpy()
    hb = bits.cpu().numpy()
    err = lambda s: int((((s.cpu().numpy() > 0.5) != hb)[d][:, pay]).sum())
    floor = sample_bytes / (tbps * 1e12) * 1e6
    out = dict(bursts=B, sps=sps, detected=int(d.sum()), sample_bytes=sample_bytes, sample_buffers_in_rotation=n_copies,
               hbm_read_tbps=tbps, hbm_bench_line=line, one_read_of_the_samples_us=round(floor, 1),
               demodulate_us=round(d_us[0], 1), demodulate_min_max_us=[round(d_us[1], 1), round(d_us[2], 1)],
               mlse_access_us=round(q_us[0], 1), mlse_access_min_max_us=[round(q_us[1], 1), round(q_us[2], 1)],
               mlse_normal_us=round(n_us[0], 1), mlse_normal_min_max_us=[round(n_us[1], 1), round(n_us[2], 1)],
               demodulate_over_one_read=round(d_us[0] / floor, 2), mlse_access_over_one_read=round(q_us[0] / floor, 2),
               mlse_normal_over_one_read=round(n_us[0] / floor, 2), mlse_access_over_demodulate=round(q_us[0] / d_us[0], 2),
               mlse_access_over_mlse_normal=round(q_us[0] / n_us[0], 2), mlse_access_ns_per_burst=round(q_us[0] * 1e3 / B, 2),
               windows=dict((str(k), int((w == k).sum())) for k in (-4, -3, -2, -1, 0, 1, 2)),
               payload_bit_errors=dict(demodulate=err(soft), mlse_access=err(soft2), of=int(d.sum()) * len(pay)),
               note="the batch: synthetic access bursts (GSM 05.02 5.2.7 head, random coded bits; a delay of 0..20 symbols and a fraction; "
                    "sigma 0 / 0.1 / 0.3 in turn) plus an echo one symbol late at 0.54 of the amplitude; amplitude and TOA from "
                    "trxsig_detect_demod_rach_batch, detected bursts only; trxsig_mlse_batch (tsc 2) runs on the same buffers for its cost "
                    "alone; medians of --reps HIP-event windows, one call each, the samples read from a buffer not touched since the "
                    "rotation came round")
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
