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
import numpy as np

import mlse_bench_lib as lib

CODED = np.r_[3:42, 106:145]


def sch_batch_torch(synth, sps, B, seed, max_delay_sym=5, chunk=8192):
    """B SCH-shaped bursts on the device (tail, 39 random bits, the extended training sequence, 39 random bits, tail; the library's
    synthetic channel: a gain, a delay of 0..max_delay_sym symbols and a fraction, noise sigma 0 / 0.1 / 0.3 in turn) with an echo
    one symbol late: (x, off, length, bits).  The equaliser does not look at the code, so the coded bits are random."""
    import torch
    from fectxbind import XTS_BITS
    xts = torch.tensor([int(c) for c in XTS_BITS], dtype=torch.uint8, device="cuda:0")

    def fill(bits, rand):
        bits[:, 42:106] = xts
        bits[:, 3:42] = rand(39)
        bits[:, 106:145] = rand(39)
    return lib.echo_bursts_torch(synth, sps, B, seed, fill, max_delay_sym, chunk)


def main():
    a, tbps, line = lib.parse(lib.parser("mlse_sch_bench.json"))

    import torch
    import _pkg
    m = _pkg.load()
    from openbts_ttsou_amd import synth
    sps, B = 4, a.bursts
    ctx = m.TrxSig(sps, 0)
    ctx.use_torch_stream()
    x, off, length, bits = sch_batch_torch(synth, sps, B, seed=3)
    rot = lib.Rotation(a.reps, x)
    xs = rot.xs[0]
    flags, amp, toa, soft, chan, win = lib.one_antenna_buffers(B, 4, 3)
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
    en = det.to(torch.uint8)
    demod = lambda k: ctx.demodulate(xs[k], off, length, amp, toa, soft[0], enable=en)
    sch = lambda k: ctx.mlse_sch(xs[k], off, length, amp, toa, soft[1], enable=en, chan=chan[0], win=win[0])
    normal = lambda k: ctx.mlse(xs[k], off, length, 2, amp, toa, soft[2], enable=en, chan=chan[1], win=win[1])      # (the cost alone: its soft bits mean nothing here)
    access = lambda k: ctx.mlse_access(xs[k], off, length, amp, toa, soft[3], enable=en, chan=chan[2], win=win[2])  # (likewise)
    d_us, q_us, n_us, c_us = rot.timed(demod, sch, normal, access)
    d = det.cpu().numpy()
    err = lib.bit_errors(bits.cpu().numpy(), d, CODED)
    out, floor = lib.one_antenna_head(B, sps, d, rot, tbps, line)
    out.update(**lib.us("demodulate", d_us), **lib.us("mlse_sch", q_us), **lib.us("mlse_normal", n_us), **lib.us("mlse_access", c_us),
               demodulate_over_one_read=round(d_us[0] / floor, 2), mlse_sch_over_one_read=round(q_us[0] / floor, 2),
               mlse_normal_over_one_read=round(n_us[0] / floor, 2), mlse_access_over_one_read=round(c_us[0] / floor, 2),
               mlse_sch_over_demodulate=round(q_us[0] / d_us[0], 2), mlse_sch_over_mlse_normal=round(q_us[0] / n_us[0], 2),
               mlse_sch_over_mlse_access=round(q_us[0] / c_us[0], 2), mlse_sch_ns_per_burst=round(q_us[0] * 1e3 / B, 2),
               windows=lib.window_counts(win[0]),
               coded_bit_errors=dict(demodulate=err(soft[0]), mlse_sch=err(soft[1]), of=int(d.sum()) * len(CODED)),
               note="the batch: synthetic SCH-shaped bursts (GSM 05.02 5.2.5 map, random coded bits; a delay of 0..5 symbols and a fraction; "
                    "sigma 0 / 0.1 / 0.3 in turn) plus an echo one symbol late at 0.54 of the amplitude; amplitude and TOA from "
                    "trxsig_l1acq_detect_sch_batch on the burst's slot, detected bursts only; trxsig_mlse_batch (tsc 2) and "
                    "trxsig_mlse_access_batch run on the same buffers for their cost alone; medians of --reps HIP-event windows, one call "
                    "each, the samples read from a buffer not touched since the rotation came round")
    lib.write(out, a.out)
    ctx.close()


if __name__ == "__main__":
    main()
