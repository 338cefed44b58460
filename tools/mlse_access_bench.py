"""Time the access-burst sequence equaliser (trxsig_mlse_access_batch, include/trxsig.h) at sps 4 on 65,536 access bursts, beside
trxsig_demodulate_batch and trxsig_mlse_batch (the normal-burst equaliser: 2 x 61 trellis steps a burst where this one has 39,
two bursts a wave where this one has four) on the same buffers with the same amplitudes and TOAs, and all three beside the time
ONE read of the batch's samples would take at the sustained HBM rate tools/hbm_bench.hip reports on the same box (--hbm-bench: the
compiled binary, run first in a process of its own; or --hbm-tbps: a figure measured elsewhere).  Medians of repeated HIP-event
windows; the sample buffers rotate, together larger than the memory-side cache, so that every timed call reads its samples from
HBM.  Side measurements: nothing is asserted.  Results go to profiles/mlse_access_bench.json (or --out) and to stdout.

    hipcc --offload-arch=gfx950 -O3 tools/hbm_bench.hip -o hbm_bench
    python tools/mlse_access_bench.py --hbm-bench ./hbm_bench [--bursts 65536] [--reps 30] [--out profiles/mlse_access_bench.json]"""
import numpy as np

import mlse_bench_lib as lib

HEAD = "00111010" "01001011011111111001100110101010001111000"      # GSM 05.02 5.2.7: extended tail and synchronisation sequence


def access_batch_torch(synth, sps, B, seed, max_delay_sym=20, chunk=8192):
    """B access bursts on the device (the library's synthetic channel: a gain, a delay of 0..max_delay_sym symbols and a fraction,
    noise sigma 0 / 0.1 / 0.3 in turn) with an echo one symbol late: (x, off, length, bits)."""
    import torch
    head = torch.tensor([int(c) for c in HEAD], dtype=torch.uint8, device="cuda:0")

    def fill(bits, rand):
        bits[:, :49] = head
        bits[:, 49:85] = rand(36)
    return lib.echo_bursts_torch(synth, sps, B, seed, fill, max_delay_sym, chunk)


def main():
    a, tbps, line = lib.parse(lib.parser("mlse_access_bench.json"))

    import torch
    import _pkg
    m = _pkg.load()
    from openbts_ttsou_amd import synth
    sps, B = 4, a.bursts
    ctx = m.TrxSig(sps, 0)
    ctx.use_torch_stream()
    x, off, length, bits = access_batch_torch(synth, sps, B, seed=3)
    rot = lib.Rotation(a.reps, x)
    xs = rot.xs[0]
    flags, amp, toa, (soft, soft2, soft3), (chan, chan3), (win, win3) = lib.one_antenna_buffers(B, 3, 2)
    ctx.detect_demod_rach(x, off, length, flags, amp, toa, soft, energy_thresh=-1.0)
    torch.cuda.synchronize()
    det = (flags & m.F_DETECT) != 0
    en = det.to(torch.uint8)
    demod = lambda k: ctx.demodulate(xs[k], off, length, amp, toa, soft, enable=en)
    access = lambda k: ctx.mlse_access(xs[k], off, length, amp, toa, soft2, enable=en, chan=chan, win=win)
    normal = lambda k: ctx.mlse(xs[k], off, length, 2, amp, toa, soft3, enable=en, chan=chan3, win=win3)      # (the cost alone: its soft bits mean nothing here)
    d_us, q_us, n_us = rot.timed(demod, access, normal)
    pay = np.arange(49, 85)
    d = det.cpu().numpy()
    err = lib.bit_errors(bits.cpu().numpy(), d, pay)
    out, floor = lib.one_antenna_head(B, sps, d, rot, tbps, line)
    out.update(**lib.us("demodulate", d_us), **lib.us("mlse_access", q_us), **lib.us("mlse_normal", n_us),
               demodulate_over_one_read=round(d_us[0] / floor, 2), mlse_access_over_one_read=round(q_us[0] / floor, 2),
               mlse_normal_over_one_read=round(n_us[0] / floor, 2), mlse_access_over_demodulate=round(q_us[0] / d_us[0], 2),
               mlse_access_over_mlse_normal=round(q_us[0] / n_us[0], 2), mlse_access_ns_per_burst=round(q_us[0] * 1e3 / B, 2),
               windows=lib.window_counts(win),
               payload_bit_errors=dict(demodulate=err(soft), mlse_access=err(soft2), of=int(d.sum()) * len(pay)),
               note="the batch: synthetic access bursts (GSM 05.02 5.2.7 head, random coded bits; a delay of 0..20 symbols and a fraction; "
                    "sigma 0 / 0.1 / 0.3 in turn) plus an echo one symbol late at 0.54 of the amplitude; amplitude and TOA from "
                    "trxsig_detect_demod_rach_batch, detected bursts only; trxsig_mlse_batch (tsc 2) runs on the same buffers for its cost "
                    "alone; medians of --reps HIP-event windows, one call each, the samples read from a buffer not touched since the "
                    "rotation came round")
    lib.write(out, a.out)
    ctx.close()


if __name__ == "__main__":
    main()
