"""Time the sequence equaliser (trxsig_mlse_batch, include/trxsig.h) at sps 4 on 65,536 normal bursts, beside
trxsig_demodulate_batch on the same batch with the same amplitudes and TOAs, and both beside the time ONE read of the batch's samples
would take at the sustained HBM rate tools/hbm_bench.hip reports on the same box (--hbm-bench: the compiled binary, run first in a
process of its own; or --hbm-tbps: a figure measured elsewhere).  Medians of repeated HIP-event windows; the sample buffers
rotate, together larger than the memory-side cache, so that every timed call reads its samples from HBM.  Side measurements:
nothing is asserted.  Results go to profiles/mlse_bench.json (or --out) and to stdout.

    hipcc --offload-arch=gfx950 -O3 tools/hbm_bench.hip -o hbm_bench
    python tools/mlse_bench.py --hbm-bench ./hbm_bench [--bursts 65536] [--reps 30] [--out profiles/mlse_bench.json]"""
import mlse_bench_lib as lib


def main():
    a, tbps, line = lib.parse(lib.parser("mlse_bench.json", tsc=True))

    import torch
    import _pkg
    m = _pkg.load()
    from openbts_ttsou_amd import synth
    sps, B, tsc = 4, a.bursts, a.tsc
    ctx = m.TrxSig(sps, 0)
    ctx.use_torch_stream()
    # the library's synthetic normal bursts, plus an echo one symbol late on every burst: a channel the equaliser has work with
    x, off, length, meta = synth.normal_batch_torch(sps, B, tsc, seed=3)
    x = lib.echoed(x, sps).contiguous()
    rot = lib.Rotation(a.reps, x)
    xs = rot.xs[0]
    flags, amp, toa, (soft, soft2), (chan,), (win,) = lib.one_antenna_buffers(B, 2, 1)
    ctx.detect_demod_normal(x, off, length, tsc, flags, amp, toa, soft, energy_thresh=-1.0)
    torch.cuda.synchronize()
    det = (flags & m.F_DETECT) != 0
    en = det.to(torch.uint8)
    demod = lambda k: ctx.demodulate(xs[k], off, length, amp, toa, soft, enable=en)
    mlse = lambda k: ctx.mlse(xs[k], off, length, tsc, amp, toa, soft2, enable=en, chan=chan, win=win)
    d_us, q_us = rot.timed(demod, mlse)
    d = det.cpu().numpy()
    err = lib.bit_errors(meta["bits"].cpu().numpy(), d, lib.PAYLOAD)
    out, floor = lib.one_antenna_head(B, sps, d, rot, tbps, line, tsc=tsc)
    out.update(**lib.us("demodulate", d_us), **lib.us("mlse", q_us),
               demodulate_over_one_read=round(d_us[0] / floor, 2), mlse_over_one_read=round(q_us[0] / floor, 2),
               mlse_over_demodulate=round(q_us[0] / d_us[0], 2), mlse_ns_per_burst=round(q_us[0] * 1e3 / B, 2),
               windows=lib.window_counts(win),
               payload_bit_errors=dict(demodulate=err(soft), mlse=err(soft2), of=int(d.sum()) * len(lib.PAYLOAD)),
               note="the batch: the library's synthetic normal bursts (sigma 0 / 0.1 / 0.3 in turn) plus an echo one symbol late at "
                    "0.54 of the amplitude; amplitude and TOA from trxsig_detect_demod_normal_batch, detected bursts only; medians of "
                    "--reps HIP-event windows, one call each, the samples read from a buffer not touched since the rotation came round")
    lib.write(out, a.out)
    ctx.close()


if __name__ == "__main__":
    main()
