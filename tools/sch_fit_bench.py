"""Time the fit detector for synchronisation bursts at sps 4 on 65,536 SCH-shaped windows (tools/mlse_sch_bench.py's batch):
trxsig_sch_fit_batch (include/trxsig.h) beside trxsig_mlse_sch_batch and trxsig_demodulate_batch on the same buffers with the same
amplitudes and TOAs, all three beside the time ONE read of the batch's samples would take at the sustained HBM rate
tools/hbm_bench.hip reports on the same box (--hbm-bench: the compiled binary, run first in a process of its own; or --hbm-tbps: a
figure measured elsewhere); and trxsig_l1acq_detect_sch_batch as a whole on TRXSIG_SCHDET_VALLEY and on TRXSIG_SCHDET_FIT, each at
its suggested threshold, on both legs.  Medians of repeated HIP-event windows; the sample buffers rotate, together larger than the
memory-side cache, so that every timed call reads its samples from HBM.  Side measurements: nothing is asserted.  Results go to
profiles/sch_fit_bench.json (or --out) and to stdout.

    hipcc --offload-arch=gfx950 -O3 tools/hbm_bench.hip -o hbm_bench
    python tools/sch_fit_bench.py --hbm-bench ./hbm_bench [--bursts 65536] [--reps 30] [--out profiles/sch_fit_bench.json]"""
import numpy as np

import mlse_bench_lib as lib


def main():
    a, tbps, line = lib.parse(lib.parser("sch_fit_bench.json"))

    import torch
    import _pkg
    from mlse_sch_bench import sch_batch_torch
    m = _pkg.load()
    from openbts_ttsou_amd import synth
    sps, B = 4, a.bursts
    ctx = m.TrxSig(sps, 0)
    ctx.use_torch_stream()
    x, off, length, _ = sch_batch_torch(synth, sps, B, seed=3)
    rot = lib.Rotation(a.reps, x)
    xs = rot.xs[0]
    f32 = lambda *shape: torch.zeros(*shape, device="cuda")
    flags = torch.zeros(B, dtype=torch.uint8, device="cuda"); amp = f32(B, 2); toa = f32(B); ptm = f32(B)
    soft = [f32(B, 148) for _ in range(3)]
    chan = f32(B, 5, 2); chan9 = f32(B, 9, 2)
    win = [torch.zeros(B, dtype=torch.int32, device="cuda") for _ in range(2)]
    E, R, q = f32(B), f32(B), f32(B)
    acq = m.L1Acq(ctx, 1, 1024)
    step = 16384                                               # a call takes at most 65,535 windows

    def detect(buf, thresh):
        for s in range(0, B, step):
            e = min(B, s + step)
            acq.detect_sch(buf, off[s:e], length[s:e], flags[s:e], amp[s:e], toa[s:e], soft[0][s:e], ptm=ptm[s:e], detect_thresh=thresh,
                           soft_stride=148)

    # amplitude and TOA of the direct calls: the valley detector's on the burst's slot, detected bursts only (mlse_sch_bench's)
    detect(x, m.ACQ_SCH_THRESH)
    torch.cuda.synchronize()
    det = (flags & m.F_DETECT) != 0
    en = det.to(torch.uint8)
    amp0, toa0 = amp.clone(), toa.clone()
    demod = lambda k: ctx.demodulate(xs[k], off, length, amp0, toa0, soft[1], enable=en)
    sch = lambda k: ctx.mlse_sch(xs[k], off, length, amp0, toa0, soft[2], enable=en, chan=chan, win=win[0])
    fit = lambda k: ctx.sch_fit(xs[k], off, length, amp0, toa0, enable=en, chan9=chan9, win=win[1], E=E, R=R, q=q)
    d_us, s_us, f_us = rot.timed(demod, sch, fit)
    qv = q.cpu().numpy()[det.cpu().numpy()]
    acq_us, detected = {}, {}
    for dname, dcode, thresh in (("valley", m.SCHDET_VALLEY, m.ACQ_SCH_THRESH), ("fit", m.SCHDET_FIT, m.ACQ_SCH_FIT_THRESH)):
        for lname, lcode in (("demod", m.SCHLEG_DEMOD), ("mlse", m.SCHLEG_MLSE)):
            acq.set_sch_detector(dcode); acq.set_sch_leg(lcode)
            for _ in range(2):
                detect(xs[0], thresh)
            torch.cuda.synchronize()
            acq_us[dname + "_" + lname] = rot.window(lambda k: detect(xs[k], thresh))
            detected[dname + "_" + lname] = int(((flags & m.F_DETECT) != 0).sum())
    acq.destroy()
    floor = rot.sample_bytes / (tbps * 1e12) * 1e6
    r1 = lambda v: round(v, 1)
    out = dict(bursts=B, sps=sps, detected_by_the_valley_rule=int(det.sum()), sample_bytes=rot.sample_bytes, sample_buffers_in_rotation=rot.n,
               hbm_read_tbps=tbps, hbm_bench_line=line, one_read_of_the_samples_us=r1(floor),
               **lib.us("sch_fit", f_us), **lib.us("mlse_sch", s_us), **lib.us("demodulate", d_us),
               sch_fit_over_one_read=round(f_us[0] / floor, 2), mlse_sch_over_one_read=round(s_us[0] / floor, 2),
               demodulate_over_one_read=round(d_us[0] / floor, 2), sch_fit_over_demodulate=round(f_us[0] / d_us[0], 2),
               sch_fit_over_mlse_sch=round(f_us[0] / s_us[0], 2), sch_fit_ns_per_burst=round(f_us[0] * 1e3 / B, 2),
               detect_sch_batch_us=dict((k, r1(v[0])) for k, v in acq_us.items()),
               detect_sch_batch_min_max_us=dict((k, [r1(v[1]), r1(v[2])]) for k, v in acq_us.items()),
               detect_sch_batch_detected=detected,
               fit_over_valley=dict(demod=round(acq_us["fit_demod"][0] / acq_us["valley_demod"][0], 3),
                                    mlse=round(acq_us["fit_mlse"][0] / acq_us["valley_mlse"][0], 3)),
               q_on_the_detected=dict(min=float(qv.min()), median=float(np.median(qv)), max=float(qv.max())) if len(qv) else None,
               windows=lib.window_counts(win[1]),
               note="the batch: tools/mlse_sch_bench.py's (synthetic SCH-shaped bursts, a delay of 0..5 symbols and a fraction, sigma 0 / 0.1 / "
                    "0.3 in turn, an echo one symbol late at 0.54 of the amplitude); the direct calls take amplitude and TOA from the valley "
                    "detector, detected bursts only; detect_sch_batch runs in four calls of 16,384 windows, each detector at its suggested "
                    "threshold; medians of --reps HIP-event windows, the samples read from a buffer not touched since the rotation came round")
    lib.write(out, a.out)
    ctx.close()


if __name__ == "__main__":
    main()
