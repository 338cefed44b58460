"""Time packet access: the access burst's decoder, and the base-station stage built on it.

Part 1: trxsig_fec_access_decode_batch (k_fec_access_decode) on 65,536 rows per format with the format given and in either-mode
(both trellis passes on every row) beside trxsig_fec_rach_decode_batch on the same rows, and the encoder.  The soft rows are the
encoder's own bursts with noise (sigma 0.2, clipped to [0, 1]).  By step count the 11-bit format would take 45/42 of the 8-bit
format's time and either-mode 87/42.

Part 2: trxsig_l1pacc_detect on the production plan -- 128 ARFCNs x 104 frames, every slot a PDCH, sps 4, one PRACH block marked
per PDCH and 52-multiframe, a handset's burst on every occasion -- beside trxsig_detect_demod_rach_batch called directly on the
same occasion list (the detector and demodulator alone: no list, no decoder, no fold), on both legs.

Both beside the time ONE read of what they touch would take at the sustained HBM rate tools/hbm_bench.hip reports on the same
box (--hbm-bench: the compiled binary, run first in a process of its own; or --hbm-tbps).  Medians of repeated HIP-event
windows; the buffers rotate, together larger than the memory-side cache, so that every timed call reads from HBM.  Side
measurements: nothing is asserted.  Results go to profiles/l1pacc_bench.json (or --out) and to stdout.

    hipcc --offload-arch=gfx950 -O3 tools/hbm_bench.hip -o hbm_bench
    python tools/l1pacc_bench.py --hbm-bench ./hbm_bench [--bursts 65536] [--arfcns 128] [--frames 104] [--reps 30]"""
import numpy as np

import mlse_bench_lib as lib

BSIC = 0x2B


def decoder(a, m, ctx, tbps):
    import torch
    n = a.bursts
    gen = torch.Generator(device="cuda"); gen.manual_seed(6)
    u8 = lambda *shape: torch.zeros(*shape, dtype=torch.uint8, device="cuda")
    bsic = torch.full((n,), BSIC, dtype=torch.uint8, device="cuda")
    bits = u8(n, 148)
    ra, ofmt, tail, ob = torch.zeros(n, dtype=torch.int16, device="cuda"), u8(n), u8(n), u8(n)
    rtail, rb, rra = u8(n), u8(n), u8(n)
    row_bytes, coded_bytes = n * 148 * 4, n * 36 * 4
    res = {}
    for name, f in (("format_8", 0), ("format_11", 1)):
        fmt = torch.full((n,), f, dtype=torch.uint8, device="cuda")
        word = torch.randint(0, 2048 if f else 256, (n,), device="cuda", generator=gen, dtype=torch.int16)
        ctx.access_encode(word, fmt, bsic, bits)
        soft = (bits.to(torch.float32) + 0.2 * torch.randn(n, 148, device="cuda", generator=gen)).clamp_(0, 1)
        rot = lib.Rotation(a.reps, torch.view_as_complex(soft.view(-1, 2)))      # (a float pair counted as one element: the bytes agree)
        assert rot.sample_bytes == row_bytes
        xs = rot.xs[0]
        dec = lambda mode: (lambda k: ctx.access_decode(xs[k].data_ptr(), n, ra, fmt_out=ofmt, tail_ok=tail, bsic_out=ob, wire=True,
                                                        fmt=mode, bsic=BSIC, n_rows=n, soft_stride=148))
        rach = lambda k: ctx.fec_rach_decode(xs[k].data_ptr(), n, rtail, rb, rra, wire=True, soft_stride=148)
        enc = lambda k: ctx.access_encode(word, fmt, bsic, bits)
        own_us, either_us, rach_us, enc_us = rot.timed(dec(f), dec(-1), rach, enc)
        dec(-1)(0)
        torch.cuda.synchronize()
        good = (tail != 0) & (ob == BSIC)
        res[name] = dict(**lib.us("access_decode", own_us), **lib.us("access_decode_either", either_us), **lib.us("rach_decode", rach_us),
                         **lib.us("access_encode", enc_us), decode_over_rach=round(own_us[0] / rach_us[0], 2),
                         either_over_rach=round(either_us[0] / rach_us[0], 2), decode_ns_per_burst=round(own_us[0] * 1e3 / n, 2),
                         either_mode_format_right=int((ofmt == f).sum()), either_mode_ok=int(good.sum()),
                         either_mode_word_right=int((good & (ofmt == f) & (ra == word)).sum()), sample_buffers_in_rotation=rot.n)
        del rot, xs, soft
    return dict(bursts=n, row_bytes=row_bytes, coded_bytes=coded_bytes, one_read_of_the_rows_us=round(row_bytes / (tbps * 1e12) * 1e6, 1),
                one_read_of_the_coded_values_us=round(coded_bytes / (tbps * 1e12) * 1e6, 1), **res,
                format_11_over_format_8=round(res["format_11"]["access_decode_us"] / res["format_8"]["access_decode_us"], 2),
                by_step_count=dict(format_11_over_format_8=round(45 / 42, 2), either_over_format_8=round(87 / 42, 2)),
                note="soft rows = the encoder's bursts plus noise of sigma 0.2, clipped to [0, 1], wire_quantise on; "
                     "trxsig_fec_rach_decode_batch runs on the same rows (for the 11-bit rows it decodes to nonsense: a timing, the work "
                     "does not depend on the values); the rows read from a buffer not touched since the rotation came round")


def stage(a, m, ctx, tbps):
    import torch
    A, F, sps = a.arfcns, a.frames, 4
    comb = np.full((A, 8), m.L1PDCH_COMB, np.uint8)
    ms, bts = m.L1Pacc(ctx, comb, BSIC), m.L1Pacc(ctx, comb, BSIC)
    n, nb = ms.channels(), ms.grid(0, F)
    gen = torch.Generator(device="cuda"); gen.manual_seed(7)
    prach = np.zeros((n, nb), np.uint8)
    prach[:, 3::12] = 1                                       # B3 of every 52-multiframe
    pk = torch.zeros(n, nb, 4, dtype=torch.uint8, device="cuda")
    pk[:, 3::12] = 1
    out = ms.encode(0, F, torch.ones(n, 16, dtype=torch.uint8, device="cuda"),
                    torch.randint(0, 256, (n, 16), device="cuda", generator=gen, dtype=torch.int16), pk,
                    torch.randint(0, 256, (n, nb, 4), device="cuda", generator=gen, dtype=torch.int16), fmt=0)
    T, cell = 8 * F, 160 * sps
    what = m._dev_tensor(ctx, out.d_what, (A, T), "|u1")
    idx = torch.nonzero(what.reshape(-1) != 0).reshape(-1)     # a * T + t of the bursts on the air
    B = idx.numel()
    t_, a_ = idx % T, idx // T
    bits = m._dev_tensor(ctx, out.d_bits, (A * T, 148), "|u1")[idx].contiguous()
    off = ((t_ * A + a_) * cell).to(torch.int32).contiguous()
    length = ((156 + (t_ % 4 == 0).to(torch.int64)) * sps).to(torch.int32).contiguous()
    x = torch.zeros(T * A * cell, 2, dtype=torch.float32, device="cuda")
    ctx.modulate(bits, (8 + (t_ % 4 == 0).to(torch.int64)).to(torch.int32).contiguous(), x, off,
                 gain=torch.full((B,), 1000.0, dtype=torch.float32, device="cuda"))
    x += 50.0 * torch.randn(x.shape, device="cuda", generator=gen)
    rot = lib.Rotation(a.reps, torch.view_as_complex(x))
    xs = rot.xs[0]
    flags = torch.zeros(B, dtype=torch.uint8, device="cuda"); amp = torch.zeros(B, 2, device="cuda"); toa = torch.zeros(B, device="cuda")
    pwr = torch.zeros(B, device="cuda"); soft = torch.zeros(B, 148, device="cuda")
    res = {}
    for name, leg, call in (("demod", m.RACHLEG_DEMOD, ctx.detect_demod_rach), ("mlse", m.RACHLEG_MLSE, ctx.mlse_rach)):
        det = lambda k: bts.detect(xs[k].data_ptr(), A * cell, cell, 0, F, prach=prach, fmt=0, leg=leg)
        alone = lambda k: call(xs[k].data_ptr(), off, length, flags, amp, toa, soft, avgpwr=pwr, detect_thresh=5.0, energy_thresh=-1.0)
        d_us, a_us = rot.timed(det, alone)
        det(0)
        r = bts.collect()
        res[name] = dict(**lib.us("l1pacc_detect", d_us), **lib.us("detector_alone", a_us), detect_over_detector=round(d_us[0] / a_us[0], 2),
                         occasions=int((r["kind"] != 0).sum()), detected=int(r["det"].sum()), ok=int(r["ok"].sum()))
    touched = B * 157 * sps * 8
    o = dict(arfcns=A, frames=F, sps=sps, pdch_slots=n, occasions=B, cell_bytes=rot.sample_bytes, sample_buffers_in_rotation=rot.n,
             occasion_sample_bytes=touched, one_read_of_the_occasions_samples_us=round(touched / (tbps * 1e12) * 1e6, 1), **res,
             note="every occasion (the PTCCH/U frames and B3 of every 52-multiframe on every PDCH) carries an 8-bit burst at amplitude "
                  "1000 over noise of sigma 50; trxsig_l1pacc_detect = the host's occasion list and its upload, the detector and "
                  "demodulator (or equaliser), k_fec_access_decode and k_l1pacc_fold; detector_alone = the same detector call on a "
                  "list already on the device")
    ms.destroy(); bts.destroy()
    return o


def main():
    ap = lib.parser("l1pacc_bench.json")
    ap.add_argument("--arfcns", type=int, default=128)
    ap.add_argument("--frames", type=int, default=104)
    a, tbps, line = lib.parse(ap)
    import _pkg
    m = _pkg.load()
    ctx = m.TrxSig(4, 0)
    ctx.use_torch_stream()
    o = dict(hbm_read_tbps=tbps, hbm_bench_line=line, decoder=decoder(a, m, ctx, tbps), stage=stage(a, m, ctx, tbps),
             note="medians of --reps HIP-event windows")
    lib.write(o, a.out)
    ctx.close()


if __name__ == "__main__":
    main()
