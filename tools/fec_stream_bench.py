#!/usr/bin/env python3
"""Side measurement for the uplink stream decoders (trxsig_fec_tch_decode_stream / _xcch_decode_stream): HIP-event time per
call for 1,024 channels x 1 block (one 20-ms tick) and 1,024 x 16 blocks, and beside them, on the same bursts and in the same
process, the batch forms: trxsig_fec_tch_decode_batch without and with the FACCH outputs, and trxsig_fec_xcch_decode_batch.
The batch forms take one channel per call; here they are timed as ONE call over all the bursts back to back (the same number
of blocks, none of the per-channel launches -- the batch form's best case), and, for the 1-block tick, also as the
1,024 per-channel calls a caller would make.  The bursts are encoder output (25 % FACCH blocks for TCH) with soft values
0.1 / 0.9 plus uniform noise.  Prints one JSON line.  Run on the GPU box: python tools/fec_stream_bench.py"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import _pkg

WARM, REPS, K = 50, 7, 100


def timed(fn, k=K, reps=REPS, warm=WARM):
    """Per-call time in microseconds: median and spread over `reps` windows of `k` calls between two HIP events."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    per = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(k):
            fn()
        b.record()
        b.synchronize()
        per.append(a.elapsed_time(b) * 1e3 / k)
    per.sort()
    return dict(us=round(per[len(per) // 2], 2), min=round(per[0], 2), max=round(per[-1], 2), calls=k * reps)


def main():
    pkg = _pkg.load()
    t = pkg.TrxSig(4, 0)
    t.use_torch_stream()
    dev = "cuda"
    g = torch.Generator(device=dev); g.manual_seed(5)
    S, NB = 1024, 16
    T = 4 * NB
    # TCH bursts: S channels x (NB + 1) encoded blocks, the stream's slots are the first T bursts of each channel
    kind = torch.where(torch.rand(S, NB + 1, device=dev, generator=g) < 0.25, pkg.TCH_FACCH, pkg.TCH_SPEECH).to(torch.uint8)
    pl = torch.randint(0, 256, (S, NB + 1, 33), device=dev, generator=g, dtype=torch.uint8)
    bits = torch.zeros(S, NB + 1, 4, 148, dtype=torch.uint8, device=dev)
    t.fec_tch_encode(kind, pl, torch.full((S,), 3, dtype=torch.uint8, device=dev), torch.zeros(S, 32, dtype=torch.uint8, device=dev), bits)

    def soften(b):
        return (b.float() * 0.8 + 0.1 + (torch.rand(b.shape, device=dev, generator=g) - 0.5) * 0.5).clamp(0, 1).contiguous()
    tsoft = soften(bits.view(S, 4 * (NB + 1), 148)[:, :T]).view(S * T, 148)
    frames = torch.randint(0, 256, (S * NB, 23), device=dev, generator=g, dtype=torch.uint8)
    xbits = torch.zeros(S * NB * 4, 148, dtype=torch.uint8, device=dev)
    t.fec_xcch_encode(frames, S * NB, 0, xbits)
    xsoft = soften(xbits)

    out = {}
    for nb in (1, NB):
        Tn = 4 * nb
        index = (torch.arange(S, device=dev, dtype=torch.int32)[:, None] * T + torch.arange(Tn, device=dev, dtype=torch.int32)[None]).contiguous()
        b0 = torch.zeros(S, dtype=torch.uint8, device=dev)
        st_t = torch.zeros(S, pkg.TCH_RX_STATE_BYTES, dtype=torch.uint8, device=dev)
        st_x = torch.zeros(S, pkg.XCCH_RX_STATE_BYTES, dtype=torch.uint8, device=dev)
        status = torch.zeros(S, nb, dtype=torch.uint8, device=dev)
        o33 = torch.zeros(S, nb, 33, dtype=torch.uint8, device=dev); o23 = torch.zeros(S, nb, 23, dtype=torch.uint8, device=dev)
        fer = torch.zeros(S, nb, dtype=torch.float32, device=dev)
        r = dict(channels=S, blocks=nb)
        r["tch_stream"] = timed(lambda: t.fec_tch_decode_stream(tsoft, index, st_t, status, o33, o23, b0=b0, fer=fer))
        r["xcch_stream"] = timed(lambda: t.fec_xcch_decode_stream(xsoft, index, st_x, status, o23, fer=fer))
        # the batch forms over the same number of blocks in one call: S*nb TCH blocks need S*nb*4 + 4 bursts
        nbl = S * nb
        src = tsoft if nb == NB else tsoft.view(S, T, 148)[:, :8].reshape(S * 8, 148)
        tb = torch.cat([src[:4 * nbl], src[:4]]).contiguous()
        bt = torch.zeros(nbl, 33, dtype=torch.uint8, device=dev); bg = torch.zeros(nbl, dtype=torch.uint8, device=dev)
        bs = torch.zeros(nbl, dtype=torch.uint8, device=dev)
        bf = torch.zeros(nbl, 23, dtype=torch.uint8, device=dev); bo = torch.zeros(nbl, dtype=torch.uint8, device=dev)
        nbu = 4 * nbl + 4
        r["tch_batch_one_call"] = timed(lambda: t.fec_tch_decode(tb, nbu, bt, bg, bs))
        r["tch_batch_facch_one_call"] = timed(lambda: t.fec_tch_decode(tb, nbu, bt, bg, bs, facch=bf, facch_ok=bo))
        r["xcch_batch_one_call"] = timed(lambda: t.fec_xcch_decode(xsoft, nbl, bf, bo))
        if nb == 1:
            # what a caller does per tick with the batch form: one call per channel over its last 8 bursts
            chans = tsoft.view(S, T, 148)

            def per_channel():
                for s in range(S):
                    t.fec_tch_decode(chans[s], 8, bt[s:s + 1], bg[s:s + 1], bs[s:s + 1], facch=bf[s:s + 1], facch_ok=bo[s:s + 1])
            r["tch_batch_facch_per_channel_calls"] = timed(per_channel, k=3, reps=5, warm=2)
        r["tch_stream_over_batch_facch"] = round(r["tch_stream"]["us"] / r["tch_batch_facch_one_call"]["us"], 3)
        out["%dx%d" % (S, nb)] = r
    print(json.dumps({"metric": "uplink stream decode, us per call (HIP events, median of %d windows)" % REPS, "unit": "us",
                      "n_gpus": 1, "data": "encoder output, soft 0.1/0.9 + U(-0.25, 0.25), wire quantisation on",
                      "results": out}), flush=True)


if __name__ == "__main__":
    main()
