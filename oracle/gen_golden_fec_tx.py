#!/usr/bin/env python3
"""Generate tests/golden/fec_tx.npz from the REAL reference (oracle/_ref) -- build container only.

    make -C oracle ref && make -C oracle -f fec_tx.mk ref && python oracle/gen_golden_fec_tx.py

The downlink L1 encode's vectors: TCHFACCHL1Encoder::dispatch streams and SCHL1Encoder::generate bursts, as the
reference's own BitVector / ViterbiR2O4 / Parity code and GSM::Time produce them (oracle/_ref/libref_fec_tx.so) for
seeded inputs.  TEST INFRASTRUCTURE ONLY."""
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import refbind  # noqa: E402
import reffectx  # noqa: E402

OUT = os.path.join(os.path.dirname(HERE), "tests", "golden")


def save(name, **kw):
    path = os.path.join(OUT, name)
    np.savez_compressed(path, **kw)
    print("wrote %s (%.1f KB)" % (name, os.path.getsize(path) / 1024.0))


def gen_fec_tx():
    """Downlink L1 encode from the REAL reference BitVector / ViterbiR2O4 / Parity code and GSM::Time
    (oracle/_ref/libref_fec_tx.so): TCHFACCHL1Encoder::dispatch streams with mixed kinds and SCHL1Encoder::generate bursts.
    The filler c[] and the SCH extended training sequence are read as data from GSM/GSML1FEC.cpp; the training
    sequences are the reference's own (refbind gsm_bits)."""
    r = reffectx.RefFecTx()
    src = open(os.path.join(os.environ.get("REF", "/root/reference"), "GSM", "GSML1FEC.cpp")).read()
    filler = np.array([int(c) for c in re.search(r'static const BitVector fillerC\("([01]+)"\)', src).group(1)], np.uint8)
    xts = np.array([int(c) for c in re.search(r'static const BitVector xts\("([01]+)"\)', src).group(1)], np.uint8)
    tscb = np.array(refbind.Ref(1).gsm_bits()[0], np.uint8)
    rng = np.random.default_rng(20261015)
    S, n = 4, 40
    F, T, X = 2, 1, 0                                     # FACCH, speech, filler
    kind = np.full((S, n), T, np.uint8)
    kind[0, 5:9] = F; kind[0, 9:14] = T; kind[0, 20:24] = X; kind[0, 24] = F; kind[0, 25] = T; kind[0, 26] = F
    kind[1] = rng.integers(0, 3, n)
    kind[2, :12] = X; kind[2, 12:30] = F; kind[2, 30:] = X
    kind[3, ::2] = F
    payload = rng.integers(0, 256, (S, n, 33)).astype(np.uint8)   # padding bits (d[260..263], FACCH octets 23..32) included
    tsc = np.array([0, 3, 5, 7], np.uint8)
    bits = np.stack([r.tch_dispatch(kind[s], payload[s], tscb[tsc[s]], filler) for s in range(S)])
    H = 26 * 51 * 2048
    fns = [0, 1, 11, 21, 31, 41, 50, 51, 52, 1325, 1326, 1327, 26 * 51 * 2047, H // 2, H - 52, H - 51, H - 2, H - 1]
    fns += [51 * k + t for k in (3, 700, 20000) for t in (0, 1, 11, 21, 31, 41, 50)]
    fns += list(rng.integers(0, H, 40))
    fn = np.array(fns, np.uint32)
    bsic = rng.integers(0, 64, len(fn)).astype(np.uint8)
    bsic[:4] = [0, 63, 0, 63]; bsic[-4:] = [63, 0, 63, 0]
    save("fec_tx.npz", filler=filler, xts=xts, tsc_bits=tscb, tch_kind=kind, tch_payload=payload, tch_tsc=tsc,
         tch_split=np.int32(17), tch_bits=bits, sch_fn=fn, sch_bsic=bsic, sch_bits=r.sch_encode(fn, bsic, xts))




if __name__ == "__main__":
    if not (refbind.available() and reffectx.available()):
        sys.exit("oracle/_ref not built: run `make -C oracle ref && make -C oracle -f fec_tx.mk ref` in the build container")
    gen_fec_tx()
