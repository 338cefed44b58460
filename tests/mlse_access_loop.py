"""The closed loop of tests/test_gpu_mlse_access_group.py and its model on the CPU: one combination-V slot at sps 4 (the RACH of
ARFCN 0's TN 0, 51 frames: 27 access bursts, every one sent with the cell's BSIC and a random RA; nothing on the SDCCH/4), each
burst through a FIXED tap set of three symbols' spread and no noise, then detectRACHBurst and either demodulateBurst or the
access-burst sequence equaliser, then the RACH decoder.  TEST INFRASTRUCTURE ONLY.

The tap set was chosen on the CPU through this module (air_model, the oracle, tests/mlse_access_model.py and the FEC oracle),
starting from tests/mlse_loop.py's, which had to be left: see TAPS_SYM below and the counts in
tests/test_gpu_mlse_access_group.py's docstring."""
import numpy as np

import air_model as am
import fecbind
import l1_ms_model as lms
import mlse_access_model as model
import mlse_loop

SPS, A, F, FN0, BSIC, BAND, TN = 4, 1, 51, 51 * 26 * 3, 21, 1800, 0
GAIN = mlse_loop.GAIN
# taps a symbol apart (the samples between are zeros): three symbols of spread, the strongest path second.  Not tests/mlse_loop.py's:
# with those (and with any scaling of them that the demodulator fails on) detectRACHBurst's peak-to-mean ratio stays below its
# threshold of 5 and no access burst is detected at all; this set came from a seeded random search over magnitudes and phases for
# "every burst detected, the equaliser decodes every RA, the demodulator does not" (the smallest peak-to-mean ratio is 8.3).
TAPS_SYM = np.array([-0.72 + 0.13j, -0.15 + 0.99j, 0.73 + 0.03j, -0.33 - 0.43j], np.complex64)


def taps():
    h = np.zeros(3 * SPS + 1, np.complex64)
    h[::SPS] = TAPS_SYM
    return h


def case(tx):
    """The plan, what the handsets send (tests/l1_ms_model.py) and the grids for L1Ms.encode."""
    comb = np.zeros((A, 8), np.uint8)
    comb[0, TN] = 5
    m = lms.MsModel(comb, BSIC, BAND, oracle=tx)
    g = lms.grids(m, lms.Content(np.random.default_rng(616), p_none=0.0, p_wrong_bsic=0.0), FN0, F)
    g["xcch_kind"][:] = 0                                     # access bursts only
    enc = m.encode(FN0, F, **g)
    walk = m.walk(m.ch[lms.RACH][0].m, FN0, F)
    sent = [(8 * k + TN, int(g["rach_ra"][j])) for j, (k, _) in enumerate(walk) if g["rach_kind"][j] == 1]      # (slot, RA)
    return dict(comb=comb, model=m, grids=g, m=enc, sent=sent)


def cpu_cells(o, c):
    """{slot: received cell}: the reference's modulator, the gain, the taps (air_model's cell form, no noise)."""
    air = am.AirModel(o)
    h = taps()
    out = {}
    for t, _ in c["sent"]:
        x = o.scale_vector(o.modulate(c["m"]["bits"][0, t].astype(np.int8), 8 + (t % 4 == 0)), GAIN)
        out[int(t)] = air.signal(x, h)
    return out


def cpu_chains(o, c, cells):
    """Both modelled chains on `cells`: dict(detected [n], ok_demod [n], ok_mlse [n]) -- ok: the RACH decoder's tail check passes, the
    BSIC is the cell's and the RA is the one sent."""
    fo = fecbind.FecOracle()
    rows_d, rows_e, det = [], [], []
    for s, _ in c["sent"]:
        x = cells[s]
        r = o.detect_rach(x)
        det.append(r["ok"])
        if not r["ok"]:
            rows_d.append(np.zeros(148, np.float32)); rows_e.append(np.zeros(148, np.float32))
            continue
        rows_d.append(o.demodulate(x, r["amp"], r["toa"])[:148])
        rows_e.append(model.access_batch(SPS, x, np.array([0], np.int32), np.array([len(x)], np.int32), r["amp"], r["toa"], oracle=o)["soft"][0])
    ra = np.array([v for _, v in c["sent"]])
    det = np.array(det)
    good = lambda d: det & (d[:, 0] != 0) & (d[:, 1] == BSIC) & (d[:, 2] == ra)
    return dict(detected=det, ok_demod=good(fo.rach_decode_batch(np.stack(rows_d))), ok_mlse=good(fo.rach_decode_batch(np.stack(rows_e))))
