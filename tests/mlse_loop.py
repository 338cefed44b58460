"""The closed loop of tests/test_gpu_mlse_group.py and its model on the CPU: one SDCCH/8 slot at sps 4 (eight SDCCH and their
SACCH, 102 frames), every block sent, each burst through a FIXED tap set of three symbols' spread and no noise, then
analyzeTrafficBurst and either demodulateBurst or the sequence equaliser, then the XCCH decoder.  TEST INFRASTRUCTURE ONLY.

The tap set was chosen on the CPU through this module (air_model, the oracle, tests/mlse_model.py and the FEC oracle): with TAPS
below every burst is detected, the modelled equalising chain decodes every block and the modelled demodulating chain loses
some (the counts are in tests/test_gpu_mlse_group.py's docstring)."""
import numpy as np

import air_model as am
import fecbind
import l1_ms_model as lms
import mlse_model
import oraclebind

SPS, A, F, FN0, BSIC, BAND, TN = 4, 1, 102, 51 * 26 * 3, 21, 1800, 1
GAIN = np.complex64(900.0 - 500.0j)
# taps a symbol apart (the samples between are zeros): three symbols of spread, the strongest path second
TAPS_SYM = np.array([0.55 + 0.2j, -0.3 + 0.75j, 0.45 - 0.1j, -0.2 - 0.35j], np.complex64)


def taps():
    h = np.zeros(3 * SPS + 1, np.complex64)
    h[::SPS] = TAPS_SYM
    return h


def case(tx):
    """The plan, what the handsets send (tests/l1_ms_model.py) and the grids for L1Ms.encode."""
    comb = np.zeros((A, 8), np.uint8)
    comb[0, TN] = 7
    model = lms.MsModel(comb, BSIC, BAND, oracle=tx)
    g = lms.grids(model, lms.Content(np.random.default_rng(515), p_none=0.0), FN0, F)
    m = model.encode(FN0, F, **g)
    return dict(comb=comb, model=model, grids=g, m=m)


def blocks(c):
    """[(channel, block index of the call, payload, [slot of burst 0..3])] for every block whose four bursts lie in the call."""
    model, g = c["model"], c["grids"]
    out = []
    for i, ch in enumerate(model.ch[lms.XCCH]):
        w = model.walk(ch.m, FN0, F)
        b = 0
        for j, (k, B) in enumerate(w):
            if B != 0:
                continue
            if j + 3 < len(w) and g["xcch_kind"][i, b] == 1:
                want = g["xcch_payload"][i, b].copy()
                if ch.sacch:
                    want[0], want[1] = lms.lmm.encode_power(BAND, ch.power) & 31, ch.ta
                out.append((i, b, want, [8 * w[j + q][0] + ch.tn for q in range(4)]))
            b += 1
    return out


def cpu_cells(o, c):
    """{slot: received cell}: the reference's modulator, the gain, the taps (air_model's cell form, no noise)."""
    air = am.AirModel(o)
    m = c["m"]
    h = taps()
    out = {}
    for t in np.flatnonzero(m["what"][0]):
        x = o.scale_vector(o.modulate(m["bits"][0, t].astype(np.int8), 8 + (t % 4 == 0)), GAIN)
        out[int(t)] = air.signal(x, h)
    return out


def cpu_chains(o, c, cells):
    """Both modelled chains on `cells`: dict(detected, blocks, ok_demod [n], ok_mlse [n], frames_mlse, soft_mlse {slot: [148]})."""
    fo = fecbind.FecOracle()
    tsc = BSIC & 7
    blk = blocks(c)
    rows_d, rows_e, det, soft_e = [], [], [], {}
    for _, _, _, slots in blk:
        for s in slots:
            x = cells[s]
            r = o.analyze_traffic(x, tsc)
            det.append(r["ok"])
            if not r["ok"]:
                rows_d.append(np.zeros(148, np.float32)); rows_e.append(np.zeros(148, np.float32))
                continue
            rows_d.append(o.demodulate(x, r["amp"], r["toa"])[:148])
            e = mlse_model.mlse_batch(SPS, x, np.array([0], np.int32), np.array([len(x)], np.int32), tsc, r["amp"], r["toa"], oracle=o)
            rows_e.append(e["soft"][0]); soft_e[s] = e["soft"][0]
    fd, okd = fo.xcch_decode_batch(np.stack(rows_d), wire=True)
    fe, oke = fo.xcch_decode_batch(np.stack(rows_e), wire=True)
    good = lambda fr, ok: np.array([bool(k) and np.array_equal(f, b[2]) for f, k, b in zip(fr, ok, blk)])
    return dict(detected=np.array(det), blocks=blk, ok_demod=good(fd, okd), ok_mlse=good(fe, oke), soft_mlse=soft_e)
