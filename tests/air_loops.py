"""The cases of the two loops through the air that tests/test_air_model.py checks on the CPU (air_model + the reference's
detectors) and tests/test_gpu_air.py runs on the device: one seeded downlink cell with eight handsets listening to its C0, and
the truth bounds both apply.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

import air_model as am
import l1_mux_model as lmm
import test_l1_msrx_model as tm

HYPER = am.HYPER
F32 = np.float32
# the bounds tests/test_gpu_l1acq.py applies to its 20 dB streams, restated: the SCH start within 0.25 sample, the offset within
# 2e-3 cycle / symbol
MAX_TIMING, MAX_OFFSET = 0.25, 2e-3


def downlink_case(sps, tx):
    """l1tx's model on tm.PLAN over 66 frames (random payloads, SIs set), and eight handsets on C0: a random cut inside the first
    51-multiframe, a delay in [0, 1) sample, an offset within +-0.02 cycle / symbol, a gain of 0.3 to 3 at any angle, 20 dB.
    A cut is drawn again while the 12 frames and two slots the handset searches would hold a frequency burst whose
    synchronisation burst they do not hold (the search takes the strongest frequency burst and would rightly stop at state 1)."""
    rng = np.random.default_rng(4100 + sps)
    bsic, band, fn0, F, H = 45, 900, 51 * 26 * 17 + 40, 66, 8
    mux, enc, grids = tm.encode_cell(rng, tx, fn0, F, bsic, band)
    T = 8 * F
    starts = np.concatenate([[0], np.cumsum([am.cell_len(t, sps) for t in range(T)])])
    fcch = [int(starts[t]) for t in range(T) if enc["what"][0, t] == lmm.W_FCCH]
    sch = [((fn0 + t // 8) % HYPER, int(starts[t])) for t in range(T) if enc["what"][0, t] == lmm.W_SCH]
    n = 12 * 1250 * sps + 313 * sps

    def orphan(c):
        return any(c - 48 * sps <= p and p + 100 * sps <= c + n < p + (1250 + 172) * sps for p in fcch)
    cut = []
    while len(cut) < H:
        c = int(rng.integers(0, 51 * 1250 * sps))
        if not orphan(c):
            cut.append(c)
    f = rng.uniform(-0.02, 0.02, H)
    step = np.round(f / sps * 2.0 ** 32).astype(np.int64) & 0xffffffff
    gain = (rng.uniform(0.3, 3.0, H) * np.exp(2j * np.pi * rng.uniform(size=H))).astype(np.complex64)
    return dict(sps=sps, bsic=bsic, band=band, fn0=fn0, F=F, H=H, mux=mux, enc=enc, grids=grids, sch=sch, n=n, cut=cut,
                delay=rng.uniform(0, 1, H).astype(F32), step=step, f=np.where(step >= 2 ** 31, step - 2.0 ** 32, step) / 2.0 ** 32 * sps,
                phase=rng.integers(0, 1 << 32, H), gain=gain, sigma=(np.abs(gain) * 10.0 ** (-20.0 / 20.0) / np.sqrt(2.0)).astype(F32),
                n0=rng.integers(0, 1 << 32, H), seed=0x5eed0000 + sps)


def modulated_cells(o, enc):
    """the encode's bursts through the reference's modulator: [a][t] complex64, empty slots zeros"""
    A, T = enc["what"].shape
    return [[o.modulate(enc["bits"][a, t].astype(np.int8), 8 + (t % 4 == 0)) if enc["what"][a, t]
             else np.zeros(am.cell_len(t, o.sps), np.complex64) for t in range(T)] for a in range(A)]


def check_handset(case, h, state, bsic, rfn, at, f_est):
    """the truth conditions for one handset: state 15, the true BSIC and FN, where the SCH burst starts, the offset.  `at`: the
    stream sample reported as bit 0 of TN 0 of frame rfn; f_est in cycles / symbol.  -> (timing error, offset error)"""
    assert state == 15, (h, state)
    place = lambda p: p - case["cut"][h] + float(case["delay"][h])
    fn, p = min(case["sch"], key=lambda s: abs(place(s[1]) - at))
    assert (bsic, rfn) == (case["bsic"], fn), (h, bsic, rfn, fn)
    return abs(at - place(p)), abs(f_est - case["f"][h])


# ---- the uplink loop ----------------------------------------------------------------------------------------------------------
UPLINK_SNR_DB = 30.0
UPLINK_STEP = int(round(1e-4 * 2.0 ** 32))                     # 1e-4 turn per sample


def uplink_case(tx):
    """The small plan of tests/test_gpu_l1ms.py's closed loop (sps 4, 2 ARFCNs, 208 frames) through its model: the handsets'
    bursts, per-channel path gains of 300 to 3000 at any angle and delays within half a sample of the handset's TA, and per cell
    what the air applies: noise UPLINK_SNR_DB below the burst (sigma = |A| 10^(-SNR / 20) / sqrt 2; in empty cells the level of
    the weakest burst), a step of 1e-4 turn per sample and a random start phase."""
    import l1_ms_model as lms
    sps, A, F, fn0, bsic, band = 4, 2, 208, 26 * 40, 21, 1800
    rng = np.random.default_rng(9100)
    comb = np.zeros((A, 8), np.uint8)
    comb[0, :3] = [5, 1, 7]; comb[0, 4] = 1; comb[1, :2] = [1, 7]
    model = lms.MsModel(comb, bsic, band, oracle=tx)
    sacch = [i for i, c in enumerate(model.ch[lms.XCCH]) if c.sacch]
    phy = [(i, int(rng.integers(0, 41)), int(rng.integers(0, 64))) for i in sacch[::2]]
    for i, p, t in phy:
        model.set_phy(i, p, t)
    grids = lms.grids(model, lms.Content(rng, p_none=0.1, speech=True), fn0, F)
    m = model.encode(fn0, F, **grids)
    n = [len(model.ch[lms.TCH]), len(model.ch[lms.XCCH]), len(grids["rach_kind"])]
    gain = [(rng.uniform(300.0, 3000.0, k) * np.exp(2j * np.pi * rng.uniform(size=k))).astype(np.complex64) for k in n]
    delay = [(rng.uniform(-0.5, 0.5, k) / sps).astype(F32) for k in n]
    for cls in (lms.TCH, lms.XCCH):
        delay[cls] = (delay[cls] + np.array([ch.handset.ta for ch in model.ch[cls]], F32)).astype(F32)
    T = 8 * F
    amp = np.zeros((A, T), F32)                                # |A| of the cell's burst; 0: empty
    for a in range(A):
        for t in range(T):
            w = int(m["what"][a, t])
            if w:
                amp[a, t] = abs(gain[w - 1][int(m["who"][a, t])])
    scale = F32(10.0 ** (-UPLINK_SNR_DB / 20.0) / np.sqrt(2.0))
    sigma = np.where(amp > 0, amp, amp[amp > 0].min()).astype(F32) * scale
    return dict(sps=sps, A=A, F=F, T=T, fn0=fn0, bsic=bsic, band=band, comb=comb, model=model, phy=phy, grids=grids, m=m, gain=gain,
                delay=delay, sigma=sigma, step=np.full((A, T), UPLINK_STEP, np.uint32), phase=rng.integers(0, 1 << 32, (A, T)),
                seed=0xa1b2c3d4e5)


def uplink_cells(o, case):
    """trxsig_l1ms_radiate of the case through the reference's primitives, amp_of_power all ones: [a][t] complex64"""
    import l1_ms_model as lms
    m, model, sps = case["m"], case["model"], case["sps"]
    out = []
    for a in range(case["A"]):
        out.append([])
        for t in range(case["T"]):
            w, who = int(m["what"][a, t]), int(m["who"][a, t])
            if not w:
                out[-1].append(np.zeros(am.cell_len(t, sps), np.complex64))
                continue
            g = case["gain"][w - 1][who]
            if w == lms.W_ACCESS:
                d = F32(case["delay"][2][who] * F32(sps))
            else:
                d = F32(F32(case["delay"][w - 1][who] - F32(model.ch[w - 1][who].handset.ta)) * F32(sps))
            x = o.modulate(m["bits"][a, t].astype(np.int8), 8 + (t % 4 == 0))
            out[-1].append(o.scale_vector(o.delay_vector(x, d), g))
    return out
