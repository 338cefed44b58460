"""The tracking receiver's model (tests/l1_trk_model.py) on its own -- no GPU: the integer rules of include/trxsig_l1trk.h on
hand-made cases, a split equal to a whole, the TOA convention the timing loop is built on (pinned against the oracle's
analyzeTrafficBurst), and the closed loop of tests/test_gpu_l1trk.py with the reference's detectors in the device's place, held
to the same truth bounds: the case is within reach of the reference's own arithmetic."""
import numpy as np
import pytest

import air_model as am
import l1_trk_model as ltm
import oraclebind

HYPER = ltm.HYPER


@pytest.fixture(scope="module")
def o4():
    return oraclebind.Oracle(4)


def test_vector_expj_is_the_oracles(o4):
    rng = np.random.default_rng(1)
    top = np.concatenate([[0, 1, (1 << 24) - 1, 1 << 23, 1 << 22, 3 << 22, 16384, 16383], rng.integers(0, 1 << 24, 4000)])
    want = np.array([o4.expjLookup(np.float32(v) * np.float32(2.0 ** -24) * am.TWO_PI_F) for v in top], np.complex64)
    assert np.array_equal(ltm.expj_many(o4, top).view(np.uint32), want.view(np.uint32))


def test_timing_rule_by_hand():
    adj = ltm.timing_adj
    # S sps / (256 N) samples rounded half up, by floor division: sps 4, one row of q = 64 (a quarter symbol) is one sample
    assert adj(64, 1, 4) == 1 and adj(63, 1, 4) == 1 and adj(32, 1, 4) == 1 and adj(31, 1, 4) == 0
    # the tie at exactly half a sample goes up on both sides of zero: +0.5 -> 1, -0.5 -> 0, -1.5 -> -1
    assert adj(32, 1, 4) == 1 and adj(-32, 1, 4) == 0 and adj(-96, 1, 4) == -1 and adj(-97, 1, 4) == -2
    # negative S with floor division (a truncating division would give 0 and -1 here)
    assert adj(-33, 1, 4) == -1 and adj(-3 * 64 - 40, 3, 4) == -1 and adj(-1000, 7, 1) == -1 and adj(-100, 7, 1) == 0
    assert adj(256 * 5, 1, 1) == 5 and adj(128, 1, 1) == 1 and adj(127, 1, 1) == 0 and adj(255 * 9, 9, 2) == 2
    # q: round half to even of toa 256 / sps, exact
    q = ltm.quantise_toa
    assert q(0.5, 4) == 32 and q(1.0 / 128, 4) == 0 and q(3.0 / 128, 4) == 2 and q(-1.0 / 128, 4) == 0 and q(-0.2578125, 1) == -66


def model(o, **kw):
    return ltm.TrkModel(o, [0, 0, 1], [0, 2], **kw)


def result(rows):
    """rows: list of (t, c, valid, toa) -> (row[T][3], valid, toa) with T = 16"""
    row = np.full((16, 3), -1, np.int32)
    valid, toa = [], []
    for i, (t, c, v, d) in enumerate(rows):
        row[t, c] = i
        valid.append(v); toa.append(d)
    return row, np.array(valid, np.uint8), np.array(toa, np.float32)


def sliced(m, fn, step=(0, 0)):
    for p in range(2):
        m.set(p, 1, fn, 5000, step[p], 7)
    m.slice(np.zeros((3, 64), np.complex64), 0, fn, 2)


def test_update_rules_by_hand(o4):
    sps, fn = 4, 51 * 7 + 3                                    # no FCCH / SCH frame in the call
    m = model(o4, toa_gate=128)
    sliced(m, fn, step=(0x01000000, 3))
    pos = list(m.pos)
    # the gate at equality: |q| = 128 is in, 129 is out; invalid rows, rows without a burst and a NaN TOA are out
    d = m.update(*result([(1, 0, 1, 2.0), (2, 1, 1, -129.0 / 64), (3, 0, 0, 0.25), (4, 1, 1, np.nan), (9, 2, 1, -0.5)]), fn)
    assert d[0] == dict(S=128, N=1, adj=2, K=0, delta=0) and d[1] == dict(S=-32, N=1, adj=0, K=0, delta=0)
    assert m.pos == [pos[0] + 2, pos[1]] and m.quiet == [0, 0]
    assert m.phase[0] == (7 + 10000 * 0x01000000 + 2 * 0x01000000) & ltm.M32   # the slice's advance, then adj * step
    # N = 0: nothing moves, quiet counts; d_use masks rows; a negative adj moves the phase back
    sliced(m, fn, step=(5, 0xfffffff0))
    use = np.ones((16, 3), np.uint8); use[1, 0] = 0
    d = m.update(*result([(1, 0, 1, 1.0), (9, 2, 1, -1.5)]), fn, use)
    assert d[0]["N"] == 0 and d[0]["adj"] == 0 and d[1] == dict(S=-96, N=1, adj=-1, K=0, delta=0)
    assert m.quiet == [1, 0] and m.pos[0] == 5000 + 10000 and m.pos[1] == 5000 + 10000 - 1
    assert m.phase[1] == (7 + 10000 * 0xfffffff0 - 0xfffffff0) & ltm.M32
    sliced(m, fn)
    m.quiet = [4, 0]
    m.update(*result([]), fn)
    assert m.quiet == [5, 1]
    # an unlocked phone is left alone
    sliced(m, fn)
    m.locked[1] = 0
    before = (m.pos[1], m.phase[1], m.step[1], m.quiet[1])
    d = m.update(*result([(9, 2, 1, 0.5)]), fn)
    assert d[1]["N"] == 0 and (m.pos[1], m.phase[1], m.step[1], m.quiet[1]) == before


def test_excluded_fcch_and_sch_slots(o4):
    # frames 51 k + 10 (FCCH) and + 11 (SCH): TN 0 of the C0 column is out, TN 0 of the phone's other column and TN 1 are in
    fn = 51 * 40 + 10
    m = model(o4)
    sliced(m, fn)
    d = m.update(*result([(0, 0, 1, 1.0), (8, 0, 1, 1.0), (0, 1, 1, 0.25), (1, 0, 1, 0.5), (9, 0, 1, 0.5), (0, 2, 1, 1.0), (8, 2, 1, 1.0)]), fn)
    assert d[0]["N"] == 3 and d[0]["S"] == 16 + 32 + 32 and d[1]["N"] == 0
    assert [ltm.timing_excluded(51 * 3 + k, 0, True) for k in (0, 1, 2, 9, 10, 11, 12, 40, 41, 42, 50)] == \
        [True, True, False, False, True, True, False, True, True, False, False]
    assert not ltm.timing_excluded(51 * 3, 0, False) and not ltm.timing_excluded(51 * 3, 1, True) and ltm.timing_excluded(51 * 3 - 1, 8, True)


def test_hyperframe_wrap_in_the_distance(o4):
    assert ltm.distance(HYPER - 2, 3) == 5 and ltm.distance(3, HYPER - 2) == -5 and ltm.distance(0, HYPER // 2) == -HYPER // 2
    assert ltm.distance(0, HYPER // 2 - 1) == HYPER // 2 - 1
    m = model(o4)
    m.set(0, 1, HYPER - 2, 10 ** 9, 0x80000001, 5)
    assert m.moved(0, 3) == (10 ** 9 + 5 * 5000, (5 + 25000 * 0x80000001) & ltm.M32)
    assert m.moved(0, HYPER - 4) == (10 ** 9 - 2 * 5000, (5 - 10000 * 0x80000001) & ltm.M32)


def test_a_split_equals_a_whole(o4):
    rng = np.random.default_rng(5)
    fn, n0, n = HYPER - 2, 1000, 5 * 5000 + 300
    x = (rng.standard_normal((3, n)) + 1j * rng.standard_normal((3, n))).astype(np.complex64)

    def fresh():
        m = model(o4)
        m.set(0, 1, (fn - 1) % HYPER, n0 + 17 - 5000, 0x00345678, 0xfffffff0)
        m.set(1, 1, (fn + 1) % HYPER, n0 + 5000 - 200, 0xff000001, 3)          # an anchor ahead of the call: the span starts before the buffer
        return m
    a = fresh()
    cw, sw, rw = a.slice(x, n0, fn, 5)
    b = fresh()
    c1, s1, r1 = b.slice(x, n0, fn, 2)
    c2, s2, r2 = b.slice(x, n0, (fn + 2) % HYPER, 3)
    for c in range(3):
        got = c1[c] + c2[c]
        assert all(np.array_equal(p.view(np.uint32), q.view(np.uint32)) for p, q in zip(cw[c], got))
    assert (a.fn, a.pos, a.phase) == (b.fn, b.pos, b.phase) and a.fn[0] == 3
    assert sw == [0, 0, ltm.CLIPPED] and not cw[2][0][:200].any() and cw[2][0][200:].all()
    assert [r["fn"] for r in rw[0]] == [r["fn"] for r in r1[0] + r2[0]] == [0]           # HYPER is a multiple of 51: frame 0 is an FCCH frame
    assert rw[0][0]["C"] == (r1[0] + r2[0])[0]["C"]


def test_toa_convention(o4):
    """A burst that starts d samples after its cell's start reports a TOA of +d from the oracle's analyzeTrafficBurst -- so a
    grid that lies early (cells start before the bursts) reads positive TOAs and adj = +d moves it later."""
    import fectxbind
    import test_l1_msrx_model as tm
    rng = np.random.default_rng(3)
    tx = fectxbind.FecTxOracle()
    _, enc, _ = tm.encode_cell(rng, tx, 0, 2, bsic=21)
    t = next(t for t in range(16) if enc["what"][0, t] in (ltm.lmm.W_BCCH, ltm.lmm.W_CCCH, ltm.lmm.W_TCH, ltm.lmm.W_XCCH))
    x = o4.modulate(enc["bits"][0, t].astype(np.int8), 8 + (t % 4 == 0))
    for d in (0.0, 1.0, 2.0, -1.0, 0.5, -0.25, 1.75):
        y = o4.delay_vector(np.concatenate([np.zeros(16, np.complex64), x, np.zeros(16, np.complex64)]), np.float32(d))[16:16 + len(x)]
        a = o4.analyze_traffic(y, 21 & 7, 3.0)
        assert a["ok"] and abs(float(a["toa"]) - d) <= 0.05, (d, a["toa"])


def test_closed_loop_on_the_model(o4):
    """The loop of tests/test_gpu_l1trk.py on the CPU: the multiplexer's model -> the reference's modulator -> the stream model at
    30 dB -> l1_acq_model.search_model -> seed, then six rounds of stream -> TrkModel.slice -> the reference's pullRadioVector
    (oracle/transceiver_model.py, demodulating leg) -> TrkModel.update -> the decoder's model, under the truth conditions."""
    import air_loops as al
    import fectxbind
    import fec_stream_model as fsm
    import l1_acq_model as acq
    import l1_msrx_model as lrm
    import test_l1_msrx_model as tm
    import transceiver_model as trm
    tx = fectxbind.FecTxOracle()
    case = ltm.loop_case(tx)
    sps, fn0, F = case["sps"], case["fn0"], case["F"]
    air = am.AirModel(o4)
    air.rot = lambda phase, step, n: ltm.expj_many(o4, ((int(phase) + np.arange(n, dtype=np.uint64) * np.uint64(int(step))) & np.uint64(ltm.M32)) >> np.uint64(8))
    cells = al.modulated_cells(o4, case["enc"])
    la = ltm.LoopAir(case)
    pr = la.params(0, 0)
    one = lambda v, k: [v] * k
    x = air.stream(cells, case["seed"], [0], [pr["cut"]], case["n"], [pr["delay"]], [pr["step"]], [pr["phase"]], [case["gain"]],
                   [case["sigma"]], [pr["n0"]])[0]
    det = acq.SchDetector(o4)
    s = acq.search_model(det, tx, x)
    assert s["state"] == 15 and s["bsic"] == case["bsic"]
    trk = ltm.TrkModel(o4, [0, 0], [0])
    trk.seed(dict(state=[s["state"]], sch_w0=[s["w0"]], sch_toa=[s["sch"]["toa"]], omega=[np.float32(s["fcch"]["omega"])], rfn=[s["rfn"]]), [0])
    fn_a = trk.fn[0]
    assert fn0 < fn_a and fn_a + ltm.LOOP_ROUNDS * ltm.LOOP_ROUND_FRAMES <= fn0 + F
    e_seed = abs(trk.pos[0] - ltm.true_start(case, fn_a, 0))
    worst_grid, worst_f, moves = 0.0, ltm.step_error(case, 0, trk.step[0]), 0
    print("seed: grid error %.3f sample, offset error %.2e cycle / symbol" % (e_seed, worst_f))
    assert e_seed <= ltm.MAX_SEED and worst_f <= al.MAX_OFFSET

    class Tap:                                                   # the oracle, remembering analyzeTrafficBurst's last answer
        def __init__(self, o): self.o, self.last = o, None
        def __getattr__(self, k): return getattr(self.o, k)
        def analyze_traffic(self, *a, **k):
            self.last = self.o.analyze_traffic(*a, **k)
            return self.last
    taps = [Tap(o4), Tap(o4)]
    trx = [trm.TransceiverModel(t, start=(fn_a, 0), need_dfe=False) for t in taps]
    for a, t in enumerate(trx):
        for cmd in ["CMD RXTUNE 935000", "CMD TXTUNE 890000", "CMD SETTSC %d" % (case["bsic"] & 7)] + \
                   ["CMD SETSLOT %d %d" % (tn, 3 if tm.PLAN[a, tn] else 0) for tn in range(8)] + ["CMD POWERON"]:
            t.control(cmd)
    rx = lrm.Model(tm.PLAN, case["bsic"], case["band"], prims=fsm.Prims())
    outs, n_sch = [], 0
    for r in range(1, ltm.LOOP_ROUNDS + 1):
        fn_r, Fr = trk.fn[0], ltm.LOOP_ROUND_FRAMES
        n0, ns = ltm.round_plan(case, trk.pos[0], r)
        pr = la.params(r, n0)
        xs = air.stream(cells, case["seed"], [0, 1], one(pr["cut"], 2), ns, one(pr["delay"], 2), one(pr["step"], 2), one(pr["phase"], 2),
                        one(case["gain"], 2), one(case["sigma"], 2), one(pr["n0"], 2))
        cl, status, rec = trk.slice(xs, n0, fn_r, Fr)
        assert status == [0, 0]
        T = 8 * Fr
        row = np.full((T, 2), -1, np.int32)
        valid, toa = [], []
        col = dict(valid=np.zeros((T, 2), bool), soft=np.zeros((T, 2, 148), np.float32), rssi=np.zeros((T, 2), np.int64), timing=np.zeros((T, 2), np.int64))
        for t in range(T):
            for a in range(2):
                if not tm.PLAN[a, t % 8]:
                    continue
                taps[a].last = None
                got = trx[a].pull_radio_vector(cl[a][t], t % 8, (fn_r + t // 8) % HYPER)
                row[t, a] = len(valid)
                valid.append(got is not None)
                toa.append(taps[a].last["toa"] if taps[a].last is not None else 0.0)
                if got is not None:
                    col["valid"][t, a], col["soft"][t, a], col["rssi"][t, a], col["timing"][t, a] = True, got[0][:148], got[1], got[2]
        did = trk.update(row, np.array(valid, np.uint8), np.array(toa, np.float32), fn_r)[0]
        moves += did["adj"] != 0
        e = abs(trk.pos[0] - ltm.true_start(case, trk.fn[0], r))
        fe = ltm.step_error(case, r, trk.step[0])
        print("round %d: N %d adj %d K %d grid error %.3f sample, offset error %.2e cycle / symbol" % (r, did["N"], did["adj"], did["K"], e, fe))
        assert e <= ltm.MAX_GRID and did["N"] > 50
        worst_grid = max(worst_grid, e)
        if did["K"]:
            assert fe <= al.MAX_OFFSET
            worst_f = max(worst_f, fe)
        for f in range(Fr):
            if ((fn_r + f) % HYPER) % 51 in ltm.SCH_T3:
                w = np.concatenate([np.zeros(ltm.SCH_LEAD * sps, np.complex64), cl[0][8 * f]])
                d = det.detect(w, None)
                ok, bsic, rfn = lrm.sch_decode(tx, d["soft"])
                assert d["flags"] & 2 and ok and bsic == case["bsic"] and rfn == (fn_r + f) % HYPER, (r, f, d["flags"], ok, rfn)
                n_sch += 1
        outs.append(rx.decode(col, fn_r))
    print("worst grid error %.3f sample, worst offset error %.2e cycle / symbol, %d moves, %d SCH" % (worst_grid, worst_f, moves, n_sch))
    assert moves >= 1 and n_sch >= 9
    n = ltm.check_span(rx, ltm.merge_outputs(outs), case["mux"], case["grids"], case, fn_a, fn_a + ltm.LOOP_ROUNDS * ltm.LOOP_ROUND_FRAMES)
    print(n)
    assert n["tch"] > 20 and n["xcch"] > 10 and n["ccch"] >= 3 and n["bcch"] >= 1, n
