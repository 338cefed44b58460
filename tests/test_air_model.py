"""The air's model (tests/air_model.py) on its own: Philox4x32-10's known answers, the moments of the Gaussian pair, distinct
counter streams, and the properties the device form is built on -- a run cut into calls equals one call, and the stream form
without impairments is the concatenated cells.  No GPU needed."""
import numpy as np
import pytest

import air_model as am
import oraclebind


def words(c):
    return " ".join("%08x" % int(v) for v in c)


def test_philox_known_answers():
    f = 0xffffffff
    assert words(am.philox4x32_10((0, 0, 0, 0), (0, 0))) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert words(am.philox4x32_10((f, f, f, f), (f, f))) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert words(am.philox4x32_10((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0))) == \
        "d16cfe09 94fdcceb 5001e420 24126ea1"


def test_gaussian_moments():
    N = 1 << 20
    g = am.stream_gauss(1, 0, 0, N)
    assert np.abs(g).max() <= 5.77
    for v in (g.real, g.imag):
        print("mean %.3e var - 1 %.3e" % (v.mean(), v.var() - 1))
        assert abs(v.mean()) <= 5 / np.sqrt(N)
        assert abs(v.var() - 1) <= 5 * np.sqrt(2 / N)
    assert abs((g.real * g.imag).mean()) <= 5 / np.sqrt(N)


def test_counter_streams_are_distinct():
    row, plane, form = np.meshgrid(np.arange(1024), np.arange(2), np.arange(2), indexing="ij")
    w = am.philox4x32_10((0, row.ravel(), plane.ravel(), form.ravel()), (1, 0))
    seen = set(zip(*[v.tolist() for v in w]))
    assert len(seen) == 4096
    # an even and an odd sample of one block take different halves; the seed's two words both matter
    assert am.gauss(1, 0, 0, 0, 0) != am.gauss(1, 1, 0, 0, 0)
    assert am.gauss(1, 0, 0, 0, 0) != am.gauss(1 << 32, 0, 0, 0, 0) != am.gauss(1 + (1 << 32), 0, 0, 0, 0)


@pytest.fixture(scope="module", params=[1, 4])
def model(request):
    return am.AirModel(oraclebind.Oracle(request.param))


def equal(a, b):
    return all(np.array_equal(np.asarray(p).view(np.uint32), np.asarray(q).view(np.uint32)) for r, s in zip(a, b) for p, q in zip(r, s))


def test_cell_call_split(model):
    sps = model.sps
    rng = np.random.default_rng(3)
    A, F, fn = 2, 4, am.HYPER - 2                              # the split falls on the hyperframe's wrap
    x = am.random_cells(rng, A, 8 * F, sps)
    taps = [[(rng.standard_normal(3) + 1j * rng.standard_normal(3)).astype(np.complex64) for _ in range(8 * F)] for _ in range(A)]
    step = rng.integers(0, 1 << 32, (A, 8 * F)); phase = rng.integers(0, 1 << 32, (A, 8 * F))
    sigma = rng.random((A, 8 * F)).astype(np.float32)
    whole = model.cells(fn, x, 7, taps, step, phase, sigma)
    cut = lambda v, lo, hi: [r[lo:hi] for r in v]
    first = model.cells(fn, cut(x, 0, 16), 7, cut(taps, 0, 16), step[:, :16], phase[:, :16], sigma[:, :16])
    second = model.cells((fn + 2) % am.HYPER, cut(x, 16, 32), 7, cut(taps, 16, 32), step[:, 16:], phase[:, 16:], sigma[:, 16:])
    assert equal(whole, [p + q for p, q in zip(first, second)])
    other = model.cells(fn, x, 8, taps, step, phase, sigma)
    assert not equal(whole, other)


def test_stream_call_split_and_identity(model):
    sps = model.sps
    rng = np.random.default_rng(4)
    x = am.random_cells(rng, 2, 10, sps)
    arfcn, cut, delay = [1, 0, 1], [-7, 100 * sps, 9 * 156 * sps], [2.4, -1.5, 0.005]
    step, phase, n0 = [12345678, 0, 0xfff00000], [5, 0xffffff00, 77], [0, 3, 0xfffffff0]
    gain, sigma = [1 + 0.5j, -0.3j, 2.0], [0.1, 0.5, 0.0]
    L, L1 = 300 * sps + 5, 123
    whole = model.stream(x, 9, arfcn, cut, L, delay, step, phase, gain, sigma, n0)
    a = model.stream(x, 9, arfcn, cut, L1, delay, step, phase, gain, sigma, n0)
    adv = lambda v, k: [(p + k * L1) & 0xffffffff for p, k in zip(v, k)]
    b = model.stream(x, 9, arfcn, [c + L1 for c in cut], L - L1, delay, step, adv(phase, step), gain, sigma, adv(n0, [1, 1, 1]))
    assert np.array_equal(whole.view(np.uint32), np.concatenate([a, b], axis=1).view(np.uint32))
    # nothing applied, and everything applied at its neutral value: the concatenated cells
    c1 = np.concatenate(x[1])
    assert np.array_equal(model.stream(x, 0, [1], [0], len(c1))[0].view(np.uint32), c1.view(np.uint32))
    assert np.array_equal(model.stream(x, 0, [1], [0], len(c1) + 9, [0.0], [0], [0], [1.0])[0, :len(c1)], c1)
    assert not model.stream(x, 0, [1], [0], len(c1) + 9, [0.0], [0], [0], [1.0])[0, len(c1):].any()


def test_downlink_case_on_the_model(model):
    """The downlink loop of tests/test_gpu_air.py on the CPU: the multiplexer's model -> the reference's modulator -> the stream
    model at 20 dB -> l1_acq_model.search_model.  Every handset reaches state 15 with the true FN and BSIC inside the truth
    bounds, so the case the device is held to is one the reference's own detectors pass."""
    import air_loops as al
    import fectxbind
    import l1_acq_model as acq
    tx = fectxbind.FecTxOracle()
    case = al.downlink_case(model.sps, tx)
    cells = al.modulated_cells(model.o, case["enc"])
    x = model.stream(cells, case["seed"], [0] * case["H"], case["cut"], case["n"], case["delay"], case["step"], case["phase"],
                     case["gain"], case["sigma"], case["n0"])
    det = acq.SchDetector(model.o)
    worst_t = worst_f = 0.0
    for h in range(case["H"]):
        r = acq.search_model(det, tx, x[h])
        dt, df = al.check_handset(case, h, r["state"], r["bsic"], r["rfn"], r["w0"] + float(r["sch"]["toa"]),
                                  r["fcch"]["arg"] / (2 * np.pi))
        worst_t, worst_f = max(worst_t, dt), max(worst_f, df)
    print("sps %d: worst timing error %.3f sample, worst offset error %.2e cycle / symbol" % (model.sps, worst_t, worst_f))
    assert worst_t <= al.MAX_TIMING and worst_f <= al.MAX_OFFSET
    assert len(set(case["cut"])) == case["H"] and max(case["cut"]) > 25 * 1250 * model.sps > min(case["cut"])
