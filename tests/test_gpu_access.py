"""GPU parity of the access burst's coders (k_fec_access_encode, k_fec_access_decode) through the C-ABI against
tests/access_model.py, byte for byte: both formats mixed inside a wave, refused rows, fmt 0 / 1 / either, the UDP hop off and
on, a d_index with missing and out-of-range rows, noisy values, a hostile batch (NaN, infinities, values outside [0, 1]),
canaries behind every output; format 0 against trxsig_fec_rach_decode_batch on the same rows; the host-side refusals."""
import numpy as np
import pytest

import _pkg
import access_model as am
import fecbind

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 4, 5, 37]                                     # one row of a wave, its tail on either side of four, ten waves
CANARY, PAD = 0xA5, 64
BSIC = 0x2B


@pytest.fixture(scope="module")
def pkg():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _pkg.load()


@pytest.fixture(scope="module")
def t(pkg):
    c = pkg.TrxSig(4, 0)
    c.use_torch_stream()
    return c


@pytest.fixture(scope="module")
def o():
    return fecbind.FecOracle()


@pytest.fixture(scope="module")
def coded(o):
    """n -> (ra, fmt, bsic, bits): the formats alternate, so both sit inside every wave that has two rows; one cell's BSIC (what
    the either-mode decoder is given) in all but the last row."""
    cache = {}

    def get(n):
        if n not in cache:
            rng = np.random.default_rng(500 + n)
            fmt = ((np.arange(n) + n) % 2).astype(np.uint8)
            ra = np.where(fmt == 1, rng.integers(0, 2048, n), rng.integers(0, 256, n)).astype(np.uint16)
            bsic = np.full(n, BSIC, np.uint8)
            if n > 1:
                bsic[n - 1] = 63 - BSIC
            bits = am.encode(o, ra, fmt, bsic)
            for a in (ra, fmt, bsic, bits):
                a.flags.writeable = False
            cache[n] = (ra, fmt, bsic, bits)
        return cache[n]
    return get


def dev(a):
    import torch
    a = np.array(a, order="C")                               # (a copy: the shared references are read-only)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.from_numpy(a).cuda()


def padded(n_bytes):
    import torch
    return torch.full((n_bytes + PAD,), CANARY, dtype=torch.uint8, device="cuda")


def taken(buf, n_bytes):
    """The first n_bytes of a padded buffer on the host, after checking that nothing behind them was written."""
    h = buf.cpu().numpy()
    assert (h[n_bytes:] == CANARY).all(), "written past the end of an output"
    return h[:n_bytes]


def gpu_encode(t, ra, fmt, bsic, misalign=0):
    import torch
    n = len(fmt)
    raw = padded(n * 148 + misalign)
    t.access_encode(dev(np.asarray(ra, np.uint16)), dev(np.asarray(fmt, np.uint8)), dev(np.asarray(bsic, np.uint8)), raw[misalign:])
    torch.cuda.synchronize()
    return taken(raw, n * 148 + misalign)[misalign:].reshape(n, 148)


def gpu_decode(t, soft, n, index=None, wire=False, fmt=-1, bsic=BSIC):
    """One trxsig_fec_access_decode_batch call -> (ra, fmt, tail_ok, bsic) on the host, canaries checked."""
    import torch
    d_soft = dev(np.asarray(soft, np.float32))
    d_index = None if index is None else dev(np.asarray(index, np.int32))
    ra = padded(2 * n)
    outs = [padded(n) for _ in range(3)]
    t.access_decode(d_soft, n, ra, *outs, index=d_index, wire=wire, fmt=fmt, bsic=bsic)
    torch.cuda.synchronize()
    return (taken(ra, 2 * n).view(np.uint16),) + tuple(taken(x, n) for x in outs)


def same(got, want, what):
    for name, g, w in zip(("ra", "fmt", "tail_ok", "bsic"), got, want):
        assert np.array_equal(g, w), (what, name, np.flatnonzero(np.asarray(g) != np.asarray(w))[:8])


def noisy(rng, bits, sigma, clip):
    v = bits.astype(np.float32)
    if sigma:
        v = (v + rng.normal(0, sigma, v.shape)).astype(np.float32)
    return np.clip(v, 0, 1) if clip else v


@pytest.mark.parametrize("n", SIZES)
def test_encoder_equals_model(t, o, coded, n):
    ra, fmt, bsic, bits = coded(n)
    assert np.array_equal(gpu_encode(t, ra, fmt, bsic), bits)
    assert np.array_equal(gpu_encode(t, ra, fmt, bsic, misalign=1), bits)        # the byte-store form
    assert bits[:, :49].any() and not bits[:, 85:].any()
    # refused rows among good ones: a format above 1, a BSIC above 63, a word that does not fit its format
    ra2, fmt2, bsic2 = ra.copy(), fmt.copy(), bsic.copy()
    if n >= 3:
        fmt2[1] = 2
        bsic2[n - 1] = 64
    if n >= 5:
        fmt2[3], ra2[3] = 0, 256
        fmt2[4], ra2[4] = 1, 2048
        fmt2[0], ra2[0] = 1, 2047
    if n >= 37:
        fmt2[8], ra2[9], bsic2[10] = 255, 65535, 255
        fmt2[12], ra2[12] = 0, 255
    want = am.encode(o, ra2, fmt2, bsic2)
    got = gpu_encode(t, ra2, fmt2, bsic2)
    assert np.array_equal(got, want)
    if n >= 5:
        assert not got[1].any() and not got[3].any() and not got[4].any() and not got[n - 1].any() and got[0].any() and got[2].any()


def test_format_0_bursts_equal_the_handsets(t, o):
    """The 8-bit format's bytes are what the mobile-side multiplexer's model writes for an access burst (tests/l1_ms_model.py)."""
    import l1_ms_model as mm
    ra = np.arange(256, dtype=np.uint16)
    for bsic in (0, 21, 63):
        got = gpu_encode(t, ra, np.zeros(256, np.uint8), np.full(256, bsic, np.uint8))
        assert np.array_equal(got, np.stack([mm.access_burst(o, int(r), bsic) for r in ra]))


@pytest.mark.parametrize("n", SIZES)
def test_decoder_equals_model(t, o, coded, n):
    """Clean and two noise levels x the UDP hop off and on x fmt 0, 1 and either, in every output."""
    ra, fmt, bsic, bits = coded(n)
    rng = np.random.default_rng(600 + n)
    for sigma in (0.0, 0.15, 0.3):
        for wire in (False, True):
            soft = noisy(rng, bits, sigma, clip=wire)        # (the hop is undefined outside [0, 1])
            for f in (-1, 0, 1):
                want = am.decode(o, soft, None, n, wire=wire, fmt=f, bsic=BSIC)
                same(gpu_decode(t, soft, n, wire=wire, fmt=f), want, (sigma, wire, f))
                if sigma == 0.0 and f == -1:                 # clean: every row of the cell's BSIC comes back as it was sent
                    mine = bsic == BSIC
                    assert np.array_equal(want[0][mine], ra[mine]) and np.array_equal(want[1][mine], fmt[mine])
                    assert want[2][mine].all() and (want[3][mine] == BSIC).all()


@pytest.mark.parametrize("n", SIZES)
def test_index_missing_and_out_of_range(t, o, coded, n):
    """d_index: a permutation into a larger array, rows missing (-1) and out of range either way; and d_index == NULL with
    fewer rows than n."""
    ra, fmt, bsic, bits = coded(n)
    rng = np.random.default_rng(700 + n)
    rows = n + 5
    perm = rng.permutation(rows)[:n]
    soft = rng.random((rows, 96)).astype(np.float32)         # a stride between 85 and 148; rows no burst uses hold noise
    soft[perm] = noisy(rng, bits, 0.2, clip=True)[:, :96]
    index = perm.astype(np.int32)
    want = am.decode(o, soft, index, n, wire=True, fmt=-1, bsic=BSIC)
    same(gpu_decode(t, soft, n, index=index, wire=True), want, "permuted")
    holes = index.copy()
    bad = np.array([-1, rows, -2 ** 31, 2 ** 31 - 1, rows + 7, -5], np.int64)
    which = rng.permutation(n)[:max(1, n // 3)]
    holes[which] = bad[rng.integers(0, len(bad), len(which))]
    for wire in (False, True):
        for f in (-1, 0, 1):
            want = am.decode(o, soft, holes, n, wire=wire, fmt=f, bsic=BSIC)
            same(gpu_decode(t, soft, n, index=holes, wire=wire, fmt=f), want, ("holes", wire, f))
    short = np.ascontiguousarray(noisy(rng, bits, 0.1, clip=True)[:max(n - 2, 0)])
    if n > 2:
        for f in (-1, 1):
            same(gpu_decode(t, short, n, wire=True, fmt=f), am.decode(o, short, None, n, wire=True, fmt=f, bsic=BSIC), ("short", f))


@pytest.mark.parametrize("n", SIZES)
def test_hostile_values(t, o, coded, n):
    """NaN, +-Inf and values outside [0, 1], no UDP hop (it is undefined for them): SoftVector::decode as it is written."""
    ra, fmt, bsic, bits = coded(n)
    rng = np.random.default_rng(800 + n)
    v = noisy(rng, bits, 0.15, clip=False) * np.float32(1.5) - np.float32(0.25)
    v[0, 60] = np.nan
    v[n // 2, 49:85] = np.nan
    v[n - 1, 49:85] = np.where(rng.random(36) < 0.5, np.inf, -np.inf)
    if n >= 5:
        v[3, 49], v[3, 84], v[2, 70] = np.inf, np.nan, -np.inf
        v[4, 49:85] = rng.choice(np.array([np.nan, np.inf, -np.inf, 7.0, -7.0, 0.5], np.float32), 36)
    with np.errstate(invalid="ignore"):
        for f in (-1, 0, 1):
            same(gpu_decode(t, v, n, fmt=f), am.decode(o, v, None, n, fmt=f, bsic=BSIC), ("hostile", f))


def test_format_0_equals_the_rach_decoder(t, coded):
    import torch
    ra, fmt, bsic, bits = coded(37)
    n = len(ra)
    rng = np.random.default_rng(9)
    for sigma, wire in ((0.0, True), (0.3, True), (0.33, False)):
        soft = noisy(rng, bits, sigma, clip=wire)
        got = gpu_decode(t, soft, n, wire=wire, fmt=0)
        tail, b, r = (torch.zeros(n, dtype=torch.uint8, device="cuda") for _ in range(3))
        t.fec_rach_decode(dev(soft), n, tail, b, r, wire=wire)
        torch.cuda.synchronize()
        assert np.array_equal(got[0], r.cpu().numpy().astype(np.uint16)) and not got[1].any()
        assert np.array_equal(got[2], tail.cpu().numpy()) and np.array_equal(got[3], b.cpu().numpy())


def test_optional_outputs_and_refusals(pkg, t, o, coded):
    import torch
    ra, fmt, bsic, bits = coded(5)
    soft = dev(bits.astype(np.float32))
    out = padded(10)
    t.access_decode(soft, 5, out, wire=False, fmt=-1, bsic=BSIC)                  # only d_ra
    f = padded(5)
    t.access_decode(soft, 5, out, fmt_out=f, wire=False, fmt=-1, bsic=BSIC)
    torch.cuda.synchronize()
    assert np.array_equal(taken(out, 10).view(np.uint16)[:4], ra[:4]) and np.array_equal(taken(f, 5)[:4], fmt[:4])
    L = pkg.lib()
    p = lambda x: x.data_ptr()
    b = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    ix = torch.zeros(64, dtype=torch.int32, device="cuda")
    dec = lambda *a: L.trxsig_fec_access_decode_batch(t.h, *a)
    enc = lambda *a: L.trxsig_fec_access_encode_batch(t.h, *a)
    assert enc(None, None, None, 0, None) == 0 and dec(None, 148, 0, None, 0, 1, -1, 0, None, None, None, None) == 0
    assert enc(p(b), p(b), p(b), -1, p(b)) == -1 and enc(p(b), p(b), p(b), (1 << 24) + 1, p(b)) == -1
    assert enc(p(b) + 1, p(b), p(b), 1, p(b)) == -1
    for i in range(4):
        a = [p(b), p(b), p(b), 1, p(b)]
        a[i if i < 3 else 4] = None
        assert enc(*a) == -1, i
    good = [p(soft), 148, 5, p(ix), 1, 0, -1, 63, p(b), p(b), p(b), p(b)]
    assert dec(*good) == 0
    for i, v in ((0, None), (1, 84), (2, -1), (4, -1), (4, (1 << 24) + 1), (6, -2), (6, 2), (7, 64), (7, -1), (8, None),
                 (3, p(ix) + 2), (8, p(b) + 1)):
        a = list(good)
        a[i] = v
        assert dec(*a) == -1, (i, v)
    a = list(good)
    a[6], a[7] = 1, 64                                       # the BSIC is not looked at where the format is given
    assert dec(*a) == 0
    assert b"trxsig_fec_access_decode_batch: bad argument" in L.trxsig_last_error(t.h)
    torch.cuda.synchronize()
