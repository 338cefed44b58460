"""GPU parity of the GPRS packet data block coders (k_fec_pdtch_encode, k_fec_pdtch_decode) through the C-ABI against
tests/pdtch_model.py, byte for byte: the schemes mixed inside a wave, bad rows, clean and noisy input, the UDP hop, forced and
detected schemes, missing and permuted bursts, flags at exactly 0.5, NaN and infinities, canaries behind every output; CS-1
against trxsig_fec_xcch_decode_batch; the host-side refusals; and one closed loop on the card."""
import numpy as np
import pytest

import _pkg
import fecbind
import fectxbind
import pdtch_model as pm

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 4, 5, 37]
CANARY, PAD = 0xA5, 64


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
    """n -> (blocks, cs, tsc, bits): mixed schemes (every scheme inside the first wave where n allows), the model's bursts."""
    cache = {}

    def get(n):
        if n not in cache:
            rng = np.random.default_rng(100 + n)
            cs = ((np.arange(n) + n) % 4).astype(np.uint8)
            if n > 8:
                cs[8:] = rng.integers(0, 4, n - 8)
            blocks = pm.random_blocks(rng, cs)
            tsc = rng.integers(0, 8, n).astype(np.uint8)
            bits = pm.encode(o, blocks, cs, tsc, fectxbind.TSC_BITS)
            for a in (blocks, cs, tsc, bits):
                a.flags.writeable = False
            cache[n] = (blocks, cs, tsc, bits)
        return cache[n]
    return get


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()             # (a copy: the shared references are read-only)


def padded(n_bytes):
    import torch
    return torch.full((n_bytes + PAD,), CANARY, dtype=torch.uint8, device="cuda")


def taken(buf, n_bytes):
    """The first n_bytes of a padded buffer on the host, after checking that nothing behind them was written."""
    h = buf.cpu().numpy()
    assert (h[n_bytes:] == CANARY).all(), "written past the end of an output"
    return h[:n_bytes]


def gpu_encode(t, blocks, cs, tsc, misalign=0):
    import torch
    n = len(cs)
    raw = padded(n * 592 + misalign)
    t.pdtch_encode(dev(blocks), dev(np.asarray(cs, np.uint8)), dev(np.asarray(tsc, np.uint8)), raw[misalign:])
    torch.cuda.synchronize()
    return taken(raw, n * 592 + misalign)[misalign:].reshape(n, 4, 148)


def gpu_decode(t, soft, n, index=None, wire=False, cs_force=-1):
    """One trxsig_fec_pdtch_decode_batch call -> (blocks, cs, dist, ok, usf) on the host, canaries checked."""
    import torch
    d_soft = dev(np.asarray(soft, np.float32))
    d_index = None if index is None else dev(np.asarray(index, np.int32))
    blocks = padded(n * 54)
    outs = [padded(n) for _ in range(4)]
    t.pdtch_decode(d_soft, n, blocks, *outs, index=d_index, wire=wire, cs_force=cs_force)
    torch.cuda.synchronize()
    return (taken(blocks, n * 54).reshape(n, 54),) + tuple(taken(x, n) for x in outs)


def same(got, want, what):
    for name, g, w in zip(("blocks", "cs", "cs_dist", "ok", "usf"), got, want):
        assert np.array_equal(g, w), (what, name, np.flatnonzero((np.asarray(g) != np.asarray(w)).reshape(len(w), -1).any(axis=1))[:8])


def noisy(rng, bits, sigma, clip):
    v = bits.reshape(-1, 148).astype(np.float32)
    if sigma:
        v = (v + rng.normal(0, sigma, v.shape)).astype(np.float32)
    return np.clip(v, 0, 1) if clip else v


@pytest.mark.parametrize("n", SIZES)
def test_encoder_equals_model(t, o, coded, n):
    blocks, cs, tsc, bits = coded(n)
    assert np.array_equal(gpu_encode(t, blocks, cs, tsc), bits)
    assert np.array_equal(gpu_encode(t, blocks, cs, tsc, misalign=1), bits)      # the byte-store form
    # bad rows among good ones, and payload bits the scheme does not carry
    rng = np.random.default_rng(n)
    cs2, tsc2 = cs.copy(), tsc.copy()
    dirty = rng.integers(0, 256, blocks.shape).astype(np.uint8)
    for i in range(n):
        k = pm.K[cs[i]]
        d = pm.payload_bits(blocks[i], int(cs[i]))
        dirty[i, :pm.OCTETS[cs[i]]] = blocks[i, :pm.OCTETS[cs[i]]]
        if k % 8:
            dirty[i, pm.OCTETS[cs[i]] - 1] |= (0xFF << (k % 8)) & 0xFF
        assert np.array_equal(pm.payload_bits(dirty[i], int(cs[i])), d)
    if n >= 3:
        cs2[1] = 4
        tsc2[n - 1] = 8
    if n >= 5:
        cs2[3], tsc2[4] = 255, 255
    want = pm.encode(o, dirty, cs2, tsc2, fectxbind.TSC_BITS)
    got = gpu_encode(t, dirty, cs2, tsc2)
    assert np.array_equal(got, want)
    if n >= 3:
        assert not got[1].any() and not got[n - 1].any() and got[0].any()


def test_cs1_bursts_equal_xcch(t, coded):
    import torch
    blocks, cs, tsc, _ = coded(37)
    n = len(cs)
    for ts in (0, 5):
        got = gpu_encode(t, blocks, np.zeros(n, np.uint8), np.full(n, ts, np.uint8))
        x = torch.full((n, 4, 148), 7, dtype=torch.uint8, device="cuda")
        t.fec_xcch_encode(dev(np.ascontiguousarray(blocks[:, :23])), n, ts, x)
        torch.cuda.synchronize()
        assert np.array_equal(got, x.cpu().numpy())


@pytest.mark.parametrize("n", SIZES)
def test_decoder_equals_model(t, o, coded, n):
    """Clean and two noise levels x the UDP hop off and on x every cs_force and detection, in every output."""
    blocks, cs, tsc, bits = coded(n)
    rng = np.random.default_rng(200 + n)
    for sigma in (0.0, 0.25, 0.45):
        for wire in (False, True):
            soft = noisy(rng, bits, sigma, clip=wire)        # (the hop is undefined outside [0, 1])
            for force in (-1, 0, 1, 2, 3):
                want = pm.decode(o, soft, None, n, wire=wire, cs_force=force)
                same(gpu_decode(t, soft, n, wire=wire, cs_force=force), want, (sigma, wire, force))
                if sigma == 0.0 and force == -1:
                    assert np.array_equal(want[0], blocks) and np.array_equal(want[1], cs) and want[3].all()
                    assert np.array_equal(want[4], blocks[:, 0] & 7) and not want[2].any()


@pytest.mark.parametrize("n", SIZES)
def test_index_missing_and_permuted(t, o, coded, n):
    """d_index: a permutation into a larger array, bursts missing (-1), out of range either way; and d_index == NULL with
    fewer rows than 4 n_blocks."""
    blocks, cs, tsc, bits = coded(n)
    rng = np.random.default_rng(300 + n)
    rows = 4 * n + 5
    perm = rng.permutation(rows)[:4 * n]
    soft = rng.random((rows, 160)).astype(np.float32)        # a stride above 148; rows no block uses hold noise
    soft[perm, :148] = noisy(rng, bits, 0.2, clip=True)
    index = perm.reshape(n, 4).astype(np.int32)
    same(gpu_decode(t, soft, n, index=index, wire=True), pm.decode(o, soft, index, n, wire=True), "permuted")
    assert np.array_equal(pm.decode(o, soft, index, n, wire=True)[1], cs)
    holes = index.copy()
    bad = np.array([-1, rows, -2 ** 31, 2 ** 31 - 1, rows + 7, -5], np.int64)
    for k in range(n):
        which = rng.permutation(4)[:(k % 4) + (n == 1)]      # 0..3 bursts of a block missing (n = 1: one)
        holes[k, which] = bad[rng.integers(0, len(bad), len(which))]
    if n >= 5:
        holes[4] = -1                                       # a whole block missing
    for wire in (False, True):
        for force in (-1, 3, 1):
            want = pm.decode(o, soft, holes, n, wire=wire, cs_force=force)
            same(gpu_decode(t, soft, n, index=holes, wire=wire, cs_force=force), want, ("holes", wire, force))
    if n >= 5:
        want = pm.decode(o, soft, holes, n)
        assert (want[1][4], want[2][4], want[3][4]) == (pm.CS3, 2, 0)       # eight flags at 0.5 slice to 00000000
    short = np.ascontiguousarray(noisy(rng, bits, 0.1, clip=True)[:4 * n - 3])
    same(gpu_decode(t, short, n, wire=True), pm.decode(o, short, None, n, wire=True), "short")


@pytest.mark.parametrize("n", SIZES)
def test_flags_at_half_nan_and_infinity(t, o, coded, n):
    blocks, cs, tsc, bits = coded(n)
    rng = np.random.default_rng(400 + n)
    soft = noisy(rng, bits, 0.15, clip=False)
    # flags at exactly 0.5 (they slice to 0): all eight of block 0, some of the others
    v = soft.reshape(n, 4, 148).copy()
    v[0, :, 60] = v[0, :, 87] = 0.5
    for k in range(1, n):
        b, pos = pm.FLAG_POS[int(rng.integers(0, 8))]
        v[k, b, pos] = 0.5
    for wire in (False, True):
        w = np.clip(v, 0, 1) if wire else v
        for force in (-1, 0, 2):
            same(gpu_decode(t, w.reshape(-1, 148), n, wire=wire, cs_force=force),
                 pm.decode(o, w.reshape(-1, 148), None, n, wire=wire, cs_force=force), ("half", wire, force))
    # a NaN, a NaN row, infinities (no UDP hop: it is undefined for them)
    v = soft.reshape(n, 4, 148).copy()
    v[0, 0, 17] = np.nan
    v[0, 1, 87] = np.nan
    v[n // 2, 2, :] = np.nan
    v[n - 1, 3, :] = np.where(rng.random(148) < 0.5, np.inf, -np.inf)
    v[n - 1, 0, 100] = np.inf
    with np.errstate(invalid="ignore"):
        for force in (-1, 0, 1, 2, 3):
            same(gpu_decode(t, v.reshape(-1, 148), n, cs_force=force), pm.decode(o, v.reshape(-1, 148), None, n, cs_force=force),
                 ("nan", force))


def test_cs1_equals_xcch_decoder(t, coded):
    import torch
    blocks, cs, tsc, bits = coded(37)
    n = len(cs)
    rng = np.random.default_rng(7)
    oks = []
    for sigma, wire in ((0.0, True), (0.3, True), (0.33, False)):
        soft = noisy(rng, bits, sigma, clip=wire)
        got = gpu_decode(t, soft, n, wire=wire, cs_force=0)
        frames = torch.zeros(n, 23, dtype=torch.uint8, device="cuda"); ok = torch.zeros(n, dtype=torch.uint8, device="cuda")
        t.fec_xcch_decode(dev(soft), n, frames, ok, wire=wire)
        torch.cuda.synchronize()
        assert np.array_equal(got[0][:, :23], frames.cpu().numpy()) and not got[0][:, 23:].any()
        assert np.array_equal(got[3], ok.cpu().numpy()) and (got[1] == 0).all()
        assert np.array_equal(got[4], got[0][:, 0] & 7)
        oks.append(got[3])
    assert np.array_equal(oks[0], cs == 0)                   # clean: exactly the CS-1 blocks pass as CS-1
    assert np.concatenate(oks[1:]).any() and not np.concatenate(oks[1:]).all()


def test_optional_outputs_and_refusals(pkg, t, o, coded):
    import torch
    blocks, cs, tsc, bits = coded(5)
    soft = dev(bits.reshape(-1, 148).astype(np.float32))
    out = padded(5 * 54)
    t.pdtch_decode(soft, 5, out, wire=False)                 # only d_blocks
    usf = padded(5)
    t.pdtch_decode(soft, 5, out, usf=usf, wire=False)
    torch.cuda.synchronize()
    assert np.array_equal(taken(out, 5 * 54).reshape(5, 54), blocks) and np.array_equal(taken(usf, 5), blocks[:, 0] & 7)
    L = pkg.lib()
    p = lambda x: x.data_ptr()
    b = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    ix = torch.zeros(64, dtype=torch.int32, device="cuda")
    dec = lambda *a: L.trxsig_fec_pdtch_decode_batch(t.h, *a)
    enc = lambda *a: L.trxsig_fec_pdtch_encode_batch(t.h, *a)
    assert enc(None, None, None, 0, None) == 0 and dec(None, 148, 0, None, 0, 1, -1, None, None, None, None, None) == 0
    assert enc(p(b), p(b), p(b), -1, p(b)) == -1 and enc(p(b), p(b), p(b), (1 << 24) + 1, p(b)) == -1
    for i in range(4):
        a = [p(b), p(b), p(b), 1, p(b)]
        a[i if i < 3 else 4] = None
        assert enc(*a) == -1, i
    good = [p(soft), 148, 20, p(ix), 1, 0, -1, p(b), p(b), p(b), p(b), p(b)]
    assert dec(*good) == 0
    for i, v in ((0, None), (1, 147), (2, -1), (4, -1), (4, (1 << 24) + 1), (6, -2), (6, 4), (7, None), (3, p(ix) + 2)):
        a = list(good)
        a[i] = v
        assert dec(*a) == -1, (i, v)
    assert b"trxsig_fec_pdtch_decode_batch: bad argument" in L.trxsig_last_error(t.h)
    torch.cuda.synchronize()


def test_closed_loop_on_the_device(pkg, t):
    """Payloads -> encode -> GMSK modulate -> noise -> TSC detect + demodulate -> decode, all on the card: every scheme's
    payloads, USFs and schemes come back, with ok set."""
    import torch
    sps, tsc, n = 4, 5, 32
    rng = np.random.default_rng(41)
    cs = (np.arange(n) % 4).astype(np.uint8)
    blocks = pm.random_blocks(rng, cs)
    blocks[:, 0] = (blocks[:, 0] & 0xF8) | (np.arange(n) // 4 % 8).astype(np.uint8)    # every USF on every scheme
    bits = torch.zeros(n, 4, 148, dtype=torch.uint8, device="cuda")
    t.pdtch_encode(dev(blocks), dev(cs), dev(np.full(n, tsc, np.uint8)), bits)
    B = 4 * n
    g = torch.Generator(device="cuda"); g.manual_seed(3)
    guard = torch.full((B,), 8, dtype=torch.int32, device="cuda")
    ns = sps * 156
    off = (torch.arange(B, dtype=torch.int32, device="cuda") * ns).contiguous()
    length = torch.full((B,), ns, dtype=torch.int32, device="cuda")
    x = torch.zeros(B * ns, 2, dtype=torch.float32, device="cuda")
    t.modulate(bits.view(B, 148), guard, x, off)
    x += 0.05 * torch.randn(x.shape, device="cuda", generator=g)
    flags = torch.zeros(B, dtype=torch.uint8, device="cuda"); amp = torch.zeros(B, 2, device="cuda"); toa = torch.zeros(B, device="cuda")
    soft = torch.zeros(B, 148, device="cuda")
    t.detect_demod_normal(x, off, length, tsc, flags, amp, toa, soft, nsoft=148, soft_stride=148)
    out = torch.zeros(n, 54, dtype=torch.uint8, device="cuda")
    ocs, dist, ok, usf = (torch.zeros(n, dtype=torch.uint8, device="cuda") for _ in range(4))
    t.pdtch_decode(soft, n, out, cs=ocs, cs_dist=dist, ok=ok, usf=usf, wire=True)
    torch.cuda.synchronize()
    assert bool(((flags & pkg.F_DETECT) != 0).all())
    assert np.array_equal(ocs.cpu().numpy(), cs) and not dist.cpu().numpy().any() and ok.cpu().numpy().all()
    assert np.array_equal(out.cpu().numpy(), blocks) and np.array_equal(usf.cpu().numpy(), blocks[:, 0] & 7)
