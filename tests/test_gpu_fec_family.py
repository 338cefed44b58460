"""The soft-bit family of tests/fec_family.py through every entry point that instantiates fec_trellis (k_fec_viterbi in its
five modes, k_fec_rx_stream in both), bit for bit against the CPU oracle (oracle/fec_oracle.c, which tests/test_fec_family.py
holds against the real reference on the same words) and the existing models: ties at a third of the steps and more, the
edges of the metric clamps, values outside [0, 1] up to +-Inf, one NaN per word at the positions where the kernel changes
path, NaN words in every row of a wave beside changing neighbours, every length around the 64-step table refill, and the
rounding ties of the UDP hop's quantisation.

Every test is parametrised by the family's class, so a failure names what the decoder got wrong:
  alphabet, lengths   a survivor decision: the strict prune, the first minimum or the order of the float adds
  edges               the metric tables
  nan, isolation      the minimum survivor under NaN costs (the reference ends on survivor 15) / one block reading another's
  wire                the quantisation"""
import numpy as np
import pytest

import _pkg
import fec_family as ff
import fec_stream_model as fsm
import fecbind
import l1_msrx_model as lrm
from test_fec_oracle import tch_bursts
from test_gpu_fec import bursts_from_ebits, dev, gpu_rach, gpu_viterbi, gpu_xcch
from test_gpu_fec_stream import gpu_stream, same, state_bytes

pytestmark = pytest.mark.gpu

CLASSES = ("alphabet", "lengths", "edges", "nan", "isolation", "wire")
CHANNEL_CLASSES = tuple(c for c in CLASSES if c != "lengths")                   # a channel has one length
# the UDP hop's conversion is undefined outside [0, 1] and for NaN, so only the wire class runs with it on
CASES = [(c, False) for c in CHANNEL_CLASSES] + [("wire", True)]
CASE_IDS = ["%s%s" % (c, "-hop" if w else "") for c, w in CASES]
_K = np.arange(456)
_J = 2 * ((49 * _K) % 57) + ((_K % 8) // 4)


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
def prims():
    return fsm.Prims()


@pytest.fixture(scope="module")
def want(o):
    """The oracle's bits for a batch of words, kept per array: computed once for every test that asks."""
    cache = {}

    def get(words, nout):
        key = (id(words), nout)
        if key not in cache:
            cache[key] = (words, np.stack([o.viterbi_decode(w, nout) for w in words]))
        return cache[key][1]
    return get


def batches(m):
    """The launches a member asks for: its words as one batch; an isolation member's groups one by one, with both sets of
    neighbours."""
    if m.groups is None:
        return [(m.name, m.soft)]
    return [("%s[%d]%s" % (m.name, i, tag), np.ascontiguousarray(w[g])) for i, g in enumerate(m.groups)
            for tag, w in (("", m.soft), ("/alt", m.alt))]


def picked(cls, entry):
    ms = ff.members(cls, entry=entry)
    assert ms, (cls, entry)
    return ms


@pytest.mark.parametrize("cls", CLASSES)
def test_viterbi_every_member_at_its_own_length(t, want, cls):
    for m in picked(cls, "viterbi"):
        got = gpu_viterbi(t, m.soft)
        assert np.array_equal(got, want(m.soft, m.nout)), (m, np.flatnonzero((got != want(m.soft, m.nout)).any(axis=1))[:8])
        if m.groups is None:
            continue
        assert np.array_equal(gpu_viterbi(t, m.alt), want(m.alt, m.nout)), m
        for g in m.groups:                                     # each batch as its own launch: the rows are the wave's
            a, b = gpu_viterbi(t, m.soft[g]), gpu_viterbi(t, m.alt[g])
            nan = m.nan_rows[g]
            assert np.array_equal(a[nan], b[nan]), (m, g, "a NaN word's output follows its neighbours")
            assert np.array_equal(a, want(m.soft, m.nout)[g]) and np.array_equal(b, want(m.alt, m.nout)[g]), (m, g)


@pytest.mark.parametrize("nout", sorted(ff.CHANNEL_NOUT))
def test_viterbi_classes_share_a_wave(t, want, nout):
    """Words of every class interleaved, so that each wave of four rows holds four different classes; ragged at the end."""
    ms = ff.members(nout=nout)
    assert {m.cls for m in ms} == {"alphabet", "edges", "nan", "isolation", "wire"} and len(ms) == 8
    take = min(len(m.soft) for m in ms)
    order = [0, 3, 4, 6, 1, 5, 7, 2]                           # garbage, edges, nan, isolation | quarter, nan, wire, hard
    words = np.stack([ms[i].soft[:take] for i in order], axis=1).reshape(take * len(ms), 2 * nout)[:-1]
    exp = np.stack([want(ms[i].soft, nout)[:take] for i in order], axis=1).reshape(take * len(ms), nout)[:-1]
    assert len(words) % 4 == 3
    assert np.array_equal(gpu_viterbi(t, words), exp)


@pytest.mark.parametrize("cls,wire", CASES, ids=CASE_IDS)
def test_xcch_decode(t, o, cls, wire):
    rng = np.random.default_rng(1)
    for m in picked(cls, "xcch"):
        for name, c in batches(m):
            e = np.zeros((len(c), 4, 114), np.float32)
            e[:, _K % 4, _J] = c                               # the interleaver (GSM 05.03 4.1.4)
            b = bursts_from_ebits(rng, e)
            frames, ok = gpu_xcch(t, b, wire)
            wf, wok = o.xcch_decode_batch(b, wire=wire, nthreads=8)
            assert np.array_equal(frames, wf) and np.array_equal(ok, wok), name


def gpu_tch(t, b, wire):
    import torch
    nbl = b.shape[0] // 4 - 1
    tch = torch.full((nbl, 33), 7, dtype=torch.uint8, device="cuda")
    outs = [torch.full((nbl,), 7, dtype=torch.uint8, device="cuda") for _ in range(3)]
    facch = torch.full((nbl, 23), 7, dtype=torch.uint8, device="cuda")
    t.fec_tch_decode(dev(b), b.shape[0], tch, outs[0], outs[1], facch=facch, facch_ok=outs[2], wire=wire)
    torch.cuda.synchronize()
    return dict(tch=tch.cpu().numpy(), good=outs[0].cpu().numpy(), stolen=outs[1].cpu().numpy(), facch=facch.cpu().numpy(),
                facch_ok=outs[2].cpu().numpy())


def flag_values(cls, wire, k):
    """k values for the Hl stealing flag (bit 60) in the member's own kind: the wire ties, or the edges and both NaNs."""
    pool = ff.WIRE_VALUES if wire or cls == "wire" else np.concatenate([ff.EDGES, np.float32([np.nan, -np.nan, 0.9, 0.1])])
    return pool[np.arange(k) % len(pool)]


@pytest.mark.parametrize("cls,wire", CASES, ids=CASE_IDS)
def test_tch_decode_with_facch(t, o, cls, wire):
    """Class 1 through the trellis (378 -> 189), class 2 (c[378..456)) and Hl sliced -- those carry the member's edge values
    and NaNs too -- and the FACCH decode of the same block (456 -> 228, the ilv8 path)."""
    rng = np.random.default_rng(2)
    for m in picked(cls, "tch"):
        if cls in ("edges", "nan"):
            assert not np.isfinite(m.soft[:, 378:]).all()     # the class-2 positions see them
        for name, c in batches(m):
            b = tch_bursts(rng, c)
            b[:, 60] = flag_values(cls, wire, len(b))
            got, exp = gpu_tch(t, b, wire), o.tch_decode_batch(b, wire=wire, nthreads=8)
            for k in ("tch", "good", "stolen", "facch", "facch_ok"):
                assert np.array_equal(got[k], exp[k]), (name, k)


@pytest.mark.parametrize("cls,wire", CASES, ids=CASE_IDS)
def test_rach_decode(t, o, cls, wire):
    rng = np.random.default_rng(3)
    for m in picked(cls, "rach"):
        for name, c in batches(m):
            b = rng.random((len(c), 148)).astype(np.float32)
            b[:, 49:85] = c
            assert np.array_equal(gpu_rach(t, b, wire), o.rach_decode_batch(b, wire=wire, nthreads=8)), name


@pytest.mark.parametrize("cls", CHANNEL_CLASSES)
def test_sch_decode(t, o, cls):
    import torch
    rng = np.random.default_rng(4)
    for m in picked(cls, "sch"):
        for name, c in batches(m):
            n = len(c)
            b = rng.random((n, 148)).astype(np.float32)
            b[:, 3:42], b[:, 106:145] = c[:, :39], c[:, 39:]
            ok = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
            bsic = torch.full((n,), 99, dtype=torch.uint8, device="cuda")
            rfn = torch.full((n,), -9, dtype=torch.int32, device="cuda")
            t.fec_sch_decode(dev(b), n, ok, bsic, rfn)
            torch.cuda.synchronize()
            got = [(bool(x), int(y), int(z)) for x, y, z in zip(ok.cpu().numpy(), bsic.cpu().numpy(), rfn.cpu().numpy())]
            assert got == [(bool(x), int(y), int(z)) for x, y, z in (lrm.sch_decode(o, v) for v in b)], name


# ---- the stream decoders ----
S_CH, T_SLOTS = 8, 16


def stream_case(tch, wire):
    """8 channels x 16 slots of family words: alphabet, edge, NaN and isolation rows mixed (the wire member's under the
    hop).  TCH: a channel's 16 bursts carry three words through the diagonal interleaver; the four closing bursts of a
    channel -- one wave of k_fec_rx_stream -- are one stolen (a 456-value row), two not (378) and one missing (an undecoded
    row), rotated from channel to channel, and the other Hl flags take the edge values and NaNs.  XCCH: four words per channel,
    one closing burst missing.  A few other bursts are missing too."""
    rng = np.random.default_rng(50 + 2 * tch + wire)
    if wire:
        pool = ff.members("wire", entry="stream")[0].soft
    else:
        ms = [m for m in ff.members(entry="stream") if m.cls != "wire"]
        pool = np.stack([m.soft[:48] for m in ms], axis=1).reshape(-1, 456)       # consecutive words from different members
    per = 3 if tch else 4
    nan_words = ff.members("nan", entry="stream")[0].soft
    rows = np.zeros((S_CH * T_SLOTS, 148), np.float32)
    for s in range(S_CH):
        c = pool[per * s:per * s + per].copy()
        if s % 4 == 0 and not wire:
            c[-1] = nan_words[s]                                # the channel's last block stays undecoded: its NaN stays in mI
        if tch:
            b = tch_bursts(rng, c)
            b[:, 60] = flag_values("wire" if wire else "edges", wire, len(b))[::-1]
        else:
            e = np.zeros((per, 4, 114), np.float32)
            e[:, _K % 4, _J] = c
            b = bursts_from_ebits(rng, e)
        rows[T_SLOTS * s:T_SLOTS * (s + 1)] = b
    index = np.arange(S_CH * T_SLOTS, dtype=np.int32).reshape(S_CH, T_SLOTS)
    index[rng.random(index.shape) < 0.08] = -1
    for s in range(S_CH):
        close = 4 * ((np.arange(4) + s) % 4) + 3
        index[s, close] = T_SLOTS * s + close                   # present, but for the last of the rotation
        index[s, close[3]] = -1
        if tch:
            rows[T_SLOTS * s + close[:3], 60] = np.float32([0.9, 0.1, 0.25])
    b0 = (np.array([0, 0, 4, 0, 0, 4, 0, 0], np.uint8) if tch else None)
    st = np.zeros((S_CH, state_bytes(tch)), np.uint8)
    st[:, fsm.HDR:] = ff.ALPHABET[rng.integers(0, 5, (S_CH, (state_bytes(tch) - fsm.HDR) // 4))].view(np.uint8)
    return rows, index, b0, st


@pytest.mark.parametrize("wire", [False, True], ids=["family", "wire-hop"])
@pytest.mark.parametrize("tch", [True, False], ids=["tch", "xcch"])
def test_streams_in_one_call_and_in_two(t, prims, tch, wire):
    rows, index, b0, st0 = stream_case(tch, wire)
    whole = fsm.run(prims, tch, rows, index, st0, b0=b0, wire=wire)
    status = whole["status"]
    assert ((status & fsm.DECODED) == 0).any(axis=1).all()      # every wave holds an undecoded row ...
    if tch:                                                      # ... a 456-value row and a 378-value one
        dec = (status & fsm.DECODED) != 0
        assert (dec & ((status & fsm.STOLEN) != 0)).any(axis=1).all() and (dec & ((status & fsm.STOLEN) == 0)).any(axis=1).all()
    if not wire:
        assert np.isnan(rows[index[index >= 0]]).any() and np.isnan(whole["state"][:, fsm.HDR:].view(np.float32)).any()
    g = gpu_stream(t, tch, rows, index, st0, b0=b0, wire=wire)
    same(g, whole, "one call")                                  # status, frames, FER bits and state bytes, NaN in mI included
    h = T_SLOTS // 2
    a = gpu_stream(t, tch, rows, index[:, :h], st0, b0=b0, wire=wire)
    ma = fsm.run(prims, tch, rows, index[:, :h], st0, b0=b0, wire=wire)
    same(a, ma, "first half")
    b = gpu_stream(t, tch, rows, index[:, h:], a["state"], b0=b0, wire=wire)     # (b0 + 8) % 8 = b0
    same(b, fsm.run(prims, tch, rows, index[:, h:], ma["state"], b0=b0, wire=wire), "second half")
    for k in ("status", "tch", "l2", "fer"):
        if k in g:
            assert np.array_equal(np.concatenate([a[k], b[k]], axis=1).view(np.uint8), g[k].view(np.uint8)), k
    assert np.array_equal(b["state"], g["state"])
