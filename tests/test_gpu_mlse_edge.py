"""The four sequence-equaliser kernels (k_mlse, k_mlse_div, k_mlse_irc, k_mlse_access) at the edges of float32 and of the burst
geometry, at sps 1, 2 and 4, against their float32 models on tests/mlse_edge_family.py (tests/test_mlse_edge_model.py proves on the
CPU that the family reaches each case): symbols from 2^-75, where every square underflows to zero, through the range where the
squares are subnormal and the window energies tie exactly, to 2^29 beside the 2^30 guard; bursts on the boundaries of k_demod's
test; covariance sets on the boundaries of step 2c.  Everything is IEEE-equal to the model ("both NaN, or =="), canaries stay behind
nsoft, a repeat gives the same bytes, and the scale identity holds on the device's own outputs with no model involved."""
import numpy as np
import pytest

import mlse_edge_family as ef
import mlse_irc_model as im
import mlse_run
from mlse_run import ctx, dev, pkg, run_access, run_div, run_irc, run_mlse  # noqa: F401  (the fixtures)
from util import GpuBatch

pytestmark = pytest.mark.gpu
F = np.float32
RUN = dict(mlse=run_mlse, div=run_div, irc=run_irc, access=run_access)


def check(got, want, nsoft=148, what=""):
    """mlse_run.check on the whole batch; a NaN tap is allowed where the model has one."""
    mlse_run.check(got, want, nsoft=nsoft, what=what, nan_taps=True)


def run_view(kernel, t, f, guard, nsoft=148, stride=160):
    """mlse_run's calls with sample tensors that are VIEWS starting `guard` samples inside their allocations (the offsets count from
    the view): a kernel that read a burst at offset -1 would stay inside the buffer.  The same outputs and canaries."""
    return mlse_run.run(kernel, t, f, nsoft=nsoft, stride=stride, loading=f.get("loading"), guard=guard)


@pytest.mark.parametrize("sps", [1, 2, 4])
@pytest.mark.parametrize("kernel", ef.KERNELS)
def test_ladder(ctx, kernel, sps):
    """35 scaled copies of three bursts, 2^-75 .. 2^29, interleaved so that a wave holds a burst that falls back beside an equalised
    one and subnormal squares beside 2^58: every output equals the model; nsoft = 100 leaves the canaries; a repeat gives the same
    bytes; and the device's own rows at 2^-50 and 2^28 are its rows at 1 (taps: times 2^k) -- no model involved."""
    f = ef.ladder(kernel, sps)
    got = RUN[kernel](ctx[sps], f)
    check(got, f["want"], what="%s sps %d ladder" % (kernel, sps))
    for k in (-50, 28):
        ef.assert_scale_identity(kernel, got, f, k)
    again = RUN[kernel](ctx[sps], f)
    for key in got:
        assert got[key].tobytes() == again[key].tobytes(), "repeat differs: " + key
    part = RUN[kernel](ctx[sps], f, nsoft=100)
    check(part, f["want"], nsoft=100, what="%s sps %d ladder, nsoft 100" % (kernel, sps))


@pytest.mark.parametrize("sps", [1, 2, 4])
@pytest.mark.parametrize("kernel", ef.KERNELS)
def test_geometry(ctx, kernel, sps):
    """27 bursts on the boundaries of k_demod's test (91 / 92, 147 / 148, 157 / 158 symbols, lengths that are no multiple of sps, TOA
    +-4096 and one float beyond, a NaN TOA, offset -1 -- on the non-primary antenna alone for the two-antenna kernels), every ordered
    pair of (equalised, fell back, skipped) within the waves: every output equals the model, a skipped burst's row is zeros up to
    nsoft and canaries behind it.  The sample tensors are views 16 samples inside their allocations."""
    f = ef.geometry(kernel, sps)
    got = run_view(kernel, ctx[sps], f, ef.GUARD)
    check(got, f["want"], what="%s sps %d geometry" % (kernel, sps))
    skipped = f["state"] == ef.SK
    assert np.all(got["win"][skipped] == 2) and not got["soft"][skipped][:, :148].any() and not got["hard"][skipped][:, :148].any()
    assert not got["chan"][skipped].any()
    again = run_view(kernel, ctx[sps], f, ef.GUARD)
    for key in got:
        assert got[key].tobytes() == again[key].tobytes(), "repeat differs: " + key


@pytest.mark.parametrize("sps", [1, 2, 4])
def test_irc_sets(ctx, sps):
    """d_cov_in rows on the boundaries of step 2c's test (mlse_edge_family.irc_sets): every output equals the model; an accepted set
    comes back as given; where the identity set is taken the outputs are the device's own trxsig_mlse_div_batch's byte for byte."""
    f = ef.irc_set_batch(sps)
    got = run_irc(ctx[sps], f, cov_in=f["cov_in"])
    check(got, f["want"], what="sps %d given sets" % sps)
    div = run_irc(ctx[sps], f, div=True)
    assert np.all(div["win"] <= 0)
    acc = f["accepted"]
    assert got["cov"][acc].tobytes() == f["cov_in"][acc].tobytes()
    assert np.all(got["cov"][~acc] == im.IDENTITY)
    for key in ("soft", "hard", "win", "chan"):
        assert got[key][~acc].tobytes() == div[key][~acc].tobytes(), "identity set: %s differs from trxsig_mlse_div_batch" % key
    assert (got["soft"][acc] != div["soft"][acc]).any(axis=1).sum() >= acc.sum() - 2


@pytest.mark.parametrize("sps", [1, 2, 4])
def test_estimated_sets(ctx, sps):
    """The estimated set where det vanishes: the same samples on both antennas at loading 0 (A == Bv == xr == 0.5, det == 0: the
    identity set, and trxsig_mlse_div_batch's bytes), antenna 1 twice antenna 0 (det is rounding error; the model says which
    bursts take the identity set) and the copy at loading 2^-20 (det about 2^-20, the set is used)."""
    for name, f, loading, identity in ef.estimated_set_cases(sps):
        want = ef.model(dict(f, loading=loading))
        got = run_irc(ctx[sps], f, loading=float(loading))
        check(got, want, what="sps %d %s" % (sps, name))
        eq = got["win"] <= 0
        ident = eq & np.all(got["cov"] == im.IDENTITY, axis=1)
        if identity is not None:
            assert np.all(ident[eq] == identity), name
        if ident.any():
            div = run_irc(ctx[sps], f, div=True)
            for key in ("soft", "hard", "win", "chan"):
                assert got[key][ident].tobytes() == div[key][ident].tobytes(), "%s: %s differs from trxsig_mlse_div_batch" % (name, key)


@pytest.mark.parametrize("sps", [1, 4])
@pytest.mark.parametrize("kernel", ef.KERNELS)
def test_batch_entry_calls(pkg, ctx, kernel, sps):
    """trxsig_mlse_normal_batch, trxsig_mlse_div_normal_batch, trxsig_mlse_irc_normal_batch and trxsig_mlse_rach_batch on the ladder's
    copies at 2^-50, 1 and 2^28 (sample powers from 2^-80 to 2^76 through the detector), in both soft modes: flags, amp and TOA do
    not depend on the mode, the copies of a burst are detected alike, and the outputs are the direct call's on the detected bursts
    with the detector's amp and TOA, byte for byte, and the model's; zeros (window word 2) on the others."""
    import torch
    f = ef.ladder(kernel, sps, ks=(-50, 0, 28))
    B = ef.nbursts(f)
    assert B == 9
    t = ctx[sps]
    two = kernel in ("div", "irc")
    first = None
    refs = []                                                  # the detector's own call, antenna by antenna
    for xk, ok in ef.antennas(f):
        ref = GpuBatch(f[xk], f[ok], f["length"])
        if kernel == "access":
            t.detect_demod_rach(ref.x, ref.off, ref.len, ref.flags, ref.amp, ref.toa, ref.soft, avgpwr=ref.pwr, energy_thresh=-1.0)
        else:
            t.detect_demod_normal(ref.x, ref.off, ref.len, f["tsc"], ref.flags, ref.amp, ref.toa, ref.soft, avgpwr=ref.pwr, energy_thresh=-1.0)
        refs.append(ref.results())
    try:
        for mode in (pkg.SOFT_EXACT, pkg.SOFT_TOLERANCE):
            t.set_soft_mode(mode)
            gb = GpuBatch(f["x0"] if two else f["x"], f["off0"] if two else f["off"], f["length"], stride=160)
            lead = (2, B) if two else (B,)
            flags = torch.zeros(lead, dtype=torch.uint8, device="cuda:0"); amp = torch.zeros(lead + (2,), dtype=torch.float32, device="cuda:0")
            toa = torch.zeros(lead, dtype=torch.float32, device="cuda:0")
            chan = torch.zeros((B, 2 if two else 1, 5, 2), dtype=torch.float32, device="cuda:0"); win = torch.zeros(B, dtype=torch.int32, device="cuda:0")
            sel = torch.full((B,), 9, dtype=torch.uint8, device="cuda:0"); cov = torch.full((B, 4), -5.0, dtype=torch.float32, device="cuda:0")
            kw = dict(chan=chan, win=win, hard=gb.hard, energy_thresh=-1.0, soft_stride=160)
            if kernel == "mlse":
                t.mlse_normal(gb.x, gb.off, gb.len, f["tsc"], flags, amp, toa, gb.soft, **kw)
            elif kernel == "access":
                t.mlse_rach(gb.x, gb.off, gb.len, flags, amp, toa, gb.soft, **kw)
            elif kernel == "div":
                t.mlse_div_normal(gb.x, gb.off, dev(f["x1"]), dev(f["off1"]), gb.len, f["tsc"], flags, amp, toa, sel, gb.soft, **kw)
            else:
                t.mlse_irc_normal(gb.x, gb.off, dev(f["x1"]), dev(f["off1"]), gb.len, f["tsc"], flags, amp, toa, sel, gb.soft, cov=cov, **kw)
            r = gb.results()
            got = dict(soft=r["soft"], hard=r["hard"], win=win.cpu().numpy())
            got["chan"] = chan.cpu().numpy().reshape(B, 2, 10).view(np.complex64) if two else chan.cpu().numpy().reshape(B, 10).view(np.complex64)
            if kernel == "irc":
                got["cov"] = cov.cpu().numpy()
            det = (flags.cpu().numpy() & pkg.F_DETECT) != 0
            h_amp = amp.cpu().numpy().reshape(lead + (2,)).view(np.complex64).reshape(lead); h_toa = toa.cpu().numpy()
            if two:
                s = sel.cpu().numpy()
                pick = (s == 1).astype(np.uint8)
                fd = dict(f, amp=h_amp[pick, np.arange(B)], toa=h_toa[pick, np.arange(B)], primary=pick)
                on = (s < 2).astype(np.uint8)
                assert np.array_equal(det[pick, np.arange(B)], on != 0)
            else:
                fd = dict(f, amp=h_amp, toa=h_toa)
                on = det.astype(np.uint8)
            # (the detector is the reference's and has its own floor: like analyzeTrafficBurst and detectRACHBurst on the CPU it finds
            #  nothing in the copies at 2^-50, which are therefore the skipped rows here)
            assert on[f["k"] == 0].any() and on[f["k"] == 28].any() and not on.all(), on
            for a, r0 in enumerate(refs):
                assert (flags[a] if two else flags).cpu().numpy().tobytes() == r0["flags"].tobytes(), "mode %d antenna %d: flags" % (mode, a)
                assert (amp[a] if two else amp).cpu().numpy().tobytes() == r0["amp"].tobytes(), "mode %d antenna %d: amp" % (mode, a)
                assert (toa[a] if two else toa).cpu().numpy().tobytes() == r0["toa"].tobytes(), "mode %d antenna %d: toa" % (mode, a)
            head = dict(flags=flags.cpu().numpy(), amp=amp.cpu().numpy(), toa=h_toa, sel=sel.cpu().numpy())
            if first is None:
                first = head
            for key in head:
                assert head[key].tobytes() == first[key].tobytes(), "mode %d: %s differs from the exact mode's" % (mode, key)
            direct = RUN[kernel](t, fd, enable=on)
            for key in got:
                assert got[key].tobytes() == direct[key].tobytes(), "mode %d: %s differs from the direct call" % (mode, key)
            check(got, ef.model(fd, enable=on), what="%s sps %d batch entry, mode %d" % (kernel, sps, mode))
            assert np.all(got["win"][on != 0] <= 0) and np.all(got["win"][on == 0] == 2)
    finally:
        t.set_soft_mode(pkg.SOFT_EXACT)
