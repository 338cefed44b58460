"""What the GPU tests of the sequence-equaliser kernels share (tests/test_gpu_mlse*.py, test_gpu_sch_fit.py,
test_gpu_l1acq_mlse.py): the `pkg` and `ctx` fixtures (a test module imports them by name), host arrays onto the device, the
canaried output buffers, the direct call of each kernel -- a family dict onto the device, one launch, the outputs back as numpy
arrays -- and the comparison of such outputs with a model's.  The output rows are filled with canaries first (soft -1, hard 255,
taps -7, window -99, set -5 with a guard row behind the batch)."""
import numpy as np
import pytest

import _pkg
import mlse_irc_model as im
from util import GpuBatch, assert_veq, assert_veq_nan

F = np.float32
ANTENNAS = {"mlse": 1, "access": 1, "sch": 1, "div": 2, "irc": 2}


@pytest.fixture(scope="module")
def pkg():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _pkg.load()


@pytest.fixture(scope="module")
def ctx(pkg):
    c = {s: pkg.TrxSig(s, 0) for s in (1, 2, 4)}
    for v in c.values():
        v.use_torch_stream()
    return c


def dev(a):
    """A host array on the device (complex64 as its float32 words)."""
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.float32).copy() if a.dtype == np.complex64 else a.copy()).cuda()


def dev_c(a):
    """A complex array on the device as float32 [..., 2]."""
    return dev(np.ascontiguousarray(a, np.complex64).view(np.float32).reshape(np.shape(a) + (2,)))


def canaries(B, shape=(5,), pad=0, cov=False):
    """The canaried outputs beside the soft and hard rows: dict(chan [B + pad, *shape, 2] of -7, win [B + pad] of -99; cov: and
    cov [B + 1, 4] of -5, the last a guard row)."""
    import torch
    out = dict(chan=torch.full((B + pad,) + tuple(shape) + (2,), -7.0, dtype=torch.float32, device="cuda:0"),
               win=torch.full((B + pad,), -99, dtype=torch.int32, device="cuda:0"))
    if cov:
        out["cov"] = torch.full((B + 1, 4), -5.0, dtype=torch.float32, device="cuda:0")
    return out


def fetched(aux, B):
    """canaries()' tensors on the host: chan as complex64 [B, *shape], win, cov [B, 4] with its guard row checked."""
    chan = aux["chan"].cpu().numpy()
    out = dict(chan=chan.reshape(chan.shape[:-2] + (2 * chan.shape[-2],)).view(np.complex64), win=aux["win"].cpu().numpy())
    if "cov" in aux:
        c = aux["cov"].cpu().numpy()
        assert np.all(c[B] == -5.0), "d_cov written past the batch"
        out["cov"] = c[:B]
    return out


def run(kernel, t, f, sel=None, enable=None, primary="own", nsoft=148, stride=160, with_aux=True, with_hard=True, loading=im.LOADING,
        cov_in=None, guard=0):
    """trxsig_mlse_batch / _div_ / _irc_ / _access_ / _sch_batch (kernel: "mlse", "div", "irc", "access", "sch") on bursts `sel` of
    family f: dict(soft [B, stride], hard, and with_aux: chan [B, 5] or [B, 2, 5], win [B], cov [B, 4] (irc)).  guard: the sample
    tensors are VIEWS starting `guard` samples inside their allocations (the offsets count from the view): a kernel that read a
    burst at offset -1 would stay inside the buffer."""
    two = ANTENNAS[kernel] == 2
    keys = (("x0", "off0"), ("x1", "off1")) if two else (("x", "off"),)
    sel = np.arange(len(f[keys[0][1]])) if sel is None else np.asarray(sel)
    B = len(sel)
    xs, offs = [], []
    for xk, ok in keys:
        off = f[ok][sel].astype(np.int32)
        assert np.all(off[off >= 0] >= guard)
        off[off >= 0] -= guard
        xs.append(dev(np.ascontiguousarray(f[xk], np.complex64))[2 * guard:]); offs.append(dev(off))
        assert xs[-1].storage_offset() == 2 * guard
    gb = GpuBatch(np.zeros(1, np.complex64), np.zeros(B, np.int32), f["length"][sel], nsoft=nsoft, stride=stride)      # (for the lengths and the rows)
    d_amp, d_toa = dev(f["amp"][sel]), dev(f["toa"][sel])
    aux = canaries(B, (2, 5) if two else (5,), cov=kernel == "irc") if with_aux else {}
    kw = dict(aux, enable=None if enable is None else dev(np.asarray(enable, np.uint8)[sel]), hard=gb.hard if with_hard else None, nsoft=nsoft,
              soft_stride=stride)
    if two:
        prim = f["primary"] if isinstance(primary, str) else primary
        kw["primary"] = None if prim is None else dev(np.asarray(prim, np.uint8)[sel])
        if kernel == "irc":
            kw.update(loading=loading, cov_in=None if cov_in is None else dev(np.asarray(cov_in, F)[sel]))
        getattr(t, "mlse_" + kernel)(xs[0], offs[0], xs[1], offs[1], gb.len, f["tsc"], d_amp, d_toa, gb.soft, **kw)
    elif kernel == "mlse":
        t.mlse(xs[0], offs[0], gb.len, f["tsc"], d_amp, d_toa, gb.soft, **kw)
    else:
        getattr(t, "mlse_" + kernel)(xs[0], offs[0], gb.len, d_amp, d_toa, gb.soft, **kw)
    r = gb.results()
    return dict(fetched(aux, B) if with_aux else {}, soft=r["soft"], hard=r["hard"])


def run_mlse(t, f, sel=None, enable=None, nsoft=148, stride=160, with_aux=True):
    """trxsig_mlse_batch on bursts `sel` of family f: dict(soft [B, stride], hard, chan [B, 5], win [B])."""
    return run("mlse", t, f, sel, enable, nsoft=nsoft, stride=stride, with_aux=with_aux)


def run_div(t, f, sel=None, enable=None, primary="own", nsoft=148, stride=160, with_aux=True):
    """trxsig_mlse_div_batch on bursts `sel` of two-antenna family f: dict(soft [B, stride], hard, chan [B, 2, 5], win [B])."""
    return run("div", t, f, sel, enable, primary, nsoft, stride, with_aux)


def run_irc(t, f, sel=None, enable=None, primary="own", nsoft=148, stride=160, with_aux=True, loading=im.LOADING, cov_in=None, div=False):
    """trxsig_mlse_irc_batch (div: trxsig_mlse_div_batch) on bursts `sel` of two-antenna family f: dict(soft [B, stride], hard, chan
    [B, 2, 5], win [B], cov [B, 4])."""
    return run("div" if div else "irc", t, f, sel, enable, primary, nsoft, stride, with_aux, loading=loading, cov_in=cov_in)


def run_access(t, f, sel=None, enable=None, nsoft=148, stride=160, with_aux=True, with_hard=True):
    """trxsig_mlse_access_batch on bursts `sel` of family f: dict(soft [B, stride], hard, chan [B, 5], win [B])."""
    return run("access", t, f, sel, enable, nsoft=nsoft, stride=stride, with_aux=with_aux, with_hard=with_hard)


def run_sch(t, f, sel=None, enable=None, nsoft=148, stride=160, with_aux=True, with_hard=True):
    """trxsig_mlse_sch_batch on bursts `sel` of family f: dict(soft [B, stride], hard, chan [B, 5], win [B])."""
    return run("sch", t, f, sel, enable, nsoft=nsoft, stride=stride, with_aux=with_aux, with_hard=with_hard)


def run_fit(t, f, sel=None, enable=None, only=None, pad=5):
    """trxsig_sch_fit_batch on bursts `sel` of family f: dict(chan9 [B, 9], win, E, R, q [B]) and the canaries checked: `pad` entries
    behind each output.  only: the one output to pass (the others NULL)."""
    import torch
    sel = np.arange(len(f["off"])) if sel is None else np.asarray(sel)
    B = len(sel)
    gb = GpuBatch(f["x"], f["off"][sel], f["length"][sel], nsoft=148, stride=148)
    aux = canaries(B, (9,), pad=pad)
    buf = dict(chan9=aux["chan"], win=aux["win"])
    for k in ("E", "R", "q"):
        buf[k] = torch.full((B + pad,), -7.0, dtype=torch.float32, device="cuda:0")
    args = {k: (v if only is None or k == only else None) for k, v in buf.items()}
    t.sch_fit(gb.x, gb.off, gb.len, dev(f["amp"][sel]), dev(f["toa"][sel]), enable=None if enable is None else dev(enable[sel]), **args)
    t.synchronize()
    out = {k: v.cpu().numpy() for k, v in buf.items()}
    out["chan9"] = out["chan9"].reshape(B + pad, 18).view(np.complex64)
    for k, v in out.items():
        canary = -99 if k == "win" else -7.0
        assert np.all(v[B:].view(np.float32 if k == "chan9" else v.dtype) == canary), "written behind the last burst: " + k
        if only is not None and k != only:
            assert np.all(v.view(np.float32 if k == "chan9" else v.dtype) == canary), "a NULL output's neighbour was written: " + k
        out[k] = v[:B]
    return out


def check(got, want, sel=None, nsoft=148, what="", nan_taps=False):
    """The outputs of a run_* against a model's on bursts `sel`, value for value (IEEE ==; NaN against NaN in the soft bits, and in
    the taps where nan_taps), and nothing written past nsoft."""
    sel = slice(None) if sel is None else sel

    def rows(c):
        return c.reshape(len(c), int(np.prod(c.shape[1:])))
    assert_veq(got["win"], want["win"][sel], what + " window word")
    assert_veq_nan(got["soft"][:, :nsoft], want["soft"][sel][:, :nsoft], what + " soft bits")
    assert_veq(got["hard"][:, :nsoft], want["hard"][sel][:, :nsoft], what + " hard bits")
    (assert_veq_nan if nan_taps else assert_veq)(rows(got["chan"]), rows(want["chan"][sel]), what + " taps")
    if "cov" in got:
        assert_veq(got["cov"], want["cov"][sel], what + " set")
    assert np.all(got["soft"][:, nsoft:] == -1.0) and np.all(got["hard"][:, nsoft:] == 255), what + ": written past nsoft"
