"""The direct calls of the four sequence-equaliser kernels for the GPU tests (tests/test_gpu_mlse.py, test_gpu_mlse_div.py,
test_gpu_mlse_irc.py, test_gpu_mlse_access.py, test_gpu_mlse_edge.py): a family dict onto the device, one launch, the outputs back
as numpy arrays.  The output rows are filled with canaries first (soft -1, hard 255, taps -7, window -99, set -5)."""
import numpy as np

import mlse_irc_model as im
from util import GpuBatch

F = np.float32


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.float32).copy() if a.dtype == np.complex64 else a.copy()).cuda()


def run_mlse(t, f, sel=None, enable=None, nsoft=148, stride=160, with_aux=True):
    """trxsig_mlse_batch on bursts `sel` of family f: dict(soft [B, stride], hard, chan [B, 5], win [B])."""
    import torch
    sel = np.arange(len(f["off"])) if sel is None else np.asarray(sel)
    gb = GpuBatch(f["x"], f["off"][sel], f["length"][sel], nsoft=nsoft, stride=stride)
    d_amp = torch.from_numpy(np.ascontiguousarray(f["amp"][sel]).view(np.float32).copy()).cuda()
    d_toa = torch.from_numpy(np.ascontiguousarray(f["toa"][sel])).cuda()
    d_en = None if enable is None else torch.from_numpy(np.ascontiguousarray(enable[sel])).cuda()
    chan = torch.full((len(sel), 5, 2), -7.0, dtype=torch.float32, device="cuda:0") if with_aux else None
    win = torch.full((len(sel),), -99, dtype=torch.int32, device="cuda:0") if with_aux else None
    t.mlse(gb.x, gb.off, gb.len, f["tsc"], d_amp, d_toa, gb.soft, enable=d_en, chan=chan, win=win, hard=gb.hard, nsoft=nsoft,
           soft_stride=stride)
    r = gb.results()
    out = dict(soft=r["soft"], hard=r["hard"])
    if with_aux:
        out["chan"] = chan.cpu().numpy().reshape(len(sel), 10).view(np.complex64)
        out["win"] = win.cpu().numpy()
    return out


def run_div(t, f, sel=None, enable=None, primary="own", nsoft=148, stride=160, with_aux=True):
    """trxsig_mlse_div_batch on bursts `sel` of two-antenna family f: dict(soft [B, stride], hard, chan [B, 2, 5], win [B])."""
    import torch
    sel = np.arange(len(f["off0"])) if sel is None else np.asarray(sel)
    B = len(sel)
    gb = GpuBatch(f["x0"], f["off0"][sel], f["length"][sel], nsoft=nsoft, stride=stride)
    x1, off1 = dev(np.ascontiguousarray(f["x1"], np.complex64)), dev(f["off1"][sel].astype(np.int32))
    d_amp, d_toa = dev(f["amp"][sel]), dev(f["toa"][sel])
    prim = f["primary"] if isinstance(primary, str) else primary
    d_prim = None if prim is None else dev(np.asarray(prim, np.uint8)[sel])
    d_en = None if enable is None else dev(np.asarray(enable, np.uint8)[sel])
    chan = torch.full((B, 2, 5, 2), -7.0, dtype=torch.float32, device="cuda:0") if with_aux else None
    win = torch.full((B,), -99, dtype=torch.int32, device="cuda:0") if with_aux else None
    t.mlse_div(gb.x, gb.off, x1, off1, gb.len, f["tsc"], d_amp, d_toa, gb.soft, primary=d_prim, enable=d_en, chan=chan, win=win,
               hard=gb.hard, nsoft=nsoft, soft_stride=stride)
    r = gb.results()
    out = dict(soft=r["soft"], hard=r["hard"])
    if with_aux:
        out["chan"] = chan.cpu().numpy().reshape(B, 2, 10).view(np.complex64)
        out["win"] = win.cpu().numpy()
    return out


def run_irc(t, f, sel=None, enable=None, primary="own", nsoft=148, stride=160, with_aux=True, loading=im.LOADING, cov_in=None, div=False):
    """trxsig_mlse_irc_batch (div: trxsig_mlse_div_batch) on bursts `sel` of two-antenna family f: dict(soft [B, stride], hard, chan
    [B, 2, 5], win [B], cov [B, 4])."""
    import torch
    sel = np.arange(len(f["off0"])) if sel is None else np.asarray(sel)
    B = len(sel)
    gb = GpuBatch(f["x0"], f["off0"][sel], f["length"][sel], nsoft=nsoft, stride=stride)
    x1, off1 = dev(np.ascontiguousarray(f["x1"], np.complex64)), dev(f["off1"][sel].astype(np.int32))
    d_amp, d_toa = dev(f["amp"][sel]), dev(f["toa"][sel])
    prim = f["primary"] if isinstance(primary, str) else primary
    d_prim = None if prim is None else dev(np.asarray(prim, np.uint8)[sel])
    d_en = None if enable is None else dev(np.asarray(enable, np.uint8)[sel])
    chan = torch.full((B, 2, 5, 2), -7.0, dtype=torch.float32, device="cuda:0") if with_aux else None
    win = torch.full((B,), -99, dtype=torch.int32, device="cuda:0") if with_aux else None
    cov = torch.full((B + 1, 4), -5.0, dtype=torch.float32, device="cuda:0") if with_aux else None      # (a canary row behind)
    if div:
        t.mlse_div(gb.x, gb.off, x1, off1, gb.len, f["tsc"], d_amp, d_toa, gb.soft, primary=d_prim, enable=d_en, chan=chan, win=win,
                   hard=gb.hard, nsoft=nsoft, soft_stride=stride)
    else:
        t.mlse_irc(gb.x, gb.off, x1, off1, gb.len, f["tsc"], d_amp, d_toa, gb.soft, primary=d_prim, enable=d_en, loading=loading,
                   cov_in=None if cov_in is None else dev(np.asarray(cov_in, F)[sel]), cov=cov, chan=chan, win=win, hard=gb.hard, nsoft=nsoft,
                   soft_stride=stride)
    r = gb.results()
    out = dict(soft=r["soft"], hard=r["hard"])
    if with_aux:
        out["chan"] = chan.cpu().numpy().reshape(B, 2, 10).view(np.complex64)
        out["win"] = win.cpu().numpy()
        if not div:
            c = cov.cpu().numpy()
            assert np.all(c[B] == -5.0), "d_cov written past the batch"
            out["cov"] = c[:B]
    return out


def run_access(t, f, sel=None, enable=None, nsoft=148, stride=160, with_aux=True, with_hard=True):
    """trxsig_mlse_access_batch on bursts `sel` of family f: dict(soft [B, stride], hard, chan [B, 5], win [B])."""
    import torch
    sel = np.arange(len(f["off"])) if sel is None else np.asarray(sel)
    gb = GpuBatch(f["x"], f["off"][sel], f["length"][sel], nsoft=nsoft, stride=stride)
    d_amp = torch.from_numpy(np.ascontiguousarray(f["amp"][sel]).view(np.float32).copy()).cuda()
    d_toa = torch.from_numpy(np.ascontiguousarray(f["toa"][sel])).cuda()
    d_en = None if enable is None else torch.from_numpy(np.ascontiguousarray(enable[sel])).cuda()
    chan = torch.full((len(sel), 5, 2), -7.0, dtype=torch.float32, device="cuda:0") if with_aux else None
    win = torch.full((len(sel),), -99, dtype=torch.int32, device="cuda:0") if with_aux else None
    t.mlse_access(gb.x, gb.off, gb.len, d_amp, d_toa, gb.soft, enable=d_en, chan=chan, win=win, hard=gb.hard if with_hard else None,
                  nsoft=nsoft, soft_stride=stride)
    r = gb.results()
    out = dict(soft=r["soft"], hard=r["hard"])
    if with_aux:
        out["chan"] = chan.cpu().numpy().reshape(len(sel), 10).view(np.complex64)
        out["win"] = win.cpu().numpy()
    return out
