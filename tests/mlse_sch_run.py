"""The direct call of the synchronisation-burst sequence equaliser for the GPU tests (tests/test_gpu_mlse_sch.py,
test_gpu_mlse_sch_ref.py): a family dict onto the device, one launch, the outputs back as numpy arrays -- tests/mlse_run.py's
run_access for trxsig_mlse_sch_batch.  The output rows are filled with canaries first (soft -1, hard 255, taps -7, window -99)."""
import numpy as np

from util import GpuBatch


def run_sch(t, f, sel=None, enable=None, nsoft=148, stride=160, with_aux=True, with_hard=True):
    """trxsig_mlse_sch_batch on bursts `sel` of family f: dict(soft [B, stride], hard, chan [B, 5], win [B])."""
    import torch
    sel = np.arange(len(f["off"])) if sel is None else np.asarray(sel)
    gb = GpuBatch(f["x"], f["off"][sel], f["length"][sel], nsoft=nsoft, stride=stride)
    d_amp = torch.from_numpy(np.ascontiguousarray(f["amp"][sel]).view(np.float32).copy()).cuda()
    d_toa = torch.from_numpy(np.ascontiguousarray(f["toa"][sel])).cuda()
    d_en = None if enable is None else torch.from_numpy(np.ascontiguousarray(enable[sel])).cuda()
    chan = torch.full((len(sel), 5, 2), -7.0, dtype=torch.float32, device="cuda:0") if with_aux else None
    win = torch.full((len(sel),), -99, dtype=torch.int32, device="cuda:0") if with_aux else None
    t.mlse_sch(gb.x, gb.off, gb.len, d_amp, d_toa, gb.soft, enable=d_en, chan=chan, win=win, hard=gb.hard if with_hard else None,
               nsoft=nsoft, soft_stride=stride)
    r = gb.results()
    out = dict(soft=r["soft"], hard=r["hard"])
    if with_aux:
        out["chan"] = chan.cpu().numpy().reshape(len(sel), 10).view(np.complex64)
        out["win"] = win.cpu().numpy()
    return out
