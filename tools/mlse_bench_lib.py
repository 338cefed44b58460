"""What the six equaliser bench tools share (tools/mlse_bench.py, mlse_access_bench.py, mlse_sch_bench.py, sch_fit_bench.py,
mlse_div_bench.py, mlse_irc_bench.py): the command line's common part with the HBM-rate step, the sample buffers in rotation and
the event-median loop over them, the echo and the synthetic burst batches, the parts of the two-antenna tools' kernel_times, the
figures' keys and the JSON writer.  Side measurements: nothing is asserted."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
PAYLOAD = np.r_[3:61, 87:145]                                 # a normal burst's payload bits
WINDOWS = (-4, -3, -2, -1, 0, 1, 2)                           # the window words


def parser(out_name, tsc=False):
    """--bursts, --reps, [--tsc,] --hbm-bench / --hbm-tbps, --out profiles/<out_name>; a tool adds its own before parse()."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--bursts", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=30)
    if tsc:
        ap.add_argument("--tsc", type=int, default=2)
    ap.add_argument("--hbm-bench", default=None, help="compiled tools/hbm_bench.hip, run before anything else")
    ap.add_argument("--hbm-tbps", type=float, default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", out_name))
    return ap


def parse(ap):
    """(arguments, sustained HBM read rate in TB/s, where it came from): the rate is measured first, in a process of its own."""
    a = ap.parse_args()
    if (a.hbm_bench is None) == (a.hbm_tbps is None):
        raise SystemExit("give --hbm-bench or --hbm-tbps")
    from air_bench import hbm_rate
    return (a,) + (hbm_rate(a.hbm_bench) if a.hbm_bench else (a.hbm_tbps, "given on the command line"))


def write(out, path):
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


class Rotation:
    """An antenna's (or each of two antennas') samples in n copies, together larger than the memory-side cache, and window(fnc): the
    median, minimum and maximum in us of `reps` HIP-event windows round fnc(k), k the copy whose turn it is."""

    def __init__(self, reps, *antennas):
        self.reps, self.turn = reps, 0
        self.sample_bytes = antennas[0].numel() * 8            # (one antenna's)
        self.n = max(2, (512 << 20) // (len(antennas) * self.sample_bytes) + 1)
        self.xs = [[x] + [x.clone() for _ in range(self.n - 1)] for x in antennas]

    def window(self, fnc):
        import torch
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ts = []
        for _ in range(self.reps):
            self.turn += 1
            ev[0].record(); fnc(self.turn % self.n); ev[1].record(); torch.cuda.synchronize()
            ts.append(ev[0].elapsed_time(ev[1]) * 1000.0)
        return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))

    def timed(self, *fncs):
        """Three warm-up rounds of all of them on copy 0, then a window() each."""
        import torch
        for _ in range(3):
            for f in fncs:
                f(0)
        torch.cuda.synchronize()
        return [self.window(f) for f in fncs]


def us(name, t):
    """A window()'s figures under the tools' keys."""
    return {name + "_us": round(t[0], 1), name + "_min_max_us": [round(t[1], 1), round(t[2], 1)]}


def window_counts(win):
    w = win.cpu().numpy()
    return dict((str(k), int((w == k).sum())) for k in WINDOWS)


def bit_errors(bits, rows, cols):
    """err(soft): hard-bit errors against bits on the bursts `rows` (a mask) and the positions cols."""
    return lambda s: int((((s.cpu().numpy() > 0.5) != bits)[rows][:, cols]).sum())


def echoed(x, late, gain=complex(0.45, -0.3)):
    """x plus its own echo `late` samples on."""
    import torch
    e = torch.zeros_like(x)
    e[late:] = x[:-late] * gain
    return x + e


def echo_bursts_torch(synth, sps, B, seed, fill, max_delay_sym, chunk=8192):
    """B bursts on the device whose 148 bits fill(bits, rand) sets (rand(n) = n columns of random bits): the library's synthetic
    channel (a gain, a delay of 0..max_delay_sym symbols and a fraction, noise sigma 0 / 0.1 / 0.3 in turn) with an echo one
    symbol late: (x, off, length, bits)."""
    import torch
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    sig = torch.tensor((0.0, 0.1, 0.3), dtype=torch.float32, device=dev)
    xs, bits_all = [], []
    for s in range(0, B, chunk):
        n = min(chunk, B - s)
        bits = torch.zeros(n, 148, dtype=torch.uint8, device=dev)
        fill(bits, lambda cols: torch.randint(0, 2, (n, cols), device=dev, generator=gen, dtype=torch.uint8))
        amp = torch.polar(300 + 2700 * torch.rand(n, device=dev, generator=gen), 2 * np.pi * torch.rand(n, device=dev, generator=gen))
        delay = (torch.randint(0, max_delay_sym + 1, (n,), device=dev, generator=gen) * sps).to(torch.float32) + \
            torch.rand(n, device=dev, generator=gen)
        x, _, _ = synth._torch_batch(bits, sps, delay, amp, sig[(torch.arange(n, device=dev) + s) % 3], dev, gen)
        xs.append(x); bits_all.append(bits)
    _, length, off = synth.burst_lengths(B, sps)
    return echoed(torch.cat(xs), sps).contiguous(), torch.from_numpy(off.astype(np.int32)).to(dev), torch.from_numpy(length).to(dev), \
        torch.cat(bits_all)


def one_antenna_buffers(B, n_soft, n_chan):
    """flags, amp, toa, n_soft soft rows, n_chan taps and n_chan window words, all zero on the device."""
    import torch
    z = lambda *shape, ty=torch.float32: torch.zeros(*shape, dtype=ty, device="cuda")
    return z(B, ty=torch.uint8), z(B, 2), z(B), [z(B, 148) for _ in range(n_soft)], [z(B, 5, 2) for _ in range(n_chan)], \
        [z(B, ty=torch.int32) for _ in range(n_chan)]


def one_antenna_head(B, sps, det, rot, tbps, line, **first):
    """(the figures every one-antenna tool starts with, the time one read of the samples takes in us)."""
    floor = rot.sample_bytes / (tbps * 1e12) * 1e6
    return dict(dict(bursts=B, sps=sps, **first), detected=int(det.sum()), sample_bytes=rot.sample_bytes, sample_buffers_in_rotation=rot.n,
                hbm_read_tbps=tbps, hbm_bench_line=line, one_read_of_the_samples_us=round(floor, 1)), floor


class TwoAntennas:
    """kernel_times' common part in the two-antenna tools: the buffers, and once the detect-then-equalise call has filled them the
    selection, the selected amplitudes and TOAs, the enable bytes, the figures the result starts with and the payload's errors."""

    def __init__(self, B):
        import torch
        z = lambda *shape, ty=torch.float32: torch.zeros(*shape, dtype=ty, device="cuda")
        self.flags, self.amp, self.toa, self.sel = z(2, B, ty=torch.uint8), z(2, B, 2), z(2, B), z(B, ty=torch.uint8)
        self.soft = [z(B, 148), z(B, 148)]
        self.chan, self.win = z(B, 2, 5, 2), z(B, ty=torch.int32)

    def select(self):
        import torch
        torch.cuda.synchronize()
        self.both, self.pick = self.sel < 2, self.sel == 1
        self.amp_s = torch.where(self.pick[:, None], self.amp[1], self.amp[0]).contiguous()
        self.toa_s = torch.where(self.pick, self.toa[1], self.toa[0]).contiguous()
        self.en = self.both.to(torch.uint8)

    def head(self, B, sps, tsc, rot, tbps, line):
        """(the figures both tools start with, the time one read of both sample sets takes in us)."""
        floor = 2 * rot.sample_bytes / (tbps * 1e12) * 1e6
        return dict(bursts=B, sps=sps, tsc=tsc, detected_by_either=int(self.both.sum().item()), selected_antenna_1=int(self.pick.sum().item()),
                    sample_bytes_both_antennas=2 * rot.sample_bytes, sample_buffers_in_rotation=rot.n, hbm_read_tbps=tbps, hbm_bench_line=line,
                    one_read_of_both_sample_sets_us=round(floor, 1)), floor

    def errors(self, bits, **soft):
        d = self.both.cpu().numpy()
        err = bit_errors(bits.cpu().numpy(), d, PAYLOAD)
        return dict(dict((k, err(v)) for k, v in soft.items()), of=int(d.sum()) * len(PAYLOAD))
