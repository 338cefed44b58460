"""bench.py --dump-outputs: the outputs of the last timed step as <name>.npy in float32 / float64, at most 64 MB in all (a
seeded sample of rows beyond that), the same from run to run -- and, on the GPU, what the timed path really computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_sizes_types_and_sample(tmp_path):
    import torch
    sys.path.insert(0, ROOT)
    import bench
    g = torch.Generator().manual_seed(7)
    B = 65536
    small = {"flags": torch.randint(0, 8, (B,), dtype=torch.uint8, generator=g), "amp": torch.randn(B, 2, generator=g),
             "toa": torch.randn(B, generator=g), "soft": torch.rand(B, 148, generator=g), "idx": torch.arange(B, dtype=torch.int32)}
    info = bench.dump_outputs(str(tmp_path / "a"), small)
    assert info["sampled_rows"] is None
    for k, v in small.items():
        a = np.load(tmp_path / "a" / (k + ".npy"))
        assert a.dtype == (np.float64 if k == "idx" else np.float32)
        assert np.array_equal(a, v.numpy())
    big = {k: torch.cat([v, v, v]) for k, v in small.items()}           # 3 x 40 MB: sampled
    big["idx"] = torch.arange(3 * B, dtype=torch.int32)                 # (each row's index)
    for d in ("b", "c"):
        info = bench.dump_outputs(str(tmp_path / d), big)
        assert info["rows"] == 3 * B and 0 < info["sampled_rows"] < 3 * B
    assert sum(os.path.getsize(tmp_path / "b" / f) for f in os.listdir(tmp_path / "b")) <= 64 << 20
    rows = np.load(tmp_path / "b" / "idx.npy").astype(np.int64)
    assert rows.size == info["sampled_rows"] and np.all(np.diff(rows) > 0) and 0 <= rows[0] and rows[-1] < 3 * B
    for k in big:                                                       # the same rows of every array, run after run
        b, c = np.load(tmp_path / "b" / (k + ".npy")), np.load(tmp_path / "c" / (k + ".npy"))
        assert np.array_equal(b, c) and np.array_equal(b, big[k].numpy()[rows]), k


@pytest.mark.gpu
def test_dumped_outputs_are_the_hot_paths(tmp_path):
    """Two short bench runs with different --steps dump the same arrays, and they are the detector's results for the bench's
    seeded batch: flags, amplitudes and TOAs equal to the CPU oracle's, soft bits within the tolerance mode's bound."""
    B = 4096
    outs = []
    for steps in (3, 8):
        d = tmp_path / ("s%d" % steps)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
                            "--bursts", str(B), "--no-cpu-baseline", "--no-fresh", "--no-lever", "--dump-outputs", str(d)],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
        assert line["steps"] == steps and line["dumped_outputs"]["sampled_rows"] is None
        outs.append({k: np.load(d / (k + ".npy")) for k in ("flags", "amp", "toa", "soft")})
    for k in outs[0]:
        assert outs[0][k].dtype == np.float32 and np.array_equal(outs[0][k], outs[1][k]), k
    import torch
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import _pkg
    import oraclebind
    pkg = _pkg.load()
    from openbts_ttsou_amd import synth
    x, off, length, _ = synth.normal_batch_torch(4, B, 2, seed=0xB5E55ED0, device=torch.device("cuda:0"))   # bench.py's batch, rank 0
    ok, amp, toa, soft = oraclebind.Oracle(4).normal_batch(x.cpu().numpy(), off.cpu().numpy(), length.cpu().numpy(), 2, nthreads=4)
    got = outs[0]
    assert np.array_equal((got["flags"].astype(np.uint8) & pkg.F_DETECT) != 0, ok.astype(bool))
    assert np.array_equal(got["amp"].view(np.complex64).ravel(), amp) and np.array_equal(got["toa"], toa)
    assert np.array_equal(got["soft"] > 0.5, soft > 0.5) and np.abs(got["soft"].astype(np.float64) - soft).max() <= 7.4e-5
