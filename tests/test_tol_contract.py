"""The parity contract for TRXSIG_SOFT_TOLERANCE soft bits -- |soft' - soft| <= 1e-6 or <= 1e-4 |soft| -- on the CPU, through the
correctly rounded restatement of the fast form (oracle/tol_oracle.c) against the reference restatement (oracle so_demodulate):
  * realistic families (synth bursts, sigma 0 .. 2 and the config-2 SNRs, amplitude scaled so that Z covers (0, ZMAX], every TOA
    fraction, sps 1 / 2 / 4): every value of every burst the fast form takes keeps the contract and the 9.2e-6 Z guarantee;
  * the adversarial family (tests/tol_family.py): the same, at Z up to ZMAX;
  * sharpness: at Z up to 8 (the former ZMAX) the same family breaks the contract -- it can catch what it is meant to catch;
  * coverage: the config-2 batch still takes the fast form (>= 95% of detected bursts).
The GPU kernel is held bit for bit to the restatement in tests/test_gpu_soft_tolerance.py."""
import os
import re

import numpy as np
import pytest

import _pkg
import oraclebind
import synth
import tol_family as tf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pkg():
    return _pkg.load()


def tables(pkg, sps):
    return pkg.build_tables_host(sps).view(pkg.tables_dtype())[0]


def test_zmax_is_the_kernels():
    src = open(os.path.join(ROOT, "openbts-ttsou_amd", "csrc", "trxsig_demod.h")).read()
    m = re.search(r"#define\s+TRX_TOL_ZMAX\s+([0-9.]+)f", src)
    assert m and float(m.group(1)) == tf.ZMAX


def grade_taken(pkg, sps, x, off, length, amp, toa, zmax, what):
    """Restatement vs reference on the bursts the fast form takes; returns (ratios, errors, ref, taken mask, Z)."""
    T = tables(pkg, sps)
    verdict, soft = oraclebind.demod_tol(T, x, off, length, amp, toa, zmax)
    ref = oraclebind.Oracle(sps).demod_batch(x, off, length, amp, toa, nthreads=8)
    assert not (verdict == oraclebind.TOL_NOT_DEMODULATED).any(), what
    taken = verdict == oraclebind.TOL_TAKEN
    Z = tf.z_of(x, off, length, amp).astype(np.float64)
    assert np.all(Z[taken] <= zmax), what
    s, r = soft[taken].astype(np.float64), ref[taken].astype(np.float64)
    # hard bits: the guard makes them the reference's
    assert np.array_equal(s > 0.5, r > 0.5), what
    err = np.abs(s - r)
    assert np.all(err <= tf.GUARANTEE * Z[taken][:, None] + 1e-12), (what, (err / Z[taken][:, None]).max())
    return tf.contract_ratio(s, r), err, r, taken, Z


REALISTIC = [(0.0,), (0.1,), (0.3,), (1.0,), (2.0,), (0.0, 0.1, 0.316)]      # the last: config 2 (SNR inf / 20 / 10 dB)


@pytest.mark.parametrize("sps", [1, 2, 4])
@pytest.mark.parametrize("sigmas", REALISTIC)
def test_realistic_families_keep_the_contract(pkg, sps, sigmas):
    B = 1024 if max(sigmas) < 1 else 4096
    x, off, length, amp, toa = tf.realistic_batch(sps, B, seed=int(100 * sum(sigmas)) + sps, sigmas=sigmas)
    ratio, err, ref, taken, Z = grade_taken(pkg, sps, x, off, length, amp, toa, tf.ZMAX, "sigma %s" % (sigmas,))
    worst = float(ratio.max(initial=0.0))
    print("sps %d sigma %s: %d of %d bursts taken, Z up to %.2f, worst err / allowance %.3f, worst err %.3g"
          % (sps, sigmas, taken.sum(), len(taken), Z[taken].max(initial=0.0), worst, err.max(initial=0.0)))
    assert worst <= 1.0, worst
    # the family does reach the fast form, and does reach up to ZMAX
    if max(sigmas) <= 0.316:
        assert taken.mean() > 0.9 and Z[taken].max() > 0.9 * tf.ZMAX, (taken.mean(), Z[taken].max())
    else:
        assert taken.sum() > 100, taken.sum()                 # (few bursts at sigma 2 are detected at all)
    # and every TOA fraction occurs among the taken bursts (k_demod filters from f = 6 / 512 on)
    f = np.round((-toa[taken] - np.floor(-toa[taken])) * 512).astype(int)
    assert len(np.unique(f)) > min(200, taken.sum() // 2)


def adversarial(pkg, sps, zmax, bursts):
    T = tables(pkg, sps)
    x, off, length, amp, toa, steered = tf.adversarial_batch(T, sps, bursts, zmax, seed=2024 + sps)
    ratio, err, ref, taken, Z = grade_taken(pkg, sps, x, off, length, amp, toa, zmax, "adversarial sps %d" % sps)
    low = ref < 0.01
    st = steered[taken]
    assert st.sum() > 10000 and np.all(ref[st] < 0.0101), st.sum()   # the steering did put these outputs in the low band
    return ratio, err, low, taken


@pytest.mark.parametrize("sps", [1, 2, 4])
def test_adversarial_family_keeps_the_contract(pkg, sps):
    ratio, err, low, taken = adversarial(pkg, sps, tf.ZMAX, 3000 * 4 // sps)
    print("sps %d: %d bursts taken, %d low-band values, worst low-band err %.3g, worst err / allowance %.3f"
          % (sps, taken.sum(), low.sum(), err[low].max(), ratio.max()))
    assert taken.mean() > 0.8
    assert ratio.max() <= 1.0, ratio.max()


def test_adversarial_family_is_sharp(pkg):
    """With the former ZMAX (8), the same seeded family contains values outside the contract: it can fail a kernel."""
    bad = 0
    for sps in (1, 2, 4):
        ratio, err, low, taken = adversarial(pkg, sps, 8.0, 3000 * 4 // sps)
        bad += int((ratio > 1.0).sum())
    assert bad >= 1, bad


def test_config2_batch_takes_the_fast_form(pkg):
    """Lowering ZMAX must not switch the mode off: on the config-2 batch (sps 4, SNR >= 10 dB) the detected bursts take it."""
    sps, tsc = 4, 2
    x, off, length, _ = synth.normal_batch(sps, 4096, tsc, seed=77, sigmas=(0.0, 0.1, 0.316))
    ok, amp, toa, _ = oraclebind.Oracle(sps).normal_batch(x, off, length, tsc, nsoft=148, nthreads=8)
    ok = ok.astype(bool)
    verdict, _ = oraclebind.demod_tol(tables(pkg, sps), x, off[ok], length[ok], amp[ok], toa[ok], tf.ZMAX)
    frac = float((verdict == oraclebind.TOL_TAKEN).mean())
    print("config-2 batch: %.4f of %d detected bursts take the fast form" % (frac, ok.sum()))
    assert frac >= 0.95, frac


def test_restatement_edges(pkg):
    """The verdicts at the edges the kernel decides on: Z at / one float step above zmax, off-grid TOA, NaN / infinite inputs,
    all-zero samples (the guard), a length k_demod does not take.  (The GPU test holds the kernel to the same verdicts.)"""
    sps = 4
    T = tables(pkg, sps)
    x, off, length, amp, toa, _ = tf.adversarial_batch(T, sps, 8, 2.0, seed=5)
    b = slice(int(off[0]), int(off[0] + length[0]))
    xs = x[b].copy()
    a = np.complex64(amp[0]); t0 = np.float32(toa[0])

    def verdict(xv, av=a, tv=t0, zmax=tf.ZMAX):
        return int(oraclebind.demod_tol(T, xv, np.array([0], np.int32), np.array([len(xv)], np.int32), av, tv, zmax)[0][0])
    assert verdict(xs) == oraclebind.TOL_TAKEN
    z = float(tf.z_of(xs, [0], [len(xs)], [a])[0])
    # Z exactly at zmax is taken, one float step above is not
    assert verdict(xs, zmax=np.float32(z)) == oraclebind.TOL_TAKEN
    assert verdict(xs, zmax=np.nextafter(np.float32(z), np.float32(0))) == oraclebind.TOL_HANDED_OVER
    assert verdict(xs, tv=np.float32(t0 + 1e-4)) == oraclebind.TOL_HANDED_OVER          # off the 1/512 grid
    assert verdict(xs, av=np.complex64(np.nan)) == oraclebind.TOL_HANDED_OVER
    y = xs.copy(); y[300] = complex(0, np.inf)
    assert verdict(y) == oraclebind.TOL_HANDED_OVER
    y = xs.copy(); y[:] = 0
    assert verdict(y) == oraclebind.TOL_HANDED_OVER                                   # every output on the slicer's 0.5
    assert verdict(xs[:-1]) == oraclebind.TOL_NOT_DEMODULATED                         # (not a multiple of sps)
    assert verdict(xs[:91 * sps]) == oraclebind.TOL_NOT_DEMODULATED                   # (too short)
    assert verdict(xs, tv=np.float32(5000.0)) == oraclebind.TOL_NOT_DEMODULATED
