"""The channel plan (openbts-ttsou_amd/csrc/trxsig_plan.h / .cpp), the one place that numbers a plan's channels for every L1
stage.  The module is plain host C++: it is built here with tests/plan_check.cpp by the host compiler under AddressSanitizer +
UBSan and run as a child process (nothing is loaded into Python).  Its answers are compared with the independent Python
statements of the same rules that the GPU suites already trust: tests/l1_demux_model.py (uplink) and tests/l1_msrx_model.py
(downlink), and the recorded mapping tables (tests/golden/tdma_*.npz).  No GPU needed."""
import os
import shutil
import subprocess

import pytest

import l1_demux_model as dm
import l1_msrx_model as mx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "openbts-ttsou_amd", "csrc")
UL, DL = 1, 0                                                    # TRX_PLAN_UL, TRX_PLAN_DL
PLAN2 = [5, 7, 1, 0, 1, 7, 0, 1, 7, 1, 1, 0, 0, 1, 7, 0]         # 2 ARFCNs
PLAN1 = [5, 7, 1, 0, 0, 0, 0, 0]

_DED = ["FACCH_TCHF"] + ["SACCH_TF_T%d" % t for t in range(8)] + \
       ["%s_%d%%s" % (n, s) for n, k in (("SDCCH_8", 8), ("SACCH_C8", 8), ("SDCCH_4", 4), ("SACCH_C4", 4)) for s in range(k)]
NAMES = {UL: [n % "U" if "%" in n else n for n in _DED] + ["RACHC5"],                       # mapping id -> name (trxsig_tdma.h)
         DL: [n % "D" if "%" in n else n for n in _DED] + ["CCCH_0", "CCCH_1", "CCCH_2", "BCCH", "SCH", "FCCH"]}
KINDS = ("FACCH_TCHF", "SACCH_TF", "SDCCH_8", "SACCH_C8", "SDCCH_4", "SACCH_C4", "RACHC5", "CCCH", "BCCH", "SCH", "FCCH")   # TRXSIG_L1_* kinds


def kind_of(name):
    return max(range(len(KINDS)), key=lambda k: (name.startswith(KINDS[k]), len(KINDS[k])))


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    """ask(lines) -> the program's answer lines"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler to build the plan module with")
    exe = str(tmp_path_factory.mktemp("plan") / "plan_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "plan_check.cpp"), os.path.join(CSRC, "trxsig_plan.cpp"), "-o", exe])

    def run(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and not r.stderr, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
        return r.stdout.splitlines()
    return run


@pytest.fixture(scope="module")
def maps():
    return {UL: dm.load_mappings(), DL: mx.load_mappings()}


def test_tables_are_the_recorded_mappings(ask, maps):
    out = ask(["maps"])
    assert out[0] == "selfcheck 1" and out[-1] == "end"
    got = {UL: {}, DL: {}}
    for ln in out[1:-1]:
        w = ln.split()
        got[UL if w[0] == "UL" else DL][int(w[1])] = (int(w[2]), [int(x) for x in w[3:]])
    for d in (UL, DL):
        assert sorted(got[d]) == list(range(len(NAMES[d])))
        for m, name in enumerate(NAMES[d]):
            assert got[d][m] == (maps[d][name].R, maps[d][name].frames), (d, m, name)


@pytest.mark.parametrize("comb", [PLAN2, PLAN1], ids=["two-arfcn", "one-arfcn"])
def test_channel_lists_are_the_models(ask, comb):
    import numpy as np
    A = len(comb) // 8
    out = ask(["plan %d %s" % (A, " ".join(map(str, comb)))])
    assert out[-1] == "end" and "refused" not in out
    c2 = np.array(comb, np.uint8).reshape(A, 8)
    up, down = dm.Model(c2, 0).ch, mx.Model(c2, 0).ch
    want = []
    for tag, d, chans, classes in (("UL", UL, up, (dm.TCH, dm.XCCH, dm.RACH)),
                                   ("DL", DL, down, (mx.TCH, mx.XCCH, mx.CCCH, mx.BCCH, mx.SCH, mx.FCCH))):
        for slot, cls in enumerate(classes):
            for i, c in enumerate(chans[cls]):
                want.append("%s %d %d %d %d %d %d %d" % (tag, slot, i, c.a, c.tn, NAMES[d].index(c.m.name), kind_of(c.m.name), c.sub))
    assert out[:-1] == want
    # the dedicated classes are the same words in both directions: what lets a key set on channel i land on l1rx's channel i
    ded = lambda tag: [ln.split()[1:] for ln in out if ln.startswith(tag) and ln.split()[1] in ("0", "1")]
    assert ded("UL") == ded("DL") and len(ded("UL")) > 0


def test_refusals(ask):
    zero = [0] * 16
    cmds = []
    for at in range(1, 16):                                      # combination V anywhere but (ARFCN 0, TN 0)
        cmds.append("plan 2 " + " ".join(str(5 if i == at else zero[i]) for i in range(16)))
    for k in (2, 3, 4, 6, 8, 255):
        for at in (0, 3, 9):
            cmds.append("plan 2 " + " ".join(str(k if i == at else PLAN2[i]) for i in range(16)))
    cmds += ["plan 0 " + " ".join(map(str, PLAN1)), "plan 65536 " + " ".join(map(str, PLAN1))]
    assert ask(cmds) == ["refused", "end"] * len(cmds)
    assert "refused" not in ask(["plan 2 " + " ".join(map(str, [5] + zero[1:]))])


def test_cell_layout_checks(ask):
    cell, T, A = 4 * 157, 16, 3
    big = 1 << 62
    got = ask(["strides %d %d %d %d %d" % a for a in [
        (T, A, cell, A * cell, cell),                            # packed, slot-major
        (T, A, cell, cell, T * cell),                            # packed, ARFCN-major
        (T, A, cell, A * cell, cell - 1),                        # a stride one sample short of a cell
        (T, A, cell, A * cell - 1, cell),                        # ... of a slot's row
        (T, A, cell, cell - 1, T * cell),
        (T, A, cell, cell, T * cell - 1),
        (1, A, cell, 0, cell),                                   # one slot: its stride is not looked at
        (T, 1, cell, cell, 0),                                   # one column
        (8, 2, cell, big, cell),                                 # 7 * 2^62 overflows int64
        (8, 4, cell, cell, big),                                 # 3 * 2^62 too
        (8, 2, cell, 1 << 56, cell),                             # past 2^58 samples
    ]])
    full = str(T * A * cell)
    assert got == ["1 " + full, "1 " + full, "0 " + str((T - 1) * A * cell + (A - 1) * (cell - 1) + cell),
                   "0 " + str((T - 1) * (A * cell - 1) + (A - 1) * cell + cell), "0 " + str((T - 1) * (cell - 1) + (A - 1) * T * cell + cell),
                   "0 " + str((T - 1) * cell + (A - 1) * (T * cell - 1) + cell),
                   "1 " + str(A * cell), "1 " + str(T * cell), "1 -", "1 -", "1 -"]           # refused by extent alone
    p = 1 << 20
    assert ask(["overlap %d 10 %d 5" % (p, p + 80), "overlap %d 5 %d 10" % (p + 80, p),      # end to start: apart
                "overlap %d 11 %d 5" % (p, p + 80), "overlap %d 5 %d 11" % (p + 80, p),      # one sample shared
                "overlap %d 10 %d 10" % (p, p), "overlap %d 100 %d 1" % (p, p + 8 * 50)]) == ["0", "0", "1", "1", "1", "1"]


def test_block_geometry_against_the_mappings(ask, maps):
    """Positions counted from the models' Mapping classes: p(u) numbers a mapping's bursts in time order from the one at its
    first listed frame; a call's blocks are groups of four positions."""
    def below(M, u):                                             # the mapping's bursts in frames [0, u)
        return (u // M.R) * len(M.frames) + sum(M.reverse(v) >= 0 for v in range(u % M.R))
    cases = [(d, m, fn, F) for d in (UL, DL) for m in range(len(NAMES[d])) for fn in (0, 1, 50, 51, 101, 103, 2715647)
             for F in (1, 8, 51, 104)]
    got = ask(["geom %d %d %d %d" % c for c in cases])
    assert len(got) == len(cases)
    for (d, m, fn, F), ln in zip(cases, got):
        M = maps[d][NAMES[d][m]]
        p0, p1 = below(M, fn) - below(M, M.frames[0]), below(M, fn + F) - below(M, M.frames[0])
        assert p1 - p0 == sum(M.reverse(u) >= 0 for u in range(fn, fn + F))
        base = p0 - (below(M, fn) - below(M, fn - fn % M.R))
        touched = len({q // 4 for q in range(p0, p1)})           # the receivers' count
        started = sum(q % 4 == 0 for q in range(p0, p1))         # the transmitters' count
        assert [int(x) for x in ln.split()] == [p0, p1, base, touched, started], (d, NAMES[d][m], fn, F)


def test_transmit_geometry_against_a_frame_by_frame_count(ask):
    """trx_plan_tx_geometry, the one geometry function of the two transmit multiplexers, for both directions on the smallest plan
    that uses every mapping (combinations I, V and VII on two ARFCNs): plan_check.cpp counts p_first, p_end, base, nb and unit0
    frame by frame with trx_map_count / trx_map_frame and checks that frame fn + k lands on base + n * Q + cnt[rem]."""
    cases = [(d, fn, F) for d in (UL, DL) for fn in (0, 25, 50, 101, 103, 5303, 2715648 - 1) for F in (1, 3, 4, 51, 104)]
    got = ask(["txgeom %d %d %d 2 %s" % (d, fn, F, " ".join(map(str, PLAN2))) for d, fn, F in cases])
    assert got == ["ok"] * len(cases), [(c, g) for c, g in zip(cases, got) if g != "ok"]


def test_encode_power_on_the_host(ask):
    """trx_encode_power (trxsig_tdma.h), the one copy the kernels and the host share: every band, power -5..45 dBm, against the
    rule written out in plan_check.cpp -- nearest code, first on ties, an exact match at once."""
    assert ask(["power"]) == ["ok"]


def test_stated_once():
    """The placement rule, the channel word's packing and the cell-layout rule are each written in one file of csrc/, and the
    256-byte rounding is one function (trx_align256: no stage file keeps a copy under the old name)."""
    src = {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".h", ".cpp"))}
    where = lambda text: [f for f, s in src.items() if text in s]
    assert where("k == 5 && a == 0 && tn == 0") == ["trxsig_plan.cpp"]
    assert where("tn << 16 | m << 20") == ["trxsig_plan.cpp"]
    assert where("bool strides_ok(") == ["trxsig_plan.h"]
    assert where("size_t trx_align256(") == ["trxsig_ctx.h"] and where("size_t al(") == []
    # what the two transmit multiplexers share is written once: the SACCH rule and encodePower (host and device), the training
    # sequences, the XCCH inverse interleaver, the position arithmetic, the last-two-blocks scan and the launch slicing
    assert where("m >= TRX_MAP_SACCH_C8 && m < TRX_MAP_SDCCH4") == ["trxsig_tdma.h"] and where("minErr = e") == ["trxsig_tdma.h"]
    assert where('"00100101110000100010010111"') == ["trxsig_bursts.h"]
    for text in ("xinv[c & 3][", "c.r26 + k", "x &= x - 1) { L2 = L;", "kMaxWg = "):
        assert where(text) == ["trxsig_l1mux_dev.h"], text
    host = lambda text: [f for f in where(text) if not f.endswith(".hip")]                  # the host's one copy of the tables
    assert host("TRX_TDMA_MAPS_INIT") == ["trxsig_plan.cpp", "trxsig_tdma.h"]
    assert host("TRX_TDMA_DL_MAPS_INIT") == ["trxsig_plan.cpp", "trxsig_tdma.h"]
