"""Record the GSM 05.02 downlink TDMA mappings the downlink L1 multiplexer uses (trxsig_l1tx.h) from the reference's
GSM/GSMTDMA.cpp into tests/golden/tdma_downlink.npz, by reading the tables' text (nothing is compiled):

    python tools/gen_tdma_downlink_golden.py /path/to/reference [tests/golden/tdma_downlink.npz]

Same layout as tools/gen_tdma_golden.py's tdma_uplink.npz (which this leaves as it is): per mapping name, repeat length,
allowed-slots mask, C0-only flag and the frame list in reverse-mapping order (-1 padded)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_tdma_golden import parse  # noqa: E402

NAMES = (["FACCH_TCHF"] + ["SACCH_TF_T%d" % t for t in range(8)] + ["SDCCH_8_%dD" % s for s in range(8)] +
         ["SACCH_C8_%dD" % s for s in range(8)] + ["SDCCH_4_%dD" % s for s in range(4)] + ["SACCH_C4_%dD" % s for s in range(4)] +
         ["CCCH_%d" % s for s in range(3)] + ["BCCH", "SCH", "FCCH"])


def tables(text):
    t = parse(text)
    width = max(len(t[n][3]) for n in NAMES)
    fr = np.full((len(NAMES), width), -1, np.int32)
    for i, n in enumerate(NAMES):
        fr[i, :len(t[n][3])] = t[n][3]
    return dict(names=np.array(NAMES), repeat=np.array([t[n][0] for n in NAMES], np.int32),
                allowed=np.array([t[n][1] for n in NAMES], np.int32), c0only=np.array([t[n][2] for n in NAMES], np.uint8),
                nframes=np.array([len(t[n][3]) for n in NAMES], np.int32), frames=fr)


def main():
    ref = sys.argv[1]
    dst = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(__file__), "..", "tests", "golden", "tdma_downlink.npz")
    with open(os.path.join(ref, "GSM", "GSMTDMA.cpp")) as f:
        np.savez(dst, **tables(f.read()))
    print("wrote", dst)


if __name__ == "__main__":
    main()
