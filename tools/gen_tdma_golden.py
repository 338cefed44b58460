"""Record the GSM 05.02 uplink TDMA mappings the uplink L1 demultiplexer uses (trxsig_l1rx.h) from the reference's
GSM/GSMTDMA.cpp into tests/golden/tdma_uplink.npz, by reading the tables' text (nothing is compiled):

    python tools/gen_tdma_golden.py /path/to/reference [tests/golden/tdma_uplink.npz]

Per mapping: name, repeat length, allowed-slots mask, C0-only flag and the frame list in reverse-mapping order (-1 padded)."""
import os
import re
import sys

import numpy as np

NAMES = (["FACCH_TCHF"] + ["SACCH_TF_T%d" % t for t in range(8)] + ["SDCCH_8_%dU" % s for s in range(8)] +
         ["SACCH_C8_%dU" % s for s in range(8)] + ["SDCCH_4_%dU" % s for s in range(4)] + ["SACCH_C4_%dU" % s for s in range(4)] +
         ["RACHC5"])


def parse(text):
    """{name: (repeat, allowed, c0only, frames)} of every MAKE_TDMA_MAPPING in the file's text."""
    frames = {m.group(1): [int(x) for x in m.group(2).split(",") if x.strip()]
              for m in re.finditer(r"const\s+unsigned\s+(\w+)Frames\[\]\s*=\s*\{([^}]*)\}", text)}
    out = {}
    for m in re.finditer(r"MAKE_TDMA_MAPPING\(\s*(\w+)\s*,\s*\w+\s*,\s*(\w+)\s*,\s*(\w+)\s*,\s*(\w+)\s*,\s*(\w+)\s*,\s*(\d+)\s*\)", text):
        name, _dl, _ul, allowed, c0, rep = m.groups()
        out[name] = (int(rep), int(allowed, 0), c0 == "true", frames[name])
    return out


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
    dst = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(__file__), "..", "tests", "golden", "tdma_uplink.npz")
    with open(os.path.join(ref, "GSM", "GSMTDMA.cpp")) as f:
        np.savez(dst, **tables(f.read()))
    print("wrote", dst)


if __name__ == "__main__":
    main()
