"""The model of the hopping stage (include/trxsig_l1hop.h) -- TEST INFRASTRUCTURE ONLY.  The reference never hops, so this file
is what pins the stage: the GSM 05.02 section 6.2.3 sequence in plain integers exactly as the header states it, the plan rules,
and the four operations on numpy arrays.

  mai(fn, hsn, maio, n)        the sequence, one entry, Python integers
  HopModel(comb, group, hsn)   the plan: ValueError where trxsig_l1hop_create returns TRXSIG_EINVAL
    .map(fn, F)                int32 [8 F][A]: the radio row of channel row a in slot t (a itself where the slot does not hop)
    .bits(to_radio, ...)       an encoder's [A][8 F][148] grid and its [A][8 F] map, hopped (copies)
    .cells(to_radio, ...)      sample cells in flat buffers with strides, as trxsig_air_cells addresses them (64-bit words)
    .result(fn, row)           a pull's d_row [8 F][A] in the channel domain
"""
import numpy as np

HYPERFRAME = 2715648
MAX_N = 64
RNTABLE = (
    48, 98, 63, 1, 36, 95, 78, 102, 94, 73, 0, 64, 25, 81, 76, 59, 124, 23, 104, 100,
    101, 47, 118, 85, 18, 56, 96, 86, 54, 2, 80, 34, 127, 13, 6, 89, 57, 103, 12, 74,
    55, 111, 75, 38, 109, 71, 112, 29, 11, 88, 87, 19, 3, 68, 110, 26, 33, 31, 8, 45,
    82, 58, 40, 107, 32, 5, 106, 92, 62, 67, 77, 108, 122, 37, 60, 66, 121, 42, 51, 126,
    117, 114, 4, 90, 43, 52, 53, 113, 120, 72, 16, 49, 7, 79, 119, 61, 22, 84, 9, 97,
    91, 15, 21, 24, 46, 39, 93, 105, 65, 70, 125, 99, 17, 123)


def s_of(fn, hsn, n, took=None):
    """S of (FN, HSN, N): MAI = (S + MAIO) mod N.  took: a list that receives True where the branch M' >= N was taken"""
    fn, hsn, n = int(fn), int(hsn), int(n)
    assert 0 <= fn < HYPERFRAME and 0 <= hsn <= 63 and 1 <= n <= MAX_N
    if hsn == 0:
        return fn % n
    t1r, t2, t3 = (fn // 1326) % 64, fn % 26, fn % 51
    nbin = n.bit_length()                                    # floor(log2 n) + 1
    m = t2 + RNTABLE[(hsn ^ t1r) + t3]
    mp, tp = m % (1 << nbin), t3 % (1 << nbin)
    if took is not None:
        took.append(mp >= n)
    return mp if mp < n else (mp + tp) % n


def mai(fn, hsn, maio, n, took=None):
    assert 0 <= int(maio) < int(n)
    return (s_of(fn, hsn, n, took) + int(maio)) % int(n)


def mai_batch(fn, hsn, maio, n):
    return np.array([mai(*e) for e in zip(fn, hsn, maio, n)], np.int32)


def cell_len(t, sps):
    return (156 + (t % 4 == 0)) * sps


class HopModel:
    def __init__(self, comb, group, hsn):
        comb, group = np.asarray(comb, np.uint8), np.asarray(group, np.int8)
        hsn = np.asarray(hsn, np.int64).reshape(-1)
        if comb.ndim != 2 or comb.shape[1] != 8 or comb.shape != group.shape or comb.shape[0] < 1:
            raise ValueError("shape")
        if (hsn < 0).any() or (hsn > 63).any():
            raise ValueError("HSN outside 0..63")
        self.A, self.G = comb.shape[0], len(hsn)
        self.comb, self.group, self.hsn = comb, group, hsn
        self.mem = {}                                        # (g, tn) -> rows, ascending
        for a in range(self.A):
            for tn in range(8):
                k, g = int(comb[a, tn]), int(group[a, tn])
                if not (k in (0, 1, 7) or (k == 5 and a == 0 and tn == 0)):
                    raise ValueError("combination")
                if g < -1 or g >= self.G:
                    raise ValueError("group id out of range")
                if g < 0:
                    continue
                if k in (0, 5):
                    raise ValueError("an OFF slot or a beacon slot cannot hop")
                rows = self.mem.setdefault((g, tn), [])
                if rows and int(comb[rows[0], tn]) != k:
                    raise ValueError("members differ in their combination")
                rows.append(a)
                if len(rows) > MAX_N:
                    raise ValueError("N > 64")

    def groups(self):
        return self.G

    def members(self, g, tn):
        return list(self.mem.get((g, tn), []))

    def map(self, fn, F):
        out = np.tile(np.arange(self.A, dtype=np.int32), (8 * F, 1))
        for t in range(8 * F):
            fnw, tn = (fn + t // 8) % HYPERFRAME, t % 8
            for (g, gtn), rows in self.mem.items():
                if gtn != tn:
                    continue
                n = len(rows)
                s = s_of(fnw, self.hsn[g], n)
                for r, a in enumerate(rows):
                    out[t, a] = rows[(s + r) % n]            # MAIO = rank; the frequency of index MAI is the row of rank MAI
        return out

    def bits(self, to_radio, fn, F, bits, what=None):
        """-> (bits, what) hopped; what None stays None"""
        bits = np.asarray(bits)
        A, T = self.A, 8 * F
        assert bits.shape[:2] == (A, T)
        radio = self.map(fn, F)                              # [T][A]
        t = np.arange(T)[None, :].repeat(A, 0)               # [A][T]
        a = np.arange(A)[:, None].repeat(T, 1)
        r = radio.T                                          # [A][T]: the radio row of (a, t)
        ob = np.empty_like(bits)
        ow = None if what is None else np.empty_like(what)
        if to_radio:
            ob[r, t] = bits[a, t]
            if ow is not None:
                ow[r, t] = np.asarray(what)[a, t]
        else:
            ob[a, t] = bits[r, t]
            if ow is not None:
                ow[a, t] = np.asarray(what)[r, t]
        return ob, ow

    def cells(self, to_radio, fn, F, src, in_slot, in_arfcn, dst, out_slot, out_arfcn, sps):
        """src, dst: flat arrays of 64-bit words (a complex64 sample each), strides in samples; dst is written in place, only
        inside cells; returns dst"""
        radio = self.map(fn, F)
        for t in range(8 * F):
            n = cell_len(t, sps)
            for a in range(self.A):
                s, d = (a, int(radio[t, a])) if to_radio else (int(radio[t, a]), a)
                i, o = t * in_slot + s * in_arfcn, t * out_slot + d * out_arfcn
                dst[o:o + n] = src[i:i + n]
        return dst

    def result(self, fn, row):
        row = np.asarray(row)
        T, A = row.shape
        assert A == self.A and T % 8 == 0
        radio = self.map(fn, T // 8)
        return np.take_along_axis(row, radio.astype(np.int64), axis=1)


# ---- the plans the tests share ----
def small_plan():
    """7 rows: row 0 has the beacon on TN 0 and a hopping combination VII on TN 1 (N = 3 with rows 2 and 5); N = 1 on TN 2; N = 2 on
    TN 3; two groups on TN 4 (N = 3 and N = 2, one of them group 1 again); row 6 is in no group.  -> (comb, group, hsn)"""
    comb = np.zeros((7, 8), np.uint8)
    group = np.full((7, 8), -1, np.int8)
    comb[0, 0] = 5
    comb[[0, 2, 5], 1] = 7; group[[0, 2, 5], 1] = 0
    comb[3, 2] = 1; group[3, 2] = 1
    comb[[1, 4], 3] = 1; group[[1, 4], 3] = 2
    comb[:6, 4] = 1; group[[0, 1, 3], 4] = 1; group[[2, 5], 4] = 3
    comb[6, 5] = 7; comb[6, 4] = 1
    return comb, group, np.array([5, 0, 63, 17], np.uint8)


def big_plan():
    """66 rows: a 64-member group on TN 3 (NBIN 7, the (M' + T') mod N branch), rows 0 and 65 outside it"""
    comb = np.zeros((66, 8), np.uint8)
    group = np.full((66, 8), -1, np.int8)
    comb[0, 0] = 5
    comb[:, 3] = 1; group[1:65, 3] = 0
    return comb, group, np.array([63], np.uint8)
