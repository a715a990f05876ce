"""ConvCode restated in numpy (include/yagi_hip.h, "ConvCode: the definition"; a helper, not a test module), in two
forms that must agree byte for byte: decode_loop walks one frame state by state in plain Python integers, exactly as the
definition is written; decode is vectorised over states and frames and is what the device and the library's host form are
compared with.  Everything is integer arithmetic, so there is no tolerance anywhere."""
import numpy as np

DECISION_BYTES = 131072
STEPS_MAX = 65536
PERIOD_MAX = 32

V27 = (7, (0x6d, 0x4f), None)
V29 = (9, (0x1af, 0x11d), None)
V39 = (9, (0x1ed, 0x19b, 0x127), None)
V27P23 = (7, (0x6d, 0x4f), ((1, 1), (1, 0)))
V27P34 = (7, (0x6d, 0x4f), ((1, 1, 0), (1, 0, 1)))


def parity(v):
    return bin(int(v)).count("1") & 1


class Code:
    def __init__(self, K, g, puncture=None, terminated=True):
        self.K, self.g, self.R, self.terminated = int(K), tuple(int(v) for v in g), len(g), bool(terminated)
        self.S = 1 << (self.K - 1)
        self.P = np.ones((self.R, 1), np.uint8) if puncture is None else np.array(puncture, np.uint8)
        self.puncture = None if puncture is None else self.P
        self.p = self.P.shape[1]
        ns = np.arange(self.S)
        # E[i][r][ns]: the output bit r of the branch from predecessor p_i into ns: parity(((p_i << 1) | b) & g[r])
        sr0, sr1 = ns, ns | (1 << (self.K - 1))             # ((p0 << 1) | b) = ns; p1 = p0 | 2^(K-2) sets the top bit
        self.E = np.array([[[parity(v & gr) for v in sr] for gr in self.g] for sr in (sr0, sr1)], np.int64)

    def steps(self, n):
        return n + (self.K - 1 if self.terminated else 0)

    def kept(self, t):
        """the outputs r kept at step t, in order"""
        return [r for r in range(self.R) if self.P[r, t % self.p]]

    def ncoded(self, n):
        """by loop; the library's closed form is compared with this"""
        return sum(len(self.kept(t)) for t in range(self.steps(n)))

    def nmax(self):
        return min(DECISION_BYTES * 8 // self.S, STEPS_MAX) - (self.K - 1 if self.terminated else 0)

    def args(self):
        """(K, polys, puncture, terminated) for yagi_amd.ConvCode and its host forms"""
        return self.K, self.g, self.puncture, self.terminated


def unpack(msg, n):
    """[F, >= ceil(n / 8)] bytes -> [F, n] bits, most significant bit first"""
    return np.unpackbits(np.asarray(msg, np.uint8)[:, :(n + 7) // 8], axis=1)[:, :n]


def pack(bits):
    return np.packbits(np.asarray(bits, np.uint8), axis=1)   # pads the last byte with zeros


def encode(code, msg, n):
    """msg [F, >= ceil(n / 8)] packed -> coded [F, ncoded(n)] of 0 / 1"""
    bits = unpack(msg, n)
    F, T = bits.shape[0], code.steps(n)
    out, sr = [], np.zeros(F, np.int64)
    for t in range(T):
        b = bits[:, t] if t < n else 0
        sr = ((sr << 1) | b) & ((1 << code.K) - 1)
        for r in code.kept(t):
            v = sr & code.g[r]
            par = np.zeros(F, np.int64)
            for k in range(code.K):
                par ^= (v >> k) & 1
            out.append(par)
    return np.stack(out, 1).astype(np.uint8)


def decode(code, soft, n):
    """soft [F, >= ncoded(n)] -> (msg [F, ceil(n / 8)] packed, metric [F] uint32); vectorised over states and frames"""
    soft = np.asarray(soft, np.uint8).astype(np.int64)
    F, T, S, K = soft.shape[0], code.steps(n), code.S, code.K
    ns = np.arange(S)
    p0 = ns >> 1
    p1 = p0 | (1 << (K - 2))
    pm = np.full((F, S), 1 << 30, np.int64)
    pm[:, 0] = 0
    dec = np.zeros((T, F, S), bool)
    rd = 0
    for t in range(T):
        c0 = np.zeros((F, S), np.int64)
        c1 = np.zeros((F, S), np.int64)
        for r in code.kept(t):
            s = soft[:, rd, None]
            rd += 1
            c0 += np.where(code.E[0][r][None, :] == 1, 255 - s, s)
            c1 += np.where(code.E[1][r][None, :] == 1, 255 - s, s)
        m0, m1 = pm[:, p0] + c0, pm[:, p1] + c1
        dec[t] = m1 < m0                                    # strict: a tie keeps p0
        pm = np.where(dec[t], m1, m0)
    assert pm.max() < 1 << 31
    e = np.zeros(F, np.int64) if code.terminated else np.argmin(pm, axis=1)    # argmin: the lowest index on a tie
    metric = pm[np.arange(F), e].astype(np.uint32)
    bits = np.zeros((F, T), np.uint8)
    fr = np.arange(F)
    for t in range(T - 1, -1, -1):
        bits[:, t] = e & 1
        e = (e >> 1) | (dec[t, fr, e].astype(np.int64) << (K - 2))
    return pack(bits[:, :n]), metric


def decode_loop(code, soft, n):
    """one frame, state by state in Python integers, as the definition reads -> (packed bytes, metric)"""
    soft = [int(v) for v in soft]
    T, S, K = code.steps(n), code.S, code.K
    pm = [0] + [1 << 30] * (S - 1)
    dec, rd = [], 0
    for t in range(T):
        sv = {}
        for r in code.kept(t):
            sv[r] = soft[rd]
            rd += 1
        nx, row = [0] * S, [0] * S
        for st in range(S):
            b, q0 = st & 1, st >> 1
            q1 = q0 | (1 << (K - 2))
            c = [sum(255 - s if parity(((q << 1) | b) & code.g[r]) else s for r, s in sv.items()) for q in (q0, q1)]
            m0, m1 = pm[q0] + c[0], pm[q1] + c[1]
            row[st] = int(m1 < m0)
            nx[st] = m1 if row[st] else m0
        dec.append(row)
        pm = nx
    e = 0
    if not code.terminated:
        for st in range(1, S):
            if pm[st] < pm[e]:
                e = st
    metric = pm[e]
    bits = [0] * T
    for t in range(T - 1, -1, -1):
        bits[t] = e & 1
        e = (e >> 1) | (dec[t][e] << (K - 2))
    return pack(np.array([bits[:n]], np.uint8))[0], metric


def messages(rng, F, n, pitch=None):
    """F random packed messages of n bits, pad bits zero; pitch > ceil(n / 8) adds junk columns that must be ignored"""
    nb = (n + 7) // 8
    m = pack(rng.integers(0, 2, (F, n)).astype(np.uint8))
    if pitch is None or pitch == nb:
        return m
    wide = rng.integers(0, 256, (F, pitch)).astype(np.uint8)
    wide[:, :nb] = m
    return wide


SOFT_KINDS = ("random", "all127", "all128", "all0", "hard", "ties")


def soft_bytes(rng, kind, F, nc):
    """soft inputs that are no codewords, so that every survivor decision matters; the constant and two-valued ones are
    full of equal metrics and exercise the strict compare and the lowest-index end state"""
    if kind == "random":
        return rng.integers(0, 256, (F, nc)).astype(np.uint8)
    if kind in ("all127", "all128", "all0"):
        return np.full((F, nc), int(kind[3:]), np.uint8)
    if kind == "hard":
        return (rng.integers(0, 2, (F, nc)) * 255).astype(np.uint8)
    if kind == "ties":
        return rng.choice(np.array([126, 127, 128, 129], np.uint8), (F, nc))
    raise ValueError(kind)
