"""MSequence and BSequence (src/sequence/msequence.rs, bsequence.rs) restated step by step in plain Python, and plain
models of the two schemes of yagi_amd/csrc/sequence_kernels.hip (a helper, not a test module).

The restatements keep the reference's arithmetic on 32-bit words: MSequence.advance() forms its bit from the whole
state and the whole of g and masks afterwards; BSequence keeps the word array, word 0 oldest and masked.

The models: GF(2) jump matrices (32 column words; T^(2^b) by squaring; a jump by the matrices of the offset's set
bits) with the kernel's split of a block into tiles, waves and lanes, and the packed stream with its funnel shifts."""
import functools

import numpy as np

MSEQUENCE_TILE = 8192        # YAGI_MSEQUENCE_TILE
BSEQUENCE_TILE = 4096        # YAGI_BSEQUENCE_TILE
BSEQUENCE_NMAX = 8192        # YAGI_BSEQUENCE_NMAX
WG = 256                     # lanes per workgroup of either kernel
M32 = 0xFFFFFFFF


def popcount(x):
    return bin(x).count("1")


class ConfigError(Exception):
    pass


# ---- MSequence -------------------------------------------------------------------------------------------------------
class MSequence:
    def __init__(self, m, g, a=1):                                 # new() :55-67
        if m > 31 or m < 2:
            raise ConfigError(f"m ({m}) not in range")
        self.m, self.g, self.a = m, g & M32, a & M32
        self.n = (1 << m) - 1
        self.state = self.a                                        # not masked

    @classmethod
    def from_genpoly(cls, g):                                      # :69-77
        t = int(g).bit_length()
        if t < 2:
            raise ConfigError(f"invalid generator polynomial: 0x{g:x}")
        return cls(t, g, 1)

    def advance(self):                                             # :116-122
        b = popcount(self.state & self.g) & 1
        self.state = (((self.state << 1) & M32) | b) & self.n
        return b

    def generate_symbol(self, bps):                                # :124-131
        s = 0
        for _ in range(bps):
            s = (s << 1) | self.advance()
        return s

    def reset(self):
        self.state = self.a

    def set_state(self, a):
        self.state = a & M32

    def measure_period(self):                                      # :147-158
        s, period = self.state, 0
        for _ in range(self.n + 1):
            self.advance()
            period += 1
            if self.state == s:
                break
        return period

    def bits(self, n):
        return np.array([self.advance() for _ in range(n)], np.uint8)

    def symbols(self, bps, n):
        return np.array([self.generate_symbol(bps) for _ in range(n)], np.uint8)


# the jump matrices
def mat_apply(M, s):
    acc = 0
    for j in range(32):
        if (s >> j) & 1:
            acc ^= M[j]
    return acc


def mat_T(g, nmask):
    """column j = advance() on the unit vector 1 << j"""
    return [((((1 << j) << 1) & M32) | (popcount((1 << j) & g) & 1)) & nmask for j in range(32)]


def mat_powers(g, nmask, count=64):
    """T^(2^b), b < count"""
    P = [mat_T(g, nmask)]
    for _ in range(1, count):
        P.append([mat_apply(P[-1], c) for c in P[-1]])
    return P


def skip(P, s, k):
    """the state k steps after s: the matrices of k's set bits"""
    b = 0
    while k:
        if k & 1:
            s = mat_apply(P[b], s)
        k >>= 1
        b += 1
    return s


def mseq_block_model(ms, bps, n, tile=MSEQUENCE_TILE):
    """the kernel's scheme: per wave a uniform jump to its first symbol, per lane the six stride matrices
    T^(run * bps * 2^b) picked by the bits of the lane number, then `run` symbols stepped serially.  ms is advanced."""
    run = tile // WG
    P = mat_powers(ms.g, ms.n)
    ident = [1 << j for j in range(32)]
    S = [[skip(P, c, (run * bps) << b) for c in ident] for b in range(6)]
    out = np.zeros(n, np.uint8)
    for t0 in range(0, n, tile):
        for wave in range(WG // 64):
            base = skip(P, ms.state, (t0 + wave * 64 * run) * bps)
            for lane in range(64):
                first = t0 + (wave * 64 + lane) * run
                if first >= n:
                    break
                s = base
                for b in range(6):
                    t = mat_apply(S[b], s)
                    s = t if (lane >> b) & 1 else s
                w = MSequence(ms.m, ms.g, ms.a)
                w.state = s
                for i in range(first, min(first + run, n)):
                    out[i] = w.generate_symbol(bps)
    ms.state = skip(P, ms.state, n * bps)
    return out


# ---- BSequence -------------------------------------------------------------------------------------------------------
class BSequence:
    def __init__(self, num_bits, nmax=BSEQUENCE_NMAX):             # new() :16-30
        if num_bits == 0:
            raise ConfigError("sequence length must be greater than zero")
        if num_bits > nmax:
            raise ConfigError("sequence too long")
        self.num_bits = num_bits
        self.num_bits_msb = 32 if num_bits % 32 == 0 else num_bits % 32
        self.bit_mask_msb = (1 << self.num_bits_msb) - 1
        self.s = [0] * ((num_bits + 31) // 32)

    @classmethod
    def from_msequence(cls, ms):                                   # :81-88
        q = cls(ms.n)
        for _ in range(ms.n):
            q.push(ms.advance())
        return q

    @classmethod
    def ccodes(cls, n):                                            # create_ccodes() :34-79
        qa, qb = cls(n), cls(n)
        create_ccodes(qa, qb)
        return qa, qb

    def clone(self):
        q = BSequence(self.num_bits)
        q.s = list(self.s)
        return q

    def reset(self):
        self.s = [0] * len(self.s)

    def init(self, v):                                             # :95-108
        for i in range(self.num_bits):
            self.push((int(v[i // 8]) >> (7 - i % 8)) & 1)

    def push(self, bit):                                           # :115-127
        s = self.s
        s[0] = ((s[0] << 1) & M32) & self.bit_mask_msb
        for i in range(1, len(s)):
            s[i - 1] |= (s[i] >> 31) & 1
            s[i] = (s[i] << 1) & M32
        s[-1] |= bit & 1

    def circshift(self):                                           # :130-134
        self.push((self.s[0] >> (self.num_bits_msb - 1)) & 1)

    def correlate(self, other):                                    # :137-150
        if len(self.s) != len(other.s):
            raise ConfigError("binary sequences must be the same length")
        rxy = sum(popcount(~(a ^ b) & M32) for a, b in zip(self.s, other.s))
        return rxy - (32 - self.num_bits_msb)

    def _combine(self, other, out, op):
        if len(self.s) != len(other.s) or len(self.s) != len(out.s):
            raise ConfigError("binary sequences must be same length")
        out.s = [op(a, b) for a, b in zip(self.s, other.s)]

    def add(self, other, out):                                     # :153-163
        self._combine(other, out, lambda a, b: a ^ b)

    def mul(self, other, out):                                     # :166-176
        self._combine(other, out, lambda a, b: a & b)

    def accumulate(self):                                          # :179-181
        return sum(popcount(w) for w in self.s)

    def index(self, i):                                            # :188-194
        if i >= self.num_bits:
            raise ConfigError(f"invalid index {i}")
        return (self.s[len(self.s) - 1 - i // 32] >> (i % 32)) & 1

    def all_bits(self):
        """index(i) for every i"""
        raw = self.as_int().to_bytes(4 * len(self.s), "little")
        return np.unpackbits(np.frombuffer(raw, np.uint8), bitorder="little")[:self.num_bits].copy()

    def load(self, v):
        """what init(v) leaves, without its num_bits pushes: the first num_bits bits of v, the first one oldest"""
        nby = (self.num_bits + 7) // 8
        self.from_int(int.from_bytes(bytes(bytearray(int(b) for b in v[:nby])), "big") >> (8 * nby - self.num_bits))

    # the word array as one integer (word 0 in the highest place) and back: what push_correlate() steps on
    def as_int(self):
        v = 0
        for w in self.s:
            v = (v << 32) | w
        return v

    def from_int(self, v):
        W = len(self.s)
        self.s = [(v >> (32 * (W - 1 - k))) & M32 for k in range(W)]


def create_ccodes(qa, qb):                                         # :34-79
    if qa.num_bits != qb.num_bits:
        raise ConfigError("sequence lengths must match")
    if qa.num_bits < 8:
        raise ConfigError("sequence too short")
    if qa.num_bits % 8 != 0:
        raise ConfigError("sequence must be multiple of 8")
    nby = qa.num_bits // 8
    a, b = [0] * nby, [0] * nby
    a[nby - 1], b[nby - 1] = 0xB8, 0xB7
    n = 1
    while n < nby:
        i1, i0 = nby - n, nby - 2 * n
        a[i0:i1] = a[i1:i1 + n]
        b[i0:i1] = a[i1:i1 + n]
        a[i1:i1 + n] = b[i1:i1 + n]
        for i in range(n):
            b[nby - i - 1] ^= 0xFF
        n *= 2
    qa.init(a)
    qb.init(b)


def push_correlate_plain(q, ref, sym, bps, want_rxy=True):
    """the block call's meaning, word array and all: slow, for short blocks"""
    if len(q.s) != len(ref.s) or q is ref or not 1 <= bps <= 8:
        raise ConfigError("push_correlate_block")
    rxy = np.zeros(len(sym), np.int32)
    for i, s in enumerate(sym):
        for j in range(bps - 1, -1, -1):
            q.push((int(s) >> j) & 1)
        if want_rxy:
            rxy[i] = ref.correlate(q)
    return rxy if want_rxy else None


def push_correlate(q, ref, sym, bps, want_rxy=True):
    """the same loop on the word arrays read as one integer each: a push is a shift under the N-bit mask, the sum of
    popcount(~(a ^ b)) over W words is 32 W - popcount(A ^ B).  tests/test_sequence_ref_cpu.py pins it to the plain loop."""
    if len(q.s) != len(ref.s) or q is ref or not 1 <= bps <= 8:
        raise ConfigError("push_correlate_block")
    W = len(q.s)
    mask = (1 << q.num_bits) - 1
    v, r = q.as_int(), ref.as_int()
    corr = 32 * W - (32 - ref.num_bits_msb)
    rxy = np.zeros(len(sym), np.int32)
    for i, s in enumerate(sym):
        s = int(s)
        for j in range(bps - 1, -1, -1):
            v = ((v << 1) | ((s >> j) & 1)) & mask
        if want_rxy:
            rxy[i] = corr - popcount(v ^ r)
    q.from_int(v)
    return rxy if want_rxy else None


def funnel(hi, lo, r):
    """((hi : lo) << r) >> 32 on uint32 arrays, 0 <= r < 32 element-wise"""
    hi, lo, r = hi.astype(np.uint64), lo.astype(np.uint64), r.astype(np.uint64)
    return ((((hi << np.uint64(32)) | lo) << r) >> np.uint64(32)).astype(np.uint32)


def popcount_u32(a):
    a = np.asarray(a, np.uint32)
    a = a - ((a >> np.uint32(1)) & np.uint32(0x55555555))
    a = (a & np.uint32(0x33333333)) + ((a >> np.uint32(2)) & np.uint32(0x33333333))
    a = (a + (a >> np.uint32(4))) & np.uint32(0x0F0F0F0F)
    return ((a * np.uint32(0x01010101)) >> np.uint32(24)).astype(np.int32)


def packed_model(q, ref, sym, bps, tile=BSEQUENCE_TILE):
    """the kernel's scheme, tile by tile.  The stream is q's window, then the symbols' bits, packed into 32-bit words
    with the earlier bit higher and 32 W - N zero bits in front: words 0 .. W-1 are q's words, symbol i sits at bits
    [32 W + i bps, 32 W + (i + 1) bps).  A tile packs the words [wlo, whi] its windows span; output i's window ends at
    e = 32 W + (i + 1) bps and its word j is funnel(packed[e / 32 - W + j], packed[e / 32 - W + j + 1], e % 32).
    Returns rxy; q gets the window the block leaves."""
    sym = np.ascontiguousarray(sym, np.uint8)
    n, W = sym.size, len(q.s)
    refw = np.array(ref.s, np.uint32)
    corr = 32 * W - (32 - ref.num_bits_msb)
    rxy = np.zeros(n, np.int32)
    smask = (1 << bps) - 1
    for t0 in range(0, n, tile):
        cnt = min(tile, n - t0)
        wlo = ((t0 + 1) * bps) >> 5
        whi = W + (((t0 + cnt) * bps) >> 5)
        pk = np.zeros(whi - wlo + 1, np.uint32)
        for k in range(pk.size):
            gw = wlo + k
            if gw < W:
                pk[k] = q.s[gw]
                continue
            sb0 = (gw - W) * 32
            i = sb0 // bps
            pos = i * bps - sb0
            acc = 0
            while pos < 32 and i < n:
                acc |= (int(sym[i]) & smask) << (48 - pos - bps)
                i += 1
                pos += bps
            pk[k] = (acc >> 16) & M32
        o = np.arange(cnt)
        e = 32 * W + (t0 + o + 1) * bps
        r, kb = e & 31, (e >> 5) - W - wlo
        diff = np.zeros(cnt, np.int32)
        for j in range(W):
            w = funnel(pk[kb + j], pk[kb + j + 1], r)
            if j == 0:
                w &= np.uint32(q.bit_mask_msb)
            diff += popcount_u32(w ^ refw[j])
        rxy[t0:t0 + cnt] = corr - diff
        if t0 + cnt == n:
            e = 32 * W + n * bps
            r, kb = np.array([e & 31] * W), (e >> 5) - W - wlo + np.arange(W)
            nxt = funnel(pk[kb], pk[kb + 1], r)
            nxt[0] &= np.uint32(q.bit_mask_msb)
    if n:
        q.s = [int(w) for w in nxt]
    return rxy


# ---- the shared (N, bps, n) grid of the block form -------------------------------------------------------------------
GRID_N = (1, 31, 32, 33, 63, 64, 255, 1023, 4095, 8192)
GRID_BPS = (1, 2, 3, 8)


def grid_lengths(N, bps, tile=BSEQUENCE_TILE):
    """n with n * bps below, at (or first above) and above N, and n around the tile"""
    at = -(-N // bps)
    return sorted({max(1, at // 2), at, at + 5, tile - 1, tile + 1, 3 * tile + 17})


@functools.lru_cache(maxsize=None)
def grid_case(N, bps):
    """one q of N bits (random start window) and one ref, pushed through every grid length in turn: a tuple of
    (n, sym, rxy, window bits after) per call plus the two start states as byte vectors for init().  Computed once."""
    rng = np.random.default_rng(1000 * N + bps)
    nby = (N + 7) // 8
    q0 = rng.integers(0, 256, nby).astype(np.uint8)
    r0 = rng.integers(0, 256, nby).astype(np.uint8)
    q, ref = BSequence(N), BSequence(N)
    q.load(q0)
    ref.load(r0)
    calls = []
    for n in grid_lengths(N, bps):
        sym = rng.integers(0, 256, n).astype(np.uint8)              # bits above bps are set on purpose
        rxy = push_correlate(q, ref, sym, bps)
        calls.append((n, sym, rxy, q.all_bits()))
    return q0, r0, tuple(calls)
