"""SymStream (include/yagi_hip.h; src/framing/symstream.rs) as the composition it is defined by (a helper, not a test
module): the library's own MSequence, Modem and FirInterpolationFilter("crcf") run one after the other, and a plain
Python model of the reference's buf / buf_index (write_samples :111-121).  The gain is applied on the float32 view, the
re and im planes separately: a complex64 x real product in numpy can flip a signed zero."""
import numpy as np

from conftest import load_golden


def golden_generator(m):
    """(m, g) of the golden table of default generator polynomials, e.g. (23, 4325376)"""
    z = load_golden("sequence")
    i = int(np.flatnonzero(z["genpoly_m"] == m)[0])
    return int(z["genpoly_m"][i]), int(z["genpoly_g"][i])


def apply_gain(v, gain):
    out = np.array(v, np.complex64)
    out.view(np.float32)[:] = out.view(np.float32) * np.float32(gain)
    return out


class SymStreamParts:
    """src: an MSequence (cloned here, as create does); modem: a Modem (cloned); h: the prototype's taps as
    FirInterpolationFilter(k, h) takes them"""

    def __init__(self, ya, k, h, modem, src):
        self.ya, self.k = ya, int(k)
        self.src = src.clone()
        self.modem = modem.clone()
        self.fir = ya.FirInterpolationFilter("crcf", k, np.asarray(h, np.float32))
        self.gain = np.float32(1.0)
        self.buf = np.zeros(self.k, np.complex64)
        self.p = 0
        self.bits = 0                                # bits drawn from the source so far

    def set_gain(self, g):
        self.gain = np.float32(g)

    def set_modem(self, modem):                      # set_scheme: Modem(scheme)
        self.modem = modem.clone()

    def reset(self):                                 # :61-65, the source stays
        self.modem.reset()
        self.fir.reset()
        self.p = 0

    def _push(self, sym):
        """the samples of the symbols `sym`, all k branches each"""
        pts = apply_gain(self.modem.modulate_block(sym), self.gain)
        y = self.fir.execute_block(pts)
        self.buf = y[-self.k:].copy()
        return y

    def write_samples(self, n):
        k, p = self.k, self.p
        head = min(n, k - p) if p else 0
        out = [self.buf[p:p + head]]
        nnew = -(-(n - head) // k)
        if nnew:
            bps = self.modem.get_bps()
            sym = self.src.generate_symbols_block(bps, nnew)
            self.bits += nnew * bps
            out.append(self._push(sym)[:n - head])
        self.p = (p + n) % k
        return np.concatenate(out).astype(np.complex64)

    def modulate_symbols(self, sym):
        assert self.p == 0
        return self._push(np.asarray(sym, np.uint8))
