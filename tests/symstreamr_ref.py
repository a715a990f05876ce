"""SymStreamR (include/yagi_hip.h; src/framing/symstreamr.rs) as the composition it is defined by (a helper, not a test
module): the library's own SymStream at k = 2 and MsResamp("crcf", 0.5 / bw, 60).  The reference pushes one sample at a
time and only when its buffer is empty (fill_buffer :101-116), so a call that misses `missing` outputs pushes the
smallest number of samples whose outputs cover them: need(q) of resamp_util's schedule with q = ceil(missing / 2^S).
Here exactly that many samples go through both objects in one call each, the outputs join a FIFO and the call pops n."""
import numpy as np

import resamp_util as ru


def fl32_rate(bw):
    """0.5 / bw as the reference forms it, in f32"""
    return np.float32(0.5) / np.float32(bw)


def stages(rate):
    """MsResamp::new (msresamp.rs:33-51): (interp, half-band stages, rate of the arbitrary resampler), in f32"""
    rate = np.float32(rate)
    interp, ns, ra = bool(rate > np.float32(1.0)), 0, rate
    if interp:
        while ra > np.float32(2.0):
            ns, ra = ns + 1, np.float32(ra * np.float32(0.5))
    else:
        while ra < np.float32(0.5):
            ns, ra = ns + 1, np.float32(ra * np.float32(2.0))
    return interp, ns, ra


def need(p0, step, q):
    """samples the arbitrary stage needs from phase p0 for q outputs: output j comes after input (p0 + j step) >> 24"""
    return 0 if q == 0 else ((p0 + (q - 1) * step) >> 24) + 1


class SymStreamRParts:
    """src: an MSequence (copied by SymStream, as create does)"""

    def __init__(self, ya, ftype, bw, m, beta, scheme, src):
        self.ya = ya
        self.S = ya.SymStream(ftype, 2, m, beta, scheme, src)
        self.rate = fl32_rate(bw)
        self.R = ya.MsResamp("crcf", self.rate, 60.0)
        self.interp, self.ns, self.ra = stages(self.rate)
        assert (int(self.interp), self.ns) == self.R.get_params()[:2] and self.ra == self.R.get_params()[2]
        self.step = ru.rust_step(self.ra)
        self.phase = 0                               # the arbitrary stage's, tracked with resamp_util's closed form
        self.fifo = np.zeros(0, np.complex64)
        self.pushed = 0                              # samples of S pushed since reset
        self.symbols = 0                             # symbols drawn since creation
        self.bits = 0                                # bits drawn from the source since creation
        self.bps = ya.Modem(scheme).get_bps()

    def set_gain(self, g):
        self.S.set_gain(g)

    def set_scheme(self, scheme):
        self.S.set_scheme(scheme)
        self.bps = self.ya.Modem(scheme).get_bps()

    def set_modem(self, modem):
        self.S.set_modem(modem)
        self.bps = modem.get_bps()

    def reset(self):
        self.S.reset()
        self.R.reset()
        self.phase, self.pushed = 0, 0
        self.fifo = np.zeros(0, np.complex64)

    def write_samples(self, n):
        missing = n - min(n, self.fifo.size)
        if missing:
            q = -(-missing // (1 << self.ns))
            nx = need(self.phase, self.step, q)
            assert ru.num_output(self.phase, self.step, nx - 1)[0] < q      # the smallest number that covers them
            n1, self.phase = ru.num_output(self.phase, self.step, nx)
            assert n1 >= q
            nnew = (self.pushed + nx + 1) // 2 - (self.pushed + 1) // 2      # symbols first needed by the new samples
            self.symbols += nnew
            self.bits += nnew * self.bps
            self.pushed += nx
            y = self.R.execute(self.S.write_samples(nx))
            assert y.size == n1 << self.ns
            self.fifo = np.concatenate([self.fifo, y]).astype(np.complex64)
        out, self.fifo = self.fifo[:n].copy(), self.fifo[n:].copy()
        return out

