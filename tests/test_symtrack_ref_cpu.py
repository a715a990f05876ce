"""SymTrack's definition locks: the f32 restatement (symtrack_ref.py) acquires gain, timing, carrier and channel on the
four cases of the design note and ends with no symbol error over the last 1000 of 3000 symbols, after the constant
delay and the constellation's quarter-turn ambiguity are resolved; the oscillator's frequency word ends within 2 % of the
carrier offset per synchroniser output sample.

Settings, those of the design note's f64 model: root-raised-cosine pulse at beta = 0.3, m = 7, the synchroniser's bank
at npfb = 32, eq_len = 9, 30 dB SNR, bw = 0.9, a carrier phase of 0.5 rad, generator seed 1.  The transmitter below is
the model's: the pulse designed at 64 samples per sample and read at the timing offset.  The 16-QAM case sits near the
edge of the decision-directed loop's pull-in range: the f64 model itself loses it at npfb = 16 or with another symbol
sequence, which is why npfb is 32 and the symbols are drawn exactly as the model draws them (model_points).

EVM over the last 1000 symbols as this test prints it (records, copied into DESIGN.md; the bound below is twice the
record of each case, so that a change of the loops that doubles the error vector shows up):
    QPSK   k = 2  tau  0.2  dphi  0.02  gain 0.1  CM    0.0241
    QPSK   k = 2  tau -0.3  dphi -0.05  gain 3.0  CM    0.0256
    QPSK   k = 4  tau  0.2  dphi  0.01  gain 0.1  CM    0.0196
    QAM16  k = 2  tau  0.2  dphi  0.02  gain 0.1  DD    0.0370
"""
import numpy as np
import pytest

import symtrack_ref as sr

NSYM, TAIL, M_, BETA, NPFB, OVER = 3000, 1000, 7, 0.3, 32, 64
#        scheme   k  tau   dphi   gain  strategy  EVM record
CASES = [("Qpsk", 2, 0.2, 0.02, 0.1, sr.CM, 0.0241),
         ("Qpsk", 2, -0.3, -0.05, 3.0, sr.CM, 0.0256),
         ("Qpsk", 4, 0.2, 0.01, 0.1, sr.CM, 0.0196),
         ("Qam16", 2, 0.2, 0.02, 0.1, sr.DD, 0.0370)]


def rrc(k, m, beta):
    """the root-raised-cosine pulse at k samples per symbol, 2 k m + 1 taps, in f64"""
    h = np.zeros(2 * k * m + 1)
    for i, t in enumerate(np.arange(-k * m, k * m + 1) / k):
        if abs(t) < 1e-9:
            h[i] = 1 - beta + 4 * beta / np.pi
        elif abs(abs(4 * beta * t) - 1) < 1e-9:
            h[i] = beta / np.sqrt(2) * ((1 + 2 / np.pi) * np.sin(np.pi / (4 * beta)) + (1 - 2 / np.pi) * np.cos(np.pi / (4 * beta)))
        else:
            h[i] = (np.sin(np.pi * t * (1 - beta)) + 4 * beta * t * np.cos(np.pi * t * (1 + beta))) / (np.pi * t * (1 - (4 * beta * t) ** 2))
    return h


def model_points(M):
    """the model's point tables, in its order: the symbols are drawn as indices into these"""
    if M == 4:
        return np.array([1 + 1j, -1 + 1j, 1 - 1j, -1 - 1j]) / np.sqrt(2)
    a = np.array([-3, -1, 1, 3])
    return np.array([x + 1j * y for x in a for y in a]) / np.sqrt(10)


def transmit(cmap, k, tau, dphi, gain, seed=1, phase=0.5, snr_db=30.0):
    """(samples[NSYM k], symbols[NSYM] as indices into cmap, the library's map)"""
    rng = np.random.default_rng(seed)
    points = model_points(cmap.size)[rng.integers(0, cmap.size, NSYM)]
    sent = np.argmin(np.abs(points[:, None] - cmap[None, :]), axis=1)
    up = np.zeros(NSYM * k * OVER, complex)
    up[::k * OVER] = points
    off = int(round(tau * k * OVER)) % (k * OVER)
    xs = np.convolve(up, rrc(k * OVER, M_, BETA))[off::OVER][:NSYM * k]
    x = gain * xs * np.exp(1j * (dphi * np.arange(xs.size) + phase))
    x = x + (rng.standard_normal(x.size) + 1j * rng.standard_normal(x.size)) * gain * 10 ** (-snr_db / 20) / np.sqrt(2)
    return x.astype(np.complex64), sent


def best_alignment(cmap, sent, sym, tail):
    """(errors, delay, quarter turns) of the received symbols' last `tail` against the sent ones, over delays and the four
    rotations of a square constellation"""
    best = None
    for rot in range(4):
        turned = cmap * np.exp(0.5j * np.pi * rot)
        relabel = np.array([int(np.argmin(np.abs(cmap - t))) for t in turned])
        want = relabel[sent]
        for delay in range(0, 40):
            a = sym[-tail:]
            lo = len(sym) - tail - delay
            if lo < 0 or lo + tail > len(want):
                continue
            b = want[lo:lo + tail]
            errs = int(np.count_nonzero(a != b))
            if best is None or errs < best[0]:
                best = (errs, delay, rot)
    return best


@pytest.mark.parametrize("scheme, k, tau, dphi, gain, strategy, evm_record", CASES)
def test_the_restatement_locks(oracle, scheme, k, tau, dphi, gain, strategy, evm_record):
    import yagi_amd as ya
    cmap = sr.constellation(scheme)
    x, sent = transmit(cmap, k, tau, dphi, gain)
    r = sr.SymTrackRef(1, ya.FirFilterShape.Rrcos, k, M_, BETA, scheme, npfb=NPFB)
    r.set_eq_strategy(strategy)
    y, sym, ny, st = r.execute(x[:, None], NSYM + 8)
    assert st[0] == 0 and ny[0] >= NSYM - 40, (ny, st)
    y, sym = y[:ny[0], 0], sym[:ny[0], 0]
    errs, delay, rot = best_alignment(cmap, sent, sym, TAIL)
    evm = float(np.sqrt(np.mean(np.abs(y[-TAIL:] - cmap[sym[-TAIL:]]) ** 2) / np.mean(np.abs(cmap) ** 2)))
    f = float(r.get_nco_frequency()[0])
    want_f = dphi * k / 2.0                                  # radians per synchroniser output sample (two per symbol)
    print(f"symtrack lock {scheme} k={k} tau={tau} dphi={dphi} gain={gain} strategy={strategy}: errors {errs} "
          f"(delay {delay}, {rot} quarter turns), EVM {evm:.4f}, nco {f:.5f} for {want_f:.5f}")
    assert errs == 0
    assert abs(f - want_f) <= 0.02 * abs(want_f)
    assert evm <= 2.0 * evm_record
