"""tests/eqlms_ref.py against itself and against the reference's own testbench: the vectorised form equals the
statement-by-statement form bit for bit in every mode (which also proves that x2_0 recomputed from the leaving sample is
WDelay's word), the result does not depend on how the stream is cut into calls, the library's |z| is compared with this
machine's hypotf, and testbench_eqlms (eqlms.rs:213-309) passes its own condition, rmse < -20 dB over the second half."""
import ctypes
import ctypes.util

import numpy as np
import pytest

import eqlms_ref as er

MODES = [None, er.NONE, er.TRAIN, er.BLIND, er.DECISION]        # None: execute_block


def run(q, k, mode, x, d=None):
    return q.execute_block(k, x) if mode is None else q.decim_block(k, mode, x, d)


def taps(h_len, seed=5):
    r = np.random.default_rng(seed)
    h = (r.standard_normal(h_len) + 1j * r.standard_normal(h_len)) * 0.3
    h[h_len // 2] += 1
    return h.astype(np.complex64)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", [1, 2, 5])
@pytest.mark.parametrize("h_len", [1, 2, 3, 29])
def test_the_two_forms_agree_bit_for_bit(h_len, k, mode):
    C, nsym = 5, 24 + -(-h_len // k)                         # the gate opens after h_len rows, 24 symbols before the end
    n = nsym * k
    x = er.streams(n, C, 100 + h_len + k, k=k)
    d = er.symbols(nsym, C, 7) if mode == er.TRAIN else None
    h = taps(h_len) if h_len != 3 else None
    q = er.EqLmsRef(C, h_len, h)
    q.set_bw(0.3)
    q.set_constellation(er.QAM16_MAP)
    y = run(q, k, mode, x, d)
    w = q.get_coefficients()
    for c in range(C):
        s = er.EqLmsScalar(h_len, h)
        s.mu, s.table = er.F(0.3), er.QAM16_MAP
        ys = s.execute_block(k, x[:, c]) if mode is None else s.decim_block(k, mode, x[:, c], None if d is None else d[:, c])
        assert er.same_words(ys, y[:, c]), (c, h_len, k, mode)
        assert er.same_words(s.get_coefficients(), w[c]), (c, h_len, k, mode)
        assert er.same_words(np.float32(s.x2_sum), q.x2_sum[c])
    if mode not in (er.NONE,) and h_len > 1:
        assert not er.same_words(w[0], q.h0)                  # the weights moved
    if mode in (er.NONE, er.TRAIN):
        assert np.isfinite(w[0]).all() and np.isfinite(w[2]).all()
    if mode != er.NONE:
        assert not np.isfinite(w[1]).all()                    # the all-zero channel: 0 / 0
        assert not np.isfinite(w[3]).all()                    # the NaN / Inf channel


@pytest.mark.parametrize("mode", MODES)
def test_the_ref_does_not_depend_on_the_cuts(mode):
    C, h_len, k, nsym = 4, 7, 2, 30
    x = er.streams(nsym * k, C, 9, k=k)
    d = er.symbols(nsym, C, 3) if mode == er.TRAIN else None
    whole = er.EqLmsRef(C, h_len)
    whole.set_constellation(er.QPSK_MAP)
    want = run(whole, k, mode, x, d)
    parts = er.EqLmsRef(C, h_len)
    parts.set_constellation(er.QPSK_MAP)
    got, at = [], 0
    for syms in (0, 1, 2, 3, nsym - 6):                        # 3 symbols = 6 rows, then row 7 = h_len crosses the gate
        rows = slice(at * k, (at + syms) * k)
        got.append(run(parts, k, mode, x[rows], None if d is None else d[at:at + syms]))
        at += syms
    assert er.same_words(np.concatenate(got), want)
    assert er.same_words(parts.get_coefficients(), whole.get_coefficients())


def hypot_inputs():
    r = np.random.default_rng(20)
    e = r.integers(-40, 40, (1_000_000, 2))
    v = (r.standard_normal((1_000_000, 2)) * np.exp2(e)).astype(np.float32)
    tiny, big = np.float32(1e-45), np.finfo(np.float32).max
    edge = [0.0, -0.0, tiny, 3 * tiny, np.finfo(np.float32).tiny, 1.0, 3.0, 4.0, big, big / 2, big / np.float32(1.5), 2.0 ** 63]
    edges = np.array([(a, b) for a in edge for b in edge] + [(s * a, s * a) for a in edge for s in (1, -1)], np.float32)
    return np.concatenate([v, edges])


def test_abs_definition_against_this_machines_hypotf(capsys):
    """The count of differing words is a recorded measurement, not a pass condition.  What is
    asserted is what follows from both being roundings of the same real number: where both are finite they are equal or
    neighbours, and zeros, infinities and overflow agree."""
    libm = ctypes.CDLL(ctypes.util.find_library("m"))
    libm.hypotf.restype, libm.hypotf.argtypes = ctypes.c_float, (ctypes.c_float, ctypes.c_float)
    v = hypot_inputs()
    ours = er.abs_def(v[:, 0], v[:, 1])
    theirs = np.fromiter(map(libm.hypotf, v[:, 0].tolist(), v[:, 1].tolist()), np.float32, len(v))
    differ = int(np.sum(ours.view(np.uint32) != theirs.view(np.uint32)))
    with capsys.disabled():
        print(f"\n|z| against hypotf: {differ} of {len(v)} words differ")
    assert np.array_equal(np.isfinite(ours), np.isfinite(theirs))
    fin = np.isfinite(ours)
    assert np.all(np.abs(ours.view(np.int32)[fin].astype(np.int64) - theirs.view(np.int32)[fin]) <= 1)
    assert ours[0] >= 0 and np.all(ours[~np.isnan(ours)] >= 0)


# eqlms.rs:311-381: (k, m, beta, init, p, mu, num_symbols, update, scheme); 10 is left out with its modem (tests/modem_ref.py
# builds no Arb64Vt)
BENCH = {"00": (2, 7, 0.3, 0, 7, 0.3, 800, 0, "qpsk"), "01": (2, 7, 0.3, 0, 7, 0.3, 800, 1, "qpsk"),
         "02": (2, 7, 0.3, 0, 7, 0.3, 800, 2, "qpsk"), "03": (2, 7, 0.3, 0, 7, 0.3, 800, 0, "qam16"),
         "04": (2, 7, 0.3, 1, 7, 0.3, 800, 0, "qam16"), "05": (2, 7, 0.3, 2, 7, 0.3, 800, 0, "qam16"),
         "06": (2, 7, 0.3, 3, 6, 0.3, 800, 0, "qam16"), "07": (2, 9, 0.3, 0, 7, 0.3, 800, 0, "qpsk"),
         "08": (2, 7, 0.2, 0, 9, 0.3, 800, 0, "qpsk"), "09": (2, 7, 0.3, 0, 3, 0.3, 800, 0, "qpsk"),
         "11": (2, 7, 0.3, 0, 7, 0.1, 800, 0, "qpsk")}


def bench_modem(name):
    import modem_ref as mr
    D = mr.design(mr.QPSK, 2) if name == "qpsk" else mr.design(mr.QAM, 4)
    return D.map


def bench_taps(init, k, p, beta):
    import yagi_amd as ya
    h_len = 2 * k * p + 1
    if init == 0:
        return h_len, er.rnyquist_h(ya.FirFilterShape.Arkaiser, k, p, beta, 0.0)
    if init == 1:
        return h_len, er.lowpass_h(h_len, 0.5 / k)
    if init == 2:
        i = np.arange(h_len)
        hp = np.sinc(i / k - p) * (0.53836 - 0.46164 * np.cos(2 * np.pi * i / (h_len - 1))) / k
        return h_len, hp.astype(np.complex64)
    return h_len, None


def run_testbench(case, make, seed=1):
    """the reference's loop in block calls: the first m + p symbols and the second half run without an update, the rest
    with `update` against the symbol m + p earlier.  `make(h_len, h, mu, cmap)` returns an object with decim_block."""
    k, m, beta, init, p, mu, N, update, scheme = BENCH[case]
    cmap = bench_modem(scheme)
    s, x = er.modulated(seed, cmap, 2 * N, k, m, beta)
    h_len, h = bench_taps(init, k, p, beta)
    q = make(h_len, h, mu, cmap)
    lag = m + p
    mode = (er.TRAIN, er.BLIND, er.DECISION)[update]
    q.decim_block(k, er.NONE, x[:lag * k, None])
    q.decim_block(k, mode, x[lag * k:N * k, None], s[:N - lag, None] if mode == er.TRAIN else None)
    out = q.decim_block(k, er.NONE, x[N * k:, None])[:, 0]
    err = np.abs(s[N - lag:2 * N - lag] - out).astype(np.float32)
    return 10 * np.log10(np.sum(err * err) / N)


def make_ref(h_len, h, mu, cmap):
    q = er.EqLmsRef(1, h_len, h)
    q.set_bw(mu)
    q.set_constellation(cmap)
    return q


@pytest.mark.parametrize("case", sorted(BENCH))
def test_the_references_testbench_on_the_ref(case, capsys):
    rmse = run_testbench(case, make_ref)
    with capsys.disabled():
        print(f"\ntestbench_eqlms {case}: rmse {rmse:.3f} dB")
    assert rmse < -20.0
