"""EqLms at the C ABI on a machine without a GPU: execute_host, the library's own sequential form, equals the restatement
(tests/eqlms_ref.py) bit for bit in every mode, the weights it leaves and pitches wider than the channel count included;
the default tap and h0 = conj(reversed h) are seen through the weights of an empty call; bad arguments are ConfigError
before any device is asked for; the constructor fails with DeviceError (no CPU fallback); the constants are the header's.
The designs of create_rnyquist and create_lowpass need an object and are compared in tests/test_gpu_eqlms.py."""
import re

import numpy as np
import pytest

import eqlms_ref as er
from conftest import ROOT, has_gpu
from test_eqlms_ref_cpu import MODES, run, taps


def host(C, h_len, h, mu, k, x, mode=None, **kw):
    import yagi_amd as ya
    return ya.EqLms.execute_host(C, h_len, h, mu, k, x, mode=None if mode is None else ya.EqLmsUpdate(mode), **kw)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("h_len,k", [(1, 1), (2, 5), (3, 2), (29, 1), (29, 2), (29, 5), (128, 2)])
def test_execute_host_equals_the_restatement(h_len, k, mode):
    C, pad = 6, 3
    nsym = 20 + -(-h_len // k)
    n = nsym * k
    x = er.streams(n, C, 11 + h_len + k, k=k)
    d = er.symbols(nsym, C, 2) if mode == er.TRAIN else None
    h = taps(h_len) if h_len != 3 else None
    r = er.EqLmsRef(C, h_len, h)
    r.set_bw(0.2)
    r.set_constellation(er.QAM16_MAP)
    want = run(r, k, mode, x, d)
    wide = np.full((n, C + pad), 7 + 7j, np.complex64)
    wide[:, :C] = x
    dw = None
    if d is not None:
        dw = np.full((nsym, C + 1), 9 - 9j, np.complex64)
        dw[:, :C] = d
    y, w0 = host(C, h_len, h, 0.2, k, wide, mode, d=dw, table=er.QAM16_MAP, x_pitch=C + pad, d_pitch=C + 1, y_pitch=C + 2)
    assert y.shape == (want.shape[0], C + 2) and not np.any(y[:, C:])
    assert er.same_words(y[:, :C], want)
    assert er.same_words(w0, r.get_coefficients())


def test_default_tap_designs_and_get_weights():
    import yagi_amd as ya
    x0 = np.zeros((0, 2), np.complex64)
    for h_len in (1, 2, 13, 128):
        _, w0 = host(2, h_len, None, 0.5, 1, x0)
        want = np.zeros(h_len, np.complex64)
        want[h_len // 2] = 1
        assert er.same_words(w0[0], want) and er.same_words(w0[1], want)
    h = taps(9)
    _, w0 = host(1, 9, h, 0.5, 1, x0[:, :1])
    assert er.same_words(w0[0], np.conj(h[::-1])) and er.same_words(w0[0], er.initial_taps(9, h))
    r = er.EqLmsRef(1, 9, h)
    assert er.same_words(r.get_weights()[0], h)                              # reversed and conjugated: h again
    for ft, k, m, beta, dt in [(ya.FirFilterShape.Arkaiser, 2, 7, 0.3, 0.0), (ya.FirFilterShape.Rrcos, 4, 3, 0.25, 0.5)]:
        hc = er.rnyquist_h(ft, k, m, beta, dt)
        assert hc.size == 2 * k * m + 1 and abs(hc.real.sum() - 1) < 0.2
    for h_len, fc in [(21, 0.12345), (29, 0.25)]:
        hc = er.lowpass_h(h_len, fc)
        assert hc.size == h_len and abs(hc.real.sum() - 1) < 0.05


def test_bad_arguments_are_config_errors_with_or_without_a_gpu():
    import yagi_amd as ya
    E, Q, sh, U = ya.ConfigError, ya.EqLms, ya.FirFilterShape, ya.EqLmsUpdate
    # the reference's (eqlms.rs:384-393, 407, 410)
    for args in [(sh.Arkaiser, 0, 12, 0.3, 0.0), (sh.Arkaiser, 2, 0, 0.3, 0.0), (sh.Arkaiser, 2, 12, 2.0, 0.0),
                 (sh.Arkaiser, 2, 12, 0.3, -2.0)]:
        with pytest.raises(E):
            Q.rnyquist(1, *args)
    for args in [(0, 0.1), (13, -0.1), (13, 0.6), (13, 0.0)]:                  # fc = 0 passes the range test and fails the design
        with pytest.raises(E):
            Q.lowpass(1, *args)
    x = np.zeros((4, 1), np.complex64)
    with pytest.raises(E):
        host(1, 5, None, -1.0, 1, x)                                          # set_bw(-1)
    with pytest.raises(E):
        host(1, 5, None, 0.5, 0, x)                                           # execute_block, k = 0
    with pytest.raises(E):
        host(1, 5, None, 0.5, 0, x, er.NONE)                                  # decim_execute, k = 0
    with pytest.raises(E):
        host(1, 0, None, 0.5, 1, x)                                           # Window::new(0)
    # the library's own: limits, whole symbols, TRAIN without d, the table
    for C, h_len in [(0, 5), (ya.EQLMS_CHANNELS_MAX + 1, 5), (1, ya.EQLMS_LEN_MAX + 1)]:
        with pytest.raises(E):
            Q(C, h_len)
    with pytest.raises(E):
        host(1, ya.EQLMS_LEN_MAX + 1, None, 0.5, 1, x)
    with pytest.raises(E):
        Q.rnyquist(1, sh.Arkaiser, 8, 9, 0.3, 0.0)                            # 2 k m + 1 = 145 taps
    with pytest.raises(E):
        Q.lowpass(1, ya.EQLMS_LEN_MAX + 1, 0.1)
    with pytest.raises(E):
        host(1, 5, None, 0.5, 3, x, er.NONE)                                  # 4 rows at k = 3
    with pytest.raises(E):
        host(1, 5, None, 0.5, 2, x, er.TRAIN)                                 # no d
    for table in (None, np.zeros(0, np.complex64), np.zeros(ya.EQLMS_TABLE_MAX + 1, np.complex64)):
        with pytest.raises(E):
            host(1, 5, None, 0.5, 2, x, er.DECISION, table=table)
    host(1, 5, None, 0.5, 2, x, er.DECISION, table=np.ones(ya.EQLMS_TABLE_MAX, np.complex64))
    for kw in (dict(x_pitch=0), dict(y_pitch=0)):
        with pytest.raises(E):
            host(1, 5, None, 0.5, 1, x if "x_pitch" not in kw else np.zeros((4, 0), np.complex64), **kw)
    with pytest.raises(E):
        host(1, 5, None, 0.5, 2, x, er.TRAIN, d=np.zeros((2, 0), np.complex64), d_pitch=0)
    with pytest.raises(E):
        Q(1, 5, kind="crcf")
    with pytest.raises(E):
        Q(1, 5, np.zeros(4, np.complex64))
    assert [int(v) for v in U] == [er.NONE, er.TRAIN, er.BLIND, er.DECISION]


@pytest.mark.skipif(has_gpu(), reason="checks the no-GPU error path")
def test_create_without_a_gpu_is_a_device_error():
    import yagi_amd as ya
    with pytest.raises(ya.DeviceError):
        ya.EqLms(4, 13)
    with pytest.raises(ya.DeviceError):
        ya.EqLms.rnyquist(4, ya.FirFilterShape.Arkaiser, 2, 7, 0.3, 0.0)
    with pytest.raises(ya.DeviceError):
        ya.EqLms.lowpass(1, 21, 0.12345)


def test_python_constants_equal_the_header():
    import yagi_amd as ya
    hdr = (ROOT / "include" / "yagi_hip.h").read_text()
    for name, ours, refs in (("LEN_MAX", ya.EQLMS_LEN_MAX, er.LEN_MAX), ("CHANNELS_MAX", ya.EQLMS_CHANNELS_MAX, er.CHANNELS_MAX),
                             ("TABLE_MAX", ya.EQLMS_TABLE_MAX, er.TABLE_MAX)):
        assert ours == int(re.search(rf"#define YAGI_EQLMS_{name} (\d+)", hdr).group(1)) == refs
    assert (ya.EQLMS_LEN_MAX, ya.EQLMS_CHANNELS_MAX, ya.EQLMS_TABLE_MAX) == (128, 1 << 20, 256)
    enum = re.search(r"enum \{ YAGI_EQLMS_NONE = (\d), YAGI_EQLMS_TRAIN = (\d), YAGI_EQLMS_BLIND = (\d), "
                     r"YAGI_EQLMS_DECISION = (\d), YAGI_EQLMS_EXECUTE = (\d) \}", hdr)
    assert [int(v) for v in enum.groups()] == [0, 1, 2, 3, 4]
