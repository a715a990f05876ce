"""SymSync at the C ABI on a machine without a GPU: execute_host, the library's own sequential form, equals the
restatement (tests/symsync_ref.py) bit for bit, the stall rule and both pitches included; the designs of create_rnyquist
and create_kaiser are the restatement's; bad arguments are ConfigError before any device is asked for; the constructor
fails with DeviceError (no CPU fallback); the constants are the header's."""
import re

import numpy as np
import pytest

import symsync_ref as sr
from conftest import ROOT, has_gpu

AMPS = [0.5, 0.5, 4.0, 0.2, 1.0]


def ark(k, m, npfb, beta=0.3):
    import yagi_amd as ya
    return sr.rnyquist_taps(ya.FirFilterShape.Arkaiser, k, m, beta, npfb)


def host(C, k, npfb, h, x, ycap, **kw):
    import yagi_amd as ya
    return ya.SymSync.execute_host(C, k, npfb, h, x, ycap, **kw)


@pytest.mark.parametrize("locked", [False, True])
@pytest.mark.parametrize("k,m,npfb,k_out", [(2, 7, 32, 1), (3, 3, 8, 2), (5, 7, 64, 4), (2, 1, 1, 1), (2, 2, 8, 4),
                                            (3, 2, 1, 1), (5, 2, 32, 2)])
def test_execute_host_equals_the_restatement(k, m, npfb, k_out, locked):
    C, n = 5, 160
    h = ark(k, m, npfb)
    x = sr.noise(k + 10 * npfb + k_out, n, C, AMPS)
    ycap = sr.default_ycap(n, k, k_out) + 100
    r = sr.SymSyncRef(C, k, npfb, h)
    r.set_output_rate(k_out)
    r.set_lf_bw(0.03)
    if locked:
        r.lock()
    want = r.execute(x, ycap)
    got = host(C, k, npfb, h, x, ycap, k_out=k_out, bw=0.03, locked=locked)
    assert want[1].min() > 0 and not want[2].any()
    assert sr.same_outputs(got, want) and sr.same_words(got[3], r.get_tau())
    assert not np.any(got[0][int(want[1].max()):])                    # rows >= ny are not touched


def test_execute_host_pitches_and_stall():
    k, npfb, C, n, xp, yp = 2, 8, 4, 90, 11, 9
    h = ark(k, 3, npfb)
    x = sr.noise(3, n, C)
    x[30, 2] = np.nan                                               # channel 2 stalls on a NaN, with ny == ycap
    ycap = 70
    r = sr.SymSyncRef(C, k, npfb, h)
    want = r.execute(x, ycap)
    assert list(want[2]) == [0, 0, 1, 0] and want[1][2] == ycap
    wide = np.full((n, xp), 7 + 7j, np.complex64)
    wide[:, :C] = x
    y, ny, st, tau = host(C, k, npfb, h, wide, ycap, x_pitch=xp, y_pitch=yp)
    assert y.shape == (ycap, yp) and sr.same_outputs((y[:, :C], ny, st), want) and not np.any(y[:, C:])
    assert sr.same_words(tau, r.get_tau())
    # ycap too small for every channel: the first ycap words are the sequential loop's
    small = host(C, k, npfb, h, x, 12)
    assert list(small[1]) == [12] * C and list(small[2]) == [1] * C and sr.same_words(small[0][:, [0, 1, 3]], want[0][:12, [0, 1, 3]])
    assert sr.same_outputs(small, sr.SymSyncRef(C, k, npfb, h).execute(x, 12))
    zero = host(C, k, npfb, h, x[:0], 0)
    assert not zero[1].any() and not zero[2].any()


def test_designs_are_the_restatements():
    import yagi_amd as ya
    for k, m, beta, npfb in [(2, 7, 0.35, 32), (5, 7, 0.25, 64), (3, 3, 0.9, 8), (2, 1, 0.2, 1)]:
        for ft in (ya.FirFilterShape.Arkaiser, ya.FirFilterShape.Rrcos, ya.FirFilterShape.Kaiser, ya.FirFilterShape.Rcos):
            assert sr.same_words(ya.SymSync.rnyquist_taps(ft, k, m, beta, npfb), sr.rnyquist_taps(ft, k, m, beta, npfb))
        assert sr.same_words(ya.SymSync.kaiser_taps(k, m, beta, npfb), sr.kaiser_taps(k, m, beta, npfb))
    # test_symsync_copy's design through the host form
    h = ya.SymSync.rnyquist_taps(ya.FirFilterShape.Arkaiser, 5, 7, 0.25, 64)
    x = sr.noise(1, 200, 1, np.sqrt(2.0))
    r = sr.SymSyncRef(1, 5, 64, h)
    r.set_lf_bw(0.02)
    assert sr.same_outputs(host(1, 5, 64, h, x, 200, bw=0.02), r.execute(x, 200))


def test_bad_arguments_are_config_errors_with_or_without_a_gpu():
    import yagi_amd as ya
    E, S, sh = ya.ConfigError, ya.SymSync, ya.FirFilterShape
    z48, z47 = np.zeros(48, np.float32), np.zeros(47, np.float32)
    good = ark(2, 3, 8)
    x = np.zeros((4, 1), np.complex64)
    bad = [(1, 0, 12, z48), (1, 2, 0, z48), (1, 2, 12, z48[:0]), (1, 2, 12, z47),             # the reference's four
           (0, 2, 8, good), (ya.SYMSYNC_CHANNELS_MAX + 1, 2, 8, good),
           (1, 2, 12, np.ones(49, np.float32)),                                              # hdh_max = 0
           (1, 2, 8, np.where(np.arange(97) == 40, np.inf, good).astype(np.float32)),        # hdh_max not finite
           (1, 2, ya.SYMSYNC_NPFB_MAX + 1, np.arange(2 * (ya.SYMSYNC_NPFB_MAX + 1) + 1, dtype=np.float32)),
           (1, 2, 1, np.arange(ya.SYMSYNC_LS_MAX + 2, dtype=np.float32))]                   # Ls = LS_MAX + 1
    for args in bad:
        with pytest.raises(E):
            S(*args)
        if args[0] == 1:
            with pytest.raises(E):
                S.execute_host(*args, x, 8)
    for args in [(sh.Rrcos, 0, 12, 0.2, 48), (sh.Rrcos, 2, 0, 0.2, 48), (sh.Rrcos, 2, 12, 7.2, 48), (sh.Rrcos, 2, 12, 0.2, 0),
                 (sh.Rkaiser, 2, 3, 0.2, 8), (sh.Rrcos, 8, 9, 0.2, 8)]:
        with pytest.raises(E):
            S.rnyquist(1, *args)
        with pytest.raises(E):
            S.rnyquist_taps(*args)
    for args in [(0, 12, 0.2, 48), (2, 0, 0.2, 48), (2, 12, 7.2, 48), (2, 12, 0.2, 0), (2, 12, 0.0, 48)]:
        with pytest.raises(E):
            S.kaiser(1, *args)
        with pytest.raises(E):
            S.kaiser_taps(*args)
    with pytest.raises(E):
        S(1, 2, 8, good, kind="rrrf")
    for kw in (dict(k_out=0), dict(bw=-1.0), dict(bw=1.5), dict(bw=float("nan")), dict(x_pitch=0), dict(y_pitch=0)):
        with pytest.raises(E):
            S.execute_host(1, 2, 8, good, x if "x_pitch" not in kw else np.zeros((4, 0), np.complex64), 8, **kw)


@pytest.mark.skipif(has_gpu(), reason="checks the no-GPU error path")
def test_create_without_a_gpu_is_a_device_error():
    import yagi_amd as ya
    with pytest.raises(ya.DeviceError):
        ya.SymSync(4, 2, 8, ark(2, 3, 8))
    with pytest.raises(ya.DeviceError):
        ya.SymSync.rnyquist(4, ya.FirFilterShape.Arkaiser, 2, 7, 0.35, 32)
    with pytest.raises(ya.DeviceError):
        ya.SymSync.kaiser(1, 2, 12, 0.2, 48)


def test_python_constants_equal_the_header():
    import yagi_amd as ya
    hdr = (ROOT / "include" / "yagi_hip.h").read_text()
    for name, ours, refs in (("NPFB_MAX", ya.SYMSYNC_NPFB_MAX, sr.NPFB_MAX), ("LS_MAX", ya.SYMSYNC_LS_MAX, sr.LS_MAX),
                             ("CHANNELS_MAX", ya.SYMSYNC_CHANNELS_MAX, sr.CHANNELS_MAX)):
        assert ours == int(re.search(rf"#define YAGI_SYMSYNC_{name} (\d+)", hdr).group(1)) == refs
    assert (ya.SYMSYNC_NPFB_MAX, ya.SYMSYNC_LS_MAX, ya.SYMSYNC_CHANNELS_MAX) == (128, 128, 1 << 20)
