"""SymTrack at the C ABI on a machine without a GPU: execute_host, the library's own sequential form built from the
functions the kernel is built from, equals the restatement (tests/symtrack_ref.py) word for word on the stimuli of
tests/test_gpu_symtrack.py; the stimulus of the PLL stall shows that reason on that channel in the restatement alone;
every constant and entry point of the header's block is declared and exported; bad arguments are ConfigError before any
device is asked for; the constructor fails with DeviceError (no CPU fallback)."""
import re

import numpy as np
import pytest

import symtrack_ref as sr
from conftest import ROOT, has_gpu

FT, BETA = sr.FT, sr.BETA


def host(C, k, m, npfb, scheme, vco, eq_len, x, **kw):
    import yagi_amd as ya
    s = sr.SCHEMES[scheme]
    return ya.symtrack_host(C, FT, k, m, BETA, ya.ModulationScheme[s] if isinstance(s, str) else s,
                            ya.OscScheme.Vco if vco else ya.OscScheme.Nco, x, npfb, eq_len, **kw)


@pytest.mark.parametrize("C,k,m,npfb,eq_len,vco,n", sr.SHAPES)
def test_execute_host_equals_the_restatement_on_every_shape(oracle, C, k, m, npfb, eq_len, vco, n):
    C = min(C, 6)                                           # the host form has no lanes: a few channels of each design
    x = sr.streams(C + n, "Qpsk", n, C, k, m, BETA)
    f = (0.04 * (np.arange(C) % 7 - 3) / 3.0).astype(np.float32)
    ph = (0.3 * (np.arange(C) % 5)).astype(np.float32)
    r = sr.SymTrackRef(C, FT, k, m, BETA, "Qpsk", vco, npfb, eq_len)
    r.set_eq_holdoff(3)
    r.set_nco_all(f, ph)
    ycap = -(-n // k) + 8
    want = r.execute(x, ycap)
    wide = np.full((n, C + 3), 5 - 5j, np.complex64)
    wide[:, :C] = x
    y, sym, ny, st = host(C, k, m, npfb, "Qpsk", vco, eq_len, wide, holdoff=3, nco_frequency=f, nco_phase=ph, ycap=ycap,
                          x_pitch=C + 3, y_pitch=C + 2, sym_pitch=C + 1)
    assert y.shape == (ycap, C + 2) and sym.shape == (ycap, C + 1) and not y[:, C:].any() and not sym[:, C:].any()
    assert not sr.same_outputs((y[:, :C], sym[:, :C], ny, st), want)
    assert ny.min() > 10 and not st.any() and np.isnan(y[:ny.min(), :C]).all() == (eq_len == 1)


@pytest.mark.parametrize("scheme,vco,strategy,eq_len", sr.KINDS)
def test_execute_host_equals_the_restatement_for_every_kind_of_decision(oracle, scheme, vco, strategy, eq_len):
    import yagi_amd as ya
    C, k, m, npfb, n = 4, 2, 2, 8, 240
    x = sr.streams(11, sr.SCHEMES[scheme], n, C, k, m, BETA)
    r = sr.SymTrackRef(C, FT, k, m, BETA, sr.SCHEMES[scheme], vco, npfb, eq_len)
    r.set_eq_strategy(strategy)
    r.set_eq_holdoff(3)
    want = r.execute(x, n)
    got = host(C, k, m, npfb, scheme, vco, eq_len, x, strategy=ya.SymTrackEq(strategy), holdoff=3, ycap=n)
    assert not sr.same_outputs(got, want)
    assert want[2].min() > 100 and len({int(s) for s in want[1][:100].reshape(-1)}) >= 2


@pytest.mark.parametrize("holdoff", [0, 3, 200])
def test_execute_host_equals_the_restatement_across_the_holdoff(oracle, holdoff):
    C, k, m, npfb = 2, 2, 2, 8
    n = 2 * (holdoff + 12)
    x = sr.streams(5, "Qpsk", n, C, k, m, BETA)
    r = sr.SymTrackRef(C, FT, k, m, BETA, "Qpsk", False, npfb, 9)
    r.set_eq_holdoff(holdoff)
    before = r.get_weights().copy()
    want = r.execute(x, n)
    assert not np.array_equal(r.get_weights(), before)
    assert not sr.same_outputs(host(C, k, m, npfb, "Qpsk", False, 9, x, holdoff=holdoff, ycap=n), want)


def test_execute_host_equals_the_restatement_on_odd_channels_and_stalls(oracle):
    C, k, m, npfb, n = 5, 2, 2, 8, 120
    x = sr.streams(31, "Qpsk", n, C, k, m, BETA)
    x[:, 1] = 0
    x[40, 3] = np.nan
    x[77, 3] = np.complex64(complex(np.inf, 1.0))
    # the NaN reaches channel 3's timing loop: b stays 0, the loop emits until the capacity rule ends it
    for ycap, reason in ((n, [0, 0, 0, sr.STALL_CAPACITY, 0]), (20, [sr.STALL_CAPACITY] * C)):
        r = sr.SymTrackRef(C, FT, k, m, BETA, "Qpsk", False, npfb, 9)
        r.set_eq_holdoff(3)
        want = r.execute(x, ycap)
        got = host(C, k, m, npfb, "Qpsk", False, 9, x, holdoff=3, ycap=ycap)
        assert not sr.same_outputs(got, want)
        assert want[3].tolist() == reason


def test_the_pll_stimulus_stalls_exactly_its_channel_in_the_restatement(oracle):
    """tests/test_gpu_symtrack.py feeds this to the device; here the restatement alone shows the reason and the channel.
    execute_host takes one bandwidth, which cannot freeze the agc and keep the PLL's gains, so the object's form of this
    case is compared on the GPU only"""
    C, k, m, npfb, n, victim = 4, 2, 2, 8, 80, 2
    r = sr.SymTrackRef(C, FT, k, m, BETA, "Qpsk", False, npfb, 9)
    r.set_eq_holdoff(3)
    r.set_bandwidths(0.0, 0.0009, 0.018, 0.0009)
    y, sym, ny, st = r.execute(sr.pll_stimulus(C, k, m, n, victim, 41), -(-n // k) + 8)
    assert st.tolist() == [0, 0, sr.STALL_PLL, 0] and 18 <= ny[victim] <= 24
    assert r.get_gain()[victim] == np.float32(1.0)
    # at the default bandwidths the sample passes the agc at the gain of that moment and stalls the channel just so:
    # this form goes through execute_host
    r = sr.SymTrackRef(C, FT, k, m, BETA, "Qpsk", False, npfb, 9)
    want = r.execute(sr.pll_stimulus(C, k, m, n, victim, 41), -(-n // k) + 8)
    assert want[3].tolist() == [0, 0, sr.STALL_PLL, 0]
    assert not sr.same_outputs(host(C, k, m, npfb, "Qpsk", False, 9, sr.pll_stimulus(C, k, m, n, victim, 41)), want)
    # with the PLL's gains at zero as well (set_bandwidth(0)) e alpha and e beta are 0 or NaN, never 256: no stall
    r = sr.SymTrackRef(C, FT, k, m, BETA, "Qpsk", False, npfb, 9)
    r.set_bandwidth(0.0)
    assert not r.execute(sr.pll_stimulus(C, k, m, n, victim, 41), -(-n // k) + 8)[3].any()


def test_bad_arguments_are_config_errors_with_or_without_a_gpu():
    import yagi_amd as ya
    E, S, N = ya.ConfigError, ya.ModulationScheme, ya.OscScheme.Nco
    x = np.zeros((4, 1), np.complex64)
    good = dict(channels=1, ftype=FT, k=2, m=3, beta=BETA, scheme=S.Qpsk, osc_scheme=N, npfb=8, eq_len=9)

    def both(**kw):
        """the constructor (decided before any device is asked for) and the host form"""
        a = dict(good, **kw)
        with pytest.raises(E):
            ya.SymTrack(a["channels"], a["ftype"], a["k"], a["m"], a["beta"], a["scheme"], a["osc_scheme"], a["npfb"], a["eq_len"])
        with pytest.raises(E):
            ya.symtrack_host(a["channels"], a["ftype"], a["k"], a["m"], a["beta"], a["scheme"], a["osc_scheme"],
                             np.zeros((4, max(a["channels"], 1)), np.complex64), a["npfb"], a["eq_len"])

    for scheme in (S.Psk2, S.Psk8, S.Psk256, S.Dpsk2, S.Dpsk4, S.Dpsk256, S.Arb, S.Apsk16):
        both(scheme=scheme)
    both(k=1)
    both(k=0)
    both(eq_len=0)
    both(eq_len=ya.EQLMS_LEN_MAX + 1)
    both(k=4, m=8, eq_len=128)                               # 32 KiB of window and 128 KiB of equalizer: over 160 KiB of LDS
    assert sr.lds_bytes(64, 128, False, 4) > sr.LDS_MAX >= sr.lds_bytes(28, 128, False, 4)
    ya.symtrack_host(1, FT, 2, 7, BETA, S.Qpsk, N, x, 8, 128)                  # 14 KiB of window: fits
    both(channels=0)
    both(m=0)
    both(beta=1.5)
    both(npfb=0)
    both(npfb=ya.SYMSYNC_NPFB_MAX + 1)
    both(k=8, m=9)                                           # 2 k m = 144 taps per branch
    both(scheme=np.ones(3, np.complex64))                    # a table of 3 points
    both(scheme=np.ones(512, np.complex64))
    with pytest.raises(E):
        ya.SymTrack(ya.SYMTRACK_CHANNELS_MAX + 1, FT, 2, 3, BETA, S.Qpsk)
    with pytest.raises(ValueError):
        ya.SymTrack(1, FT, 2, 3, BETA, S.Qpsk, 7)            # no such oscillator
    for kw in (dict(bw=-0.1), dict(bw=float("nan")), dict(bw=60.0),          # 0.02 bw is the agc's bandwidth, at most 1
               dict(nco_frequency=np.array([np.inf], np.float32)), dict(nco_phase=np.array([-np.inf], np.float32)),
               dict(nco_frequency=np.array([1e30], np.float32)), dict(nco_frequency=np.zeros(2, np.float32)),
               dict(ycap=2 ** 31), dict(x_pitch=0), dict(y_pitch=0), dict(sym_pitch=0)):
        with pytest.raises(E):
            ya.symtrack_host(1, FT, 2, 3, BETA, S.Qpsk, N, x if "x_pitch" not in kw else np.zeros((4, 0), np.complex64), 8, 9, **kw)
    with pytest.raises(ValueError):
        ya.symtrack_host(1, FT, 2, 3, BETA, S.Qpsk, N, x, 8, 9, strategy=3)
    y, sym, ny, st = ya.symtrack_host(1, FT, 2, 3, BETA, S.Qpsk, N, x, 8, 9, bw=0.0, nco_frequency=np.array([99.0], np.float32))
    assert ny.tolist() == [2] and not st.any()
    assert [int(v) for v in ya.SymTrackEq] == [sr.OFF, sr.CM, sr.DD]


@pytest.mark.skipif(has_gpu(), reason="checks the no-GPU error path")
def test_create_without_a_gpu_is_a_device_error():
    import yagi_amd as ya
    with pytest.raises(ya.DeviceError):
        ya.SymTrack(4, FT, 2, 7, BETA, ya.ModulationScheme.Qpsk)
    with pytest.raises(ya.DeviceError):
        ya.SymTrack(4, FT, 2, 7, BETA, sr.ARB8, ya.OscScheme.Vco, 16, 9)


ENTRY_POINTS = ("create create_from_table destroy clone set_stream reset reset_channel set_bandwidth get_bandwidth "
                "set_bandwidths set_eq_strategy set_eq_holdoff set_nco set_nco_all get_channels get_tau get_gain get_rssi "
                "get_nco_frequency get_nco_phase get_nco_state get_weights get_num_syms get_stalled execute execute_dev "
                "execute_host").split()


def test_the_headers_block_is_declared_and_exported():
    import yagi_amd as ya
    hdr = (ROOT / "include" / "yagi_hip.h").read_text()
    block = hdr[hdr.index("/* ---- SymTrack:"):hdr.index("/* ---- design helpers")]
    comment = block[:block.index("*/")]
    for name in ENTRY_POINTS:
        assert re.search(rf"\bint yagi_hip_symtrack_cccf_{name}\(", block), name
        assert hasattr(ya.lib, f"yagi_hip_symtrack_cccf_{name}"), name
        assert re.search(rf"\b{name}\b", comment), name      # the block comment lists it
    declared = set(re.findall(r"\bint yagi_hip_symtrack_cccf_(\w+)\(", block))
    assert declared == set(ENTRY_POINTS), declared ^ set(ENTRY_POINTS)
    assert int(re.search(r"#define YAGI_SYMTRACK_CHANNELS_MAX (\d+)", block).group(1)) == ya.SYMTRACK_CHANNELS_MAX == sr.CHANNELS_MAX
    assert float(re.search(r"#define YAGI_SYMTRACK_PLL_ARG_MAX ([\d.]+)f", block).group(1)) == ya.SYMTRACK_PLL_ARG_MAX == sr.PLL_ARG_MAX
    eq = re.search(r"enum \{ YAGI_SYMTRACK_EQ_OFF = (\d), YAGI_SYMTRACK_EQ_CM = (\d), YAGI_SYMTRACK_EQ_DD = (\d) \}", block)
    assert [int(v) for v in eq.groups()] == [sr.OFF, sr.CM, sr.DD]
    stall = re.search(r"enum \{ YAGI_SYMTRACK_STALL_NONE = (\d), YAGI_SYMTRACK_STALL_CAPACITY = (\d), "
                      r"YAGI_SYMTRACK_STALL_PLL = (\d) \}", block)
    assert [int(v) for v in stall.groups()] == [0, sr.STALL_CAPACITY, sr.STALL_PLL]
    assert (ya.SYMTRACK_STALL_CAPACITY, ya.SYMTRACK_STALL_PLL) == (sr.STALL_CAPACITY, sr.STALL_PLL)
    for name in ("YAGI_SYMTRACK_PLL_ARG_MAX", "YAGI_SYMTRACK_STALL_CAPACITY", "YAGI_SYMTRACK_STALL_PLL",
                 "YAGI_SYMTRACK_EQ_OFF", "YAGI_SYMTRACK_CHANNELS_MAX"):
        assert name in comment, name
