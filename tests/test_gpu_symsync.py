"""SymSync on the GPU against tests/symsync_ref.py, bit for bit: y below ny, ny, stalled and get_tau, through the host
path (execute) and the device path (execute_devptr).  Channel counts put a lone lane, a partial wave, the wave seam and
several workgroups on the chip; the designs cover the tap table in LDS below and above 64 KiB and in global memory;
the streams pull the lanes of a wave apart (timing offsets, loud channels whose q clamps, two outputs per step)."""
import numpy as np
import pytest

import symsync_ref as sr

pytestmark = pytest.mark.gpu

N = 300
CHANNELS = [1, 63, 64, 65, 200]
#          k  m  npfb   (m = None: raw taps with Ls = 128 at npfb = 128)
DESIGNS = [(2, 7, 32), (3, 3, 8), (5, 7, 64), (2, 1, 1), (2, None, 128)]


@pytest.fixture(scope="module")
def ya():
    import yagi_amd
    return yagi_amd


def taps(ya, k, m, npfb):
    if m is None:
        h = ya.fir_design_kaiser(npfb * 128 + 1, 0.5 / npfb, 60.0, 0.0)
        return np.asarray(h, np.float32)
    return ya.SymSync.rnyquist_taps(ya.FirFilterShape.Arkaiser, k, m, 0.35 if m > 1 else 0.5, npfb)


def pair(ya, C, k, m, npfb):
    h = taps(ya, k, m, npfb)
    return ya.SymSync(C, k, npfb, h), sr.SymSyncRef(C, k, npfb, h)


def check(ya, q, r, got, want, C):
    assert sr.same_outputs(got, want)
    assert sr.same_words(q.get_tau(), r.get_tau())
    assert np.array_equal(q.get_stalled(), r.stalled.astype(np.uint32))


@pytest.mark.parametrize("k,m,npfb", DESIGNS)
@pytest.mark.parametrize("C", CHANNELS)
def test_host_and_device_paths(ya, C, k, m, npfb):
    q, r = pair(ya, C, k, m, npfb)
    ls = q.branch_length
    assert ls == r.ls == (128 if m is None else (2 * npfb * k * m + 1) // npfb)
    x = sr.streams(k, N, C, 11 * C + k)
    ycap = sr.default_ycap(N, k, 1) + 40
    want = r.execute(x, ycap)
    assert not want[2].any() and want[1].min() > 0
    if C >= 63 and m not in (1, None):
        assert np.unique(want[1]).size > 1                          # the lanes did come apart
    d = q.clone()
    got = sr.run_dev(ya, d, x, ycap)                                # one call on device buffers
    check(ya, d, r, got, want, C)
    parts, pos = [], 0                                              # the host path, cut into calls of 0, 1, Ls - 1 and the rest
    for ln in (0, 1, ls - 1, N - ls):
        parts.append(q.execute(x[pos:pos + ln], ycap))
        pos += ln
    assert not parts[0][1].any()
    assert all(sr.same_words(a, b) for a, b in zip(sr.concat(parts, C), sr.below(want[0], want[1])))
    assert sr.same_words(q.get_tau(), r.get_tau()) and not q.get_stalled().any()


@pytest.mark.parametrize("k_out", [2, 4])
def test_output_rates(ya, k_out):
    C, k = 65, 2
    q, r = pair(ya, C, k, 7, 32)
    for o in (q, r):
        o.set_output_rate(k_out)
        o.set_lf_bw(0.05)
    x = sr.streams(k, N, C, 5 + k_out)
    ycap = sr.default_ycap(N, k, k_out) + 40
    assert q.default_ycap(N) == sr.default_ycap(N, k, k_out)
    want = r.execute(x, ycap)
    assert not want[2].any() and want[1].min() > N * k_out // k // 2
    if k_out == 4:
        assert want[1].max() > N                                    # two outputs in one step
    check(ya, q, r, sr.run_dev(ya, q, x, ycap), want, C)


@pytest.mark.parametrize("piece", [1, 2, 27, 28, 97])
def test_cuts_across_device_calls(ya, piece):
    C, k, n = 65, 2, 200
    q, r = pair(ya, C, k, 7, 32)
    x = sr.streams(k, n, C, 3)
    want = r.execute(x, 2 * n)
    xd = ya.DeviceArray.from_numpy(x)
    yd = ya.DeviceArray(C * (2 * piece + 8), np.complex64)
    sd = ya.DeviceArray(2 * C, np.uint32)
    outs = [[] for _ in range(C)]
    for pos in range(0, n, piece):
        ln = min(piece, n - pos)
        q.execute_devptr(xd.ptr + 8 * C * pos, C, ln, yd.ptr, C, 2 * ln + 8, sd.ptr)
        ya.synchronize()
        st, y = sd.to_numpy(), yd.to_numpy().reshape(-1, C)
        assert not st[C:].any()
        for c in range(C):
            outs[c].append(y[:st[c], c].copy())
    assert all(sr.same_words(np.concatenate(o), w) for o, w in zip(outs, sr.below(want[0], want[1])))
    assert sr.same_words(q.get_tau(), r.get_tau())


def test_state_changes_between_calls(ya):
    C, k = 65, 2
    q, r = pair(ya, C, k, 7, 32)
    x = sr.streams(k, 4 * 151, C, 9)
    ycap = 400
    blocks = [x[i * 151:(i + 1) * 151] for i in range(4)]
    for o in (q, r):
        o.set_lf_bw(0.05)
    check(ya, q, r, sr.run_dev(ya, q, blocks[0], ycap), r.execute(blocks[0], ycap), C)
    q2, r2 = q.clone(), r.clone()                                   # a clone after an odd number of steps
    for o in (q, r):
        o.lock()                                                    # lock mid-stream
        o.reset_channel(17)
    assert q.is_locked() and not q2.is_locked()
    check(ya, q, r, sr.run_dev(ya, q, blocks[1], ycap), r.execute(blocks[1], ycap), C)
    check(ya, q2, r2, sr.run_dev(ya, q2, blocks[1], ycap), r2.execute(blocks[1], ycap), C)
    for o in (q, r):
        o.unlock()
        o.set_output_rate(2)
        o.set_lf_bw(0.3)
    check(ya, q, r, q.execute(blocks[2], ycap), r.execute(blocks[2], ycap), C)
    for o in (q, r):
        o.reset()                                                   # the derivative window survives: not a fresh object
    got, want = sr.run_dev(ya, q, blocks[3], ycap), r.execute(blocks[3], ycap)
    check(ya, q, r, got, want, C)
    fresh = sr.SymSyncRef(C, k, 32, taps(ya, k, 7, 32))
    fresh.set_output_rate(2)
    fresh.set_lf_bw(0.3)
    assert not sr.same_outputs(fresh.execute(blocks[3], ycap), want)


def stall_case(ya):
    """a block whose channel 0 writes more outputs than every other channel: loud noise under a wide loop makes its
    rate wander, and the search keeps a stream on which it wanders down"""
    C, k, n = 70, 2, 200
    h = taps(ya, k, 7, 32)
    for seed in range(40):
        x = sr.noise(seed, n, C, np.where(np.arange(C) == 0, 20.0, 0.3))
        r = sr.SymSyncRef(C, k, 32, h)
        r.set_lf_bw(1.0)
        _, ny, st = r.execute(x, 2 * n)
        if ny[0] >= ny[1:].max() + 3 and not st.any():
            return C, k, h, x, int(ny[1:].max())
    raise AssertionError("no seed gives channel 0 the most outputs")


def test_stall(ya):
    C, k, h, x, ycap = stall_case(ya)
    x[50, 66] = np.nan                                              # and a NaN on a channel of the second workgroup
    q, r = ya.SymSync(C, k, 32, h), sr.SymSyncRef(C, k, 32, h)
    clean = sr.SymSyncRef(C, k, 32, h)
    for o in (q, r, clean):
        o.set_lf_bw(1.0)
    want = r.execute(x, ycap)
    stalled = np.zeros(C, np.uint32)
    stalled[[0, 66]] = 1
    assert np.array_equal(want[2], stalled) and want[1][0] == want[1][66] == ycap
    got = sr.run_dev(ya, q, x, ycap)
    check(ya, q, r, got, want, C)
    ok = np.flatnonzero(stalled == 0)                               # every other channel is untouched by it
    xc = x.copy()
    xc[50, 66] = 0
    free = clean.execute(xc, 2 * x.shape[0])
    assert np.array_equal(got[1][ok], free[1][ok])
    assert all(sr.same_words(got[0][:got[1][c], c], free[0][:free[1][c], c]) for c in ok)
    assert sr.same_words(got[0][:ycap, 0], free[0][:ycap, 0])       # channel 0's first ycap words are right
    more = sr.noise(77, 100, C, 0.3)                                # the next call: ny = 0 for both, tau kept
    tau = q.get_tau()
    got, want = sr.run_dev(ya, q, more, 300), r.execute(more, 300)
    assert got[1][0] == got[1][66] == 0 and got[2][0] == got[2][66] == 1
    check(ya, q, r, got, want, C)
    assert sr.same_words(q.get_tau()[[0, 66]], tau[[0, 66]])
    for o in (q, r):
        o.reset_channel(0)                                          # revives it; channel 66 keeps the NaN in its derivative
        o.reset_channel(66)                                         # window (the reference's quirk) and stalls again
    got, want = q.execute(more, 300), r.execute(more, 300)
    assert got[1][0] > 0 and got[2][0] == 0 and got[1][66] == 300 and got[2][66] == 1
    check(ya, q, r, got, want, C)


def test_pitches_on_a_channelizer_sub_band(ya):
    C, M, c0, nf, k = 25, 32, 3, 200, 2
    ch = ya.FirPfbCh(M, 4, ya.fir_design_kaiser(M * 4, 0.4 / M, 60.0, 0.0))
    x = sr.noise(21, nf * M, 1, 4.0).reshape(-1)
    xd = ya.DeviceArray.from_numpy(x)
    bands = ya.DeviceArray(nf * M, np.complex64)
    ch.analyzer_execute_dev(xd, nf, bands)
    ya.synchronize()
    sub = bands.to_numpy().reshape(nf, M)[:, c0:c0 + C]
    q, r = pair(ya, C, k, 7, 32)
    ycap = 150
    want = r.execute(sub, ycap)
    assert want[1].min() > 50
    yd = ya.DeviceArray.from_numpy(np.full(ycap * M, np.nan + 0j, np.complex64))
    sd = ya.DeviceArray(2 * C, np.uint32)
    q.execute_devptr(bands.ptr + 8 * c0, M, nf, yd.ptr + 8 * c0, M, ycap, sd.ptr)      # x_pitch = y_pitch = C + 7
    ya.synchronize()
    st, y = sd.to_numpy(), yd.to_numpy().reshape(ycap, M)
    check(ya, q, r, (y[:, c0:c0 + C], st[:C], st[C:]), want, C)
    written = np.zeros((ycap, M), bool)
    for c in range(C):
        written[:st[c], c0 + c] = True
    assert np.isnan(y[~written]).all() and np.isfinite(y[written]).all()
    assert np.array_equal(bands.to_numpy().reshape(nf, M)[:, c0:c0 + C], sub)       # the input is intact


def test_lock_property(ya):
    k, m, nsym = 2, 7, 600
    streams = [sr.qpsk_stream(nsym, tau) for tau in sr.LOCK_TAUS]
    x = np.stack([xs for _, xs in streams], axis=1)
    q = ya.SymSync.rnyquist(4, ya.FirFilterShape.Arkaiser, k, m, 0.35, 32)
    r = sr.SymSyncRef.rnyquist(4, ya.FirFilterShape.Arkaiser, k, m, 0.35, 32)
    for o in (q, r):
        o.set_lf_bw(0.02)
    got = q.execute(x, nsym + 64)
    check(ya, q, r, got, r.execute(x, nsym + 64), 4)
    for c, (s, _) in enumerate(streams):
        err = sr.lock_errors(got[0][:, c], int(got[1][c]), s)
        print(f"tau {sr.LOCK_TAUS[c]}: nz {got[1][c]}, max error over the last 100 outputs {err.max():.4f}")
        assert err.max() < sr.LOCK_TOL


def test_kaiser_design_and_the_copy_case(ya):
    """create_kaiser against the restatement's, and the reference's test_symsync_copy on the device"""
    q, r = ya.SymSync.kaiser(3, 2, 12, 0.2, 48), sr.SymSyncRef.kaiser(3, 2, 12, 0.2, 48)
    x = sr.noise(31, 120, 3)
    check(ya, q, r, q.execute(x, 200), r.execute(x, 200), 3)
    q0 = ya.SymSync.rnyquist(1, ya.FirFilterShape.Arkaiser, 5, 7, 0.25, 64)
    q0.set_lf_bw(0.02)
    q0.execute(sr.noise(1, 640, 1, np.sqrt(2.0)), 640)
    q1 = q0.clone()
    x = sr.noise(2, 640, 1, np.sqrt(2.0))
    a, b = q0.execute(x, 640), q1.execute(x, 640)
    assert a[1][0] == b[1][0] > 100 and sr.same_outputs(a, b) and sr.same_words(q0.get_tau(), q1.get_tau())
