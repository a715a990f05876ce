"""Every launch plan of the half-band resamplers on the GPU, bit for bit against the oracle, at the shapes of
tests/halfband_shapes.py.

A case is a row of the table and a sample type.  It first asserts that the library's plan query reports the row's key on
this machine, so the kernels the case is about are the kernels that run, then makes three device calls that continue one
stream -- the row's shape, then 1 output, then 5, so the windows that the first call's last workgroup wrote for every
stage are read back in -- on integer prototypes and integer samples (tests/test_halfband_plan_cpu.py proves per row that
every partial sum is exact in f32).  The concatenated output equals, element for element over its whole length, the
oracle's sequential C loop: oracle.Resamp2 stages run one after the other on the host, the decimator's zeta folded into
its last stage as MsResamp2Obj::init folds it.  Decimator rows go through MsResamp2.from_taps, interpolator rows
likewise, Resamp2 rows through Resamp2(kind, hf, m) in its DECIM form.

The oracle chain over the whole block of the two largest rows (tpw 4: 2^26 complex samples in; tpw 8: 2^27 floats in)
was measured at 1.9 s and 3.8 s of CPU time, well under ten seconds, so every row, these included, is compared in full;
none uses windows.

test_designed_taps_per_decimator_key runs one row per decimator key (the longest) on Kaiser prototypes and Gaussian
data: the output has the bits of the same stages run as separate Resamp2 calls short enough for resamp2_kernel -- the
claim in the kernels' comments -- and is within 3e-6 in rel. L2 of the oracle, the bound of test_msresamp2_vs_oracle."""
import numpy as np
import pytest

import halfband_shapes as hs
from gpu_util import SEED, rand_samples, rel_l2

pytestmark = pytest.mark.gpu

SHORT = (1 << 18) + 2 * 101          # samples of a Resamp2 call that stays on resamp2_kernel (below 2^19), no tile multiple


@pytest.fixture(scope="module")
def ya():
    import yagi_amd
    assert yagi_amd.device_count() > 0
    return yagi_amd


def check_key(ya, row, kind):
    key, plan = hs.query(ya, row, kind)
    assert key == row.key, (key, row)
    return plan


def stream_length(row):
    """input samples of the three calls together"""
    total = sum(hs.call_sizes(row))
    return total << len(row.shape[0]) if row.family == "decim" else total


def run_device(ya, row, kind, hfs, x):
    """the row's three calls on device buffers; the concatenated output"""
    ms = hs.row_stages(row)
    item = x.dtype.itemsize
    xd = ya.DeviceArray.from_numpy(x)
    if row.family == "resamp2":
        q = ya.Resamp2(kind, hfs[0], ms[0])
        yd = ya.DeviceArray(x.size // 2, x.dtype)
        xo = 0
        for nx in hs.call_sizes(row):
            q.execute_block_dev(ya.Resamp2.DECIM, xd.ptr + xo * item, nx, yd.ptr + (xo // 2) * item)
            xo += nx
    else:
        interp = row.family == "interp"
        order = hs.object_order(row.family, range(len(ms)))                  # the object's stage g is processing stage order[g]
        q = ya.MsResamp2.from_taps(kind, ya.MsResamp2.INTERP if interp else ya.MsResamp2.DECIM, [ms[k] for k in order],
                                   [hfs[k] for k in order])
        assert q.get_stage_lengths() == hs.object_order(row.family, ms)
        rate = 1 << len(ms)
        yd = ya.DeviceArray(x.size * rate if interp else x.size // rate, x.dtype)
        done = 0
        for n in hs.call_sizes(row):
            xo, yo = (done, done * rate) if interp else (done * rate, done)
            q.execute_block_dev(xd.ptr + xo * item, n, yd.ptr + yo * item)
            done += n
    ya.synchronize()
    return yd.to_numpy()


def params():
    cs = hs.cases()
    return pytest.mark.parametrize("row,kind", cs, ids=[hs.case_id(r, k) for r, k in cs])


@params()
def test_row_equals_the_oracle_chain_bit_for_bit(ya, oracle, row, kind):
    check_key(ya, row, kind)
    hfs = hs.prototypes(row)
    rng = np.random.default_rng(SEED + hs.TABLE.index(row))
    x = hs.int_stream(rng, kind, stream_length(row))
    got = run_device(ya, row, kind, hfs, x)
    want = hs.oracle_chain(oracle, kind, row.family, hs.row_stages(row), hfs, x)
    assert got.shape == want.shape and want.any()
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError(f"{kind} {row.key} {row.shape}: {bad.size} of {want.size} outputs differ, the first at "
                             f"{bad[0]} (got {got[bad[0]]}, want {want[bad[0]]}), the last at {bad[-1]}")


def decimator_keys():
    """(row, kind) per decimator key: the row with the longest call, the sample types taken in turn"""
    best = {}
    for row in hs.TABLE:
        if row.family != "interp" and (row.key not in best or row.shape[1] > best[row.key].shape[1]):
            best[row.key] = row
    return [(row, row.kinds[i % len(row.kinds)]) for i, row in enumerate(best.values())]


def rand_stream(rng, kind, n):
    out = np.empty(n, np.float32 if kind == "rrrf" else np.complex64)
    for o in range(0, n, 1 << 22):
        c = min(1 << 22, n - o)
        out[o:o + c] = rand_samples(rng, kind, c)
    return out


def short_calls(ya, kind, ms, hfs, x, zeta):
    """the stages in processing order as Resamp2 objects, each fed in calls of at most SHORT samples"""
    item = x.dtype.itemsize
    src, n, keep = ya.DeviceArray.from_numpy(x), x.size, []
    for k, (m, hf) in enumerate(zip(ms, hfs)):
        q = ya.Resamp2(kind, hf, m)
        if k + 1 == len(ms):
            q.set_scale(zeta)
        dst = ya.DeviceArray(n // 2, x.dtype)
        for off in range(0, n, SHORT):
            cnt = min(SHORT, n - off)
            assert ya.plan_resamp2(item, ya.Resamp2.DECIM, m, cnt).chain == 0
            q.execute_block_dev(ya.Resamp2.DECIM, src.ptr + off * item, cnt, dst.ptr + (off // 2) * item)
        keep.append(src)                                            # alive while the next stage reads it
        src, n = dst, n // 2
    ya.synchronize()
    return src.to_numpy()


@pytest.mark.parametrize("row,kind", decimator_keys(), ids=[hs.case_id(r, k) for r, k in decimator_keys()])
def test_designed_taps_per_decimator_key(ya, oracle, row, kind):
    check_key(ya, row, kind)
    ms = hs.row_stages(row)
    hfs = [oracle.halfband_kaiser(m, 60.0) for m in ms]
    x = rand_stream(np.random.default_rng(SEED + 500 + hs.TABLE.index(row)), kind, stream_length(row))
    got = run_device(ya, row, kind, hfs, x)
    zeta = 1.0 if row.family == "resamp2" else 1.0 / (1 << len(ms))
    chain = short_calls(ya, kind, ms, hfs, x, zeta)
    assert np.array_equal(got, chain), (kind, row.key, row.shape, int(np.count_nonzero(got != chain)))
    want = hs.oracle_chain(oracle, kind, row.family, ms, hfs, x)
    err = rel_l2(got, want)
    print(f"halfband {kind} {row.key} {row.shape}: rel L2 against the oracle {err:.3e}")
    assert err <= 3e-6, (kind, row.key, err)
