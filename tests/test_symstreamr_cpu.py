"""SymStreamR's schedule and argument checks, without a GPU: the planner's need(q) against the reference's control loop
run sample by sample (resamp_util.loop_count), its split of the rate against msresamp.rs:33-51, the bound on the
leftover, ConfigError before any device is asked for and DeviceError from the constructor where there is none."""
import ctypes as C

import numpy as np
import pytest

import resamp_util as ru
from conftest import has_gpu
from symstream_ref import golden_generator
from symstreamr_ref import fl32_rate, need, stages

# bw -> (half-band stages, rate of the arbitrary stage): 0.5, 0.649.., 1.0, 1.25, 2.0 and 1.0417 are the rates asked for
RATES = {1.0: (0, 0.5), 0.77: (0, 0.64935064), 0.5: (0, 1.0), 0.4: (0, 1.25), 0.25: (0, 2.0), 0.03: (4, 1.0416667)}
STAGES = {1.0: 0, 0.77: 0, 0.5: 0, 0.4: 0, 0.25: 0, 0.2: 1, 0.03: 4, 0.001: 8}


@pytest.mark.parametrize("bw", sorted(RATES))
def test_need_against_the_control_loop_sample_by_sample(bw):
    import yagi_amd as ya
    ns, ra = RATES[bw]
    assert stages(fl32_rate(bw))[1:] == (ns, np.float32(ra))
    step = ru.rust_step(np.float32(ra))
    rng = np.random.default_rng(int(bw * 1000))
    for p0 in [0, step - 1] + [int(v) for v in rng.integers(0, step, 62)]:
        # the loop, one input at a time: outputs so far and the phase after each input
        cum, phases, p = [0], [p0], p0
        while cum[-1] < 301:
            c, p = ru.loop_count(p, step, 1)
            cum.append(cum[-1] + c)
            phases.append(p)
        for q in range(301):
            nx = next(i for i, c in enumerate(cum) if c >= q)
            plan = ya.plan_symstreamr(bw, 7, q << ns, p0)
            assert plan.step == step and plan.q == q
            assert plan.need == nx == need(p0, step, q), (bw, p0, q)
            assert plan.outputs_arb == cum[nx] and plan.phase_next == phases[nx], (bw, p0, q)
            assert plan.outputs == cum[nx] << ns and plan.leftover == (cum[nx] - q) << ns


@pytest.mark.parametrize("bw", sorted(STAGES))
def test_split_of_the_rate(bw):
    import yagi_amd as ya
    interp, ns, ra = stages(fl32_rate(bw))
    plan = ya.plan_symstreamr(bw, 7, 1000)
    assert (plan.interp, plan.stages, plan.rate_arb, plan.rate) == (int(interp), ns, ra, fl32_rate(bw))
    assert ns == STAGES[bw] and np.float32(0.5) <= ra <= np.float32(2.0)
    assert interp == (bw < 0.5)                       # the half-band decimator chain never occurs
    assert plan.step == ru.rust_step(ra)
    assert plan.tile == ya.plan_resamp(8, 14, plan.step).tile and 1 <= plan.wg_tiles <= plan.max_wg_tiles
    assert plan.lds <= 64 * 1024


def test_leftover_never_exceeds_two_groups():
    import yagi_amd as ya
    rng = np.random.default_rng(7)
    for bw in list(STAGES) + [float(v) for v in rng.uniform(0.001, 1.0, 40)]:
        ns = ya.plan_symstreamr(bw, 7, 1).stages
        step = ya.plan_symstreamr(bw, 7, 1).step
        for n, p0 in zip(rng.integers(1, 1 << 20, 50), rng.integers(0, step, 50)):
            plan = ya.plan_symstreamr(bw, 7, int(n), int(p0))
            assert plan.outputs >= n and plan.leftover == plan.outputs - n
            assert plan.leftover < 2 << ns, (bw, n, p0, plan)
            assert ru.num_output(int(p0), step, plan.need - 1)[0] << ns < n        # one sample fewer does not cover n


def _create(ya, src, ftype, bw, m, beta, scheme):
    """the C entry point itself: src may be None (a null handle), which is all a machine without a GPU can pass"""
    hd = C.c_void_p()
    rc = ya.lib.yagi_hip_symstreamrcf_create_linear(int(ftype), bw, m, beta, int(scheme), None if src is None else src._h,
                                                    C.byref(hd))
    if rc == 0:
        ya._check(ya.lib.yagi_hip_symstreamrcf_destroy(hd))
    else:
        assert not hd.value
    ya._check(rc)


def test_bad_arguments_are_config_errors_with_or_without_a_gpu():
    """every check comes before the device is asked for, the null source last: without a GPU no MSequence can be made,
    so the source is null there and every call below is a ConfigError for its own reason or for that one"""
    import yagi_amd as ya
    S, F = ya.ModulationScheme, ya.FirFilterShape
    src = ya.MSequence(*golden_generator(23)) if has_gpu() else None
    for bw in (0.0009, 1.001, 0.0, -0.5, float("nan"), float("inf"), float("-inf")):
        with pytest.raises(ya.ConfigError, match="bandwidth"):
            _create(ya, src, F.Arkaiser, bw, 7, 0.3, S.Qpsk)
        with pytest.raises(ya.ConfigError, match="bandwidth"):
            ya.plan_symstreamr(bw, 7, 100)
    for args, why in [((F.Arkaiser, 0.4, 0, 0.3, S.Qpsk), "delay"), ((F.Arkaiser, 0.4, 7, 1.5, S.Qpsk), "excess bandwidth"),
                      ((F.Arkaiser, 0.4, 7, -0.1, S.Qpsk), "excess bandwidth"),
                      ((F.Arkaiser, 0.4, 7, float("nan"), S.Qpsk), "excess bandwidth"),
                      ((F.Arkaiser, 0.4, 7, 0.3, 999), None), ((999, 0.4, 7, 0.3, S.Qpsk), None)]:
        with pytest.raises(ya.ConfigError, match=why) as e:       # whatever SymStream's create_linear refuses
            _create(ya, src, *args)
        assert "null handle" not in str(e.value)
    with pytest.raises(ya.ConfigError, match="null handle"):
        _create(ya, None, F.Arkaiser, 0.4, 7, 0.3, S.Qpsk)
    with pytest.raises(ya.ConfigError):
        ya.plan_symstreamr(0.4, 0, 100)
    if src is not None:
        _create(ya, src, F.Arkaiser, 0.4, 7, 0.3, S.Qpsk)
        _create(ya, src, F.Arkaiser, 0.001, 7, 0.3, S.Qpsk)
        _create(ya, src, F.Arkaiser, 1.0, 7, 0.3, S.Qpsk)


@pytest.mark.skipif(has_gpu(), reason="checks the no-GPU error path")
def test_create_without_a_gpu_is_a_device_error():
    """no CPU fallback: the source a SymStreamR needs is already a DeviceError, so the constructor cannot be reached
    with valid arguments on such a machine"""
    import yagi_amd as ya
    with pytest.raises(ya.DeviceError):
        ya.SymStreamR(ya.FirFilterShape.Arkaiser, 0.4, 7, 0.3, ya.ModulationScheme.Qpsk, ya.MSequence(*golden_generator(23)))
