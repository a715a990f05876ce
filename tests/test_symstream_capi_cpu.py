"""SymStream at the C ABI on a machine without a GPU.  An MSequence cannot be made there (no CPU fallback), so what the
host-only build can check is everything create decides before it needs the source or the device: the reference's own
argument checks (symstream.rs:31-39), Modem's scheme errors, the design's errors, the null source; and that a null
handle is refused by every entry point instead of being dereferenced."""
import ctypes as C

import numpy as np
import pytest

from conftest import has_gpu


def _create_linear(ya, ftype, k, m, beta, scheme, src=None):
    h = C.c_void_p()
    rc = ya.lib.yagi_hip_symstreamcf_create_linear(int(ftype), k, m, beta, int(scheme), src, C.byref(h))
    return rc, h.value, ya.lib.yagi_hip_last_error().decode()


def test_create_linear_argument_errors_come_first():
    import yagi_amd as ya
    F, S = ya.FirFilterShape, ya.ModulationScheme
    CONFIG = 2
    for args, what in [((F.Arkaiser, 1, 7, 0.3, S.Qpsk), "samples/symbol"), ((F.Arkaiser, 2, 0, 0.3, S.Qpsk), "filter delay"),
                       ((F.Arkaiser, 2, 7, -0.1, S.Qpsk), "excess bandwidth"), ((F.Arkaiser, 2, 7, 1.5, S.Qpsk), "excess bandwidth"),
                       ((F.Arkaiser, 2, 7, float("nan"), S.Qpsk), "excess bandwidth"),
                       ((F.Arkaiser, 2, 7, 0.3, S.Apsk16), "not built"), ((F.Arkaiser, 2, 7, 0.3, S.Arb), "from_table"),
                       ((F.Arkaiser, 2, 7, 0.3, 99), "not supported"), ((F.Pm, 2, 7, 0.3, S.Qpsk), "not built"),
                       ((F.Arkaiser, 2, 1, 0.05, S.Qpsk), "leaves (0, 1)"), ((F.Arkaiser, 2, 7, 1.0, S.Qpsk), "(0,1)"),
                       ((F.Rrcos, 2, 7, 0.0, S.Qpsk), "out of range"), ((F.Arkaiser, 2, 7, 0.3, S.Qpsk), "null handle")]:
        rc, h, msg = _create_linear(ya, *args)
        assert rc == CONFIG and h is None and what in msg, (args, rc, msg)


def test_create_taps_argument_errors_come_first():
    import yagi_amd as ya
    S = ya.ModulationScheme
    h = np.ones(9, np.float32)
    out = C.c_void_p()
    fn = ya.lib.yagi_hip_symstreamcf_create_taps
    for k, hp, hl, scheme, what in [(1, h.ctypes.data, 9, S.Qpsk, "samples/symbol"), (2, None, 9, S.Qpsk, "null pointer"),
                                    (4, h.ctypes.data, 3, S.Qpsk, "filter length"), (2, h.ctypes.data, 9, S.V29, "not built"),
                                    (2, h.ctypes.data, 9, S.Qpsk, "null handle")]:
        rc = fn(k, hp, hl, int(scheme), None, C.byref(out))
        assert rc == 2 and out.value is None and what in ya.lib.yagi_hip_last_error().decode(), (k, hl, scheme)
    assert ya.lib.yagi_hip_symstreamcf_create_linear(6, 2, 7, 0.3, int(S.Qpsk), None, None) == 2     # null out pointer


def test_null_handles_are_config_errors():
    import yagi_amd as ya
    lib = ya.lib
    v = C.c_size_t()
    assert lib.yagi_hip_symstreamcf_get_k(None, C.byref(v)) == 2
    assert lib.yagi_hip_symstreamcf_get_delay(None, C.byref(v)) == 2
    assert lib.yagi_hip_symstreamcf_reset(None) == 2
    assert lib.yagi_hip_symstreamcf_set_gain(None, 1.0) == 2
    assert lib.yagi_hip_symstreamcf_set_scheme(None, 40) == 2
    assert lib.yagi_hip_symstreamcf_write_samples(None, None, 4) == 2
    assert lib.yagi_hip_symstreamcf_write_samples_dev(None, None, 4) == 2
    assert lib.yagi_hip_symstreamcf_modulate_symbols(None, None, 4, None) == 2
    out = C.c_void_p()
    assert lib.yagi_hip_symstreamcf_clone(None, C.byref(out)) == 2
    assert lib.yagi_hip_symstreamcf_destroy(None) == 0           # like free(NULL)


def test_shape_enum_is_the_header_s():
    import re

    import yagi_amd as ya
    from conftest import ROOT
    hdr = (ROOT / "include" / "yagi_hip.h").read_text()
    body = re.search(r"enum yagi_fir_shape \{(.*?)\};", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [t.strip() for t in body.split(",") if t.strip()]
    assert names[-1].replace(" ", "") == "YAGI_FIR_SHAPE_UNKNOWN=-1"
    first = names[0].replace(" ", "")
    assert first == "YAGI_FIR_SHAPE_KAISER=0"
    want = ["Kaiser", "Pm", "Rcos", "Fexp", "Fsech", "Farcsech", "Arkaiser", "Rkaiser", "Rrcos", "Hm3", "Gmsktx", "Gmskrx",
            "Rfexp", "Rfsech", "Rfarcsech"]                         # design/mod.rs:41-77
    got = ["KAISER"] + [n.replace("YAGI_FIR_SHAPE_", "") for n in names[1:-1]]
    assert [w.upper() for w in want] == got
    assert [int(ya.FirFilterShape[w]) for w in want] == list(range(15)) and int(ya.FirFilterShape.Unknown) == -1


@pytest.mark.skipif(has_gpu(), reason="checks the no-GPU error path")
def test_the_source_itself_needs_a_device():
    import yagi_amd as ya
    with pytest.raises(ya.DeviceError):
        ya.MSequence(23, 4325376)
