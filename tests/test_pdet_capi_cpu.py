"""PreambleDetector at the C ABI on a machine without a GPU: the constructor fails with DeviceError (no CPU fallback), bad
arguments are ConfigError before any device is asked for, and the constants and the event layout the Python package names
are the header's."""
import re

import numpy as np
import pytest

from conftest import ROOT, has_gpu

P = np.exp(1j * np.pi / 2 * np.arange(8)).astype(np.complex64)


@pytest.mark.skipif(has_gpu(), reason="checks the no-GPU error path")
def test_create_without_a_gpu_is_a_device_error():
    import yagi_amd as ya
    with pytest.raises(ya.DeviceError):
        ya.PreambleDetector(P, [0.0, 0.1], 0.5)
    with pytest.raises(ya.DeviceError):
        ya.PreambleDetector(np.ones(ya.PDET_LMAX, np.complex64), np.zeros(ya.PDET_KMAX, np.float32), 0.5, 0.0, 2 ** 40)


def test_bad_arguments_are_config_errors_with_or_without_a_gpu():
    import yagi_amd as ya
    ok = [0.0, 0.1]
    inf, nan = float("inf"), float("nan")
    huge = np.full(8, 3e19 + 0j, np.complex64)                     # its energy overflows f32
    bad = [(P[:0], ok, 0.5), (np.ones(ya.PDET_LMAX + 1, np.complex64), ok, 0.5),
           (P, [], 0.5), (P, np.zeros(ya.PDET_KMAX + 1, np.float32), 0.5),
           (P, [0.0, nan], 0.5), (P, [inf], 0.5), (P, [-inf, 0.0], 0.5),
           (np.zeros(8, np.complex64), ok, 0.5), (huge, ok, 0.5), (np.full(8, nan, np.complex64), ok, 0.5),
           (P, ok, 0.0), (P, ok, -0.5), (P, ok, nan), (P, ok, inf),
           (P, ok, 0.5, -1.0), (P, ok, 0.5, nan), (P, ok, 0.5, inf), (P, ok, 0.5, 0.0, 0)]
    for args in bad:
        with pytest.raises(ya.ConfigError):
            ya.PreambleDetector(*args)
        with pytest.raises(ya.ConfigError):
            ya.preamble_detect_host(np.zeros(4, np.complex64), *args)
    for kind in ("rrrf", "crcf", "cccc"):
        with pytest.raises(ya.ConfigError):
            ya.PreambleDetector(P, ok, 0.5, kind=kind)
        with pytest.raises(ya.ConfigError):
            ya.preamble_detect_host(np.zeros(4, np.complex64), P, ok, 0.5, kind=kind)
    for p, dphi in [(P[:0], ok), (np.ones(ya.PDET_LMAX + 1, np.complex64), ok), (P, []),
                    (P, np.zeros(ya.PDET_KMAX + 1, np.float32)), (P, [nan])]:
        with pytest.raises(ya.ConfigError):
            ya.preamble_templates(p, dphi)


def test_python_constants_and_event_layout_equal_the_header():
    import yagi_amd as ya
    import pdet_ref as pr
    hdr = (ROOT / "include" / "yagi_hip.h").read_text()
    for name, ours, refs in (("LMAX", ya.PDET_LMAX, pr.LMAX), ("KMAX", ya.PDET_KMAX, pr.KMAX),
                             ("TILE", ya.PDET_TILE, pr.TILE), ("SEGMAX", ya.PDET_SEGMAX, pr.SEGMAX)):
        assert ours == int(re.search(rf"#define YAGI_PDET_{name} (\d+)", hdr).group(1)) == refs
    assert (ya.PDET_LMAX, ya.PDET_KMAX, ya.PDET_SEGMAX) == (1024, 32, 8192)
    body = re.search(r"typedef struct yagi_preamble_event \{(.*?)\} yagi_preamble_event;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    types = {"uint64_t": np.uint64, "float": np.float32, "uint32_t": np.uint32}
    fields = []
    for ctype, names in re.findall(r"(uint64_t|uint32_t|float)\s+([^;]+);", body):
        fields += [(n.strip(), types[ctype]) for n in names.split(",")]
    assert np.dtype(fields) == ya.PREAMBLE_EVENT == pr.EVENT
    assert ya.PREAMBLE_EVENT.itemsize == 48 and ya.PREAMBLE_EVENT.fields["hypothesis"][1] == 40
    assert ya.PREAMBLE_EVENT.fields["ratio"][1] == 24
