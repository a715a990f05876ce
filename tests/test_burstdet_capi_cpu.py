"""BurstDetector at the C ABI on a machine without a GPU: the constructor fails with DeviceError (no CPU fallback), bad
arguments are ConfigError before any device is asked for, and the constants and the event layout the Python package names
are the header's."""
import re

import numpy as np
import pytest

from conftest import ROOT, has_gpu


@pytest.mark.skipif(has_gpu(), reason="checks the no-GPU error path")
def test_create_without_a_gpu_is_a_device_error():
    import yagi_amd as ya
    for kind in ("cccf", "rrrf"):
        with pytest.raises(ya.DeviceError):
            ya.BurstDetector(kind, 8, 8, 0.5)


def test_bad_arguments_are_config_errors_with_or_without_a_gpu():
    import yagi_amd as ya
    for kind in ("cccf", "rrrf"):
        for args in [(0, 1, 0.5), (ya.AUTOCORR_WMAX + 1, 1, 0.5), (8, ya.AUTOCORR_DMAX + 1, 0.5), (8, 8, 0.0),
                     (8, 8, -0.5), (8, 8, float("nan")), (8, 8, float("inf")), (8, 8, 0.5, -1.0),
                     (8, 8, 0.5, float("nan")), (8, 8, 0.5, float("inf")), (8, 8, 0.5, 0.0, 0)]:
            with pytest.raises(ya.ConfigError):
                ya.BurstDetector(kind, *args)
    with pytest.raises(ya.ConfigError):
        ya.BurstDetector("crcf", 8, 8, 0.5)


def test_python_constants_and_event_layout_equal_the_header():
    import yagi_amd as ya
    import burstdet_ref as bdr
    hdr = (ROOT / "include" / "yagi_hip.h").read_text()
    assert ya.BURSTDET_SEGMAX == int(re.search(r"#define YAGI_BURSTDET_SEGMAX (\d+)", hdr).group(1)) == bdr.SEGMAX == 8192
    body = re.search(r"typedef struct yagi_burst_event \{(.*?)\} yagi_burst_event;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for ctype, names in re.findall(r"(uint64_t|float)\s+([^;]+);", body):
        fields += [(n.strip(), np.uint64 if ctype == "uint64_t" else np.float32) for n in names.split(",")]
    assert np.dtype(fields) == ya.BURST_EVENT == bdr.EVENT
    assert ya.BURST_EVENT.itemsize == 40 and ya.BURST_EVENT.fields["ratio"][1] == 24
