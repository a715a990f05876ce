"""Autocorr at the C ABI on a machine without a GPU: the constructor fails with DeviceError (no CPU fallback), and the
limits the Python package names are the header's."""
import re

import pytest

from conftest import ROOT, has_gpu


@pytest.mark.skipif(has_gpu(), reason="checks the no-GPU error path")
def test_create_without_a_gpu_is_a_device_error():
    import yagi_amd as ya
    for kind in ("cccf", "rrrf"):
        with pytest.raises(ya.DeviceError):
            ya.Autocorr(kind, 8, 8)


def test_python_constants_equal_the_header():
    import yagi_amd as ya
    hdr = (ROOT / "include" / "yagi_hip.h").read_text()
    for name in ("WMAX", "DMAX", "TILE"):
        want = int(re.search(rf"#define YAGI_AUTOCORR_{name} (\d+)", hdr).group(1))
        assert getattr(ya, f"AUTOCORR_{name}") == want, name
    assert (ya.AUTOCORR_WMAX, ya.AUTOCORR_DMAX) == (1024, 65536)
    import autocorr_ref as acr
    assert (acr.WMAX, acr.DMAX, acr.TILE) == (ya.AUTOCORR_WMAX, ya.AUTOCORR_DMAX, ya.AUTOCORR_TILE)
