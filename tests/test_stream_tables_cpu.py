"""The lane-major tables of the headline stream kernel are host code (yagi_amd/csrc/stream_tables.hpp, called by capi.hip):
a small program over the same builder dumps the table, and the paired parts are rebuilt here from the W_4096 part
and the six lane-indexed rows, in the pair layout the kernel's 16-byte loads read, and compared bit for bit -- the kernel
must multiply by the very values it gathered before.  The slots of the two scaled device tables (correction sum, FFT{h})
come from the same header and are checked to be that layout and a permutation."""
import subprocess

import numpy as np
import pytest

from conftest import ROOT

N_W, N_ROWS, N_MAIN, N_CORR = 4096, 6 * 256, 6 * 256, 6 * 64


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    d = tmp_path_factory.mktemp("stream_tables")
    exe = d / "stream_tables"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{ROOT / 'yagi_amd' / 'csrc'}",
                           str(ROOT / "tests" / "c" / "stream_tables_main.cpp"), "-o", str(exe)])
    raw = subprocess.check_output([str(exe)])
    ntab = N_W + N_ROWS + N_MAIN + N_CORR
    assert len(raw) == 8 * ntab + 4 * 512 + 4 * 4096
    tab = np.frombuffer(raw[: 8 * ntab], np.uint32).reshape(ntab, 2)
    slot = np.frombuffer(raw[8 * ntab: 8 * ntab + 4 * 512], np.uint32)
    hslot = np.frombuffer(raw[8 * ntab + 4 * 512:], np.uint32)
    return tab, slot, hslot


def test_w4096_and_rows_are_the_f64_values_rounded_once(dump):
    tab = dump[0]
    vals = tab.view(np.float32)
    m = np.arange(4096)
    a = -2.0 * np.pi * m / 4096.0
    want = np.stack([np.cos(a), np.sin(a)], 1)
    # libm and numpy may differ in the last bit of the f64 value: at most one f32 ulp (2^-24 at |w| <= 1) after rounding
    assert np.max(np.abs(vals[:4096].astype(np.float64) - want)) <= 2.0 ** -24
    t = np.arange(256)
    rows = tab[4096:4096 + N_ROWS].reshape(6, 256, 2)
    for k in range(4):
        assert np.array_equal(rows[k], tab[(t << k) & 4095])
    assert np.array_equal(rows[4], tab[((t & 15) * (t >> 4)) & 4095])
    assert np.array_equal(rows[5], tab[(16 * (((t & 15) * (t >> 4)) & 255)) & 4095])


def test_main_lane_table_is_the_six_rows_in_pairs(dump):
    """three arrays of 256 lanes x 2 entries: rows (0, 1), (2, 3), (4, 5) -- lane t's 16-byte load p at 16 t + 4096 p"""
    tab = dump[0]
    rows = tab[4096:4096 + N_ROWS].reshape(3, 2, 256, 2)
    main = tab[4096 + N_ROWS: 4096 + N_ROWS + N_MAIN].reshape(3, 256, 2, 2)
    assert np.array_equal(main, rows.transpose(0, 2, 1, 3))


def test_correction_lane_table_is_the_six_gathers(dump):
    tab = dump[0]
    corr = tab[4096 + N_ROWS + N_MAIN:].reshape(3, 64, 2, 2)          # pairs (w1 w2), (w4 u1), (u2 u4) of lane l
    l = np.arange(64)
    bp = l & 7
    for j, idx in enumerate((8 * l, 16 * l, 32 * l, 64 * bp, 128 * bp, 256 * bp)):     # freq_load_corr_fft's old gathers
        assert np.array_equal(corr[j // 2, :, j % 2], tab[idx]), j


def test_gc_slots_are_lane_pairs_and_a_permutation(dump):
    """entry l + 64 d of the correction table: pair array d // 2, lane l, half d % 2"""
    _, slot, hslot = dump
    assert sorted(slot.tolist()) == list(range(512))
    for l in range(64):
        for d in range(8):
            assert slot[l + 64 * d] == 128 * (d // 2) + 2 * l + d % 2
    # FFT{h}: lane t reads entries t + 256 d; its 16-byte load d // 2 sits at 16 t + 4096 (d // 2) bytes
    assert sorted(hslot.tolist()) == list(range(4096))
    t, d = np.meshgrid(np.arange(256), np.arange(16), indexing="ij")
    assert np.array_equal(hslot[t + 256 * d], 512 * (d // 2) + 2 * t + d % 2)
