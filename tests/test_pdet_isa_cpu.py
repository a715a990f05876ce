"""PreambleDetector's kernels as built (pdet_kernels.hip), read from the gfx950 code object as tests/test_burstdet_isa_cpu.py
reads BurstDetector's: the tile, the stitch and the correlate kernel are there, none uses scratch, the tile and the
correlate kernel hold the LDS that YAGI_PDET_TILE, YAGI_PDET_LMAX and the workgroup of 256 lanes imply and stay within 64 KiB,
and none holds an f32 fused multiply-add: the sums, the threshold test and the ratio keep every rounding (the ratio is
an f64 quotient, whose expansion holds f64 FMAs only).  No kernel's name matches Autocorr's or BurstDetector's pattern."""
import re
import subprocess

from conftest import ROOT
from test_autocorr_isa_cpu import F32_FMA, LLVM, WG, _code_objects

KERNELS = ("pdet_tile_kernel", "pdet_stitch_kernel", "pdet_correlate_kernel")


def _bank_lds():
    """per staged sample (TILE + LMAX of them, in rows of TILE / 256 padded by 16 bytes) the sample, two floats, and in rows
    of its own its energy term"""
    hdr = (ROOT / "include" / "yagi_hip.h").read_text()
    tile, lmax = (int(re.search(rf"#define YAGI_PDET_{name} (\d+)", hdr).group(1)) for name in ("TILE", "LMAX"))
    r = tile // WG
    rows = (tile + lmax) // r
    return rows * (r * 8 + 16) + rows * (r * 4 + 16)


def test_pdet_kernels_present_without_scratch_and_within_lds(tmp_path):
    found = {}
    for co in _code_objects(tmp_path):
        notes = subprocess.run([str(LLVM / "llvm-readelf"), "--notes", str(co)], capture_output=True, text=True).stdout
        for m in re.finditer(r"\.name:\s+(\S*pdet_\w*kernel\S*)", notes):
            lo = notes.rfind("- .agpr_count", 0, m.start())
            hi = notes.find("- .agpr_count", m.end())
            found[m.group(1)] = notes[lo: hi if hi > 0 else len(notes)]
    assert not [name for name in found if re.search(r"(autocorr|burstdet)_\w*kernel", name)]
    for key in KERNELS:
        hits = [name for name in found if key in name]
        assert len(hits) == 1, (key, sorted(found))
        meta = found[hits[0]]
        pm = re.search(r"\.private_segment_fixed_size:\s+(\d+)", meta)
        assert pm and int(pm.group(1)) == 0, (hits[0], pm and pm.group(1))
        gm = re.search(r"\.group_segment_fixed_size:\s+(\d+)", meta)
        assert gm and int(gm.group(1)) <= 65536, (hits[0], gm and gm.group(1))
        if key == "pdet_tile_kernel":
            # the pool base the last lane broadcasts and a hit flag per wave besides
            assert int(gm.group(1)) == _bank_lds() + 24, (hits[0], gm.group(1))
        elif key == "pdet_correlate_kernel":
            assert int(gm.group(1)) == _bank_lds(), (hits[0], gm.group(1))
        else:
            # 1024 tile slots of 16 bytes, their first segments and 256 more of 32 bytes, a ballot per wave
            assert int(gm.group(1)) == 1024 * 16 + 1024 * 32 + 256 * 32 + 16 * 8, (hits[0], gm.group(1))


def test_pdet_kernels_have_no_f32_fma(tmp_path):
    seen = set()
    for co in _code_objects(tmp_path):
        syms = subprocess.run([str(LLVM / "llvm-readelf"), "-s", "-W", str(co)], capture_output=True, text=True).stdout
        names = sorted({l.split()[-1] for l in syms.splitlines() if "pdet_" in l and "kernel" in l and " FUNC " in l})
        for name in names:
            dis = subprocess.run([str(LLVM / "llvm-objdump"), "-d", f"--disassemble-symbols={name}", str(co)],
                                 capture_output=True, text=True).stdout
            ops = [l.split("//")[0].strip() for l in dis.splitlines() if "\t" in l]
            ops = [o for o in ops if o]
            if "advance" in name:
                continue                                           # two stores, no arithmetic
            assert len(ops) > 50, (name, "not the device listing")
            if "tile" in name or "correlate" in name:
                assert sum(o.startswith("v_mul_f32") or o.startswith("v_pk_mul_f32") for o in ops) >= 1, name
            if "tile" in name:
                assert sum(o.startswith("v_div_scale_f64") for o in ops) >= 1, (name, "the ratio is an f64 quotient")
            bad = [o for o in ops if F32_FMA.match(o)]
            assert not bad, (name, bad[:4])
            seen.add(next(k for k in KERNELS if k in name))
    assert seen == set(KERNELS), seen
