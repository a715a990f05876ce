"""BurstDetector's kernels as built (burstdet_kernels.hip), read from the gfx950 code object as tests/test_autocorr_isa_cpu.py
reads Autocorr's: the two tile kernels (cccf, rrrf) and the stitch kernel are there, none uses scratch, the tile kernels
hold Autocorr's LDS for the same kind with energy plus 24 bytes (the pool base they broadcast, a hit flag per wave) and
stay within 64 KiB, and none holds an f32 fused multiply-add: the sums, the threshold test and the ratio keep every rounding (the
ratio is an f64 quotient, whose expansion holds f64 FMAs only).  No kernel's name matches Autocorr's pattern."""
import re
import subprocess

from test_autocorr_isa_cpu import F32_FMA, LLVM, _code_objects, _lds

# template arguments as mangled: <float>, <yagi_cf32>
TILE_KERNELS = {"burstdet_tile_kernelIfE": "rrrf", "burstdet_tile_kernelI9yagi_cf32E": "cccf"}
STITCH = "burstdet_stitch_kernel"


def test_burstdet_kernels_present_without_scratch_and_within_lds(tmp_path):
    found = {}
    for co in _code_objects(tmp_path):
        notes = subprocess.run([str(LLVM / "llvm-readelf"), "--notes", str(co)], capture_output=True, text=True).stdout
        for m in re.finditer(r"\.name:\s+(\S*burstdet_\w*kernel\S*)", notes):
            lo = notes.rfind("- .agpr_count", 0, m.start())
            hi = notes.find("- .agpr_count", m.end())
            found[m.group(1)] = notes[lo: hi if hi > 0 else len(notes)]
    assert len(found) == len(TILE_KERNELS) + 1, sorted(found)
    assert not [name for name in found if re.search(r"autocorr_\w*kernel", name)]
    for key in list(TILE_KERNELS) + [STITCH]:
        hits = [name for name in found if key in name]
        assert len(hits) == 1, (key, sorted(found))
        meta = found[hits[0]]
        pm = re.search(r"\.private_segment_fixed_size:\s+(\d+)", meta)
        assert pm and int(pm.group(1)) == 0, (hits[0], pm and pm.group(1))
        gm = re.search(r"\.group_segment_fixed_size:\s+(\d+)", meta)
        assert gm and int(gm.group(1)) <= 65536, (hits[0], gm and gm.group(1))
        if key in TILE_KERNELS:
            assert int(gm.group(1)) == _lds(TILE_KERNELS[key], True) + 24, (hits[0], gm.group(1))
        else:
            # 1024 tile slots of 16 bytes, their first segments and 256 more of 32 bytes, a ballot per wave
            assert int(gm.group(1)) == 1024 * 16 + 1024 * 32 + 256 * 32 + 16 * 8, (hits[0], gm.group(1))


def test_burstdet_kernels_have_no_f32_fma(tmp_path):
    seen = 0
    for co in _code_objects(tmp_path):
        syms = subprocess.run([str(LLVM / "llvm-readelf"), "-s", "-W", str(co)], capture_output=True, text=True).stdout
        names = sorted({l.split()[-1] for l in syms.splitlines() if "burstdet_" in l and "kernel" in l and " FUNC " in l})
        for name in names:
            dis = subprocess.run([str(LLVM / "llvm-objdump"), "-d", f"--disassemble-symbols={name}", str(co)],
                                 capture_output=True, text=True).stdout
            ops = [l.split("//")[0].strip() for l in dis.splitlines() if "\t" in l]
            ops = [o for o in ops if o]
            assert len(ops) > 50, (name, "not the device listing")
            if "tile" in name:
                assert sum(o.startswith("v_mul_f32") or o.startswith("v_pk_mul_f32") for o in ops) >= 1, name
                assert sum(o.startswith("v_div_scale_f64") for o in ops) >= 1, (name, "the ratio is an f64 quotient")
            bad = [o for o in ops if F32_FMA.match(o)]
            assert not bad, (name, bad[:4])
            seen += 1
    assert seen == len(TILE_KERNELS) + 1, seen
