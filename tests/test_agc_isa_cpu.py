"""Agc's kernels as built (agc_kernels.hip), read from the gfx950 code object: no scratch and no LDS (the state and the
rows requested ahead live in statically indexed registers), no f32 fused multiply-add, since every product and add of
the reference's loop keeps its own rounding, and none of the hardware's f32 approximations: ln, exp and log10 are the
library's f64 words, whose one quotient is an f64 division."""
import re
import shutil
import subprocess
from pathlib import Path

from conftest import ROOT

LIB = ROOT / "yagi_amd" / "libyagi_hip.so"
LLVM = Path("/opt/rocm/lib/llvm/bin")
F32_FMA = re.compile(r"^(v_fma_f32|v_fmac_f32|v_fmaak_f32|v_fmamk_f32|v_pk_fma_f32|v_mad_f32|v_mac_f32|v_fma_mix\w*)")
F32_APPROX = re.compile(r"^(v_log_f32|v_exp_f32|v_rcp_f32|v_rsq_f32|v_sqrt_f32|v_log_legacy_f32|v_exp_legacy_f32"
                        r"|v_rcp_iflag_f32)")
N_LOOP = 8         # agc_kernel<T, SQUELCH, STATUS>: two types, squelch off / on, status off / on
N_INIT = 2         # agc_init_kernel<T>


def _code_objects(tmp_path):
    so = tmp_path / "lib.so"
    shutil.copy(LIB, so)
    subprocess.run([str(LLVM / "llvm-objdump"), "--offloading", str(so)], capture_output=True, text=True, cwd=tmp_path)
    return sorted(tmp_path.glob("lib.so.*gfx950"))


def test_agc_kernels_use_no_scratch_and_no_lds(tmp_path):
    seen = 0
    for co in _code_objects(tmp_path):
        notes = subprocess.run([str(LLVM / "llvm-readelf"), "--notes", str(co)], capture_output=True, text=True).stdout
        for m in re.finditer(r"\.name:\s+(\S*agc_\w*kernel\S*)", notes):
            lo = notes.rfind("- .agpr_count", 0, m.start())
            hi = notes.find("- .agpr_count", m.end())
            meta = notes[lo: hi if hi > 0 else len(notes)]
            pm = re.search(r"\.private_segment_fixed_size:\s+(\d+)", meta)
            gm = re.search(r"\.group_segment_fixed_size:\s+(\d+)", meta)
            assert pm and int(pm.group(1)) == 0, (m.group(1), pm and pm.group(1))
            assert gm and int(gm.group(1)) == 0, (m.group(1), gm and gm.group(1))
            seen += 1
    assert seen == N_LOOP + N_INIT, seen


def test_agc_kernels_keep_every_rounding(tmp_path):
    seen = dividing = 0
    for co in _code_objects(tmp_path):
        syms = subprocess.run([str(LLVM / "llvm-readelf"), "-s", "-W", str(co)], capture_output=True, text=True).stdout
        names = sorted({l.split()[-1] for l in syms.splitlines() if "agc_" in l and "kernel" in l and " FUNC " in l})
        for name in names:
            dis = subprocess.run([str(LLVM / "llvm-objdump"), "-d", f"--disassemble-symbols={name}", str(co)],
                                 capture_output=True, text=True).stdout
            ops = [l.split("//")[0].strip() for l in dis.splitlines() if "\t" in l]
            ops = [o for o in ops if o]
            assert sum(o.startswith("v_mul_f32") or o.startswith("v_pk_mul_f32") for o in ops) >= 1, \
                (name, "not the device listing")
            bad = [o for o in ops if F32_FMA.match(o) or F32_APPROX.match(o)]
            assert not bad, (name, bad[:4])
            dividing += any(o.startswith("v_div_scale_f64") for o in ops)     # ln's quotient is an f64 division
            seen += 1
    assert seen == N_LOOP + N_INIT and dividing == N_LOOP, (seen, dividing)
