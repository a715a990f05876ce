"""Modem's kernels as built (modem_kernels.hip), read from the gfx950 code object: the expected set of kernels, no scratch
anywhere, and no f32 fused multiply-add in the decision and soft-bit kernels, whose residuals, squared distances and soft
metrics must round every operation on its own.

The PSK and DPSK demodulators call the device library's atan2f (and DPSK sincosf for x_hat).  Those routines evaluate
their own polynomials with fused operations, which is their business and inside the few-ulp error the tests allow them;
so for these two kinds the FMA check cannot be made on the whole kernel and is made on the kinds that share the same
decision and soft-bit source (md_demod) without a library call: ASK, QAM, BPSK, QPSK, OOK and Arb."""
import re
import shutil
import subprocess
from pathlib import Path

from conftest import ROOT

LIB = ROOT / "yagi_amd" / "libyagi_hip.so"
LLVM = Path("/opt/rocm/lib/llvm/bin")
F32_FMA = re.compile(r"^(v_fma_f32|v_fmac_f32|v_fmaak_f32|v_fmamk_f32|v_pk_fma_f32|v_mad_f32|v_mac_f32|v_fma_mix\w*)")
# kinds as in kernels.hpp: PSK 0, DPSK 1, ASK 2, QAM 3, BPSK 4, QPSK 5, OOK 6; Arb has a kernel of its own
N_DEMOD = 2 * (8 + 8 + 8 + 7 + 1 + 1 + 1)      # {hard, soft} x (PSK, DPSK, ASK bps 1..8, QAM 2..8, BPSK, QPSK, OOK)
N_ARB = 2 * 8                                  # {hard, soft} x bps 1..8
N_MOD = 2 + 1 + 2                              # check {plain, DPSK}, scan, modulate {plain, DPSK}
N_KERNELS = N_DEMOD + N_ARB + N_MOD
N_LIBM = 2 * (8 + 8)                           # the PSK and DPSK demodulators


def _code_objects(tmp_path):
    so = tmp_path / "lib.so"
    shutil.copy(LIB, so)
    subprocess.run([str(LLVM / "llvm-objdump"), "--offloading", str(so)], capture_output=True, text=True, cwd=tmp_path)
    return sorted(tmp_path.glob("lib.so.*gfx950"))


def _kernel_names(co):
    syms = subprocess.run([str(LLVM / "llvm-readelf"), "-s", "-W", str(co)], capture_output=True, text=True).stdout
    return sorted({l.split()[-1] for l in syms.splitlines() if re.search(r"modem_\w+_kernel", l) and " FUNC " in l})


def test_modem_kernels_use_no_scratch(tmp_path):
    seen = 0
    for co in _code_objects(tmp_path):
        notes = subprocess.run([str(LLVM / "llvm-readelf"), "--notes", str(co)], capture_output=True, text=True).stdout
        for m in re.finditer(r"\.name:\s+(\S*modem_\w+_kernel\S*)", notes):
            lo = notes.rfind("- .agpr_count", 0, m.start())
            hi = notes.find("- .agpr_count", m.end())
            meta = notes[lo: hi if hi > 0 else len(notes)]
            pm = re.search(r"\.private_segment_fixed_size:\s+(\d+)", meta)
            assert pm and int(pm.group(1)) == 0, (m.group(1), pm and pm.group(1))
            seen += 1
    assert seen == N_KERNELS, seen


def test_modem_kernel_set(tmp_path):
    names = [n for co in _code_objects(tmp_path) for n in _kernel_names(co)]
    assert len(names) == N_KERNELS, len(names)
    assert sum("modem_demod_kernel" in n for n in names) == N_DEMOD
    assert sum("modem_arb_kernel" in n for n in names) == N_ARB
    assert sum("modem_check_kernel" in n or "modem_scan_kernel" in n or "modem_modulate_kernel" in n for n in names) == N_MOD


def test_modem_decision_kernels_have_no_f32_fma(tmp_path):
    seen = libm = 0
    for co in _code_objects(tmp_path):
        for name in _kernel_names(co):
            if "modem_demod_kernel" not in name and "modem_arb_kernel" not in name:
                continue
            dis = subprocess.run([str(LLVM / "llvm-objdump"), "-d", f"--disassemble-symbols={name}", str(co)],
                                 capture_output=True, text=True).stdout
            ops = [l.split("//")[0].strip() for l in dis.splitlines() if "\t" in l]
            ops = [o for o in ops if o]
            assert any(o.startswith("s_endpgm") for o in ops), (name, "not the device listing")
            # itanium mangling of <KIND, BPS, SOFT>: ...ILi<kind>ELi<bps>ELb<soft>E...
            km = re.search(r"modem_demod_kernelILi(\d)ELi(\d)ELb([01])E", name)
            if km and km.group(1) in "01":
                libm += 1                                   # atan2f / sincosf inside: see the module docstring
                continue
            if "modem_arb_kernel" in name:                  # the table loop: distances from separate products and one add
                assert any(o.startswith("v_mul_f32") or o.startswith("v_pk_mul_f32") for o in ops), name
                assert any(o.startswith("ds_read_b64") or o.startswith("ds_read2_b32") or o.startswith("ds_read_b128")
                           or o.startswith("ds_read2_b64") for o in ops), name
            bad = [o for o in ops if F32_FMA.match(o)]
            assert not bad, (name, bad[:4])
            seen += 1
    assert libm == N_LIBM, libm
    assert seen == N_DEMOD + N_ARB - N_LIBM, seen


def test_modem_block_bytes_move_sixteen_at_a_time(tmp_path):
    """Every demodulating kernel stores its symbols and soft bytes 16 at a time: x_hat leaves 8 bytes per lane and the state
    in dwords, so the only dwordx4 stores of these kernels are md_store_bytes', which each kernel must hold once per byte
    output (symbols; symbols and soft bytes).  The modulating kernels load 16 symbols per lane at once and store two
    points (16 bytes) per lane and step."""
    demod = mod = 0
    for co in _code_objects(tmp_path):
        for name in _kernel_names(co):
            is_demod = "modem_demod_kernel" in name or "modem_arb_kernel" in name
            if not is_demod and "modem_modulate_kernel" not in name:
                continue
            dis = subprocess.run([str(LLVM / "llvm-objdump"), "-d", f"--disassemble-symbols={name}", str(co)],
                                 capture_output=True, text=True).stdout
            ops = [l.split("//")[0].strip() for l in dis.splitlines() if "\t" in l]
            st16 = sum(o.startswith("global_store_dwordx4") for o in ops)
            if is_demod:
                soft = re.search(r"ELb1EEEv", name) is not None
                assert st16 >= (2 if soft else 1), (name, st16)
                assert not any(o.startswith("global_store_short") for o in ops), name
                demod += 1
            else:
                assert st16 >= 1, name
                assert any(o.startswith("global_load_dwordx4") for o in ops), name
                mod += 1
    assert demod == N_DEMOD + N_ARB, demod
    assert mod == 2, mod
