"""ctypes binding of libyagi_hip.so (include/yagi_hip.h).

Loading rules
  * The library is built in-tree (yagi_amd/libyagi_hip.so) by ``__graft_entry__.build()`` or
    ``make -C yagi_amd/csrc``.  If it is missing this module raises ImportError -- there is no
    CPU fallback anywhere in the package.
  * torch is imported first when available so the process holds ONE HIP runtime (torch's
    bundled libamdhip64 has the SONAME our DT_NEEDED asks for; see csrc/Makefile).
"""
import ctypes as C
import os
from pathlib import Path

_HERE = Path(__file__).resolve().parent
# YAGI_HIP_LIB lets the kernel-tuning scripts under tools/ load an alternative build of the SAME
# library (different compile flags); it is never a different back-end.
LIB_PATH = Path(os.environ.get("YAGI_HIP_LIB") or (_HERE / "libyagi_hip.so"))


class cf32(C.Structure):
    """num_complex::Complex<f32> / yagi_cf32"""
    _fields_ = [("re", C.c_float), ("im", C.c_float)]


def _load():
    if not LIB_PATH.exists():
        raise ImportError(
            f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C yagi_amd/csrc`; yagi_amd has no CPU fallback")
    if os.environ.get("YAGI_NO_TORCH_PRELOAD", "0") != "1":
        try:
            import torch  # noqa: F401  (maps torch's HIP runtime before ours is resolved)
        except Exception:
            pass
    return C.CDLL(str(LIB_PATH))


lib = _load()

vp, sz, ci, f32, u64 = C.c_void_p, C.c_size_t, C.c_int, C.c_float, C.c_uint64
pvp = C.POINTER(C.c_void_p)


def _sig(name, *argtypes, restype=ci):
    fn = getattr(lib, name)
    fn.argtypes = list(argtypes)
    fn.restype = restype
    return fn


_sig("yagi_hip_last_error", restype=C.c_char_p)
_sig("yagi_hip_version", restype=C.c_char_p)
_sig("yagi_hip_device_count", C.POINTER(ci))
_sig("yagi_hip_set_device", ci)
_sig("yagi_hip_malloc", pvp, sz)
_sig("yagi_hip_free", vp)
_sig("yagi_hip_memcpy_h2d", vp, vp, sz)
_sig("yagi_hip_memcpy_d2h", vp, vp, sz)
_sig("yagi_hip_memset_dev", vp, ci, sz)
_sig("yagi_hip_device_synchronize")
_sig("yagi_hip_stream_synchronize", vp)
_sig("yagi_hip_gen_real_dev", u64, u64, sz, vp, vp)
_sig("yagi_hip_gen_complex_dev", u64, u64, sz, vp, vp)
_sig("yagi_hip_fir_design_kaiser", sz, f32, f32, f32, vp)
_sig("yagi_hip_estimate_req_filter_stopband_attenuation", f32, sz, C.POINTER(f32))
_sig("yagi_hip_fir_design_prototype", ci, sz, sz, f32, f32, vp)

for _k in ("rrrf", "rccf", "crcf", "cccf"):
    _sig(f"yagi_hip_dotprod_{_k}", vp, vp, sz, vp)
    _sig(f"yagi_hip_dotprod_{_k}_dev", vp, vp, sz, vp, vp)

# (T, C) ctypes for by-value scalar arguments
KIND_TYPES = {"rrrf": (f32, f32), "crcf": (cf32, f32), "cccf": (cf32, cf32)}

for _k, (_T, _Cc) in KIND_TYPES.items():
    p = f"yagi_hip_firfilt_{_k}_"
    _sig(p + "create", vp, sz, pvp)
    _sig(p + "create_kaiser", sz, f32, f32, f32, pvp)
    _sig(p + "create_rnyquist", ci, sz, sz, f32, f32, pvp)
    _sig(p + "freqresponse", vp, f32, vp)
    _sig(p + "groupdelay", vp, f32, vp)
    _sig(p + "create_rect", sz, pvp)
    _sig(p + "create_dc_blocker", sz, f32, pvp)
    _sig(p + "create_notch", sz, f32, f32, pvp)
    _sig(p + "destroy", vp)
    _sig(p + "clone", vp, pvp)
    _sig(p + "set_stream", vp, vp)
    _sig(p + "set_coefficients", vp, vp, sz)
    _sig(p + "reset", vp)
    _sig(p + "push", vp, _T)
    _sig(p + "write", vp, vp, sz)
    _sig(p + "execute", vp, vp)
    _sig(p + "execute_one", vp, _T, vp)
    _sig(p + "execute_block", vp, vp, sz, vp, sz)
    _sig(p + "execute_block_dev", vp, vp, sz, vp)
    _sig(p + "set_pipeline", vp, ci)
    _sig(p + "join", vp)
    _sig(p + "set_scale", vp, _Cc)
    _sig(p + "get_scale", vp, vp)
    _sig(p + "get_length", vp, C.POINTER(sz))
    _sig(p + "get_coefficients", vp, vp, sz)
    p = f"yagi_hip_firdecim_{_k}_"
    _sig(p + "create", sz, vp, sz, pvp)
    _sig(p + "create_kaiser", sz, sz, f32, pvp)
    _sig(p + "create_prototype", ci, sz, sz, f32, f32, pvp)
    _sig(p + "destroy", vp)
    _sig(p + "clone", vp, pvp)
    _sig(p + "set_stream", vp, vp)
    _sig(p + "reset", vp)
    _sig(p + "get_decim_rate", vp, C.POINTER(sz))
    _sig(p + "set_scale", vp, _Cc)
    _sig(p + "get_scale", vp, vp)
    _sig(p + "execute", vp, vp, sz, vp)
    _sig(p + "execute_block", vp, vp, sz, sz, vp)
    _sig(p + "execute_block_dev", vp, vp, sz, vp)
    _sig(f"yagi_hip_firdecim_{_k}_freqresp", vp, f32, vp)
    p = f"yagi_hip_firpfb_{_k}_"
    _sig(p + "create", sz, vp, sz, pvp)
    _sig(p + "create_kaiser", sz, sz, f32, f32, pvp)
    _sig(p + "create_default", sz, sz, pvp)
    _sig(p + "destroy", vp)
    _sig(p + "clone", vp, pvp)
    _sig(p + "set_stream", vp, vp)
    _sig(p + "reset", vp)
    _sig(p + "set_scale", vp, _Cc)
    _sig(p + "get_scale", vp, vp)
    _sig(p + "push", vp, _T)
    _sig(p + "write", vp, vp, sz)
    _sig(p + "execute", vp, sz, vp)
    _sig(p + "execute_block", vp, sz, vp, sz, vp, sz)
    _sig(p + "execute_block_dev", vp, sz, vp, sz, vp)
    _sig(p + "execute_all_dev", vp, vp, sz, vp)
    _sig(p + "execute_select_dev", vp, vp, vp, sz, vp)

    p = f"yagi_hip_firinterp_{_k}_"
    _sig(p + "create", sz, vp, sz, pvp)
    _sig(p + "create_kaiser", sz, sz, f32, pvp)
    _sig(p + "create_prototype", ci, sz, sz, f32, f32, pvp)
    _sig(p + "create_linear", sz, pvp)
    _sig(p + "create_window", sz, sz, pvp)
    _sig(p + "destroy", vp)
    _sig(p + "clone", vp, pvp)
    _sig(p + "set_stream", vp, vp)
    _sig(p + "reset", vp)
    _sig(p + "get_interp_rate", vp, C.POINTER(sz))
    _sig(p + "get_sub_len", vp, C.POINTER(sz))
    _sig(p + "set_scale", vp, _Cc)
    _sig(p + "get_scale", vp, vp)
    _sig(p + "execute", vp, _T, vp, sz)
    _sig(p + "execute_block", vp, vp, sz, vp, sz)
    _sig(p + "execute_block_dev", vp, vp, sz, vp)
    _sig(p + "flush", vp, vp, sz)
    p = f"yagi_hip_rresamp_{_k}_"
    _sig(p + "create", sz, sz, sz, vp, sz, pvp)
    _sig(p + "create_kaiser", sz, sz, sz, f32, f32, pvp)
    _sig(p + "create_default", sz, sz, pvp)
    _sig(p + "destroy", vp)
    _sig(p + "set_stream", vp, vp)
    _sig(p + "reset", vp)
    _sig(p + "set_scale", vp, _Cc)
    _sig(p + "get_scale", vp, vp)
    _sig(p + "get_params", vp, C.POINTER(sz), C.POINTER(sz), C.POINTER(sz), C.POINTER(sz))
    _sig(p + "write", vp, vp, sz)
    _sig(p + "execute", vp, vp, sz, vp, sz)
    _sig(p + "execute_block", vp, vp, sz, sz, vp, sz)
    _sig(p + "execute_block_dev", vp, vp, sz, vp)
    p = f"yagi_hip_fftfilt_{_k}_"
    _sig(p + "create", vp, sz, sz, pvp)
    _sig(p + "destroy", vp)
    _sig(p + "clone", vp, pvp)
    _sig(p + "set_stream", vp, vp)
    _sig(p + "reset", vp)
    _sig(p + "set_scale", vp, _Cc)
    _sig(p + "get_scale", vp, vp)
    _sig(p + "get_length", vp, C.POINTER(sz))
    _sig(p + "execute", vp, vp, sz, vp, sz)
    _sig(p + "execute_blocks", vp, vp, sz, vp)
    _sig(p + "execute_blocks_dev", vp, vp, sz, vp)

for _k in ("rrrf", "crcf", "cccf"):
    _sig(f"yagi_hip_firfilt_{_k}_set_kernel", vp, ci)

class plan(C.Structure):
    """yagi_hip_plan"""
    _fields_ = [("kind", ci), ("nt", ci), ("r", ci), ("tile", ci), ("staging", ci), ("lds", sz)]


_pplan = C.POINTER(plan)
_sig("yagi_hip_plan_fir_block", sz, sz, sz, sz, _pplan)
_sig("yagi_hip_plan_firpfb_all", sz, sz, sz, sz, _pplan)
_sig("yagi_hip_plan_rresamp", sz, sz, sz, sz, _pplan)
_sig("yagi_hip_plan_resamp", sz, sz, C.c_uint32, _pplan)
_sig("yagi_hip_plan_fir_block_range", sz, sz, sz, sz, sz, vp)
_sig("yagi_hip_plan_firpfb_all_range", sz, sz, sz, sz, sz, vp)
_sig("yagi_hip_plan_rresamp_range", sz, sz, sz, sz, sz, vp)
_sig("yagi_hip_plan_resamp_range", sz, sz, sz, C.c_uint32, vp)


class spgram_plan(C.Structure):
    """yagi_hip_spgram_plan"""
    _fields_ = [("fused", ci), ("group", ci), ("slab", ci), ("workgroups", ci), ("rows", ci), ("folded", ci),
                ("fold_rows", ci), ("accum_slab", ci), ("launch_frames", sz)]


_sig("yagi_hip_plan_spgram", sz, sz, C.POINTER(spgram_plan))

class msresamp2_plan(C.Structure):
    """yagi_hip_msresamp2_plan"""
    _fields_ = [("fused", ci), ("tpw", ci), ("fast_tpw", ci), ("F", ci), ("n", ci * 3), ("cnt0", ci), ("U", ci),
                ("walk", ci * 4), ("walk_q", ci * 4), ("long_halo", ci), ("lds", sz), ("fast_lds", sz), ("head_tiles", sz),
                ("fast_tiles", sz), ("tail_first", sz), ("tiles", sz)]


class resamp2_plan(C.Structure):
    """yagi_hip_resamp2_plan"""
    _fields_ = [("chain", ci), ("tiles", sz), ("lds", sz)]


_sig("yagi_hip_plan_msresamp2", sz, ci, sz, vp, sz, C.POINTER(msresamp2_plan))
_sig("yagi_hip_plan_resamp2", sz, ci, sz, sz, C.POINTER(resamp2_plan))

for _k, _T in (("cf", cf32), ("f", f32)):
    p = f"yagi_hip_spgram{_k}_"
    _sig(p + "create", sz, ci, sz, sz, pvp)
    _sig(p + "create_default", sz, pvp)
    _sig(p + "destroy", vp)
    _sig(p + "set_stream", vp, vp)
    _sig(p + "clear", vp)
    _sig(p + "reset", vp)
    _sig(p + "set_alpha", vp, f32)
    _sig(p + "get_alpha", vp, C.POINTER(f32))
    _sig(p + "set_freq", vp, f32)
    _sig(p + "set_rate", vp, f32)
    _sig(p + "get_params", vp, C.POINTER(sz), C.POINTER(sz), C.POINTER(sz), C.POINTER(ci))
    _sig(p + "get_counters", vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64), C.POINTER(u64))
    _sig(p + "push", vp, _T)
    _sig(p + "write", vp, vp, sz)
    _sig(p + "write_dev", vp, vp, sz)
    _sig(p + "get_psd_mag", vp, vp, sz)
    _sig(p + "get_psd", vp, vp, sz)
    _sig(p + "estimate_psd", sz, vp, sz, vp)

_sig("yagi_hip_fft_create", sz, ci, pvp)
_sig("yagi_hip_fft_destroy", vp)
_sig("yagi_hip_fft_clone", vp, pvp)
_sig("yagi_hip_fft_len", vp, C.POINTER(sz))
class fft_info(C.Structure):
    """yagi_hip_fft_info"""
    _fields_ = [("path", ci), ("batch_chunk", sz), ("n1", sz), ("n2", sz), ("bluestein_m", sz),
                ("nested_n", sz), ("nested_path", ci), ("nested_batch_chunk", sz)]


_sig("yagi_hip_fft_describe", vp, C.POINTER(fft_info))
_sig("yagi_hip_fft_run", vp, vp, sz, vp, sz)
_sig("yagi_hip_fft_run_batch_dev", vp, vp, vp, sz, vp)
_sig("yagi_hip_fft_shift", vp, sz)
_sig("yagi_hip_fft_shift_dev", vp, sz, sz, vp)
_sig("yagi_hip_fft_run_oneshot", vp, vp, sz, ci)

_sig("yagi_hip_firfft_crcf_create", vp, sz, sz, pvp)
_sig("yagi_hip_firfft_crcf_destroy", vp)
_sig("yagi_hip_firfft_crcf_set_stream", vp, vp)
_sig("yagi_hip_firfft_crcf_set_scale", vp, f32)
_sig("yagi_hip_firfft_crcf_reset", vp)
_sig("yagi_hip_firfft_crcf_set_variant", vp, ci)
_sig("yagi_hip_firfft_crcf_execute", vp, vp, sz, vp)
_sig("yagi_hip_firfft_crcf_execute_dev", vp, vp, sz, vp)
_sig("yagi_hip_firfft_crcf_set_pipeline", vp, ci)
_sig("yagi_hip_firfft_crcf_join", vp)

_sig("yagi_hip_firpfbch_crcf_create", sz, sz, vp, pvp)
_sig("yagi_hip_firpfbch_crcf_create_kaiser", sz, sz, f32, pvp)
_sig("yagi_hip_firpfbch_crcf_destroy", vp)
_sig("yagi_hip_firpfbch_crcf_set_stream", vp, vp)
_sig("yagi_hip_firpfbch_crcf_reset", vp)
_sig("yagi_hip_firpfbch_crcf_analyzer_execute", vp, vp, sz, vp)
_sig("yagi_hip_firpfbch_crcf_analyzer_execute_dev", vp, vp, sz, vp)
_sig("yagi_hip_firpfbch_crcf_synthesizer_execute", vp, vp, sz, vp)
_sig("yagi_hip_firpfbch_crcf_synthesizer_execute_dev", vp, vp, sz, vp)

_sig("yagi_hip_firpfbch2_crcf_create", sz, sz, vp, pvp)
_sig("yagi_hip_firpfbch2_crcf_create_kaiser", sz, sz, f32, pvp)
_sig("yagi_hip_firpfbch2_crcf_create_kaiser_synthesizer", sz, sz, f32, pvp)
_sig("yagi_hip_firpfbch2_crcf_synthesizer_execute", vp, vp, sz, vp)
_sig("yagi_hip_firpfbch2_crcf_synthesizer_execute_dev", vp, vp, sz, vp)
_sig("yagi_hip_firpfbch2_crcf_destroy", vp)
_sig("yagi_hip_firpfbch2_crcf_set_stream", vp, vp)
_sig("yagi_hip_firpfbch2_crcf_reset", vp)
_sig("yagi_hip_firpfbch2_crcf_analyzer_execute", vp, vp, sz, vp)
_sig("yagi_hip_firpfbch2_crcf_analyzer_execute_dev", vp, vp, sz, vp)
_sig("yagi_hip_firpfbch2_crcf_analyzer_execute_shard_dev", vp, vp, sz, ci, ci, vp)
_sig("yagi_hip_firpfbch2_crcf_assemble_dev", vp, sz, sz, ci, vp, vp)

_sig("yagi_hip_firpfbchr_crcf_create", sz, sz, sz, vp, pvp)
_sig("yagi_hip_firpfbchr_crcf_create_kaiser", sz, sz, sz, f32, pvp)
_sig("yagi_hip_firpfbchr_crcf_create_kaiser_synthesizer", sz, sz, sz, f32, pvp)
_sig("yagi_hip_firpfbchr_crcf_destroy", vp)
_sig("yagi_hip_firpfbchr_crcf_set_stream", vp, vp)
_sig("yagi_hip_firpfbchr_crcf_reset", vp)
_sig("yagi_hip_firpfbchr_crcf_set_kernel", vp, ci)
_sig("yagi_hip_firpfbchr_crcf_get_last_kernel", vp, C.POINTER(ci))
_sig("yagi_hip_firpfbchr_crcf_analyzer_execute", vp, vp, sz, vp)
_sig("yagi_hip_firpfbchr_crcf_analyzer_execute_dev", vp, vp, sz, vp)
_sig("yagi_hip_firpfbchr_crcf_synthesizer_execute", vp, vp, sz, vp)
_sig("yagi_hip_firpfbchr_crcf_synthesizer_execute_dev", vp, vp, sz, vp)

# ---- multi-GPU (RCCL through the C ABI) ---------------------------------------------------------
_sig("yagi_hip_comm_unique_id", vp)
_sig("yagi_hip_comm_create", vp, ci, ci, pvp)
_sig("yagi_hip_comm_destroy", vp)
_sig("yagi_hip_comm_rank", vp, C.POINTER(ci), C.POINTER(ci))
_sig("yagi_hip_comm_all_gather_dev", vp, vp, vp, sz, vp)
_sig("yagi_hip_firpfbch2_crcf_analyzer_execute_sharded_dev", vp, vp, sz, vp, ci, vp)

# ---- Resamp2 / MsResamp2 and Rresamp clone ---------------------------------
for _k, (_T, _Cc) in KIND_TYPES.items():
    _sig(f"yagi_hip_rresamp_{_k}_clone", vp, pvp)
    p = f"yagi_hip_resamp2_{_k}_"
    _sig(p + "create", vp, sz, f32, pvp)
    _sig(p + "create_kaiser", sz, f32, f32, pvp)
    _sig(p + "destroy", vp)
    _sig(p + "clone", vp, pvp)
    _sig(p + "reset", vp)
    _sig(p + "set_stream", vp, vp)
    _sig(p + "set_scale", vp, _Cc)
    _sig(p + "get_scale", vp, vp)
    _sig(p + "get_delay", vp, C.POINTER(sz))
    _sig(p + "execute_block", vp, ci, vp, sz, vp, sz)
    _sig(p + "execute_block_dev", vp, ci, vp, sz, vp, sz)
    p = f"yagi_hip_msresamp2_{_k}_"
    _sig(p + "create", ci, sz, f32, f32, f32, pvp)
    _sig(p + "create_taps", ci, sz, vp, vp, pvp)
    _sig(p + "destroy", vp)
    _sig(p + "clone", vp, pvp)
    _sig(p + "reset", vp)
    _sig(p + "set_stream", vp, vp)
    _sig(p + "get_params", vp, C.POINTER(ci), C.POINTER(sz), C.POINTER(f32), vp)
    _sig(p + "execute_block", vp, vp, sz, vp, sz)
    _sig(p + "execute_block_dev", vp, vp, sz, vp, sz)

# ---- Resamp / MsResamp (arbitrary-rate resamplers) ---------------------------------------------
for _k, (_T, _Cc) in KIND_TYPES.items():
    p = f"yagi_hip_resamp_{_k}_"
    _sig(p + "create", f32, sz, f32, f32, sz, pvp)
    _sig(p + "create_default", f32, pvp)
    _sig(p + "create_taps", f32, sz, sz, vp, sz, pvp)
    _sig(p + "destroy", vp)
    _sig(p + "clone", vp, pvp)
    _sig(p + "set_stream", vp, vp)
    _sig(p + "reset", vp)
    _sig(p + "set_rate", vp, f32)
    _sig(p + "adjust_rate", vp, f32)
    _sig(p + "get_rate", vp, C.POINTER(f32))
    _sig(p + "get_delay", vp, C.POINTER(sz))
    _sig(p + "get_num_output", vp, sz, C.POINTER(sz))
    _sig(p + "execute", vp, _T, vp, sz, C.POINTER(sz))
    _sig(p + "execute_block", vp, vp, sz, vp, sz, C.POINTER(sz))
    _sig(p + "execute_block_dev", vp, vp, sz, vp, sz, C.POINTER(sz))
    p = f"yagi_hip_msresamp_{_k}_"
    _sig(p + "create", f32, f32, pvp)
    _sig(p + "destroy", vp)
    _sig(p + "clone", vp, pvp)
    _sig(p + "set_stream", vp, vp)
    _sig(p + "reset", vp)
    _sig(p + "get_rate", vp, C.POINTER(f32))
    _sig(p + "get_delay", vp, C.POINTER(f32))
    _sig(p + "get_params", vp, C.POINTER(ci), C.POINTER(sz), C.POINTER(f32))
    _sig(p + "get_num_output", vp, sz, C.POINTER(sz))
    _sig(p + "execute", vp, vp, sz, vp, sz, C.POINTER(sz))
    _sig(p + "execute_dev", vp, vp, sz, vp, sz, C.POINTER(sz))

# ---- IirFilter -------------------------------------------------------------------------------------
for _k, (_T, _Cc) in KIND_TYPES.items():
    p = f"yagi_hip_iirfilt_{_k}_"
    _sig(p + "create", vp, sz, vp, sz, pvp)
    _sig(p + "create_sos", vp, vp, sz, pvp)
    _sig(p + "create_dc_blocker", f32, pvp)
    _sig(p + "create_integrator", pvp)
    _sig(p + "create_differentiator", pvp)
    _sig(p + "create_pll", f32, f32, f32, pvp)
    _sig(p + "destroy", vp)
    _sig(p + "clone", vp, pvp)
    _sig(p + "set_stream", vp, vp)
    _sig(p + "reset", vp)
    _sig(p + "set_scale", vp, _Cc)
    _sig(p + "get_scale", vp, vp)
    _sig(p + "get_length", vp, C.POINTER(sz))
    _sig(p + "execute", vp, _T, vp)
    _sig(p + "execute_block", vp, vp, sz, vp, sz)
    _sig(p + "execute_block_dev", vp, vp, sz, vp)
    _sig(p + "freqresponse", vp, f32, C.POINTER(cf32))
    _sig(p + "get_psd", vp, f32, C.POINTER(f32))
    _sig(p + "groupdelay", vp, f32, C.POINTER(f32))

# ---- IIR design, IirDecimationFilter, IirInterpolationFilter, IirHilbertFilter --------------------
_sig("yagi_hip_iir_design_lowpass_sos", ci, sz, f32, f32, f32, vp, vp)
for _k, (_T, _Cc) in KIND_TYPES.items():
    _sig(f"yagi_hip_iirfilt_{_k}_create_prototype", ci, sz, f32, f32, f32, pvp)
    _sig(f"yagi_hip_iirfilt_{_k}_create_lowpass", sz, f32, pvp)
    for _n, _get, _x in (("iirdecim", "get_decim", vp), ("iirinterp", "get_interp", _T)):
        p = f"yagi_hip_{_n}_{_k}_"
        _sig(p + "create", sz, vp, sz, vp, sz, pvp)
        _sig(p + "create_sos", sz, vp, vp, sz, pvp)
        _sig(p + "create_prototype", sz, ci, sz, f32, f32, f32, pvp)
        _sig(p + "create_default", sz, sz, pvp)
        _sig(p + "destroy", vp)
        _sig(p + "clone", vp, pvp)
        _sig(p + "set_stream", vp, vp)
        _sig(p + "reset", vp)
        _sig(p + "execute", vp, _x, vp)
        _sig(p + "execute_block", vp, vp, sz, vp)
        _sig(p + "execute_block_dev", vp, vp, sz, vp)
        _sig(p + "groupdelay", vp, f32, C.POINTER(f32))
        _sig(p + _get, vp, C.POINTER(sz))
        _sig(p + "set_scale", vp, _Cc)
        _sig(p + "get_scale", vp, vp)
_p = "yagi_hip_iirhilbf_"
_sig(_p + "create", ci, sz, f32, f32, pvp)
_sig(_p + "create_default", sz, pvp)
_sig(_p + "create_sos", vp, vp, sz, pvp)
_sig(_p + "destroy", vp)
_sig(_p + "clone", vp, pvp)
_sig(_p + "set_stream", vp, vp)
_sig(_p + "reset", vp)
_sig(_p + "get_state", vp, C.POINTER(ci))
_sig(_p + "r2c_execute", vp, f32, C.POINTER(cf32))
_sig(_p + "c2r_execute", vp, cf32, C.POINTER(f32))
_sig(_p + "decim_execute", vp, vp, C.POINTER(cf32))
_sig(_p + "interp_execute", vp, cf32, vp)
for _n in ("r2c", "c2r", "decim", "interp"):
    _sig(_p + _n + "_execute_block", vp, vp, sz, vp)
    _sig(_p + _n + "_execute_block_dev", vp, vp, sz, vp)

# ---- Osc ---------------------------------------------------------------------------------------
u32 = C.c_uint32
_p = "yagi_hip_osc_"
_sig(_p + "create", ci, pvp)
_sig(_p + "destroy", vp)
_sig(_p + "clone", vp, pvp)
_sig(_p + "set_stream", vp, vp)
_sig(_p + "reset", vp)
for _n in ("set_frequency", "adjust_frequency", "set_phase", "adjust_phase", "pll_set_bandwidth", "pll_step"):
    _sig(_p + _n, vp, f32)
_sig(_p + "step", vp)
for _n in ("get_phase", "get_frequency", "sin", "cos"):
    _sig(_p + _n, vp, C.POINTER(f32))
_sig(_p + "sin_cos", vp, C.POINTER(f32), C.POINTER(f32))
_sig(_p + "cexp", vp, C.POINTER(cf32))
_sig(_p + "get_state", vp, C.POINTER(u32), C.POINTER(u32))
_sig(_p + "mix_up", vp, cf32, C.POINTER(cf32))
_sig(_p + "mix_down", vp, cf32, C.POINTER(cf32))
_sig(_p + "mix_block_up", vp, vp, sz, vp, sz)
_sig(_p + "mix_block_down", vp, vp, sz, vp, sz)
_sig(_p + "mix_block_up_dev", vp, vp, sz, vp)
_sig(_p + "mix_block_down_dev", vp, vp, sz, vp)

# ---- Ddc / Duc ---------------------------------------------------------------------------------
for _o, _rate in (("ddc", "get_decim_rate"), ("duc", "get_interp_rate")):
    for _k in ("crcf", "cccf"):
        _Cc = KIND_TYPES[_k][1]
        _p = f"yagi_hip_{_o}_{_k}_"
        _sig(_p + "create", ci, sz, vp, sz, pvp)
        _sig(_p + "create_kaiser", ci, sz, sz, f32, pvp)
        _sig(_p + "destroy", vp)
        _sig(_p + "clone", vp, pvp)
        _sig(_p + "set_stream", vp, vp)
        _sig(_p + "reset", vp)
        for _n in ("set_frequency", "adjust_frequency", "set_phase", "adjust_phase"):
            _sig(_p + _n, vp, f32)
        for _n in ("get_frequency", "get_phase"):
            _sig(_p + _n, vp, C.POINTER(f32))
        _sig(_p + "get_state", vp, C.POINTER(u32), C.POINTER(u32))
        _sig(_p + "set_state", vp, u32, u32)
        _sig(_p + "set_scale", vp, _Cc)
        _sig(_p + "get_scale", vp, vp)
        _sig(_p + _rate, vp, C.POINTER(sz))
        _sig(_p + "set_kernel", vp, ci)
        _sig(_p + "get_last_kernel", vp, C.POINTER(ci))
        _sig(_p + "execute", vp, vp, vp)
        _sig(_p + "execute_block", vp, vp, sz, vp)
        _sig(_p + "execute_block_dev", vp, vp, sz, vp)

# ---- FirHilbertFilter --------------------------------------------------------------------------
_p = "yagi_hip_firhilb_"
_sig(_p + "create", sz, f32, pvp)
_sig(_p + "destroy", vp)
_sig(_p + "clone", vp, pvp)
_sig(_p + "set_stream", vp, vp)
_sig(_p + "reset", vp)
_sig(_p + "r2c_execute", vp, f32, C.POINTER(cf32))
_sig(_p + "c2r_execute", vp, cf32, C.POINTER(f32), C.POINTER(f32))
_sig(_p + "decim_execute", vp, vp, C.POINTER(cf32))
_sig(_p + "interp_execute", vp, cf32, vp)
for _n in ("r2c", "c2r", "decim", "interp"):
    _sig(_p + _n + "_execute_block", vp, vp, sz, vp, sz)
    _sig(_p + _n + "_execute_block_dev", vp, vp, sz, vp)
_sig(_p + "design", sz, f32, vp)

# ---- Fdelay ------------------------------------------------------------------------------------
for _k, (_T, _Cc) in KIND_TYPES.items():
    _p = f"yagi_hip_fdelay_{_k}_"
    _sig(_p + "create", sz, sz, sz, pvp)
    _sig(_p + "create_default", sz, pvp)
    _sig(_p + "destroy", vp)
    _sig(_p + "clone", vp, pvp)
    _sig(_p + "set_stream", vp, vp)
    _sig(_p + "reset", vp)
    _sig(_p + "get_delay", vp, C.POINTER(f32))
    _sig(_p + "set_delay", vp, f32)
    _sig(_p + "adjust_delay", vp, f32)
    _sig(_p + "get_nmax", vp, C.POINTER(sz))
    _sig(_p + "get_m", vp, C.POINTER(sz))
    _sig(_p + "get_npfb", vp, C.POINTER(sz))
    _sig(_p + "push", vp, _T)
    _sig(_p + "write", vp, vp, sz)
    _sig(_p + "execute", vp, vp)
    _sig(_p + "execute_block", vp, vp, sz, vp, sz)
    _sig(_p + "execute_block_dev", vp, vp, sz, vp)
    _sig(_p + "execute_track", vp, vp, vp, sz, vp)
    _sig(_p + "execute_track_dev", vp, vp, vp, sz, vp)

# ---- OrdFilt -----------------------------------------------------------------------------------
_p = "yagi_hip_ordfilt_rrrf_"
_sig(_p + "create", sz, sz, pvp)
_sig(_p + "create_medfilt", sz, pvp)
_sig(_p + "destroy", vp)
_sig(_p + "clone", vp, pvp)
_sig(_p + "set_stream", vp, vp)
_sig(_p + "reset", vp)
_sig(_p + "set_kernel", vp, ci)
_sig(_p + "get_n", vp, C.POINTER(sz))
_sig(_p + "get_k", vp, C.POINTER(sz))
_sig(_p + "push", vp, f32)
_sig(_p + "write", vp, vp, sz)
_sig(_p + "execute", vp, C.POINTER(f32))
_sig(_p + "execute_one", vp, f32, C.POINTER(f32))
_sig(_p + "execute_block", vp, vp, sz, vp)
_sig(_p + "execute_block_dev", vp, vp, sz, vp)

# ---- Modem -------------------------------------------------------------------------------------
_p = "yagi_hip_modem_"
_sig(_p + "create", ci, pvp)
_sig(_p + "create_from_table", vp, sz, pvp)
_sig(_p + "destroy", vp)
_sig(_p + "clone", vp, pvp)
_sig(_p + "set_stream", vp, vp)
_sig(_p + "reset", vp)
_sig(_p + "get_bps", vp, C.POINTER(sz))
_sig(_p + "get_scheme", vp, C.POINTER(ci))
_sig(_p + "get_constellation_size", vp, C.POINTER(sz))
_sig(_p + "get_constellation", vp, vp)
_sig(_p + "get_neighbours", vp, vp, sz, C.POINTER(sz))
_sig(_p + "modulate", vp, C.c_uint, C.POINTER(cf32))
_sig(_p + "demodulate", vp, cf32, C.POINTER(C.c_uint))
_sig(_p + "demodulate_soft", vp, cf32, C.POINTER(C.c_uint), vp)
_sig(_p + "get_demodulator_sample", vp, C.POINTER(cf32))
_sig(_p + "get_demodulator_phase_error", vp, C.POINTER(f32))
_sig(_p + "get_demodulator_evm", vp, C.POINTER(f32))
for _n in ("modulate_block", "modulate_block_dev"):
    _sig(_p + _n, vp, vp, sz, vp)
for _n in ("demodulate_block", "demodulate_block_dev", "demodulate_soft_block", "demodulate_soft_block_dev"):
    _sig(_p + _n, vp, vp, sz, vp, vp)

# ---- MSequence / BSequence ---------------------------------------------------------------------
cu = C.c_uint
pcu = C.POINTER(cu)
_p = "yagi_hip_msequence_"
_sig(_p + "create", cu, cu, cu, pvp)
_sig(_p + "create_genpoly", cu, pvp)
_sig(_p + "destroy", vp)
_sig(_p + "clone", vp, pvp)
_sig(_p + "set_stream", vp, vp)
_sig(_p + "reset", vp)
_sig(_p + "advance", vp, pcu)
_sig(_p + "generate_symbol", vp, cu, pcu)
_sig(_p + "set_state", vp, cu)
for _n in ("get_state", "get_genpoly", "get_genpoly_length", "get_length", "measure_period"):
    _sig(_p + _n, vp, pcu)
_sig(_p + "skip", vp, u64)
for _n in ("generate_bits_block", "generate_bits_block_dev"):
    _sig(_p + _n, vp, sz, vp)
for _n in ("generate_symbols_block", "generate_symbols_block_dev"):
    _sig(_p + _n, vp, cu, sz, vp)
_p = "yagi_hip_bsequence_"
_sig(_p + "create", sz, pvp)
_sig(_p + "create_from_msequence", vp, pvp)
_sig(_p + "create_ccodes", vp, vp)
_sig(_p + "destroy", vp)
_sig(_p + "clone", vp, pvp)
_sig(_p + "set_stream", vp, vp)
_sig(_p + "reset", vp)
_sig(_p + "init", vp, vp, sz)
_sig(_p + "push", vp, cu)
_sig(_p + "circshift", vp)
_sig(_p + "correlate", vp, vp, C.POINTER(C.c_int32))
_sig(_p + "add", vp, vp, vp)
_sig(_p + "mul", vp, vp, vp)
_sig(_p + "accumulate", vp, pcu)
_sig(_p + "index", vp, sz, pcu)
_sig(_p + "get_length", vp, C.POINTER(sz))
for _n in ("push_correlate_block", "push_correlate_block_dev"):
    _sig(_p + _n, vp, vp, vp, sz, cu, vp)

# ---- Autocorr ----------------------------------------------------------------------------------
for _k, _T in (("cccf", cf32), ("rrrf", f32)):
    _p = f"yagi_hip_autocorr_{_k}_"
    _sig(_p + "create", sz, sz, pvp)
    _sig(_p + "destroy", vp)
    _sig(_p + "clone", vp, pvp)
    _sig(_p + "set_stream", vp, vp)
    _sig(_p + "reset", vp)
    _sig(_p + "get_window_size", vp, C.POINTER(sz))
    _sig(_p + "get_delay", vp, C.POINTER(sz))
    _sig(_p + "push", vp, _T)
    _sig(_p + "write", vp, vp, sz)
    _sig(_p + "execute", vp, vp)
    _sig(_p + "get_energy", vp, C.POINTER(f32))
    _sig(_p + "execute_block", vp, vp, sz, vp, vp)
    _sig(_p + "execute_block_dev", vp, vp, sz, vp, vp)

# ---- BurstDetector -----------------------------------------------------------------------------
for _k in ("cccf", "rrrf"):
    _p = f"yagi_hip_burstdet_{_k}_"
    _sig(_p + "create", sz, sz, f32, f32, u64, pvp)
    _sig(_p + "destroy", vp)
    _sig(_p + "clone", vp, pvp)
    _sig(_p + "set_stream", vp, vp)
    _sig(_p + "reset", vp)
    _sig(_p + "get_window_size", vp, C.POINTER(sz))
    _sig(_p + "get_delay", vp, C.POINTER(sz))
    _sig(_p + "get_threshold", vp, C.POINTER(f32))
    _sig(_p + "get_energy_floor", vp, C.POINTER(f32))
    _sig(_p + "get_min_length", vp, C.POINTER(u64))
    _sig(_p + "get_position", vp, C.POINTER(u64))
    _sig(_p + "get_pending", vp, C.POINTER(ci), vp)
    _sig(_p + "detect_block", vp, vp, sz, vp, sz, C.POINTER(sz), C.POINTER(ci))
    _sig(_p + "detect_block_dev", vp, vp, sz, vp, sz, vp)
    _sig(_p + "flush", vp, vp, sz, C.POINTER(sz))
    _sig(_p + "detect_host", sz, sz, f32, f32, u64, vp, sz, vp, sz, C.POINTER(sz), C.POINTER(ci), C.POINTER(ci), vp)

# ---- PreambleDetector --------------------------------------------------------------------------
_sig("yagi_hip_pdet_templates", vp, sz, vp, sz, vp)
_p = "yagi_hip_pdet_cccf_"
_sig(_p + "create", vp, sz, vp, sz, f32, f32, u64, pvp)
_sig(_p + "destroy", vp)
_sig(_p + "clone", vp, pvp)
_sig(_p + "set_stream", vp, vp)
_sig(_p + "reset", vp)
_sig(_p + "get_length", vp, C.POINTER(sz))
_sig(_p + "get_hypotheses", vp, C.POINTER(sz))
_sig(_p + "get_threshold", vp, C.POINTER(f32))
_sig(_p + "get_energy_floor", vp, C.POINTER(f32))
_sig(_p + "get_min_length", vp, C.POINTER(u64))
_sig(_p + "get_preamble_energy", vp, C.POINTER(f32))
_sig(_p + "get_dphi", vp, vp)
_sig(_p + "get_templates", vp, vp)
_sig(_p + "get_position", vp, C.POINTER(u64))
_sig(_p + "get_pending", vp, C.POINTER(ci), vp)
_sig(_p + "detect_block", vp, vp, sz, vp, sz, C.POINTER(sz), C.POINTER(ci))
_sig(_p + "detect_block_dev", vp, vp, sz, vp, sz, vp)
_sig(_p + "correlate_block", vp, vp, sz, vp, vp)
_sig(_p + "correlate_block_dev", vp, vp, sz, vp, vp)
_sig(_p + "flush", vp, vp, sz, C.POINTER(sz))
_sig(_p + "detect_host", vp, sz, vp, sz, f32, f32, u64, vp, sz, vp, sz, C.POINTER(sz), C.POINTER(ci), C.POINTER(ci), vp)

# ---- SymSync -----------------------------------------------------------------------------------
_p = "yagi_hip_symsync_crcf_"
_sig(_p + "create", sz, sz, sz, vp, sz, pvp)
_sig(_p + "create_rnyquist", sz, ci, sz, sz, f32, sz, pvp)
_sig(_p + "create_kaiser", sz, sz, sz, f32, sz, pvp)
_sig(_p + "rnyquist_taps", ci, sz, sz, f32, sz, vp)
_sig(_p + "kaiser_taps", sz, sz, f32, sz, vp)
_sig(_p + "destroy", vp)
_sig(_p + "clone", vp, pvp)
_sig(_p + "set_stream", vp, vp)
_sig(_p + "reset", vp)
_sig(_p + "reset_channel", vp, sz)
_sig(_p + "lock", vp)
_sig(_p + "unlock", vp)
_sig(_p + "is_locked", vp, C.POINTER(ci))
_sig(_p + "set_output_rate", vp, sz)
_sig(_p + "set_lf_bw", vp, f32)
_sig(_p + "get_channels", vp, C.POINTER(sz))
_sig(_p + "get_branch_length", vp, C.POINTER(sz))
_sig(_p + "get_tau", vp, vp)
_sig(_p + "get_stalled", vp, vp)
_sig(_p + "execute", vp, vp, sz, sz, vp, sz, sz, vp, vp)
_sig(_p + "execute_dev", vp, vp, sz, sz, vp, sz, sz, vp)
_sig(_p + "execute_host", sz, sz, sz, vp, sz, sz, f32, ci, vp, sz, sz, vp, sz, sz, vp, vp, vp)

# ---- EqLms -------------------------------------------------------------------------------------
_p = "yagi_hip_eqlms_cccf_"
_sig(_p + "create", sz, vp, sz, pvp)
_sig(_p + "create_rnyquist", sz, ci, sz, sz, f32, f32, pvp)
_sig(_p + "create_lowpass", sz, sz, f32, pvp)
_sig(_p + "destroy", vp)
_sig(_p + "clone", vp, pvp)
_sig(_p + "set_stream", vp, vp)
_sig(_p + "reset", vp)
_sig(_p + "reset_channel", vp, sz)
_sig(_p + "set_bw", vp, f32)
_sig(_p + "get_bw", vp, C.POINTER(f32))
_sig(_p + "get_length", vp, C.POINTER(sz))
_sig(_p + "get_channels", vp, C.POINTER(sz))
_sig(_p + "get_coefficients", vp, vp)
_sig(_p + "get_weights", vp, vp)
_sig(_p + "set_constellation", vp, vp, sz)
_sig(_p + "execute_block", vp, sz, vp, sz, sz, vp, sz)
_sig(_p + "execute_block_dev", vp, sz, vp, sz, sz, vp, sz)
_sig(_p + "decim_block", vp, sz, ci, vp, sz, sz, vp, sz, vp, sz)
_sig(_p + "decim_block_dev", vp, sz, ci, vp, sz, sz, vp, sz, vp, sz)
_sig(_p + "execute_host", sz, vp, sz, f32, ci, sz, vp, sz, sz, vp, sz, vp, sz, vp, sz, vp)

# ---- EqRls -------------------------------------------------------------------------------------
_p = "yagi_hip_eqrls_cccf_"
_sig(_p + "create", sz, vp, sz, pvp)
_sig(_p + "recreate", vp, vp, sz)
_sig(_p + "destroy", vp)
_sig(_p + "clone", vp, pvp)
_sig(_p + "set_stream", vp, vp)
_sig(_p + "reset", vp)
_sig(_p + "reset_channel", vp, sz)
_sig(_p + "set_bw", vp, f32)
_sig(_p + "get_bw", vp, C.POINTER(f32))
_sig(_p + "get_length", vp, C.POINTER(sz))
_sig(_p + "get_channels", vp, C.POINTER(sz))
_sig(_p + "get_coefficients", vp, vp)
_sig(_p + "get_weights", vp, vp)
_sig(_p + "get_matrix", vp, vp)
_sig(_p + "set_constellation", vp, vp, sz)
_sig(_p + "set_lanes", vp, sz)
_sig(_p + "get_lanes", vp, C.POINTER(sz))
_sig(_p + "step_block", vp, sz, ci, vp, sz, sz, vp, sz, vp, sz)
_sig(_p + "step_block_dev", vp, sz, ci, vp, sz, sz, vp, sz, vp, sz)
_sig(_p + "train", vp, vp, vp, sz, sz, vp, sz)
_sig(_p + "train_dev", vp, vp, vp, sz, sz, vp, sz)
_sig(_p + "execute_host", sz, vp, sz, f32, ci, sz, vp, sz, sz, vp, sz, vp, sz, vp, sz, vp, vp, vp)
_sig("yagi_hip_eqrls_plan", sz, sz, C.POINTER(sz), C.POINTER(sz), C.POINTER(C.c_uint))

# ---- Agc ---------------------------------------------------------------------------------------
u8p =C.POINTER(C.c_uint8)
for _n in ("lnf", "expf", "log10f"):
    _sig("yagi_hip_" + _n, vp, sz, vp)
for _k in ("crcf", "rrrf"):
    _p = f"yagi_hip_agc_{_k}_"
    _sig(_p + "create", sz, pvp)
    _sig(_p + "clone", vp, pvp)
    _sig(_p + "set_stream", vp, vp)
    _sig(_p + "reset_channel", vp, sz)
    for _n in ("destroy", "reset", "lock", "unlock", "squelch_enable", "squelch_disable"):
        _sig(_p + _n, vp)
    for _n in ("is_locked", "squelch_is_enabled"):
        _sig(_p + _n, vp, C.POINTER(ci))
    for _n in ("set_locked", "get_locked", "set_gains", "get_gain", "get_signal_level", "get_rssi", "squelch_get_status"):
        _sig(_p + _n, vp, vp)
    for _n in ("set_bandwidth", "set_scale", "set_gain", "set_signal_level", "set_rssi", "squelch_set_threshold"):
        _sig(_p + _n, vp, f32)
    for _n in ("get_bandwidth", "get_scale", "squelch_get_threshold"):
        _sig(_p + _n, vp, C.POINTER(f32))
    _sig(_p + "get_channels", vp, C.POINTER(sz))
    _sig(_p + "squelch_set_timeout", vp, u64)
    _sig(_p + "squelch_get_timeout", vp, C.POINTER(u64))
    for _n in ("init", "init_dev"):
        _sig(_p + _n, vp, vp, sz, sz)
    for _n in ("execute_block", "execute_block_dev"):
        _sig(_p + _n, vp, vp, sz, sz, vp, sz, vp, sz)
    _sig(_p + "execute_host", sz, f32, f32, f32, ci, ci, f32, u64, vp, sz, sz, vp, sz, vp, sz, vp, vp)

# ---- SymTrack ----------------------------------------------------------------------------------
_p = "yagi_hip_symtrack_cccf_"
_sig(_p + "create", sz, ci, sz, sz, f32, ci, ci, sz, sz, pvp)
_sig(_p + "create_from_table", sz, ci, sz, sz, f32, vp, sz, ci, sz, sz, pvp)
_sig(_p + "destroy", vp)
_sig(_p + "clone", vp, pvp)
_sig(_p + "set_stream", vp, vp)
_sig(_p + "reset", vp)
_sig(_p + "reset_channel", vp, sz)
_sig(_p + "set_bandwidth", vp, f32)
_sig(_p + "get_bandwidth", vp, C.POINTER(f32))
_sig(_p + "set_bandwidths", vp, f32, f32, f32, f32)
_sig(_p + "set_eq_strategy", vp, ci)
_sig(_p + "set_eq_holdoff", vp, u64)
_sig(_p + "set_nco", vp, sz, f32, f32)
_sig(_p + "set_nco_all", vp, vp, vp)
_sig(_p + "get_channels", vp, C.POINTER(sz))
for _n in ("get_tau", "get_gain", "get_rssi", "get_nco_frequency", "get_nco_phase", "get_weights", "get_num_syms",
           "get_stalled"):
    _sig(_p + _n, vp, vp)
_sig(_p + "get_nco_state", vp, vp, vp)
_sig(_p + "execute", vp, vp, sz, sz, vp, sz, vp, sz, sz, vp, vp)
_sig(_p + "execute_dev", vp, vp, sz, sz, vp, sz, vp, sz, sz, vp)
_sig(_p + "execute_host", sz, ci, sz, sz, f32, ci, vp, sz, ci, sz, sz, f32, ci, u64, vp, vp, vp, sz, sz, vp, sz, vp, sz, sz,
     vp, vp)

# ---- Channel -----------------------------------------------------------------------------------
class channel_shape(C.Structure):
    """yagi_hip_channel_shape"""
    _fields_ = [("links", C.c_uint), ("rows", C.c_uint), ("tile_steps", sz), ("lds_bytes", sz)]


_p = "yagi_hip_channel_cccf_"
_sig("yagi_hip_channel_plan", sz, sz, sz, ci, ci, C.POINTER(channel_shape))
_sig(_p + "create", sz, sz, ci, pvp)
_sig(_p + "clone", vp, pvp)
_sig(_p + "set_stream", vp, vp)
_sig(_p + "destroy", vp)
_sig(_p + "reset", vp)
_sig(_p + "reset_channel", vp, sz)
for _n in ("set_awgn", "set_gain_noise", "set_carrier_offset"):
    _sig(_p + _n, vp, sz, f32, f32)
    _sig(_p + _n + "_all", vp, vp, vp)
_sig(_p + "set_multipath", vp, sz, vp)
for _n in ("set_multipath_all", "get_multipath", "set_position_all", "get_position"):
    _sig(_p + _n, vp, vp)
_sig(_p + "set_seed", vp, u64)
_sig(_p + "get_seed", vp, C.POINTER(u64))
_sig(_p + "set_position", vp, sz, u64)
for _n in ("get_gain_noise", "get_osc_state"):
    _sig(_p + _n, vp, vp, vp)
for _n in ("get_channels", "get_taps"):
    _sig(_p + _n, vp, C.POINTER(sz))
_sig(_p + "set_shape", vp, C.c_uint, C.c_uint)
_sig(_p + "get_shape", vp, sz, ci, C.POINTER(channel_shape))
for _n in ("execute", "execute_dev"):
    _sig(_p + _n, vp, vp, sz, sz, vp, sz)
for _n in ("execute_bcast", "execute_bcast_dev"):
    _sig(_p + _n, vp, vp, sz, vp, sz)
_sig(_p + "execute_host", sz, sz, ci, ci, u64, vp, vp, vp, vp, vp, vp, vp, sz, sz, vp, sz)
_sig("yagi_hip_channel_awgn_words", f32, f32, C.POINTER(f32), C.POINTER(f32))
_sig("yagi_hip_channel_cos_sin", vp, sz, vp, vp)
_sig("yagi_hip_channel_radius", vp, sz, vp)
_sig("yagi_hip_channel_noise", u64, u64, u64, sz, vp)
_sig("yagi_hip_channel_constrain", f32, C.POINTER(C.c_uint32))

# ---- ConvCode ----------------------------------------------------------------------------------
class convcode_shape(C.Structure):
    """yagi_hip_convcode_shape"""
    _fields_ = [("frames_per_wave", C.c_uint), ("waves", C.c_uint), ("states_per_lane", C.c_uint), ("chunk_steps", C.c_uint),
                ("frames_per_wg", sz), ("lds_bytes", sz)]


_p = "yagi_hip_convcode_"
_sig(_p + "plan", ci, ci, sz, sz, C.POINTER(convcode_shape))
_sig(_p + "create", ci, vp, ci, vp, ci, ci, pvp)
_sig(_p + "destroy", vp)
_sig(_p + "clone", vp, pvp)
_sig(_p + "set_stream", vp, vp)
for _n in ("get_K", "get_R"):
    _sig(_p + _n, vp, C.POINTER(ci))
_sig(_p + "get_rate", vp, C.POINTER(sz), C.POINTER(sz))
_sig(_p + "get_ncoded", vp, sz, C.POINTER(sz))
_sig(_p + "get_nmax", vp, C.POINTER(sz))
_sig(_p + "set_shape", vp, C.c_uint, C.c_uint)
_sig(_p + "get_shape", vp, sz, sz, C.POINTER(convcode_shape))
for _n in ("encode_block", "encode_block_dev"):
    _sig(_p + _n, vp, vp, sz, sz, sz, vp, sz)
for _n in ("decode_block", "decode_block_dev"):
    _sig(_p + _n, vp, vp, sz, sz, sz, vp, sz, vp)
_sig(_p + "encode_host", ci, vp, ci, vp, ci, ci, vp, sz, sz, sz, vp, sz)
_sig(_p + "decode_host", ci, vp, ci, vp, ci, ci, vp, sz, sz, sz, vp, sz, vp)
_sig(_p + "ncoded_host", ci, ci, vp, ci, ci, sz, C.POINTER(sz), C.POINTER(sz))

# ---- Packetizer --------------------------------------------------------------------------------
_p = "yagi_hip_packetizer_"
_sig(_p + "plan", ci, ci, sz, ci, sz, C.POINTER(convcode_shape))
_sig(_p + "create", sz, ci, ci, vp, ci, vp, ci, ci, sz, ci, pvp)
_sig(_p + "destroy", vp)
_sig(_p + "clone", vp, pvp)
_sig(_p + "set_stream", vp, vp)
for _n in ("get_payload_len", "get_crc_len", "get_msg_bits", "get_enc_len", "get_columns"):
    _sig(_p + _n, vp, C.POINTER(sz))
_sig(_p + "get_nsym", vp, C.c_uint, C.POINTER(sz))
_sig(_p + "set_shape", vp, C.c_uint, C.c_uint)
_sig(_p + "get_shape", vp, sz, C.POINTER(convcode_shape))
for _n in ("encode_block", "encode_block_dev"):
    _sig(_p + _n, vp, vp, sz, sz, C.c_uint, vp, sz)
for _n in ("decode_block", "decode_block_dev"):
    _sig(_p + _n, vp, vp, sz, sz, vp, sz, vp, vp, vp)
_sig(_p + "encode_host", sz, ci, ci, vp, ci, vp, ci, ci, sz, ci, vp, sz, sz, C.c_uint, vp, sz)
_sig(_p + "decode_host", sz, ci, ci, vp, ci, vp, ci, ci, sz, ci, vp, sz, sz, vp, sz, vp, vp, vp)
_sig(_p + "permutation", sz, sz, vp)
_sig("yagi_hip_crc_host", ci, vp, sz, C.POINTER(C.c_uint32))
for _n in ("scramble_data", "unscramble_data", "unscramble_data_soft"):
    _sig("yagi_hip_" + _n, vp, sz)

# ---- SymStream ---------------------------------------------------------------------------------
_p = "yagi_hip_symstreamcf_"
_sig(_p + "create_linear", ci, sz, sz, f32, ci, vp, pvp)
_sig(_p + "create_taps", sz, vp, sz, ci, vp, pvp)
_sig(_p + "destroy", vp)
_sig(_p + "clone", vp, pvp)
_sig(_p + "set_stream", vp, vp)
_sig(_p + "reset", vp)
_sig(_p + "source_set_state", vp, cu)
_sig(_p + "source_get_state", vp, pcu)
for _n in ("get_ftype", "get_scheme", "is_fused"):
    _sig(_p + _n, vp, C.POINTER(ci))
for _n in ("get_k", "get_m", "get_delay", "get_buf_index"):
    _sig(_p + _n, vp, C.POINTER(sz))
for _n in ("get_beta", "get_gain"):
    _sig(_p + _n, vp, C.POINTER(f32))
_sig(_p + "set_scheme", vp, ci)
_sig(_p + "set_modem", vp, vp)
_sig(_p + "set_gain", vp, f32)
for _n in ("write_samples", "write_samples_dev"):
    _sig(_p + _n, vp, vp, sz)
for _n in ("modulate_symbols", "modulate_symbols_dev"):
    _sig(_p + _n, vp, vp, sz, vp)

# ---- SymStreamR --------------------------------------------------------------------------------
_p = "yagi_hip_symstreamrcf_"
_sig(_p + "create_linear", ci, f32, sz, f32, ci, vp, pvp)
_sig(_p + "destroy", vp)
_sig(_p + "clone", vp, pvp)
_sig(_p + "set_stream", vp, vp)
_sig(_p + "reset", vp)
_sig(_p + "source_set_state", vp, cu)
_sig(_p + "source_get_state", vp, pcu)
for _n in ("get_ftype", "get_scheme", "is_fused"):
    _sig(_p + _n, vp, C.POINTER(ci))
for _n in ("get_m", "get_pending"):
    _sig(_p + _n, vp, C.POINTER(sz))
for _n in ("get_bw", "get_beta", "get_gain", "get_delay"):
    _sig(_p + _n, vp, C.POINTER(f32))
_sig(_p + "get_params", vp, C.POINTER(ci), C.POINTER(sz), C.POINTER(f32))
_sig(_p + "set_scheme", vp, ci)
_sig(_p + "set_modem", vp, vp)
_sig(_p + "set_gain", vp, f32)
for _n in ("write_samples", "write_samples_dev"):
    _sig(_p + _n, vp, vp, sz)


class symstreamr_plan(C.Structure):
    """yagi_hip_symstreamr_plan"""
    _fields_ = [("interp", ci), ("tile", ci), ("max_wg_tiles", ci), ("wg_tiles", ci), ("step", C.c_uint32),
                ("phase_next", C.c_uint32), ("rate", f32), ("rate_arb", f32), ("stages", sz), ("lds", sz), ("q", sz),
                ("need", sz), ("outputs_arb", sz), ("outputs", sz), ("leftover", sz)]


_sig("yagi_hip_plan_symstreamr", f32, sz, sz, C.c_uint32, C.POINTER(symstreamr_plan))
