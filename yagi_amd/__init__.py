"""yagi_amd -- Python host mirror of yagi's FIR/FFT object API over libyagi_hip.so (MI355X).

The classes keep the reference's names, argument meaning and error behaviour
(reference = EEGKit/yagi, paths relative to its root):

    DotProd / dotprod          src/dotprod/mod.rs:13-73
    FirFilter                  src/filter/fir/firfilt.rs:10-15,63-314
    FirDecimationFilter        src/filter/fir/firdecim.rs:12-17,38-205
    FirPfbFilter               src/filter/fir/firpfb.rs:10-15,34-301
    Fft, Direction, fft_run    src/fft/mod.rs:13-69
    Error variants             src/error.rs:4-14
    FirPfbCh / FirPfbCh2       (absent from the reference: src/multichannel/mod.rs is empty)
    FirFftStream               the headline composition FirFilter::execute_block -> Fft::run
    Rresamp / Resamp2 / MsResamp2  src/filter/resampler/{rresamp,resamp2,msresamp2}.rs
    Resamp / MsResamp          src/filter/resampler/resamp.rs:8-165, msresamp.rs:10-176
    Osc, OscScheme             src/nco/osc.rs:13-201 (nco.rs, vco.rs)
    Modem, ModulationScheme    src/modem/modem.rs:27-575 (the linear schemes and from_table)
    MSequence / BSequence      src/sequence/msequence.rs:41-164, bsequence.rs:8-195
    Autocorr                   (absent from the reference: src/filter/autocorr.rs is empty)
    BurstDetector              (absent from the reference: Autocorr, threshold and run / peak extraction fused)
    PreambleDetector           (absent from the reference: a bank of known-preamble correlators, threshold and events)
    SymSync                    src/filter/symsync.rs:37-276, one object per channel of a bank
    EqLms, EqLmsUpdate         src/equalization/eqlms.rs:25-199, one object per channel of a bank
    EqRls, EqRlsUpdate         src/equalization/eqrls.rs:31-176, one object per channel of a bank
    SymTrack, SymTrackEq       (src/framing/symtrack.rs is empty: Agc -> SymSync -> Osc -> EqLms -> Modem, loops closed)
    ConvCode                   (src/fec/mod.rs is empty: convolutional encoder and Viterbi decoder for a bank of frames)
    Packetizer, CrcScheme      src/random/scramble.rs for the mask; CRC, ConvCode, block interleaver and scrambler fused
    scramble_data, unscramble_data, unscramble_data_soft    src/random/scramble.rs:7-53 (host)

Generic parameters <T, Coeff> are spelled with liquid-dsp's suffixes: "rrrf" = <f32,f32>,
"crcf" = <Complex32,f32>, "cccf" = <Complex32,Complex32>.  Every numeric result comes from a HIP
kernel through the C ABI (include/yagi_hip.h); importing this package fails if the library is
not built, and every call fails with DeviceError if no GPU is present.
"""
import collections
import ctypes as C
import enum

import numpy as np

from . import _capi
from ._capi import cf32, lib

__all__ = [
    "YagiError", "InternalError", "ConfigError", "ValueError_", "RangeError", "ModeError",
    "NoConvergenceError", "DeviceError", "Direction", "dotprod", "FirFilter", "FirDecimationFilter",
    "FirPfbFilter", "FirInterpolationFilter", "Rresamp", "Resamp", "MsResamp", "IirFilter", "IirFilterShape", "iir_design_lowpass_sos", "IirDecimationFilter", "IirInterpolationFilter", "IirHilbertFilter", "Osc", "OscScheme", "Ddc", "Duc", "FirHilbertFilter", "Fdelay", "OrdFilt", "ORDFILT_NMAX", "ORDFILT_TILE", "ORDFILT_REG_NMAX", "Autocorr", "BurstDetector", "BURST_EVENT", "BURSTDET_SEGMAX", "burst_detect_host", "PreambleDetector", "PREAMBLE_EVENT", "PDET_LMAX", "PDET_KMAX", "PDET_TILE", "PDET_SEGMAX", "preamble_templates", "preamble_detect_host", "SymSync", "SYMSYNC_NPFB_MAX", "SYMSYNC_LS_MAX", "SYMSYNC_CHANNELS_MAX", "EqLms", "EqLmsUpdate", "EqRls", "EqRlsUpdate", "eqrls_plan", "EQRLS_LEN_MAX", "EQRLS_CHANNELS_MAX", "EQRLS_MATRIX_MAX", "ConvCode", "convcode_plan", "CONVCODE_DECISION_BYTES", "CONVCODE_STEPS_MAX", "CONVCODE_FRAMES_MAX", "CONVCODE_PERIOD_MAX", "Packetizer", "CrcScheme", "crc", "packetizer_permutation", "packetizer_plan", "scramble_data", "unscramble_data", "unscramble_data_soft", "PACKETIZER_COLUMNS_MAX", "SymTrack", "SymTrackEq", "symtrack_host", "SYMTRACK_CHANNELS_MAX", "SYMTRACK_PLL_ARG_MAX", "SYMTRACK_STALL_CAPACITY", "SYMTRACK_STALL_PLL", "EQLMS_LEN_MAX", "EQLMS_CHANNELS_MAX", "EQLMS_TABLE_MAX", "AUTOCORR_WMAX", "AUTOCORR_DMAX", "AUTOCORR_TILE", "MSequence", "BSequence", "MSEQUENCE_TILE", "BSEQUENCE_TILE", "BSEQUENCE_NMAX", "Modem", "ModulationScheme", "gray_encode", "gray_decode", "pack_soft_bits", "unpack_soft_bits", "FftFilt", "Fft", "FftPath", "FftInfo", "fft_run", "Spgram", "WindowType", "FirFftStream", "FirPfbCh", "FirPfbCh2", "FirPfbChr", "DeviceArray",
    "Plan", "SpgramPlan", "plan_spgram", "MsResamp2Plan", "Resamp2Plan", "plan_msresamp2", "plan_resamp2", "plan_fir_block","plan_firpfb_all", "plan_rresamp", "plan_resamp", "plan_fir_block_range",
    "plan_firpfb_all_range", "plan_rresamp_range", "plan_resamp_range",
    "fir_design_kaiser", "firhilb_design", "FirFilterShape", "fir_design_prototype",
    "estimate_req_filter_stopband_attenuation", "Agc", "AgcSquelchMode", "AGC_CHANNELS_MAX", "lnf", "expf", "log10f", "SymStream", "SymStreamR", "SymStreamRPlan", "plan_symstreamr", "device_count", "synchronize", "gen_complex_dev", "gen_real_dev",
]


# ---- error::Error (src/error.rs:7-14) ---------------------------------------------------------
class YagiError(Exception):
    pass


class InternalError(YagiError):
    pass


class ConfigError(YagiError):
    pass


class ValueError_(YagiError):
    pass


class RangeError(YagiError):
    pass


class ModeError(YagiError):
    pass


class NoConvergenceError(YagiError):
    pass


class DeviceError(YagiError):
    pass


_ERR = {1: InternalError, 2: ConfigError, 3: ValueError_, 4: RangeError, 5: ModeError,
        6: NoConvergenceError, 7: DeviceError}


def _check(rc):
    if rc != 0:
        raise _ERR.get(rc, YagiError)(lib.yagi_hip_last_error().decode())


class Direction(enum.Enum):
    """fft::Direction (src/fft/mod.rs:13-17)"""
    Forward = 0
    Backward = 1


KINDS = {"rrrf": (np.float32, np.float32), "crcf": (np.complex64, np.float32),
         "cccf": (np.complex64, np.complex64)}


def _arr(a, dt):
    return np.ascontiguousarray(np.asarray(a, dtype=dt))


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if isinstance(a, np.ndarray) else C.c_void_p(a)


def _out(y, n, dt):
    """a caller-supplied output array handed to the C ABI as a raw pointer: it must be exactly what the library
    will write -- dtype dt, C-contiguous, n elements -- or a fresh array when None"""
    if y is None:
        return np.empty(n, dt)
    if not (isinstance(y, np.ndarray) and y.dtype == np.dtype(dt) and y.flags.c_contiguous and y.size == n):
        raise ConfigError(f"output must be a C-contiguous {np.dtype(dt).name} array of {n} elements")
    return y


def _byval(v, ctype):
    if ctype is cf32:
        v = complex(v)
        return cf32(v.real, v.imag)
    return C.c_float(float(np.real(v)))


def _devptr(x):
    """device pointer from a DeviceArray, a torch tensor (data_ptr) or a raw int."""
    if isinstance(x, DeviceArray):
        return C.c_void_p(x.ptr)
    if hasattr(x, "data_ptr"):
        return C.c_void_p(x.data_ptr())
    return C.c_void_p(int(x))


# ---- device plumbing --------------------------------------------------------------------------
def device_count():
    n = C.c_int(0)
    rc = lib.yagi_hip_device_count(C.byref(n))
    return n.value if rc == 0 else 0


def synchronize():
    _check(lib.yagi_hip_device_synchronize())


class DeviceArray:
    """A typed HBM allocation owned through yagi_hip_malloc/free."""

    def __init__(self, n, dtype):
        self.dtype = np.dtype(dtype)
        self.n = int(n)
        p = C.c_void_p()
        _check(lib.yagi_hip_malloc(C.byref(p), self.n * self.dtype.itemsize))
        self.ptr = p.value

    @classmethod
    def from_numpy(cls, a):
        a = np.ascontiguousarray(a)
        d = cls(a.size, a.dtype)
        _check(lib.yagi_hip_memcpy_h2d(d.ptr, _ptr(a), a.nbytes))
        return d

    def to_numpy(self, n=None, offset=0):
        n = self.n - offset if n is None else n
        out = np.empty(n, self.dtype)
        _check(lib.yagi_hip_memcpy_d2h(_ptr(out), C.c_void_p(self.ptr + offset * self.dtype.itemsize), out.nbytes))
        return out

    def zero(self):
        _check(lib.yagi_hip_memset_dev(self.ptr, 0, self.n * self.dtype.itemsize))

    def free(self):
        if getattr(self, "ptr", None) and lib is not None:        # lib is None while the interpreter shuts down
            lib.yagi_hip_free(self.ptr)
            self.ptr = None

    def __del__(self):
        self.free()


def gen_complex_dev(seed, n, out=None, first=0, stream=None):
    out = out if out is not None else DeviceArray(n, np.complex64)
    _check(lib.yagi_hip_gen_complex_dev(seed, first, n, _devptr(out), stream))
    return out


def gen_real_dev(seed, n, out=None, first=0, stream=None):
    out = out if out is not None else DeviceArray(n, np.float32)
    _check(lib.yagi_hip_gen_real_dev(seed, first, n, _devptr(out), stream))
    return out


def fir_design_kaiser(n, fc, as_, mu=0.0):
    """filter::fir_design_kaiser (src/filter/fir/design/kaiser.rs:16-51)"""
    h = np.zeros(max(int(n), 1), np.float32)
    _check(lib.yagi_hip_fir_design_kaiser(n, fc, as_, mu, _ptr(h)))
    return h[:n]


class FirFilterShape(enum.IntEnum):
    """filter::FirFilterShape (src/filter/fir/design/mod.rs:41-77), numbered as yagi_fir_shape.  fir_design_prototype
    builds Kaiser, Rcos, Rrcos and Arkaiser; the others are a ConfigError.  Unknown has no reference counterpart: what
    a SymStream made from external taps reports."""
    Unknown = -1
    Kaiser = 0
    Pm = 1
    Rcos = 2
    Fexp = 3
    Fsech = 4
    Farcsech = 5
    Arkaiser = 6
    Rkaiser = 7
    Rrcos = 8
    Hm3 = 9
    Gmsktx = 10
    Gmskrx = 11
    Rfexp = 12
    Rfsech = 13
    Rfarcsech = 14


def estimate_req_filter_stopband_attenuation(df, n):
    """filter::estimate_req_filter_stopband_attenuation (src/filter/fir/design/mod.rs:161-184)"""
    v = C.c_float()
    _check(lib.yagi_hip_estimate_req_filter_stopband_attenuation(df, n, C.byref(v)))
    return np.float32(v.value)


def fir_design_prototype(ftype, k, m, beta, dt=0.0):
    """filter::fir_design_prototype (src/filter/fir/design/mod.rs:392-451): 2km+1 taps"""
    h = np.zeros(2 * max(int(k), 0) * max(int(m), 0) + 1, np.float32)
    _check(lib.yagi_hip_fir_design_prototype(int(ftype), k, m, beta, dt, _ptr(h)))
    return h


def firhilb_design(m, as_):
    """extension: the 2m quadrature taps hq of FirHilbertFilter::new (src/filter/fir/firhilb.rs:43-64)"""
    hq = np.zeros(2 * max(int(m), 1), np.float32)
    _check(lib.yagi_hip_firhilb_design(m, as_, _ptr(hq)))
    return hq


# ---- plan queries (diagnostics: what a FIR-family block call would launch; no device needed) ----
Plan = collections.namedtuple("Plan", "kind nt r tile staging lds")
PLAN_FIR_CONSEC, PLAN_FIR_DECIM, PLAN_FIR_STAGED, PLAN_FIR_UNSTAGED = range(4)
PLAN_PFB_FEW, PLAN_PFB_TAPS_LDS, PLAN_PFB_TAPS_GLOBAL, PLAN_PFB_NONE = range(4)
PLAN_STAGE_ELEMENT, PLAN_STAGE_DESCRIPTOR, PLAN_STAGE_POW2 = range(3)
PLAN_DTYPE = np.dtype([("kind", "i4"), ("nt", "i4"), ("r", "i4"), ("tile", "i4"), ("staging", "i4"), ("lds", "u8")],
                      align=True)
assert PLAN_DTYPE.itemsize == C.sizeof(_capi.plan)


def _plan(fn, *args):
    p = _capi.plan()
    _check(fn(*args, C.byref(p)))
    return Plan(p.kind, p.nt, p.r, p.tile, p.staging, p.lds)


def _plan_range(fn, count, *args):
    out = np.zeros(int(count), PLAN_DTYPE)
    _check(fn(*args, _ptr(out)))
    return out


def plan_fir_block(elem, L, M, ny):
    """yagi_hip_plan_fir_block: FirFilter kernel 1 (M = 1), FirDecimationFilter, Ddc's fused kernel"""
    return _plan(lib.yagi_hip_plan_fir_block, elem, L, M, ny)


SpgramPlan = collections.namedtuple("SpgramPlan",
                                    "fused group slab workgroups rows folded fold_rows launch_frames accum_slab")


def plan_spgram(nfft, nframes):
    """yagi_hip_plan_spgram: what a Spgram write of nframes transforms launches (its first launch; a call is cut every
    launch_frames transforms)"""
    p = _capi.spgram_plan()
    _check(lib.yagi_hip_plan_spgram(nfft, nframes, C.byref(p)))
    return SpgramPlan(p.fused, p.group, p.slab, p.workgroups, p.rows, p.folded, p.fold_rows, p.launch_frames,
                      p.accum_slab)


MsResamp2Plan = collections.namedtuple(
    "MsResamp2Plan", "fused lds tiles tpw head_tiles fast_tiles tail_first fast_tpw fast_lds F n cnt0 U walk walk_q long_halo")
Resamp2Plan = collections.namedtuple("Resamp2Plan", "chain tiles lds")
PLAN_WALK_GENERAL, PLAN_WALK_R1, PLAN_WALK_R2, PLAN_WALK_R4_RHO0, PLAN_WALK_R4_RHO2 = range(5)


def plan_msresamp2(elem, interp, m_stage, n):
    """yagi_hip_plan_msresamp2: what MsResamp2.execute_block of n execute() calls launches.  m_stage in the object's
    stage order (get_stage_lengths); n, walk and walk_q of the answer in the decimator kernels' processing order,
    where stage g of the object is processing stage len(m_stage) - 1 - g"""
    ms = np.array(list(m_stage) or [0], np.uint64)
    p = _capi.msresamp2_plan()
    _check(lib.yagi_hip_plan_msresamp2(elem, int(bool(interp)), len(m_stage), _ptr(ms), n, C.byref(p)))
    return MsResamp2Plan(p.fused, p.lds, p.tiles, p.tpw, p.head_tiles, p.fast_tiles, p.tail_first, p.fast_tpw,
                         p.fast_lds, p.F, tuple(p.n), p.cnt0, p.U, tuple(p.walk), tuple(p.walk_q), p.long_halo)


def plan_resamp2(elem, mode, m, nx):
    """yagi_hip_plan_resamp2: resamp2_kernel (chain = 0) or, for a long decimator block, the one-stage case of the
    MsResamp2 chain kernels (chain = 1: plan_msresamp2(elem, False, [m], nx // 2) has the details)"""
    p = _capi.resamp2_plan()
    _check(lib.yagi_hip_plan_resamp2(elem, mode, m, nx, C.byref(p)))
    return Resamp2Plan(p.chain, p.tiles, p.lds)


def plan_firpfb_all(elem, coeff_elem, nf, Ls):
    """yagi_hip_plan_firpfb_all: FirPfbFilter.execute_all, FirInterpolationFilter, Duc"""
    return _plan(lib.yagi_hip_plan_firpfb_all, elem, coeff_elem, nf, Ls)


def plan_rresamp(elem, P, Q, Ls):
    """yagi_hip_plan_rresamp: tile = primitive blocks per workgroup; ConfigError where the block call raises it"""
    return _plan(lib.yagi_hip_plan_rresamp, elem, P, Q, Ls)


def plan_resamp(elem, Ls, step):
    """yagi_hip_plan_resamp: tile = outputs per workgroup; ConfigError where the branch length does not fit"""
    return _plan(lib.yagi_hip_plan_resamp, elem, Ls, step)


def plan_fir_block_range(elem, L0, count, M, ny):
    """plans of L = L0 .. L0 + count - 1 as a PLAN_DTYPE array"""
    return _plan_range(lib.yagi_hip_plan_fir_block_range, count, elem, L0, count, M, ny)


def plan_firpfb_all_range(elem, coeff_elem, nf, Ls0, count):
    return _plan_range(lib.yagi_hip_plan_firpfb_all_range, count, elem, coeff_elem, nf, Ls0, count)


def plan_rresamp_range(elem, P, Q, Ls0, count):
    """tile = 0 where the shape does not fit"""
    return _plan_range(lib.yagi_hip_plan_rresamp_range, count, elem, P, Q, Ls0, count)


def plan_resamp_range(elem, Ls0, count, step):
    """tile = 0 where the shape does not fit"""
    return _plan_range(lib.yagi_hip_plan_resamp_range, count, elem, Ls0, count, step)


# ---- dotprod (trait DotProd, src/dotprod/mod.rs:13-73) ----------------------------------------
def dotprod(a, b):
    """a.dotprod(b): the impl is picked from the element types like the Rust trait impls."""
    a, b = np.asarray(a), np.asarray(b)
    ca, cb = np.iscomplexobj(a), np.iscomplexobj(b)
    name = {(False, False): "rrrf", (False, True): "rccf", (True, False): "crcf", (True, True): "cccf"}[(ca, cb)]
    a = _arr(a, np.complex64 if ca else np.float32)
    b = _arr(b, np.complex64 if cb else np.float32)
    # zip() semantics: the shorter slice decides (slice impls, mod.rs:23-25)
    n = min(a.size, b.size)
    y = np.zeros(1, np.complex64 if (ca or cb) else np.float32)
    _check(getattr(lib, f"yagi_hip_dotprod_{name}")(_ptr(a), _ptr(b), n, _ptr(y)))
    return y[0]


# ---- handle base ------------------------------------------------------------------------------
class _Handle:
    _prefix = None

    def _fn(self, name):
        return getattr(lib, f"{self._prefix}{name}")

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and lib is not None:                 # lib is None while the interpreter shuts down
            self._fn("destroy")(h)
            self._h = None

    def set_stream(self, stream):
        """stream: a hipStream_t as int (e.g. torch.cuda.current_stream().cuda_stream)"""
        _check(self._fn("set_stream")(self._h, stream))

    def reset(self):
        _check(self._fn("reset")(self._h))


class _FirBase(_Handle):
    def _init_kind(self, kind):
        if kind not in KINDS:
            raise ConfigError(f"unknown type combination {kind!r}")
        self.kind = kind
        self.T, self.Cdt = KINDS[kind]
        self._Tc, self._Cc = _capi.KIND_TYPES[kind]

    def set_scale(self, scale):
        _check(self._fn("set_scale")(self._h, _byval(scale, self._Cc)))

    def get_scale(self):
        s = np.zeros(1, self.Cdt)
        _check(self._fn("get_scale")(self._h, _ptr(s)))
        return s[0]

    def clone(self):
        new = object.__new__(type(self))
        new.__dict__.update({k: v for k, v in self.__dict__.items() if k != "_h"})
        h = C.c_void_p()
        _check(self._fn("clone")(self._h, C.byref(h)))
        new._h = h
        return new


class FirFilter(_FirBase):
    """FirFilter<T,Coeff> (src/filter/fir/firfilt.rs)."""

    def __init__(self, kind, h):
        self._init_kind(kind)
        self._prefix = f"yagi_hip_firfilt_{kind}_"
        h = _arr(h, self.Cdt)
        hd = C.c_void_p()
        _check(self._fn("create")(_ptr(h), h.size, C.byref(hd)))
        self._h = hd

    @classmethod
    def _from(cls, kind, creator, *args):
        self = object.__new__(cls)
        self._init_kind(kind)
        self._prefix = f"yagi_hip_firfilt_{kind}_"
        hd = C.c_void_p()
        _check(self._fn(creator)(*args, C.byref(hd)))
        self._h = hd
        return self

    @classmethod
    def new_kaiser(cls, kind, n, fc, as_, mu=0.0):          # firfilt.rs:93-97
        return cls._from(kind, "create_kaiser", n, fc, as_, mu)

    @classmethod
    def new_rnyquist(cls, kind, ftype, k, m, beta, mu=0.0):  # firfilt.rs:112-116
        return cls._from(kind, "create_rnyquist", int(ftype), k, m, beta, mu)

    @classmethod
    def new_rect(cls, kind, n):                              # firfilt.rs:149-155
        return cls._from(kind, "create_rect", n)

    @classmethod
    def new_dc_blocker(cls, kind, m, as_):                   # firfilt.rs:166-170
        return cls._from(kind, "create_dc_blocker", m, as_)

    @classmethod
    def new_notch(cls, kind, m, as_, f0):                    # firfilt.rs:183-186
        return cls._from(kind, "create_notch", m, as_, f0)

    def set_coefficients(self, h):                           # :193-206
        h = _arr(h, self.Cdt)
        _check(self._fn("set_coefficients")(self._h, _ptr(h), h.size))

    def push(self, x):                                       # :220-223
        _check(self._fn("push")(self._h, _byval(x, self._Tc)))

    def write(self, x):                                      # :230-234
        x = _arr(x, self.T)
        _check(self._fn("write")(self._h, _ptr(x), x.size))

    def execute(self):                                       # :241-246
        y = np.zeros(1, self.T)
        _check(self._fn("execute")(self._h, _ptr(y)))
        return y[0]

    def execute_one(self, x):                                # :256-259
        y = np.zeros(1, self.T)
        _check(self._fn("execute_one")(self._h, _byval(x, self._Tc), _ptr(y)))
        return y[0]

    def execute_block(self, x, y=None):                      # :267-278
        x = _arr(x, self.T)
        if y is None:
            y = np.empty_like(x)
        elif y.dtype != self.T or not y.flags.c_contiguous:
            raise ConfigError("output must be a contiguous array of the sample type")
        _check(self._fn("execute_block")(self._h, _ptr(x), x.size, _ptr(y), y.size))
        return y

    def execute_block_dev(self, x_dev, n, y_dev):
        _check(self._fn("execute_block_dev")(self._h, _devptr(x_dev), n, _devptr(y_dev)))

    def set_pipeline(self, on=True):
        """pipelined block calls (include/yagi_hip.h): consecutive execute_block_dev calls overlap on two streams of the
        object; outputs (and the right to overwrite the inputs) are ordered on the object's stream after join()"""
        _check(self._fn("set_pipeline")(self._h, 1 if on else 0))

    def join(self):
        _check(self._fn("join")(self._h))

    def get_length(self):                                    # :301-303
        n = C.c_size_t()
        _check(self._fn("get_length")(self._h, C.byref(n)))
        return n.value

    def get_coefficients(self):                              # :310-312
        n = self.get_length()
        h = np.empty(n, self.Cdt)
        _check(self._fn("get_coefficients")(self._h, _ptr(h), n))
        return h

    def freqresponse(self, fc):                              # :325-328
        H = np.zeros(1, np.complex64)
        _check(self._fn("freqresponse")(self._h, fc, _ptr(H)))
        return H[0]

    def groupdelay(self, fc):                                # :339-342
        d = C.c_float()
        _check(self._fn("groupdelay")(self._h, fc, C.byref(d)))
        return d.value

    def set_kernel(self, choice):
        """0 auto, 1 general direct form, 4 overlap-save fast convolution; crcf also 2 register-sliding and
        3 MFMA Toeplitz direct forms (include/yagi_hip.h)."""
        _check(self._fn("set_kernel")(self._h, choice))


class FirDecimationFilter(_FirBase):
    """FirDecimationFilter<T,Coeff> (src/filter/fir/firdecim.rs)."""

    def __init__(self, kind, decimation_factor, h, h_len=None):
        self._init_kind(kind)
        self._prefix = f"yagi_hip_firdecim_{kind}_"
        h = _arr(h, self.Cdt)
        hd = C.c_void_p()
        _check(self._fn("create")(decimation_factor, _ptr(h), h.size if h_len is None else h_len, C.byref(hd)))
        self._h = hd

    @classmethod
    def new_kaiser(cls, kind, decimation_factor, m, as_):    # firdecim.rs:70-87
        self = object.__new__(cls)
        self._init_kind(kind)
        self._prefix = f"yagi_hip_firdecim_{kind}_"
        hd = C.c_void_p()
        _check(self._fn("create_kaiser")(decimation_factor, m, as_, C.byref(hd)))
        self._h = hd
        return self

    @classmethod
    def new_prototype(cls, kind, ftype, decimation_factor, m, beta, dt=0.0):   # firdecim.rs:102-121
        self = object.__new__(cls)
        self._init_kind(kind)
        self._prefix = f"yagi_hip_firdecim_{kind}_"
        hd = C.c_void_p()
        _check(self._fn("create_prototype")(int(ftype), decimation_factor, m, beta, dt, C.byref(hd)))
        self._h = hd
        return self

    def get_decim_rate(self):                                # :130-132
        n = C.c_size_t()
        _check(self._fn("get_decim_rate")(self._h, C.byref(n)))
        return n.value

    def execute(self, x):                                    # :179-191
        x = _arr(x, self.T)
        y = np.zeros(1, self.T)
        _check(self._fn("execute")(self._h, _ptr(x), x.size, _ptr(y)))
        return y[0]

    def execute_block(self, x, n):                           # :200-205
        x = _arr(x, self.T)
        y = np.empty(n, self.T)
        _check(self._fn("execute_block")(self._h, _ptr(x), x.size, n, _ptr(y)))
        return y

    def execute_block_dev(self, x_dev, n, y_dev):
        _check(self._fn("execute_block_dev")(self._h, _devptr(x_dev), n, _devptr(y_dev)))

    def freqresp(self, fc):                                  # firdecim.rs:164-168
        H = np.zeros(1, np.complex64)
        _check(self._fn("freqresp")(self._h, fc, _ptr(H)))
        return H[0]


class FirPfbFilter(_FirBase):
    """FirPfbFilter<T,Coeff> (src/filter/fir/firpfb.rs)."""

    def __init__(self, kind, num_filters, h, h_len=None):
        self._init_kind(kind)
        self._prefix = f"yagi_hip_firpfb_{kind}_"
        h = _arr(h, self.Cdt)
        hd = C.c_void_p()
        _check(self._fn("create")(num_filters, _ptr(h), h.size if h_len is None else h_len, C.byref(hd)))
        self._h = hd
        self.num_filters = num_filters

    @classmethod
    def _from(cls, kind, num_filters, creator, *args):
        self = object.__new__(cls)
        self._init_kind(kind)
        self._prefix = f"yagi_hip_firpfb_{kind}_"
        hd = C.c_void_p()
        _check(self._fn(creator)(num_filters, *args, C.byref(hd)))
        self._h = hd
        self.num_filters = num_filters
        return self

    @classmethod
    def new_kaiser(cls, kind, num_filters, m, fc, as_):      # firpfb.rs:94-114
        return cls._from(kind, num_filters, "create_kaiser", m, fc, as_)

    @classmethod
    def default(cls, kind, num_filters, m):                  # firpfb.rs:79-81
        return cls._from(kind, num_filters, "create_default", m)

    def push(self, x):                                       # :255-257
        _check(self._fn("push")(self._h, _byval(x, self._Tc)))

    def write(self, x):                                      # :264-266
        x = _arr(x, self.T)
        _check(self._fn("write")(self._h, _ptr(x), x.size))

    def execute(self, i):                                    # :277-286
        y = np.zeros(1, self.T)
        _check(self._fn("execute")(self._h, i, _ptr(y)))
        return y[0]

    def execute_block(self, i, x):                           # :295-301
        x = _arr(x, self.T)
        y = np.empty_like(x)
        _check(self._fn("execute_block")(self._h, i, _ptr(x), x.size, _ptr(y), y.size))
        return y

    def execute_block_dev(self, i, x_dev, n, y_dev):
        _check(self._fn("execute_block_dev")(self._h, i, _devptr(x_dev), n, _devptr(y_dev)))

    def execute_all_dev(self, x_dev, n, y_dev):
        _check(self._fn("execute_all_dev")(self._h, _devptr(x_dev), n, _devptr(y_dev)))

    def execute_select_dev(self, idx_dev, x_dev, n, y_dev):
        _check(self._fn("execute_select_dev")(self._h, _devptr(idx_dev), _devptr(x_dev), n, _devptr(y_dev)))

    def execute_all(self, x):
        """host convenience over execute_all_dev: returns y[n, num_filters]"""
        x = _arr(x, self.T)
        dx = DeviceArray.from_numpy(x)
        dy = DeviceArray(x.size * self.num_filters, self.T)
        self.execute_all_dev(dx, x.size, dy)
        synchronize()
        return dy.to_numpy().reshape(x.size, self.num_filters)

    def execute_select(self, idx, x):
        x = _arr(x, self.T)
        idx = _arr(idx, np.uint32)
        if idx.size != x.size:
            raise ConfigError("index and sample blocks must have equal length")
        if idx.size and idx.max() >= self.num_filters:
            raise ConfigError(f"filterbank index ({idx.max()}) exceeds maximum ({self.num_filters})")
        dx, di = DeviceArray.from_numpy(x), DeviceArray.from_numpy(idx)
        dy = DeviceArray(x.size, self.T)
        self.execute_select_dev(di, dx, x.size, dy)
        synchronize()
        return dy.to_numpy()


class FirInterpolationFilter(_FirBase):
    """FirInterpolationFilter<T,Coeff> (src/filter/fir/firinterp.rs)."""

    def __init__(self, kind, interp, h, h_len=None):         # new(interp, h, h_len) :36-60
        self._init_kind(kind)
        self._prefix = f"yagi_hip_firinterp_{kind}_"
        h = _arr(h, self.Cdt)
        hd = C.c_void_p()
        _check(self._fn("create")(interp, _ptr(h), h.size if h_len is None else h_len, C.byref(hd)))
        self._h = hd

    @classmethod
    def _from(cls, kind, creator, *args):
        self = object.__new__(cls)
        self._init_kind(kind)
        self._prefix = f"yagi_hip_firinterp_{kind}_"
        hd = C.c_void_p()
        _check(self._fn(creator)(*args, C.byref(hd)))
        self._h = hd
        return self

    @classmethod
    def new_kaiser(cls, kind, interp, m, as_):               # :73-90
        return cls._from(kind, "create_kaiser", interp, m, as_)

    @classmethod
    def new_prototype(cls, kind, ftype, interp, m, beta, dt=0.0):   # :105-124
        return cls._from(kind, "create_prototype", int(ftype), interp, m, beta, dt)

    @classmethod
    def new_linear(cls, kind, interp):                       # :135-147
        return cls._from(kind, "create_linear", interp)

    @classmethod
    def new_window(cls, kind, interp, m):                    # :159-174
        return cls._from(kind, "create_window", interp, m)

    def get_interp_rate(self):                               # :186-188
        n = C.c_size_t()
        _check(self._fn("get_interp_rate")(self._h, C.byref(n)))
        return n.value

    def get_sub_len(self):                                   # :195-197
        n = C.c_size_t()
        _check(self._fn("get_sub_len")(self._h, C.byref(n)))
        return n.value

    def execute(self, x):                                    # :224-231 -> interp outputs
        y = np.empty(self.get_interp_rate(), self.T)
        _check(self._fn("execute")(self._h, _byval(x, self._Tc), _ptr(y), y.size))
        return y

    def execute_block(self, x):                              # :239-244 -> n*interp outputs
        x = _arr(x, self.T)
        y = np.empty(x.size * self.get_interp_rate(), self.T)
        _check(self._fn("execute_block")(self._h, _ptr(x), x.size, _ptr(y), y.size))
        return y

    def execute_block_dev(self, x_dev, n, y_dev):
        _check(self._fn("execute_block_dev")(self._h, _devptr(x_dev), n, _devptr(y_dev)))

    def flush(self):                                         # :251-253
        y = np.empty(self.get_interp_rate(), self.T)
        _check(self._fn("flush")(self._h, _ptr(y), y.size))
        return y


class Rresamp(_FirBase):
    """Rresamp<T,Coeff> (src/filter/resampler/rresamp.rs): rational-rate resampler, P outputs per Q inputs."""

    def __init__(self, kind, interp, decim, m, h):           # new(interp, decim, m, h) :28-57
        self._init_kind(kind)
        self._prefix = f"yagi_hip_rresamp_{kind}_"
        h = _arr(h, self.Cdt)
        hd = C.c_void_p()
        _check(self._fn("create")(interp, decim, m, _ptr(h), h.size, C.byref(hd)))
        self._h = hd

    @classmethod
    def _from(cls, kind, creator, *args):
        self = object.__new__(cls)
        self._init_kind(kind)
        self._prefix = f"yagi_hip_rresamp_{kind}_"
        hd = C.c_void_p()
        _check(self._fn(creator)(*args, C.byref(hd)))
        self._h = hd
        return self

    @classmethod
    def new_kaiser(cls, kind, interp, decim, m, bw, as_):    # :59-82
        return cls._from(kind, "create_kaiser", interp, decim, m, bw, as_)

    @classmethod
    def new_default(cls, kind, interp, decim):               # :99-104
        return cls._from(kind, "create_default", interp, decim)

    def _params(self):
        v = [C.c_size_t() for _ in range(4)]
        _check(self._fn("get_params")(self._h, *[C.byref(a) for a in v]))
        return tuple(a.value for a in v)                     # interp, decim, m, block_len

    def get_interp(self): return self._params()[0]           # :138-140
    def get_decim(self): return self._params()[1]            # :146-148
    def get_delay(self): return self._params()[2]            # :118-120
    def get_block_len(self): return self._params()[3]        # :122-124
    def get_rate(self):                                      # :126-128
        p, q, _, _ = self._params()
        return np.float32(p) / np.float32(q)
    def get_p(self): return self._params()[0] * self._params()[3]     # :130-132
    def get_q(self): return self._params()[1] * self._params()[3]     # :142-144

    def write(self, buf):                                    # :150-152
        buf = _arr(buf, self.T)
        _check(self._fn("write")(self._h, _ptr(buf), buf.size))

    def execute(self, x):                                    # :154-161  Q*block_len in -> P*block_len out
        x = _arr(x, self.T)
        y = np.empty(self.get_p(), self.T)
        _check(self._fn("execute")(self._h, _ptr(x), x.size, _ptr(y), y.size))
        return y

    def execute_block(self, x, n):                           # :163-170  n times execute
        x = _arr(x, self.T)
        y = np.empty(n * self.get_p(), self.T)
        _check(self._fn("execute_block")(self._h, _ptr(x), x.size, n, _ptr(y), y.size))
        return y

    def execute_block_dev(self, x_dev, n, y_dev):
        _check(self._fn("execute_block_dev")(self._h, _devptr(x_dev), n, _devptr(y_dev)))



class Resamp2(_FirBase):
    """Resamp2<T,Coeff> (src/filter/resampler/resamp2.rs): half-band filter / two-channel bank / x2 resampler.
    The reference designs its prototype with Parks-McClellan (design code, out of scope): `Resamp2(kind, hf, m, f0)`
    takes the designed prototype hf[4m+1]; `Resamp2.new(kind, m, f0, as_)` is the reference's constructor signature
    with a Kaiser-windowed half-band prototype."""
    FILTER, ANALYZER, SYNTHESIZER, DECIM, INTERP = range(5)

    def __init__(self, kind, hf, m, f0=0.0):                  # new() :44-88, from the designed prototype
        self._init_kind(kind)
        self._prefix = f"yagi_hip_resamp2_{kind}_"
        hf = _arr(hf, np.float32)
        if hf.size != 4 * m + 1:
            raise ConfigError("half-band prototype must hold 4*m+1 taps")
        hd = C.c_void_p()
        _check(self._fn("create")(_ptr(hf), m, f0, C.byref(hd)))
        self._h, self.m = hd, int(m)

    @classmethod
    def new(cls, kind, m, f0, as_):                           # Resamp2::new(m, f0, as_) :44
        """The reference's signature with a Kaiser-windowed half-band prototype.  NOT tap-compatible with the reference,
        whose prototype comes from its Parks-McClellan design code (resamp2.rs:58, out of scope): same structure, delay
        and stop-band specification, different tap values.  For the reference's taps pass them to the constructor."""
        self = object.__new__(cls)
        self._init_kind(kind)
        self._prefix = f"yagi_hip_resamp2_{kind}_"
        hd = C.c_void_p()
        _check(self._fn("create_kaiser")(m, f0, as_, C.byref(hd)))
        self._h, self.m = hd, int(m)
        return self

    def get_delay(self):                                      # :104-106
        d = C.c_size_t()
        _check(self._fn("get_delay")(self._h, C.byref(d)))
        return d.value

    @staticmethod
    def _out_count(mode, nx):
        return 2 * nx if mode in (0, 4) else nx // 2 if mode == 3 else nx

    def execute_block(self, mode, x):
        x = _arr(x, self.T)
        y = np.empty(self._out_count(mode, x.size), self.T)
        _check(self._fn("execute_block")(self._h, mode, _ptr(x), x.size, _ptr(y), y.size))
        return y

    def execute_block_dev(self, mode, x_dev, nx, y_dev, ny=None):
        """ny = samples the output buffer holds (default: what the form produces from nx)"""
        ny = self._out_count(mode, nx) if ny is None else ny
        _check(self._fn("execute_block_dev")(self._h, mode, _devptr(x_dev), nx, _devptr(y_dev), ny))

    # the reference's per-call forms
    def filter_execute(self, x):                              # :108-130 -> (y0, y1)
        y = self.execute_block(self.FILTER, np.array([x], self.T))
        return y[0], y[1]

    def analyzer_execute(self, x):                            # :132-143  x[2] -> y[2]
        return self.execute_block(self.ANALYZER, x)

    def synthesizer_execute(self, x):                         # :145-157  x[2] -> y[2]
        return self.execute_block(self.SYNTHESIZER, x)

    def decim_execute(self, x):                               # :159-169  x[2] -> y
        return self.execute_block(self.DECIM, x)[0]

    def interp_execute(self, x):                              # :171-180  x -> y[2]
        return self.execute_block(self.INTERP, np.array([x], self.T))


class MsResamp2(_FirBase):
    """MsResamp2<T,Coeff> (src/filter/resampler/msresamp2.rs): 2^num_stages interpolator / decimator, a chain of
    half-band stages (Kaiser prototypes; `from_taps` takes externally designed ones)."""
    DECIM, INTERP = 0, 1                                      # ResampType :27-31

    def __init__(self, kind, type_, num_stages, fc, f0, as_):  # new() :38-93
        self._init_kind(kind)
        self._prefix = f"yagi_hip_msresamp2_{kind}_"
        hd = C.c_void_p()
        _check(self._fn("create")(int(type_), num_stages, fc, f0, as_, C.byref(hd)))
        self._h = hd

    @classmethod
    def from_taps(cls, kind, type_, m_stage, hf_stages):
        self = object.__new__(cls)
        self._init_kind(kind)
        self._prefix = f"yagi_hip_msresamp2_{kind}_"
        ms = np.array(list(m_stage) or [0], np.uint64)
        hf = _arr(np.concatenate([np.asarray(h, np.float32) for h in hf_stages]) if len(m_stage) else np.zeros(1), np.float32)
        hd = C.c_void_p()
        _check(self._fn("create_taps")(int(type_), len(m_stage), _ptr(ms), _ptr(hf), C.byref(hd)))
        self._h = hd
        return self

    def _params(self):
        it, ns, d = C.c_int(), C.c_size_t(), C.c_float()
        ms = np.zeros(16, np.uint64)
        _check(self._fn("get_params")(self._h, C.byref(it), C.byref(ns), C.byref(d), _ptr(ms)))
        return it.value, ns.value, d.value, [int(v) for v in ms[: ns.value]]

    def get_type(self): return self._params()[0]              # :113-115
    def get_num_stages(self): return self._params()[1]        # :109-111
    def get_delay(self): return self._params()[2]             # :117-135
    def get_stage_lengths(self): return self._params()[3]
    def get_rate(self):                                       # :102-107
        it, ns, _, _ = self._params()
        return float(1 << ns) if it else 1.0 / (1 << ns)

    def set_scale(self, scale):
        raise ConfigError("MsResamp2 has no scale (msresamp2.rs)")

    get_scale = set_scale

    def execute_block(self, x, n=None):
        """n execute() calls (:137-152): interp: n inputs -> n*rate outputs; decim: n*rate inputs -> n outputs.
        x must hold exactly the n calls' input (the reference's copy_from_slice panics otherwise, :181)"""
        x = _arr(x, self.T)
        it, ns, _, _ = self._params()
        rate = 1 << ns
        n = (x.size if it else x.size // rate) if n is None else n
        y = np.empty(n * rate if it else n, self.T)
        _check(self._fn("execute_block")(self._h, _ptr(x), x.size, _ptr(y), y.size))
        return y

    def execute_block_dev(self, x_dev, n, y_dev, nx=None, ny=None):
        """n execute() calls on device buffers of nx / ny samples (defaults: exactly what n calls consume / produce)"""
        it, ns, _, _ = self._params()
        rate = 1 << ns
        nx = (n if it else n * rate) if nx is None else nx
        ny = (n * rate if it else n) if ny is None else ny
        _check(self._fn("execute_block_dev")(self._h, _devptr(x_dev), nx, _devptr(y_dev), ny))

    def execute(self, x):                                     # :137-152
        return self.execute_block(x, 1)


class Resamp(_FirBase):
    """Resamp<T,Coeff> (src/filter/resampler/resamp.rs): arbitrary-rate resampler, rate in [0.004, 250], a bank of
    npfb (rounded up to a power of two) branches of 2m taps selected by a 24-bit fractional phase."""

    def __init__(self, kind, rate, m, fc, as_, npfb):          # new(rate, m, fc, as_, npfb) :24-71
        self._init_kind(kind)
        self._prefix = f"yagi_hip_resamp_{kind}_"
        hd = C.c_void_p()
        _check(self._fn("create")(rate, m, fc, as_, npfb, C.byref(hd)))
        self._h = hd

    @classmethod
    def _from(cls, kind, creator, *args):
        self = object.__new__(cls)
        self._init_kind(kind)
        self._prefix = f"yagi_hip_resamp_{kind}_"
        hd = C.c_void_p()
        _check(self._fn(creator)(*args, C.byref(hd)))
        self._h = hd
        return self

    @classmethod
    def new_default(cls, kind, rate):                         # :73-84  m 7, fc 0.25, 60 dB, npfb 256
        return cls._from(kind, "create_default", rate)

    @classmethod
    def from_taps(cls, kind, rate, m, npfb, h):
        """the bank from external taps h[0 .. 2 m npfb) (npfb a power of two in [2, 2^16])"""
        if kind not in KINDS:
            raise ConfigError(f"unknown type combination {kind!r}")
        h = _arr(h, KINDS[kind][1])
        return cls._from(kind, "create_taps", rate, m, npfb, _ptr(h), h.size)

    def set_scale(self, scale):
        raise ConfigError("Resamp has no scale (resamp.rs)")

    get_scale = set_scale

    def set_rate(self, rate):                                 # :95-106
        _check(self._fn("set_rate")(self._h, rate))

    def adjust_rate(self, gamma):                             # :112-118
        _check(self._fn("adjust_rate")(self._h, gamma))

    def get_rate(self):                                       # :108-110
        r = C.c_float()
        _check(self._fn("get_rate")(self._h, C.byref(r)))
        return np.float32(r.value)

    def get_delay(self):                                      # :91-93
        d = C.c_size_t()
        _check(self._fn("get_delay")(self._h, C.byref(d)))
        return d.value

    def get_num_output(self, num_input):                      # :128-139
        n = C.c_size_t()
        _check(self._fn("get_num_output")(self._h, num_input, C.byref(n)))
        return n.value

    def execute(self, x):                                     # :141-154  one sample in
        y = np.empty(max(self.get_num_output(1), 1), self.T)
        nw = C.c_size_t()
        _check(self._fn("execute")(self._h, _byval(x, self._Tc), _ptr(y), y.size, C.byref(nw)))
        return y[: nw.value]

    def execute_block(self, x):                               # :156-165
        x = _arr(x, self.T)
        y = np.empty(max(self.get_num_output(x.size), 1), self.T)
        nw = C.c_size_t()
        _check(self._fn("execute_block")(self._h, _ptr(x), x.size, _ptr(y), y.size, C.byref(nw)))
        return y[: nw.value]

    def execute_block_dev(self, x_dev, nx, y_dev, ny_cap):
        """nx device samples in; y_dev holds ny_cap samples (>= get_num_output(nx)); returns the outputs written"""
        nw = C.c_size_t()
        _check(self._fn("execute_block_dev")(self._h, _devptr(x_dev), nx, _devptr(y_dev), ny_cap, C.byref(nw)))
        return nw.value


class IirFilter(_FirBase):
    """IirFilter<T,Coeff> (src/filter/iir/iirfilt.rs): transfer-function (n = max(na, nb) <= 33; the shorter of b and
    a is zero-padded) or second-order-section form.  Block calls on the device run the chunked state scan of
    iir_kernels.hip; execute() and short host blocks run the reference's recurrence on the host mirror of the state."""

    def __init__(self, kind, b, a):                           # new(b, a) :65-100
        self._init_kind(kind)
        self._prefix = f"yagi_hip_iirfilt_{kind}_"
        b, a = _arr(b, self.Cdt), _arr(a, self.Cdt)
        hd = C.c_void_p()
        _check(self._fn("create")(_ptr(b), b.size, _ptr(a), a.size, C.byref(hd)))
        self._h = hd

    @classmethod
    def _from(cls, kind, creator, *args):
        self = object.__new__(cls)
        self._init_kind(kind)
        self._prefix = f"yagi_hip_iirfilt_{kind}_"
        hd = C.c_void_p()
        _check(self._fn(creator)(*args, C.byref(hd)))
        self._h = hd
        return self

    @classmethod
    def new_sos(cls, kind, b, a, nsos):                       # :111-137  b, a = [nsos][3]
        if kind not in KINDS:
            raise ConfigError(f"unknown type combination {kind!r}")
        b, a = _arr(b, KINDS[kind][1]).ravel(), _arr(a, KINDS[kind][1]).ravel()
        if b.size < 3 * nsos or a.size < 3 * nsos:
            raise ConfigError("second-order sections need 3*nsos coefficients in b and a")
        return cls._from(kind, "create_sos", _ptr(b), _ptr(a), nsos)

    @classmethod
    def new_dc_blocker(cls, kind, alpha):                     # :290-305
        return cls._from(kind, "create_dc_blocker", alpha)

    @classmethod
    def new_integrator(cls, kind):                            # :204-246
        return cls._from(kind, "create_integrator")

    @classmethod
    def new_differentiator(cls, kind):                        # :248-288
        return cls._from(kind, "create_differentiator")

    @classmethod
    def new_pll(cls, kind, w, zeta, k):                       # :310-330
        return cls._from(kind, "create_pll", w, zeta, k)

    @classmethod
    def new_prototype(cls, kind, shape, order, fc, ap, as_):  # :148-184  (Lowpass, SecondOrderSections)
        return cls._from(kind, "create_prototype", int(IirFilterShape(shape)), order, fc, ap, as_)

    @classmethod
    def new_lowpass(cls, kind, order, fc):                    # :189-201
        return cls._from(kind, "create_lowpass", order, fc)

    def get_length(self):                                     # :410-413
        n = C.c_size_t()
        _check(self._fn("get_length")(self._h, C.byref(n)))
        return n.value

    def execute(self, x):                                     # :385-390
        y = np.zeros(1, self.T)
        _check(self._fn("execute")(self._h, _byval(x, self._Tc), _ptr(y)))
        return y[0]

    def execute_block(self, x, y=None):                       # :393-407
        x = _arr(x, self.T)
        if y is None:
            y = np.empty_like(x)
        elif y.dtype != self.T or not y.flags.c_contiguous:
            raise ConfigError("output must be a contiguous array of the sample type")
        _check(self._fn("execute_block")(self._h, _ptr(x), x.size, _ptr(y), y.size))
        return y

    def execute_block_dev(self, x_dev, n, y_dev):
        _check(self._fn("execute_block_dev")(self._h, _devptr(x_dev), n, _devptr(y_dev)))

    def freqresponse(self, fc):                               # :416-451
        h = cf32()
        _check(self._fn("freqresponse")(self._h, fc, C.byref(h)))
        return np.complex64(complex(h.re, h.im))

    def get_psd(self, fc):                                    # :453-457
        v = C.c_float()
        _check(self._fn("get_psd")(self._h, fc, C.byref(v)))
        return np.float32(v.value)

    def groupdelay(self, fc):                                 # :459-480
        v = C.c_float()
        _check(self._fn("groupdelay")(self._h, fc, C.byref(v)))
        return np.float32(v.value)


class IirFilterShape(enum.IntEnum):
    """design::IirFilterShape (src/filter/iir/design/mod.rs:32-38); Butter and Cheby2 are built"""
    Butter = 0
    Cheby1 = 1
    Cheby2 = 2
    Ellip = 3
    Bessel = 4


def iir_design_lowpass_sos(shape, order, fc, ap=0.1, as_=60.0):
    """iir_design() (design/mod.rs:567-717), low-pass band, second-order sections: (b, a), each [(order + 1) // 2][3].
    No device needed."""
    ns = max((order + 1) // 2, 1)
    b, a = np.zeros(3 * ns, np.float32), np.zeros(3 * ns, np.float32)
    _check(lib.yagi_hip_iir_design_lowpass_sos(int(IirFilterShape(shape)), order, fc, ap, as_, _ptr(b), _ptr(a)))
    return b.reshape(ns, 3), a.reshape(ns, 3)


class _IirRateBase(_FirBase):
    """shared by IirDecimationFilter and IirInterpolationFilter: one IirFilter over the virtual stream of n*M steps"""
    _name = _get = None

    def __init__(self, kind, M, b, a):                        # new(M, b, a)
        self._init_kind(kind)
        self._prefix = f"yagi_hip_{self._name}_{kind}_"
        b, a = _arr(b, self.Cdt), _arr(a, self.Cdt)
        hd = C.c_void_p()
        _check(self._fn("create")(M, _ptr(b), b.size, _ptr(a), a.size, C.byref(hd)))
        self._h = hd

    @classmethod
    def _from(cls, kind, creator, *args):
        self = object.__new__(cls)
        self._init_kind(kind)
        self._prefix = f"yagi_hip_{cls._name}_{kind}_"
        hd = C.c_void_p()
        _check(self._fn(creator)(*args, C.byref(hd)))
        self._h = hd
        return self

    @classmethod
    def new_sos(cls, kind, M, b, a, nsos):                    # extension: external second-order sections
        if kind not in KINDS:
            raise ConfigError(f"unknown type combination {kind!r}")
        b, a = _arr(b, KINDS[kind][1]).ravel(), _arr(a, KINDS[kind][1]).ravel()
        if b.size < 3 * nsos or a.size < 3 * nsos:
            raise ConfigError("second-order sections need 3*nsos coefficients in b and a")
        return cls._from(kind, "create_sos", M, _ptr(b), _ptr(a), nsos)

    @classmethod
    def new_prototype(cls, kind, M, shape, order, fc, ap, as_):
        return cls._from(kind, "create_prototype", M, int(IirFilterShape(shape)), order, fc, ap, as_)

    @classmethod
    def new_default(cls, kind, M, order):
        return cls._from(kind, "create_default", M, order)

    def get_rate(self):
        m = C.c_size_t()
        _check(self._fn(self._get)(self._h, C.byref(m)))
        return m.value

    def groupdelay(self, fc):
        v = C.c_float()
        _check(self._fn("groupdelay")(self._h, fc, C.byref(v)))
        return np.float32(v.value)

    def execute_block_dev(self, x_dev, n, y_dev):
        """n units on device arrays (decimator: n*M samples in, n out; interpolator: n in, n*M out)"""
        _check(self._fn("execute_block_dev")(self._h, _devptr(x_dev), n, _devptr(y_dev)))


class IirDecimationFilter(_IirRateBase):
    """IirDecimationFilter<T,Coeff> (src/filter/iir/iirdecim.rs): the filter runs over all n*M inputs and the output of
    step i*M is kept.  new_default: Butterworth, fc 0.5/M (:63-75)."""
    _name, _get = "iirdecim", "get_decim"
    get_decim = _IirRateBase.get_rate

    def execute(self, x):                                     # :128-137  x[M] -> one sample
        x = _arr(x, self.T)
        if x.size != self.get_rate():
            raise ConfigError("execute() takes exactly M samples")
        y = np.zeros(1, self.T)
        _check(self._fn("execute")(self._h, _ptr(x), _ptr(y)))
        return y[0]

    def execute_block(self, x, n=None):                       # :145-149  n*M samples -> n
        x = _arr(x, self.T)
        m = self.get_rate()
        n = x.size // m if n is None else n
        if x.size < n * m:
            raise ConfigError("execute_block() needs n*M input samples")
        y = np.empty(n, self.T)
        _check(self._fn("execute_block")(self._h, _ptr(x), n, _ptr(y)))
        return y


class IirInterpolationFilter(_IirRateBase):
    """IirInterpolationFilter<T,Coeff> (src/filter/iir/iirinterp.rs): x[i] at step i*M, +0.0 at the M - 1 steps after
    it, every output kept.  new_default: Chebyshev-II, fc 0.5/M, 0.1, 60 (:34-46); prototypes set the scale to M."""
    _name, _get = "iirinterp", "get_interp"
    get_interp = _IirRateBase.get_rate

    def execute(self, x):                                     # :93-103  one sample -> y[M]
        y = np.zeros(self.get_rate(), self.T)
        _check(self._fn("execute")(self._h, _byval(x, self._Tc), _ptr(y)))
        return y

    def execute_block(self, x):                               # :106-115  n samples -> n*M
        x = _arr(x, self.T)
        y = np.empty(x.size * self.get_rate(), self.T)
        _check(self._fn("execute_block")(self._h, _ptr(x), x.size, _ptr(y)))
        return y


class IirHilbertFilter(_Handle):
    """IirHilbertFilter (src/filter/iir/iirhilb.rs): the reference's two real filters run as one crcf IirFilter over a
    complex stream, the four modes as input / output maps selected by the 2-bit state.  decim / interp after r2c / c2r
    left the state at 2 or 3 raise ModeError (the reference underflows a u8): reset first."""
    _prefix = "yagi_hip_iirhilbf_"

    def __init__(self, shape, n, ap, as_):                    # new() :15-36
        hd = C.c_void_p()
        _check(lib.yagi_hip_iirhilbf_create(int(IirFilterShape(shape)), n, ap, as_, C.byref(hd)))
        self._h = hd

    @classmethod
    def new_default(cls, n):                                  # :38-47
        self = object.__new__(cls)
        hd = C.c_void_p()
        _check(lib.yagi_hip_iirhilbf_create_default(n, C.byref(hd)))
        self._h = hd
        return self

    @classmethod
    def new_sos(cls, b, a, nsos):                             # extension: external real sections
        b, a = _arr(b, np.float32).ravel(), _arr(a, np.float32).ravel()
        if b.size < 3 * nsos or a.size < 3 * nsos:
            raise ConfigError("second-order sections need 3*nsos coefficients in b and a")
        self = object.__new__(cls)
        hd = C.c_void_p()
        _check(lib.yagi_hip_iirhilbf_create_sos(_ptr(b), _ptr(a), nsos, C.byref(hd)))
        self._h = hd
        return self

    def clone(self):                                          # derive(Clone)
        new = object.__new__(type(self))
        h = C.c_void_p()
        _check(lib.yagi_hip_iirhilbf_clone(self._h, C.byref(h)))
        new._h = h
        return new

    def get_state(self):
        v = C.c_int()
        _check(lib.yagi_hip_iirhilbf_get_state(self._h, C.byref(v)))
        return v.value

    def r2c_execute(self, x):                                 # :55-82
        y = cf32()
        _check(lib.yagi_hip_iirhilbf_r2c_execute(self._h, float(x), C.byref(y)))
        return np.complex64(complex(y.re, y.im))

    def c2r_execute(self, x):                                 # :90-117
        y = C.c_float()
        _check(lib.yagi_hip_iirhilbf_c2r_execute(self._h, _byval(x, cf32), C.byref(y)))
        return np.float32(y.value)

    def decim_execute(self, x):                               # :125-139, x: 2 real samples
        x = _arr(x, np.float32)
        if x.size != 2:
            raise ConfigError("decim_execute() takes exactly 2 samples")
        y = cf32()
        _check(lib.yagi_hip_iirhilbf_decim_execute(self._h, _ptr(x), C.byref(y)))
        return np.complex64(complex(y.re, y.im))

    def interp_execute(self, x):                              # :147-158 -> 2 real samples
        y = np.zeros(2, np.float32)
        _check(lib.yagi_hip_iirhilbf_interp_execute(self._h, _byval(x, cf32), _ptr(y)))
        return y

    _SHAPES = {"r2c": (np.float32, 1, np.complex64, 1), "c2r": (np.complex64, 1, np.float32, 1),
               "decim": (np.float32, 2, np.complex64, 1), "interp": (np.complex64, 1, np.float32, 2)}

    def _block(self, name, x):
        xdt, xin, ydt, yout = self._SHAPES[name]
        x = _arr(x, xdt)
        if x.size % xin:
            raise ConfigError("decim_execute_block() takes an even number of samples")
        n = x.size // xin
        y = np.empty(n * yout, ydt)
        _check(getattr(lib, f"{self._prefix}{name}_execute_block")(self._h, _ptr(x), n, _ptr(y)))
        return y

    def r2c_execute_block(self, x): return self._block("r2c", x)          # :84-88
    def c2r_execute_block(self, x): return self._block("c2r", x)          # :119-123
    def decim_execute_block(self, x): return self._block("decim", x)      # :141-145: 2n real -> n complex
    def interp_execute_block(self, x): return self._block("interp", x)    # :160-164: n complex -> 2n real

    def _dev(self, name, x_dev, n, y_dev):
        _check(getattr(lib, f"{self._prefix}{name}_execute_block_dev")(self._h, _devptr(x_dev), n, _devptr(y_dev)))

    def r2c_execute_block_dev(self, x_dev, n, y_dev): self._dev("r2c", x_dev, n, y_dev)        # n float32 -> n complex64
    def c2r_execute_block_dev(self, x_dev, n, y_dev): self._dev("c2r", x_dev, n, y_dev)        # n complex64 -> n float32
    def decim_execute_block_dev(self, x_dev, n, y_dev): self._dev("decim", x_dev, n, y_dev)    # 2n float32 -> n complex64
    def interp_execute_block_dev(self, x_dev, n, y_dev): self._dev("interp", x_dev, n, y_dev)  # n complex64 -> 2n float32


class OscScheme(enum.Enum):
    """nco::OscScheme (src/nco/osc.rs:13-17)"""
    Nco = 0
    Vco = 1


class Osc(_Handle):
    """nco::Osc (src/nco/osc.rs): NCO (1024-entry sine table) or VCO (interpolated table) with PLL and mixers.  The
    state (two u32 words, the PLL gains) lives on the host; mix_block_*_dev runs osc_kernels.hip on device arrays and
    every output word equals the reference's sequential loop."""
    _prefix = "yagi_hip_osc_"

    def __init__(self, scheme):                               # new() :37-57
        scheme = OscScheme(scheme)
        hd = C.c_void_p()
        _check(lib.yagi_hip_osc_create(scheme.value, C.byref(hd)))
        self._h = hd
        self.scheme = scheme

    def clone(self):                                          # derive(Clone)
        new = object.__new__(type(self))
        new.scheme = self.scheme
        h = C.c_void_p()
        _check(lib.yagi_hip_osc_clone(self._h, C.byref(h)))
        new._h = h
        return new

    def set_frequency(self, dtheta):                          # :66-68
        _check(lib.yagi_hip_osc_set_frequency(self._h, dtheta))

    def adjust_frequency(self, df):                           # :71-73
        _check(lib.yagi_hip_osc_adjust_frequency(self._h, df))

    def set_phase(self, phi):                                 # :76-78
        _check(lib.yagi_hip_osc_set_phase(self._h, phi))

    def adjust_phase(self, dphi):                             # :81-83
        _check(lib.yagi_hip_osc_adjust_phase(self._h, dphi))

    def step(self):                                           # :86-88
        _check(lib.yagi_hip_osc_step(self._h))

    def _f32(self, name):
        v = C.c_float()
        _check(getattr(lib, self._prefix + name)(self._h, C.byref(v)))
        return np.float32(v.value)

    def get_phase(self):                                      # :91-93
        return self._f32("get_phase")

    def get_frequency(self):                                  # :96-103
        return self._f32("get_frequency")

    def sin(self):                                            # :106-111
        return self._f32("sin")

    def cos(self):                                            # :114-119
        return self._f32("cos")

    def sin_cos(self):                                        # :122-127  (sin, cos)
        s, c = C.c_float(), C.c_float()
        _check(lib.yagi_hip_osc_sin_cos(self._h, C.byref(s), C.byref(c)))
        return np.float32(s.value), np.float32(c.value)

    def cexp(self):                                           # :130-133
        v = cf32()
        _check(lib.yagi_hip_osc_cexp(self._h, C.byref(v)))
        return np.complex64(complex(v.re, v.im))

    def get_state(self):
        """extension: the raw u32 words (theta, d_theta)"""
        t, d = C.c_uint32(), C.c_uint32()
        _check(lib.yagi_hip_osc_get_state(self._h, C.byref(t), C.byref(d)))
        return t.value, d.value

    def pll_set_bandwidth(self, bw):                          # :138-144
        _check(lib.yagi_hip_osc_pll_set_bandwidth(self._h, bw))

    def pll_step(self, dphi):                                 # :147-150
        _check(lib.yagi_hip_osc_pll_step(self._h, dphi))

    def _mix1(self, name, x):
        y = cf32()
        _check(getattr(lib, self._prefix + name)(self._h, _byval(x, cf32), C.byref(y)))
        return np.complex64(complex(y.re, y.im))

    def mix_up(self, x):                                      # :155-158
        return self._mix1("mix_up", x)

    def mix_down(self, x):                                    # :173-176
        return self._mix1("mix_down", x)

    def _block(self, name, x, y):
        x = _arr(x, np.complex64)
        if y is None:
            y = np.empty_like(x)
        elif not (isinstance(y, np.ndarray) and y.dtype == np.complex64 and y.flags.c_contiguous):
            raise ConfigError("output must be a C-contiguous complex64 array")
        _check(getattr(lib, self._prefix + name)(self._h, _ptr(x), x.size, _ptr(y), y.size))
        return y

    def mix_block_up(self, x, y=None):                        # :161-170 (len(x) != len(y) -> RangeError)
        return self._block("mix_block_up", x, y)

    def mix_block_down(self, x, y=None):                      # :179-188
        return self._block("mix_block_down", x, y)

    def mix_block_up_dev(self, x_dev, n, y_dev):
        _check(lib.yagi_hip_osc_mix_block_up_dev(self._h, _devptr(x_dev), n, _devptr(y_dev)))

    def mix_block_down_dev(self, x_dev, n, y_dev):
        _check(lib.yagi_hip_osc_mix_block_down_dev(self._h, _devptr(x_dev), n, _devptr(y_dev)))


class _DdcBase(_FirBase):
    """what Ddc and Duc share: the oscillator words, the filter's scale and rate, the kernel choice"""
    _obj = None
    _rate_fn = None

    def __init__(self, kind, scheme, rate, h, h_len=None):
        self._init_ddc(kind, scheme)
        h = _arr(h, self.Cdt)
        hd = C.c_void_p()
        _check(self._fn("create")(self.scheme.value, rate, _ptr(h), h.size if h_len is None else h_len, C.byref(hd)))
        self._h = hd

    def _init_ddc(self, kind, scheme):
        if kind not in ("crcf", "cccf"):
            raise ConfigError(f"{type(self).__name__} mixes complex samples: kind must be 'crcf' or 'cccf', not {kind!r}")
        self._init_kind(kind)
        self._prefix = f"yagi_hip_{self._obj}_{kind}_"
        self.scheme = OscScheme(scheme)

    @classmethod
    def new_kaiser(cls, kind, scheme, rate, m, as_):
        self = object.__new__(cls)
        self._init_ddc(kind, scheme)
        hd = C.c_void_p()
        _check(self._fn("create_kaiser")(self.scheme.value, rate, m, as_, C.byref(hd)))
        self._h = hd
        return self

    def set_frequency(self, dtheta):
        _check(self._fn("set_frequency")(self._h, dtheta))

    def adjust_frequency(self, df):
        _check(self._fn("adjust_frequency")(self._h, df))

    def set_phase(self, phi):
        _check(self._fn("set_phase")(self._h, phi))

    def adjust_phase(self, dphi):
        _check(self._fn("adjust_phase")(self._h, dphi))

    def _f32(self, name):
        v = C.c_float()
        _check(self._fn(name)(self._h, C.byref(v)))
        return np.float32(v.value)

    def get_frequency(self):
        return self._f32("get_frequency")

    def get_phase(self):
        return self._f32("get_phase")

    def get_state(self):
        """extension: the raw u32 words (theta, d_theta)"""
        t, d = C.c_uint32(), C.c_uint32()
        _check(self._fn("get_state")(self._h, C.byref(t), C.byref(d)))
        return t.value, d.value

    def set_state(self, theta, d_theta):
        """extension: set the raw u32 words"""
        _check(self._fn("set_state")(self._h, theta & 0xFFFFFFFF, d_theta & 0xFFFFFFFF))

    def _rate(self):
        n = C.c_size_t()
        _check(self._fn(self._rate_fn)(self._h, C.byref(n)))
        return n.value

    def set_kernel(self, choice):
        """0 auto (fused where a fused kernel serves the shape), 1 two launches, 2 fused where served"""
        _check(self._fn("set_kernel")(self._h, choice))

    def get_last_kernel(self):
        """1 (two launches) or 2 (fused): what the last block call ran; 0 before the first"""
        k = C.c_int()
        _check(self._fn("get_last_kernel")(self._h, C.byref(k)))
        return k.value

    def execute_block_devptr(self, x_dev, n, y_dev):
        """x_dev, y_dev: complex64 on the device, not overlapping (ConfigError), 8-byte aligned; Ddc reads n*M samples
        and writes n, Duc reads n and writes n*I; asynchronous on the object's stream"""
        _check(self._fn("execute_block_dev")(self._h, _devptr(x_dev), n, _devptr(y_dev)))


class Ddc(_DdcBase):
    """Digital down-converter: Osc.mix_block_down followed by FirDecimationFilter.execute_block in one launch
    (ddc_kernels.hip), kinds crcf and cccf.  Every output word equals the two objects' composition; the decimator's
    window holds mixed samples."""
    _obj = "ddc"
    _rate_fn = "get_decim_rate"

    def get_decim_rate(self):
        return self._rate()

    def execute(self, x):
        """M samples -> one output, on the host"""
        x = _arr(x, np.complex64)
        if x.size < self._rate():
            raise ConfigError(f"input block too short: need {self._rate()} samples, got {x.size}")
        y = np.zeros(1, np.complex64)
        _check(self._fn("execute")(self._h, _ptr(x), _ptr(y)))
        return y[0]

    def execute_block(self, x, n):
        """n outputs from the first n*M samples of x"""
        x = _arr(x, np.complex64)
        if x.size < n * self._rate():
            raise ConfigError(f"input block too short: need {n * self._rate()} samples, got {x.size}")
        y = np.empty(n, np.complex64)
        _check(self._fn("execute_block")(self._h, _ptr(x), n, _ptr(y)))
        return y


class Duc(_DdcBase):
    """Digital up-converter: FirInterpolationFilter.execute_block followed by Osc.mix_block_up in one launch
    (ddc_kernels.hip), kinds crcf and cccf.  Every output word equals the two objects' composition."""
    _obj = "duc"
    _rate_fn = "get_interp_rate"

    def get_interp_rate(self):
        return self._rate()

    def execute(self, x):
        """one sample -> I outputs, on the host"""
        xv = np.array([x], np.complex64)
        y = np.empty(self._rate(), np.complex64)
        _check(self._fn("execute")(self._h, _ptr(xv), _ptr(y)))
        return y

    def execute_block(self, x):
        """n samples -> n*I outputs"""
        x = _arr(x, np.complex64)
        y = np.empty(x.size * self._rate(), np.complex64)
        _check(self._fn("execute_block")(self._h, _ptr(x), x.size, _ptr(y)))
        return y


class FirHilbertFilter(_Handle):
    """FirHilbertFilter (src/filter/fir/firhilb.rs): real <-> complex Hilbert transform, 2:1 real-to-complex decimator,
    1:2 complex-to-real interpolator.  The four windows and the toggle are shared by every mode; the per-sample calls run
    on the host, the *_dev block forms run firhilb_kernels.hip on device arrays, and every output word equals the
    reference's sequential loop."""
    _prefix = "yagi_hip_firhilb_"

    def __init__(self, m, as_):                              # new() :38-84
        hd = C.c_void_p()
        _check(lib.yagi_hip_firhilb_create(m, as_, C.byref(hd)))
        self._h = hd
        self.m = int(m)

    def clone(self):                                          # derive(Clone)
        new = object.__new__(type(self))
        new.m = self.m
        h = C.c_void_p()
        _check(lib.yagi_hip_firhilb_clone(self._h, C.byref(h)))
        new._h = h
        return new

    def r2c_execute(self, x):                                 # :104-137
        y = cf32()
        _check(lib.yagi_hip_firhilb_r2c_execute(self._h, float(np.float32(x)), C.byref(y)))
        return np.complex64(complex(y.re, y.im))

    def c2r_execute(self, x):                                 # :149-180  (lsb, usb)
        a, b = C.c_float(), C.c_float()
        _check(lib.yagi_hip_firhilb_c2r_execute(self._h, _byval(x, cf32), C.byref(a), C.byref(b)))
        return np.float32(a.value), np.float32(b.value)

    def decim_execute(self, x):                               # :191-211, x: 2 real samples
        x = _arr(x, np.float32)
        if x.size < 2:
            raise RangeError("decim_execute needs 2 input samples")
        y = cf32()
        _check(lib.yagi_hip_firhilb_decim_execute(self._h, _ptr(x), C.byref(y)))
        return np.complex64(complex(y.re, y.im))

    def interp_execute(self, x, y=None):                      # :233-248 -> 2 real samples
        y = _out(y, 2, np.float32)
        _check(lib.yagi_hip_firhilb_interp_execute(self._h, _byval(x, cf32), _ptr(y)))
        return y

    def _block(self, name, x, xdt, y, ydt, ny):
        x = _arr(x, xdt)
        y = np.empty(ny(x.size), ydt) if y is None else y
        if not (isinstance(y, np.ndarray) and y.dtype == np.dtype(ydt) and y.flags.c_contiguous):
            raise ConfigError(f"output must be a C-contiguous {np.dtype(ydt).name} array")
        _check(getattr(lib, self._prefix + name)(self._h, _ptr(x), x.size, _ptr(y), y.size))
        return y

    def decim_execute_block(self, x, y=None):                 # :220-225: 2n real -> n complex (else RangeError)
        return self._block("decim_execute_block", x, np.float32, y, np.complex64, lambda n: n // 2)

    def interp_execute_block(self, x, y=None):                # :257-262: n complex -> 2n real
        return self._block("interp_execute_block", x, np.complex64, y, np.float32, lambda n: 2 * n)

    def r2c_execute_block(self, x, y=None):
        """extension: n repeated r2c_execute calls, n real -> n complex"""
        return self._block("r2c_execute_block", x, np.float32, y, np.complex64, lambda n: n)

    def c2r_execute_block(self, x, y=None):
        """extension: n repeated c2r_execute calls, n complex -> 2n real, (lsb, usb) of input i at y[2i], y[2i + 1]"""
        return self._block("c2r_execute_block", x, np.complex64, y, np.float32, lambda n: 2 * n)

    def _dev(self, name, x_dev, n, y_dev):
        _check(getattr(lib, self._prefix + name)(self._h, _devptr(x_dev), n, _devptr(y_dev)))

    def decim_execute_block_dev(self, x_dev, n, y_dev):      # x_dev: 2n float32, y_dev: n complex64
        self._dev("decim_execute_block_dev", x_dev, n, y_dev)

    def interp_execute_block_dev(self, x_dev, n, y_dev):     # x_dev: n complex64, y_dev: 2n float32
        self._dev("interp_execute_block_dev", x_dev, n, y_dev)

    def r2c_execute_block_dev(self, x_dev, n, y_dev):        # x_dev: n float32, y_dev: n complex64
        self._dev("r2c_execute_block_dev", x_dev, n, y_dev)

    def c2r_execute_block_dev(self, x_dev, n, y_dev):        # x_dev: n complex64, y_dev: 2n float32
        self._dev("c2r_execute_block_dev", x_dev, n, y_dev)


class Fdelay(_FirBase):
    """Fdelay<T,Coeff> (src/filter/fdelay.rs): fractional delay, 0 <= delay <= nmax, as a whole-sample lag in front of
    one branch of FirPfbFilter::default(npfb, m).  The per-sample calls run on the host; execute_block and the
    per-sample-delay execute_track run fdelay_kernels.hip, and every output word equals the reference's sequential loop,
    also where the delay changes between or inside calls."""

    def __init__(self, kind, nmax, m=8, npfb=64):             # new() :26-53, new_default() :55-57
        self._init_kind(kind)
        self._prefix = f"yagi_hip_fdelay_{kind}_"
        hd = C.c_void_p()
        if (m, npfb) == (8, 64):
            _check(self._fn("create_default")(nmax, C.byref(hd)))
        else:
            _check(self._fn("create")(nmax, m, npfb, C.byref(hd)))
        self._h = hd

    def set_scale(self, scale):
        raise ConfigError("Fdelay has no scale (fdelay.rs)")

    def get_scale(self):
        raise ConfigError("Fdelay has no scale (fdelay.rs)")

    def get_delay(self):                                      # :67-69
        d = C.c_float()
        _check(self._fn("get_delay")(self._h, C.byref(d)))
        return np.float32(d.value)

    def set_delay(self, delay):                               # :71-97
        _check(self._fn("set_delay")(self._h, float(np.float32(delay))))

    def adjust_delay(self, delta):                            # :99-101
        _check(self._fn("adjust_delay")(self._h, float(np.float32(delta))))

    def _get(self, name):
        v = C.c_size_t()
        _check(self._fn(name)(self._h, C.byref(v)))
        return v.value

    def get_nmax(self):                                       # :103-105
        return self._get("get_nmax")

    def get_m(self):                                          # :107-109
        return self._get("get_m")

    def get_npfb(self):                                       # :111-113
        return self._get("get_npfb")

    def push(self, x):                                        # :115-118
        _check(self._fn("push")(self._h, _byval(x, self._Tc)))

    def write(self, x):                                       # :120-124
        x = _arr(x, self.T)
        _check(self._fn("write")(self._h, _ptr(x), x.size))

    def execute(self):                                        # :126-128
        y = np.zeros(1, self.T)
        _check(self._fn("execute")(self._h, _ptr(y)))
        return y[0]

    def execute_block(self, x, y=None):                       # :130-136
        x = _arr(x, self.T)
        y = _out(y, x.size, self.T)
        _check(self._fn("execute_block")(self._h, _ptr(x), x.size, _ptr(y), y.size))
        return y

    def execute_block_dev(self, x_dev, n, y_dev):
        _check(self._fn("execute_block_dev")(self._h, _devptr(x_dev), n, _devptr(y_dev)))

    def execute_track(self, delay, x, y=None):
        """extension: one delay per sample, `for i: set_delay(delay[i]); push(x[i]); y[i] = execute()`; a delay outside
        [0, nmax] anywhere in the array is a ConfigError and leaves the object unchanged"""
        x = _arr(x, self.T)
        delay = _arr(delay, np.float32)
        if delay.size != x.size:
            raise ConfigError("delay and sample blocks must have equal length")
        y = _out(y, x.size, self.T)
        _check(self._fn("execute_track")(self._h, _ptr(delay), _ptr(x), x.size, _ptr(y)))
        return y

    def execute_track_dev(self, delay_dev, x_dev, n, y_dev):
        """delay_dev: n float32 on the device, each clamped into [0, nmax] (what is not >= 0 counts as 0)"""
        _check(self._fn("execute_track_dev")(self._h, _devptr(delay_dev), _devptr(x_dev), n, _devptr(y_dev)))


ORDFILT_NMAX = 1025      # YAGI_ORDFILT_NMAX: the longest window of OrdFilt
ORDFILT_TILE = 4096      # YAGI_ORDFILT_TILE: outputs per workgroup of ordfilt_kernels.hip
ORDFILT_REG_NMAX = 9     # YAGI_ORDFILT_REG_NMAX: the longest window of the register-resident kernel form


class OrdFilt(_Handle):
    """OrdFilt<f32> (src/filter/ordfilt.rs): the sample of rank k (0-based, ascending) among the last n, the median for
    OrdFilt.medfilt(m).  The per-sample calls run on the host; execute_block runs ordfilt_kernels.hip, and every output
    word equals the reference's sequential loop (stable sort, so the older of -0.0 / +0.0 comes first).  NaN, which the
    reference leaves unspecified, sorts beyond the infinity of its sign (yagi_hip.h).  n <= ORDFILT_NMAX."""
    _prefix = "yagi_hip_ordfilt_rrrf_"

    def __init__(self, n, k):                                 # new() :16-30
        hd = C.c_void_p()
        _check(lib.yagi_hip_ordfilt_rrrf_create(n, k, C.byref(hd)))
        self._h = hd

    @classmethod
    def medfilt(cls, m):                                      # new_medfilt() :32-34
        new = object.__new__(cls)
        hd = C.c_void_p()
        _check(lib.yagi_hip_ordfilt_rrrf_create_medfilt(m, C.byref(hd)))
        new._h = hd
        return new

    def clone(self):                                          # derive(Clone)
        new = object.__new__(type(self))
        hd = C.c_void_p()
        _check(lib.yagi_hip_ordfilt_rrrf_clone(self._h, C.byref(hd)))
        new._h = hd
        return new

    def reset(self):                                          # :36-38
        _check(lib.yagi_hip_ordfilt_rrrf_reset(self._h))

    def set_kernel(self, choice):
        """0 auto, 1 the LDS form, 2 the register-resident form (2 <= n <= ORDFILT_REG_NMAX); the same bits either way"""
        _check(lib.yagi_hip_ordfilt_rrrf_set_kernel(self._h, choice))

    def _get(self, name):
        v = C.c_size_t()
        _check(self._fn(name)(self._h, C.byref(v)))
        return v.value

    @property
    def n(self):
        return self._get("get_n")

    @property
    def k(self):
        return self._get("get_k")

    def push(self, x):                                        # :40-42
        _check(lib.yagi_hip_ordfilt_rrrf_push(self._h, float(np.float32(x))))

    def write(self, x):                                       # :44-46
        x = _arr(x, np.float32)
        _check(lib.yagi_hip_ordfilt_rrrf_write(self._h, _ptr(x), x.size))

    def execute(self):                                        # :48-53
        y = C.c_float()
        _check(lib.yagi_hip_ordfilt_rrrf_execute(self._h, C.byref(y)))
        return np.float32(y.value)

    def execute_one(self, x):                                 # :55-58
        y = C.c_float()
        _check(lib.yagi_hip_ordfilt_rrrf_execute_one(self._h, float(np.float32(x)), C.byref(y)))
        return np.float32(y.value)

    def execute_block(self, x, y=None):                       # :60-65
        x = _arr(x, np.float32)
        y = _out(y, x.size, np.float32)
        _check(lib.yagi_hip_ordfilt_rrrf_execute_block(self._h, _ptr(x), x.size, _ptr(y)))
        return y

    def execute_block_devptr(self, x_dev, n, y_dev):
        """x_dev, y_dev: n float32 on the device, not overlapping (ConfigError); asynchronous on the object's stream"""
        _check(lib.yagi_hip_ordfilt_rrrf_execute_block_dev(self._h, _devptr(x_dev), n, _devptr(y_dev)))


AUTOCORR_WMAX = 1024     # YAGI_AUTOCORR_WMAX: the longest window of Autocorr
AUTOCORR_DMAX = 65536    # YAGI_AUTOCORR_DMAX: the longest delay of Autocorr
AUTOCORR_TILE = 2048     # YAGI_AUTOCORR_TILE: outputs per workgroup of autocorr_kernels.hip


class Autocorr(_Handle):
    """Autocorr<T>(window_size W, delay d), T = Complex<f32> ("cccf") or f32 ("rrrf"): after each sample n,
    rxx[n] = sum_i X[n-W+1+i] conj(X[n-W+1+i-d]) and energy[n] = sum_i |X[n-W+1+i]|^2 over i = 0 .. W-1, X = 0 before the
    stream starts.  The reference leaves the object empty (src/filter/autocorr.rs); it is defined here as its Window and
    dotprod composed (yagi_hip.h): sequential f32 sums from +0.0, products and adds unfused, and
    every output word equals that composition.  The per-sample calls run on the host; execute_block runs
    autocorr_kernels.hip.  W <= AUTOCORR_WMAX, d <= AUTOCORR_DMAX."""

    def __init__(self, kind, window_size, delay):
        if kind not in ("cccf", "rrrf"):
            raise ConfigError(f"unknown type combination {kind!r}")
        self.kind = kind
        self.T = KINDS[kind][0]
        self._prefix = f"yagi_hip_autocorr_{kind}_"
        hd = C.c_void_p()
        _check(self._fn("create")(window_size, delay, C.byref(hd)))
        self._h = hd

    def clone(self):
        new = object.__new__(type(self))
        new.kind, new.T, new._prefix = self.kind, self.T, self._prefix
        hd = C.c_void_p()
        _check(self._fn("clone")(self._h, C.byref(hd)))
        new._h = hd
        return new

    def _get(self, name):
        v = C.c_size_t()
        _check(self._fn(name)(self._h, C.byref(v)))
        return v.value

    @property
    def window_size(self):
        return self._get("get_window_size")

    @property
    def delay(self):
        return self._get("get_delay")

    def push(self, x):
        _check(self._fn("push")(self._h, _byval(x, cf32 if self.kind == "cccf" else C.c_float)))

    def write(self, x):
        x = _arr(x, self.T)
        _check(self._fn("write")(self._h, _ptr(x), x.size))

    def execute(self):
        """rxx of the window as it stands"""
        y = np.zeros(1, self.T)
        _check(self._fn("execute")(self._h, _ptr(y)))
        return y[0]

    def get_energy(self):
        """the energy of the last window_size samples"""
        e = C.c_float()
        _check(self._fn("get_energy")(self._h, C.byref(e)))
        return np.float32(e.value)

    def execute_block(self, x, rxx=None, energy=False):
        """pushes x and returns rxx after each sample, or (rxx, energy) where energy is True"""
        x = _arr(x, self.T)
        rxx = _out(rxx, x.size, self.T)
        e = np.empty(x.size, np.float32) if energy else None
        _check(self._fn("execute_block")(self._h, _ptr(x), x.size, _ptr(rxx), _ptr(e) if energy else None))
        return (rxx, e) if energy else rxx

    def execute_block_devptr(self, x_dev, n, rxx_dev, energy_dev=None):
        """x_dev, rxx_dev: n samples on the device; energy_dev: n float32 or None.  The buffers must not overlap
        (ConfigError); asynchronous on the object's stream"""
        _check(self._fn("execute_block_dev")(self._h, _devptr(x_dev), n, _devptr(rxx_dev),
                                             None if energy_dev is None else _devptr(energy_dev)))


BURSTDET_SEGMAX = 8192   # YAGI_BURSTDET_SEGMAX: segments a BurstDetector call may hold beyond one per tile
# yagi_burst_event: start, length and peak are absolute sample indices; ratio, energy and rxx are taken at the peak
BURST_EVENT = np.dtype([("start", np.uint64), ("length", np.uint64), ("peak", np.uint64), ("ratio", np.float32),
                        ("energy", np.float32), ("rxx_re", np.float32), ("rxx_im", np.float32)])


class BurstDetector(_Handle):
    """BurstDetector<T>(W, d, threshold, energy_floor=0, min_length=1), T = Complex<f32> ("cccf") or f32 ("rrrf"):
    Autocorr(W, d), the test hit[n] = energy[n] > energy_floor and |rxx[n]|^2 > threshold^2 energy[n]^2, and the runs
    of consecutive hits with their peaks (the largest |rxx|^2 / energy^2, the earliest on ties), all in f32 and rounded
    as yagi_hip.h and DESIGN.md section 6 say.  A block call reads the samples and returns only the events they close
    (BURST_EVENT records, ordered by start); a run that reaches the call's last sample stays pending for the next call
    or flush().  A call whose runs fall into more than tiles + BURSTDET_SEGMAX per-tile segments reports overflow and no
    events.  The block calls run burstdet_kernels.hip."""

    def __init__(self, kind, window_size, delay, threshold, energy_floor=0.0, min_length=1):
        if kind not in ("cccf", "rrrf"):
            raise ConfigError(f"unknown type combination {kind!r}")
        if not (isinstance(min_length, (int, np.integer)) and 0 <= min_length < 2 ** 64):
            raise ConfigError("min_length must be an integer of at least one")
        self.kind = kind
        self.T = KINDS[kind][0]
        self._prefix = f"yagi_hip_burstdet_{kind}_"
        hd = C.c_void_p()
        _check(self._fn("create")(window_size, delay, threshold, energy_floor, min_length, C.byref(hd)))
        self._h = hd

    def clone(self):
        new = object.__new__(type(self))
        new.kind, new.T, new._prefix = self.kind, self.T, self._prefix
        hd = C.c_void_p()
        _check(self._fn("clone")(self._h, C.byref(hd)))
        new._h = hd
        return new

    def _get(self, name, ctype):
        v = ctype()
        _check(self._fn(name)(self._h, C.byref(v)))
        return v.value

    window_size = property(lambda self: self._get("get_window_size", C.c_size_t))
    delay = property(lambda self: self._get("get_delay", C.c_size_t))
    threshold = property(lambda self: np.float32(self._get("get_threshold", C.c_float)))
    energy_floor = property(lambda self: np.float32(self._get("get_energy_floor", C.c_float)))
    min_length = property(lambda self: self._get("get_min_length", C.c_uint64))

    @property
    def position(self):
        """samples seen since reset(); synchronises"""
        return self._get("get_position", C.c_uint64)

    @property
    def pending(self):
        """the run that reaches the last sample seen, as a BURST_EVENT record so far, or None; synchronises"""
        has, ev = C.c_int(), np.zeros(1, BURST_EVENT)
        _check(self._fn("get_pending")(self._h, C.byref(has), _ptr(ev)))
        return ev[0] if has.value else None

    def detect_block(self, x, cap=None):
        """pushes x and returns (events, overflow): the BURST_EVENT records the block closes, at most cap of them where
        cap is given (events.size is then min(count, cap); the count is the third item of the tuple in that case)"""
        x = _arr(x, self.T)
        room = (x.size + AUTOCORR_TILE - 1) // AUTOCORR_TILE + BURSTDET_SEGMAX + 1 if cap is None else int(cap)
        ev = np.zeros(room, BURST_EVENT)
        count, over = C.c_size_t(), C.c_int()
        _check(self._fn("detect_block")(self._h, _ptr(x), x.size, _ptr(ev), room, C.byref(count), C.byref(over)))
        ev = ev[:min(count.value, room)].copy()
        return (ev, bool(over.value)) if cap is None else (ev, bool(over.value), count.value)

    def detect_block_devptr(self, x_dev, n, events_dev, cap, status_dev):
        """x_dev: n samples; events_dev: room for cap BURST_EVENT records (None where cap is 0); status_dev: two uint32
        that receive (count, overflow).  min(count, cap) records are written.  The buffers must not overlap
        (ConfigError); asynchronous on the object's stream, no host synchronisation"""
        x_dev, events_dev, status_dev = (None if p is None else _devptr(p) for p in (x_dev, events_dev, status_dev))
        _check(self._fn("detect_block_dev")(self._h, x_dev, n, events_dev, cap, status_dev))

    def flush(self):
        """closes the pending run: one event if it is long enough, else none; position is unchanged"""
        ev, count = np.zeros(1, BURST_EVENT), C.c_size_t()
        _check(self._fn("flush")(self._h, _ptr(ev), 1, C.byref(count)))
        return ev[:count.value].copy()


def burst_detect_host(kind, x, window_size, delay, threshold, energy_floor=0.0, min_length=1):
    """BurstDetector's definition on the host alone, no device needed: one call on a stream from reset().  Returns
    (events, overflow, pending), pending a BURST_EVENT record or None.  It is the library's own sequential form (the
    state machine over Autocorr's host arithmetic), slow and meant for checks."""
    if kind not in ("cccf", "rrrf"):
        raise ConfigError(f"unknown type combination {kind!r}")
    x = _arr(x, KINDS[kind][0])
    room = (x.size + AUTOCORR_TILE - 1) // AUTOCORR_TILE + BURSTDET_SEGMAX + 1
    ev, pend = np.zeros(room, BURST_EVENT), np.zeros(1, BURST_EVENT)
    count, over, has = C.c_size_t(), C.c_int(), C.c_int()
    _check(getattr(lib, f"yagi_hip_burstdet_{kind}_detect_host")(
        window_size, delay, threshold, energy_floor, min_length, _ptr(x), x.size, _ptr(ev), room, C.byref(count),
        C.byref(over), C.byref(has), _ptr(pend)))
    return ev[:min(count.value, room)].copy(), bool(over.value), (pend[0] if has.value else None)


PDET_LMAX = 1024         # YAGI_PDET_LMAX: the longest preamble of PreambleDetector
PDET_KMAX = 32           # YAGI_PDET_KMAX: the most carrier-offset hypotheses
PDET_TILE = 2048         # YAGI_PDET_TILE: outputs per workgroup of pdet_kernels.hip
PDET_SEGMAX = 8192       # YAGI_PDET_SEGMAX: segments a PreambleDetector call may hold beyond one per tile
# yagi_preamble_event: start, length and peak are absolute sample indices; ratio, energy, rxy and hypothesis are taken
# at the peak
PREAMBLE_EVENT = np.dtype([("start", np.uint64), ("length", np.uint64), ("peak", np.uint64), ("ratio", np.float32),
                           ("energy", np.float32), ("rxy_re", np.float32), ("rxy_im", np.float32),
                           ("hypothesis", np.uint32), ("pad", np.uint32)])


def _pdet_args(p, dphi, min_length, kind):
    if kind != "cccf":
        raise ConfigError(f"unknown type combination {kind!r}")
    if not (isinstance(min_length, (int, np.integer)) and 0 <= min_length < 2 ** 64):
        raise ConfigError("min_length must be an integer of at least one")
    p, dphi = _arr(p, np.complex64), _arr(dphi, np.float32)
    if p.ndim != 1 or dphi.ndim != 1:
        raise ConfigError("the preamble and the hypotheses are one-dimensional")
    return p, dphi


def preamble_templates(p, dphi):
    """PreambleDetector's templates, no device needed: row k is v_k[i] = conj(p[i]) e^{-j dphi_k i}, evaluated in f64 and
    rounded once per component (yagi_hip.h)"""
    p, dphi = _pdet_args(p, dphi, 1, "cccf")
    out = np.zeros((dphi.size, p.size), np.complex64)
    _check(lib.yagi_hip_pdet_templates(_ptr(p), p.size, _ptr(dphi), dphi.size, _ptr(out)))
    return out


class PreambleDetector(_Handle):
    """PreambleDetector(p, dphi, threshold, energy_floor=0, min_length=1), Complex<f32> only: the stream is correlated
    with the preamble p (L samples) under the K carrier-offset hypotheses dphi (radians per sample), rxy_k[n] =
    dotprod(last L samples, conj(p) e^{-j dphi_k i}); with m the largest |rxy_k[n]|^2 (the lowest k on ties), hit[n] =
    energy[n] > energy_floor and m > threshold^2 energy[n] ep, ep the preamble's energy, and the runs of consecutive
    hits with their peaks (the largest m / (energy ep), the earliest on ties), all in f32 and rounded as yagi_hip.h and
    DESIGN.md section 6 say.  A block call reads the samples and returns only the events they close (PREAMBLE_EVENT
    records, ordered by start); a run that reaches the call's last sample stays pending for the next call or flush().
    peak - (L - 1) is where the preamble starts, dphi[hypothesis] the coarse carrier offset, arg(rxy) the carrier phase.
    A call whose runs fall into more than tiles + PDET_SEGMAX per-tile segments reports overflow and no events.  The
    block calls run pdet_kernels.hip.  L <= PDET_LMAX, K <= PDET_KMAX."""
    _prefix = "yagi_hip_pdet_cccf_"

    def __init__(self, p, dphi, threshold, energy_floor=0.0, min_length=1, kind="cccf"):
        p, dphi = _pdet_args(p, dphi, min_length, kind)
        self.kind, self.T = kind, np.complex64
        hd = C.c_void_p()
        _check(self._fn("create")(_ptr(p), p.size, _ptr(dphi), dphi.size, threshold, energy_floor, min_length,
                                  C.byref(hd)))
        self._h = hd

    def clone(self):
        new = object.__new__(type(self))
        new.kind, new.T = self.kind, self.T
        hd = C.c_void_p()
        _check(self._fn("clone")(self._h, C.byref(hd)))
        new._h = hd
        return new

    def _get(self, name, ctype):
        v = ctype()
        _check(self._fn(name)(self._h, C.byref(v)))
        return v.value

    length = property(lambda self: self._get("get_length", C.c_size_t))
    hypotheses = property(lambda self: self._get("get_hypotheses", C.c_size_t))
    threshold = property(lambda self: np.float32(self._get("get_threshold", C.c_float)))
    energy_floor = property(lambda self: np.float32(self._get("get_energy_floor", C.c_float)))
    min_length = property(lambda self: self._get("get_min_length", C.c_uint64))
    preamble_energy = property(lambda self: np.float32(self._get("get_preamble_energy", C.c_float)))

    @property
    def dphi(self):
        out = np.zeros(self.hypotheses, np.float32)
        _check(self._fn("get_dphi")(self._h, _ptr(out)))
        return out

    def get_templates(self):
        """the K x L templates the object correlates with"""
        out = np.zeros((self.hypotheses, self.length), np.complex64)
        _check(self._fn("get_templates")(self._h, _ptr(out)))
        return out

    @property
    def position(self):
        """samples seen since reset(); synchronises"""
        return self._get("get_position", C.c_uint64)

    @property
    def pending(self):
        """the run that reaches the last sample seen, as a PREAMBLE_EVENT record so far, or None; synchronises"""
        has, ev = C.c_int(), np.zeros(1, PREAMBLE_EVENT)
        _check(self._fn("get_pending")(self._h, C.byref(has), _ptr(ev)))
        return ev[0] if has.value else None

    def detect_block(self, x, cap=None):
        """pushes x and returns (events, overflow): the PREAMBLE_EVENT records the block closes, at most cap of them
        where cap is given (events.size is then min(count, cap); the count is the third item of the tuple in that case)"""
        x = _arr(x, self.T)
        room = (x.size + PDET_TILE - 1) // PDET_TILE + PDET_SEGMAX + 1 if cap is None else int(cap)
        ev = np.zeros(room, PREAMBLE_EVENT)
        count, over = C.c_size_t(), C.c_int()
        _check(self._fn("detect_block")(self._h, _ptr(x), x.size, _ptr(ev), room, C.byref(count), C.byref(over)))
        ev = ev[:min(count.value, room)].copy()
        return (ev, bool(over.value)) if cap is None else (ev, bool(over.value), count.value)

    def detect_block_devptr(self, x_dev, n, events_dev, cap, status_dev):
        """x_dev: n samples; events_dev: room for cap PREAMBLE_EVENT records (None where cap is 0); status_dev: two
        uint32 that receive (count, overflow).  min(count, cap) records are written.  The buffers must not overlap
        (ConfigError); asynchronous on the object's stream, no host synchronisation"""
        x_dev, events_dev, status_dev = (None if p is None else _devptr(p) for p in (x_dev, events_dev, status_dev))
        _check(self._fn("detect_block_dev")(self._h, x_dev, n, events_dev, cap, status_dev))

    def correlate_block(self, x, rxy=None):
        """the bank's raw output: pushes x and returns (rxy, energy), rxy[k, i] = rxy_k and energy[i] after sample i.  The
        sample counter advances; a pending run is dropped"""
        x = _arr(x, self.T)
        k = self.hypotheses
        rxy = _out(rxy, k * x.size, self.T)
        e = np.empty(x.size, np.float32)
        _check(self._fn("correlate_block")(self._h, _ptr(x), x.size, _ptr(rxy), _ptr(e)))
        return rxy.reshape(k, x.size), e

    def correlate_block_devptr(self, x_dev, n, rxy_dev, energy_dev=None):
        """x_dev: n samples; rxy_dev: K n samples, row k at k n; energy_dev: n float32 or None.  The buffers must not
        overlap (ConfigError); asynchronous on the object's stream"""
        x_dev, rxy_dev, energy_dev = (None if p is None else _devptr(p) for p in (x_dev, rxy_dev, energy_dev))
        _check(self._fn("correlate_block_dev")(self._h, x_dev, n, rxy_dev, energy_dev))

    def flush(self):
        """closes the pending run: one event if it is long enough, else none; position is unchanged"""
        ev, count = np.zeros(1, PREAMBLE_EVENT), C.c_size_t()
        _check(self._fn("flush")(self._h, _ptr(ev), 1, C.byref(count)))
        return ev[:count.value].copy()


def preamble_detect_host(x, p, dphi, threshold, energy_floor=0.0, min_length=1, kind="cccf"):
    """PreambleDetector's definition on the host alone, no device needed: one call on a stream from reset().  Returns
    (events, overflow, pending), pending a PREAMBLE_EVENT record or None.  It is the library's own sequential form,
    slow and meant for checks."""
    p, dphi = _pdet_args(p, dphi, min_length, kind)
    x = _arr(x, np.complex64)
    room = (x.size + PDET_TILE - 1) // PDET_TILE + PDET_SEGMAX + 1
    ev, pend = np.zeros(room, PREAMBLE_EVENT), np.zeros(1, PREAMBLE_EVENT)
    count, over, has = C.c_size_t(), C.c_int(), C.c_int()
    _check(lib.yagi_hip_pdet_cccf_detect_host(
        _ptr(p), p.size, _ptr(dphi), dphi.size, threshold, energy_floor, min_length, _ptr(x), x.size, _ptr(ev), room,
        C.byref(count), C.byref(over), C.byref(has), _ptr(pend)))
    return ev[:min(count.value, room)].copy(), bool(over.value), (pend[0] if has.value else None)


SYMSYNC_NPFB_MAX = 128             # YAGI_SYMSYNC_NPFB_MAX: the most branches of SymSync's two banks
SYMSYNC_LS_MAX = 128               # YAGI_SYMSYNC_LS_MAX: the most taps per branch (h_len div npfb)
SYMSYNC_CHANNELS_MAX = 1 << 20     # YAGI_SYMSYNC_CHANNELS_MAX


def _symsync_size(v, what):
    if not (isinstance(v, (int, np.integer)) and 0 <= v < 2 ** 63):
        raise ConfigError(f"{what} must be a non-negative integer")
    return int(v)


class SymSync(_Handle):
    """SymSync(channels, k, npfb, h): `channels` independent filter::symsync::Symsync<Complex32> objects of one design
    (src/filter/symsync.rs), Complex<f32> only.  execute takes a block x[n, channels] (step, channel) and returns, per
    channel, the outputs the reference's execute would write for that channel's samples, bit for bit its sequential loop:
    a polyphase matched filter and derivative matched filter over one window, the timing error Re(conj(mf) dmf), the
    second-order loop filter and the fractional index tau that picks the branch of the next output (yagi_hip.h).  reset()
    clears the matched filter's window and not the derivative filter's, as the reference does.
    Capacity: a channel writes at most ycap outputs per call; a channel that would write more (or that a NaN reached)
    is stalled: it ignores all further input and reports ny = 0 until reset() or reset_channel(c).
    The block calls run symsync_kernels.hip, one lane per channel.  npfb <= SYMSYNC_NPFB_MAX, h.size div npfb <=
    SYMSYNC_LS_MAX, channels <= SYMSYNC_CHANNELS_MAX."""
    _prefix = "yagi_hip_symsync_crcf_"

    def __init__(self, channels, k, npfb, h, kind="crcf"):
        if kind != "crcf":
            raise ConfigError(f"unknown type combination {kind!r}")
        channels, k, npfb = (_symsync_size(v, w) for v, w in ((channels, "channels"), (k, "k"), (npfb, "npfb")))
        h = _arr(h, np.float32)
        if h.ndim != 1:
            raise ConfigError("the taps are one-dimensional")
        hd = C.c_void_p()
        _check(self._fn("create")(channels, k, npfb, _ptr(h), h.size, C.byref(hd)))
        self._set(hd, channels, k)

    def _set(self, hd, channels, k):
        self._h, self.kind, self.T, self.channels, self.k, self.k_out = hd, "crcf", np.complex64, channels, k, 1

    @classmethod
    def rnyquist(cls, channels, ftype, k, m, beta, npfb):
        """Symsync::new_rnyquist (:112-131)"""
        channels, k, m, npfb = (_symsync_size(v, "argument") for v in (channels, k, m, npfb))
        new, hd = object.__new__(cls), C.c_void_p()
        _check(new._fn("create_rnyquist")(channels, int(ftype), k, m, beta, npfb, C.byref(hd)))
        new._set(hd, channels, k)
        return new

    @classmethod
    def kaiser(cls, channels, k, m, beta, npfb):
        """Symsync::new_kaiser (:133-158)"""
        channels, k, m, npfb = (_symsync_size(v, "argument") for v in (channels, k, m, npfb))
        new, hd = object.__new__(cls), C.c_void_p()
        _check(new._fn("create_kaiser")(channels, k, m, beta, npfb, C.byref(hd)))
        new._set(hd, channels, k)
        return new

    @staticmethod
    def rnyquist_taps(ftype, k, m, beta, npfb):
        """the prototype rnyquist designs: 2 npfb k m + 1 taps, no device needed"""
        k, m, npfb = (_symsync_size(v, "argument") for v in (k, m, npfb))
        h = np.zeros(2 * npfb * k * m + 1, np.float32)
        _check(lib.yagi_hip_symsync_crcf_rnyquist_taps(int(ftype), k, m, beta, npfb, _ptr(h)))
        return h

    @staticmethod
    def kaiser_taps(k, m, beta, npfb):
        """the prototype kaiser designs: 2 npfb k m + 1 taps, no device needed"""
        k, m, npfb = (_symsync_size(v, "argument") for v in (k, m, npfb))
        h = np.zeros(2 * npfb * k * m + 1, np.float32)
        _check(lib.yagi_hip_symsync_crcf_kaiser_taps(k, m, beta, npfb, _ptr(h)))
        return h

    def clone(self):
        new, hd = object.__new__(type(self)), C.c_void_p()
        _check(self._fn("clone")(self._h, C.byref(hd)))
        new._set(hd, self.channels, self.k)
        new.k_out = self.k_out
        return new

    def reset_channel(self, c):
        _check(self._fn("reset_channel")(self._h, _symsync_size(c, "channel")))

    def lock(self):
        _check(self._fn("lock")(self._h))

    def unlock(self):
        _check(self._fn("unlock")(self._h))

    def is_locked(self):
        v = C.c_int()
        _check(self._fn("is_locked")(self._h, C.byref(v)))
        return bool(v.value)

    def set_output_rate(self, k_out):
        """sets rate and del at once, for every channel"""
        _check(self._fn("set_output_rate")(self._h, _symsync_size(k_out, "k_out")))
        self.k_out = int(k_out)

    def set_lf_bw(self, bw):
        _check(self._fn("set_lf_bw")(self._h, bw))

    @property
    def branch_length(self):
        v = C.c_size_t()
        _check(self._fn("get_branch_length")(self._h, C.byref(v)))
        return v.value

    def get_tau(self):
        """tau_decim of every channel; synchronises"""
        out = np.zeros(self.channels, np.float32)
        _check(self._fn("get_tau")(self._h, _ptr(out)))
        return out

    def get_stalled(self):
        """the stalled word of every channel; synchronises"""
        out = np.zeros(self.channels, np.uint32)
        _check(self._fn("get_stalled")(self._h, _ptr(out)))
        return out

    def default_ycap(self, n):
        """2 ceil(n k_out / k) + 8: a default, not a bound (a loop far from lock can write more)"""
        return 2 * -(-int(n) * self.k_out // self.k) + 8

    def execute(self, x, ycap=None):
        """x[n, channels] -> (y[ycap, channels], ny[channels], stalled[channels]); y[j, c] is an output for j < ny[c]
        and zero below.  ycap defaults to default_ycap(n)"""
        x = _arr(x, self.T)
        if x.ndim != 2 or x.shape[1] != self.channels:
            raise ConfigError(f"the block is [steps, {self.channels}]")
        n = x.shape[0]
        ycap = self.default_ycap(n) if ycap is None else _symsync_size(ycap, "ycap")
        y = np.zeros((ycap, self.channels), self.T)
        ny, st = np.zeros(self.channels, np.uint32), np.zeros(self.channels, np.uint32)
        _check(self._fn("execute")(self._h, _ptr(x), self.channels, n, _ptr(y), self.channels, ycap, _ptr(ny), _ptr(st)))
        return y, ny, st

    def execute_devptr(self, x_dev, x_pitch, n, y_dev, y_pitch, ycap, status_dev):
        """x_dev: n rows of pitch x_pitch samples; y_dev: ycap rows of pitch y_pitch; status_dev: 2 channels uint32 that
        receive ny, then stalled.  Rows >= ny[c] of a channel are not touched.  Asynchronous on the object's stream (the
        C ABI's execute_dev; named as Ddc.execute_block_devptr is)"""
        x_dev, y_dev, status_dev = (None if p is None else _devptr(p) for p in (x_dev, y_dev, status_dev))
        _check(self._fn("execute_dev")(self._h, x_dev, x_pitch, n, y_dev, y_pitch, ycap, status_dev))

    @staticmethod
    def execute_host(channels, k, npfb, h, x, ycap=None, k_out=1, bw=0.01, locked=False, x_pitch=None, y_pitch=None):
        """the definition on the host alone, no device needed: one call from reset().  x is [n, x_pitch] (x_pitch
        defaults to channels); returns (y[ycap, y_pitch], ny, stalled, tau).  The library's own sequential form, slow and
        meant for checks"""
        channels, k, npfb, k_out = (_symsync_size(v, "argument") for v in (channels, k, npfb, k_out))
        if not 1 <= channels <= SYMSYNC_CHANNELS_MAX:
            raise ConfigError("channels must be in 1 .. SYMSYNC_CHANNELS_MAX")
        h = _arr(h, np.float32)
        x_pitch = channels if x_pitch is None else _symsync_size(x_pitch, "x_pitch")
        y_pitch = channels if y_pitch is None else _symsync_size(y_pitch, "y_pitch")
        x = _arr(x, np.complex64)
        if h.ndim != 1 or x.ndim != 2 or x.shape[1] != x_pitch:
            raise ConfigError("the taps are one-dimensional and the block is [steps, x_pitch]")
        n = x.shape[0]
        ycap = 2 * -(-n * k_out // max(k, 1)) + 8 if ycap is None else _symsync_size(ycap, "ycap")
        y = np.zeros((ycap, y_pitch), np.complex64)
        ny, st, tau = np.zeros(channels, np.uint32), np.zeros(channels, np.uint32), np.zeros(channels, np.float32)
        _check(lib.yagi_hip_symsync_crcf_execute_host(channels, k, npfb, _ptr(h), h.size, k_out, bw, int(bool(locked)),
                                                      _ptr(x), x_pitch, n, _ptr(y), y_pitch, ycap, _ptr(ny), _ptr(st),
                                                      _ptr(tau)))
        return y, ny, st, tau


EQLMS_LEN_MAX = 128                # YAGI_EQLMS_LEN_MAX: the most taps of EqLms
EQLMS_CHANNELS_MAX = 1 << 20       # YAGI_EQLMS_CHANNELS_MAX
EQLMS_TABLE_MAX = 256              # YAGI_EQLMS_TABLE_MAX: the most points of DECISION's constellation


class EqLmsUpdate(enum.IntEnum):
    """what EqLms.decim_block does after each symbol, numbered as YAGI_EQLMS_*"""
    NONE = 0        # a fixed decimating filter
    TRAIN = 1       # step(d, y) against known symbols
    BLIND = 2       # step_blind(y): constant modulus
    DECISION = 3    # step(table[j], y) against the nearest point of set_constellation's table
_EQLMS_EXECUTE = 4  # YAGI_EQLMS_EXECUTE: execute_host's word for execute_block


class EqLms(_Handle):
    """EqLms(channels, h_len, h=None): `channels` independent equalization::eqlms::Eqlms<Complex32> objects of one design
    (src/equalization/eqlms.rs), Complex<f32> only.  A block is x[n, channels] (step, channel); per channel every output
    word and every weight is the reference's sequential loop bit for bit: y = sum conj(w0[i]) r[i] over the window oldest
    first, x2_sum a running f32 sum, and w0[i] += ((mu conj(d - y)) r[i]) / x2_sum once count >= h_len (yagi_hip.h).
    Two stated deviations: |z| of the blind update is (float)sqrt((double)re^2 + (double)im^2), not the platform's
    hypotf, and DECISION picks the first table entry at the least unfused squared distance (Modem's Arb rule), not the
    reference's get_demodulator_sample.
    The block calls run eqlms_kernels.hip, one lane per channel.  h_len <= EQLMS_LEN_MAX, channels <= EQLMS_CHANNELS_MAX."""
    _prefix = "yagi_hip_eqlms_cccf_"

    def __init__(self, channels, h_len, h=None, kind="cccf"):
        """Eqlms::new (:25-49): h0[i] = conj(h[h_len - 1 - i]); h = None: h0[h_len // 2] = 1"""
        if kind != "cccf":
            raise ConfigError(f"unknown type combination {kind!r}")
        channels, h_len = _symsync_size(channels, "channels"), _symsync_size(h_len, "h_len")
        if h is not None:
            h = _arr(h, np.complex64)
            if h.ndim != 1 or h.size != h_len:
                raise ConfigError("the taps are one-dimensional, h_len of them")
        hd = C.c_void_p()
        _check(self._fn("create")(channels, None if h is None else _ptr(h), h_len, C.byref(hd)))
        self._set(hd, channels)

    def _set(self, hd, channels):
        self._h, self.kind, self.T, self.channels = hd, "cccf", np.complex64, channels
        v = C.c_size_t()
        _check(self._fn("get_length")(self._h, C.byref(v)))
        self.h_len = v.value

    @classmethod
    def rnyquist(cls, channels, ftype, k, m, beta, dt):
        """Eqlms::new_rnyquist (:51-76)"""
        channels, k, m = (_symsync_size(v, "argument") for v in (channels, k, m))
        new, hd = object.__new__(cls), C.c_void_p()
        _check(new._fn("create_rnyquist")(channels, int(ftype), k, m, beta, dt, C.byref(hd)))
        new._set(hd, channels)
        return new

    @classmethod
    def lowpass(cls, channels, h_len, fc):
        """Eqlms::new_lowpass (:78-90)"""
        channels, h_len = (_symsync_size(v, "argument") for v in (channels, h_len))
        new, hd = object.__new__(cls), C.c_void_p()
        _check(new._fn("create_lowpass")(channels, h_len, fc, C.byref(hd)))
        new._set(hd, channels)
        return new

    def clone(self):
        new, hd = object.__new__(type(self)), C.c_void_p()
        _check(self._fn("clone")(self._h, C.byref(hd)))
        new._set(hd, self.channels)
        return new

    def reset_channel(self, c):
        _check(self._fn("reset_channel")(self._h, _symsync_size(c, "channel")))

    def set_bw(self, mu):
        """the step size mu >= 0, one value for the bank"""
        _check(self._fn("set_bw")(self._h, mu))

    def get_bw(self):
        v = C.c_float()
        _check(self._fn("get_bw")(self._h, C.byref(v)))
        return v.value

    def get_length(self):
        return self.h_len

    def get_coefficients(self):
        """w0[channels, h_len]; synchronises"""
        out = np.zeros((self.channels, self.h_len), self.T)
        _check(self._fn("get_coefficients")(self._h, _ptr(out)))
        return out

    def get_weights(self):
        """w0 reversed and conjugated, [channels, h_len] (:121-123); synchronises"""
        out = np.zeros((self.channels, self.h_len), self.T)
        _check(self._fn("get_weights")(self._h, _ptr(out)))
        return out

    def set_constellation(self, table):
        """DECISION's table, 1 .. EQLMS_TABLE_MAX points"""
        table = _arr(table, self.T)
        if table.ndim != 1:
            raise ConfigError("the constellation is one-dimensional")
        _check(self._fn("set_constellation")(self._h, _ptr(table), table.size))

    def _block(self, x):
        x = _arr(x, self.T)
        if x.ndim != 2 or x.shape[1] != self.channels:
            raise ConfigError(f"the block is [steps, {self.channels}]")
        return x

    def execute_block(self, k, x):
        """Eqlms::execute_block (:153-168): x[n, channels] -> y[n, channels], a blind update where (count + k - 1) % k == 0"""
        x = self._block(x)
        y = np.zeros_like(x)
        _check(self._fn("execute_block")(self._h, _symsync_size(k, "k"), _ptr(x), self.channels, x.shape[0], _ptr(y),
                                         self.channels))
        return y

    def decim_block(self, k, mode, x, d=None):
        """x[n k, channels] -> y[n, channels]: per symbol decim_execute (:142-151), then one update of `mode`
        (EqLmsUpdate); d[n, channels] are TRAIN's known symbols"""
        x, k = self._block(x), _symsync_size(k, "k")
        if d is not None:
            d = self._block(d)
            if k and d.shape[0] * k != x.shape[0]:
                raise ConfigError("d holds one row per symbol")
        y = np.zeros((x.shape[0] // max(k, 1), self.channels), self.T)
        _check(self._fn("decim_block")(self._h, k, int(mode), _ptr(x), self.channels, x.shape[0],
                                       None if d is None else _ptr(d), self.channels, _ptr(y), self.channels))
        return y

    def execute_block_devptr(self, k, x_dev, x_pitch, n, y_dev, y_pitch):
        """x_dev: n rows of pitch x_pitch samples; y_dev: n rows of pitch y_pitch.  Asynchronous on the object's stream
        (the C ABI's execute_block_dev; named as Ddc.execute_block_devptr is)"""
        x_dev, y_dev = (None if p is None else _devptr(p) for p in (x_dev, y_dev))
        _check(self._fn("execute_block_dev")(self._h, k, x_dev, x_pitch, n, y_dev, y_pitch))

    def decim_block_devptr(self, k, mode, x_dev, x_pitch, n, d_dev, d_pitch, y_dev, y_pitch):
        """x_dev: n rows (a multiple of k); d_dev: n / k rows of known symbols, None unless TRAIN; y_dev: n / k rows.
        Asynchronous on the object's stream (the C ABI's decim_block_dev)"""
        x_dev, d_dev, y_dev = (None if p is None else _devptr(p) for p in (x_dev, d_dev, y_dev))
        _check(self._fn("decim_block_dev")(self._h, k, int(mode), x_dev, x_pitch, n, d_dev, d_pitch, y_dev, y_pitch))

    @staticmethod
    def execute_host(channels, h_len, h, mu, k, x, mode=None, d=None, table=None, x_pitch=None, d_pitch=None, y_pitch=None):
        """the definition on the host alone, no device needed: one call from reset().  mode = None runs execute_block,
        an EqLmsUpdate runs decim_block.  x is [n, x_pitch] (the pitches default to channels); returns (y[rows, y_pitch],
        w0[channels, h_len]).  The library's own sequential form, slow and meant for checks"""
        channels, h_len, k = (_symsync_size(v, "argument") for v in (channels, h_len, k))
        if not 1 <= channels <= EQLMS_CHANNELS_MAX:
            raise ConfigError("channels must be in 1 .. EQLMS_CHANNELS_MAX")
        x_pitch, d_pitch, y_pitch = (channels if p is None else _symsync_size(p, "pitch") for p in (x_pitch, d_pitch, y_pitch))
        x = _arr(x, np.complex64)
        if x.ndim != 2 or x.shape[1] != x_pitch:
            raise ConfigError("the block is [steps, x_pitch]")
        if h is not None:
            h = _arr(h, np.complex64)
            if h.ndim != 1 or h.size != h_len:
                raise ConfigError("the taps are one-dimensional, h_len of them")
        if d is not None:
            d = _arr(d, np.complex64)
            if d.ndim != 2 or d.shape[1] != d_pitch or d.shape[0] * max(k, 1) != x.shape[0]:
                raise ConfigError("d is [symbols, d_pitch]")
        if table is not None:
            table = _arr(table, np.complex64).reshape(-1)
        call = _EQLMS_EXECUTE if mode is None else int(mode)
        n = x.shape[0]
        rows = n if mode is None else n // max(k, 1)
        y = np.zeros((rows, y_pitch), np.complex64)
        w0 = np.zeros((channels, min(h_len, EQLMS_LEN_MAX)), np.complex64)
        _check(lib.yagi_hip_eqlms_cccf_execute_host(
            channels, None if h is None else _ptr(h), h_len, mu, call, k, _ptr(x), x_pitch, n,
            None if d is None else _ptr(d), d_pitch, None if table is None else _ptr(table),
            0 if table is None else table.size, _ptr(y), y_pitch, _ptr(w0)))
        return y, w0


EQRLS_LEN_MAX = 32                 # YAGI_EQRLS_LEN_MAX: the largest order p of EqRls
EQRLS_CHANNELS_MAX = 1 << 20       # YAGI_EQRLS_CHANNELS_MAX
EQRLS_MATRIX_MAX = 1 << 26         # YAGI_EQRLS_MATRIX_MAX: channels p p, 512 MiB of P


class EqRlsUpdate(enum.IntEnum):
    """what EqRls.step_block does after each symbol's output, numbered as YAGI_EQRLS_* (and so as EqLmsUpdate)"""
    NONE = 0        # a fixed filter
    TRAIN = 1       # step(d, y) against known symbols
    DECISION = 3    # step(table[j], y) against the nearest point of set_constellation's table


def eqrls_plan(channels, p):
    """the launch shape of EqRls(channels, p): (L, lds_bytes, admissible).  L lanes share one channel's step, a wave
    holds 64 // L channels in lds_bytes of LDS; admissible lists every L that set_lanes accepts.  No device needed"""
    channels, p = _symsync_size(channels, "channels"), _symsync_size(p, "p")
    L, lds, mask = C.c_size_t(), C.c_size_t(), C.c_uint()
    _check(lib.yagi_hip_eqrls_plan(channels, p, C.byref(L), C.byref(lds), C.byref(mask)))
    return L.value, lds.value, [1 << b for b in range(7) if mask.value >> b & 1]


class EqRls(_Handle):
    """EqRls(channels, p, h=None): `channels` independent equalization::eqrls::Eqrls<Complex32> objects of one design
    (src/equalization/eqrls.rs), Complex<f32> only.  A block is x[n, channels] (step, channel); per channel every output
    word and every word of w0, w1 and P0 is the reference's sequential loop bit for bit: y = sum w0[i] r[i] over the window
    oldest first (no conjugate), and the O(p^3) update of step (:112-146) with every product, sum and complex quotient
    rounded on its own (yagi_hip.h).  lambda = 0.99 and delta = 0.1 after create.
    get_weights is w1 reversed, not w0, as in the reference: zero before the first update and kept across reset().
    The block calls run eqrls_kernels.hip, L lanes per channel (eqrls_plan, set_lanes); the words do not depend on L.
    p <= EQRLS_LEN_MAX, channels <= EQRLS_CHANNELS_MAX, channels p p <= EQRLS_MATRIX_MAX."""
    _prefix = "yagi_hip_eqrls_cccf_"

    def __init__(self, channels, p, h=None, kind="cccf"):
        """Eqrls::new (:31-62): h0 = h as given; h = None: h0[p - 1] = 1"""
        if kind != "cccf":
            raise ConfigError(f"unknown type combination {kind!r}")
        channels, p = _symsync_size(channels, "channels"), _symsync_size(p, "p")
        h = self._taps(h, p)
        hd = C.c_void_p()
        _check(self._fn("create")(channels, None if h is None else _ptr(h), p, C.byref(hd)))
        self._set(hd, channels)

    @staticmethod
    def _taps(h, p):
        if h is not None:
            h = _arr(h, np.complex64)
            if h.ndim != 1 or h.size != p:
                raise ConfigError("the taps are one-dimensional, p of them")
        return h

    def _set(self, hd, channels):
        self._h, self.kind, self.T, self.channels = hd, "cccf", np.complex64, channels
        v = C.c_size_t()
        _check(self._fn("get_length")(self._h, C.byref(v)))
        self.p = v.value

    def recreate(self, p, h=None):
        """Eqrls::recreate (:64-74): the same p only replaces h0 (where h is given) and resets nothing; another p is a new
        bank of the same channel count"""
        p = _symsync_size(p, "p")
        h = self._taps(h, p)
        _check(self._fn("recreate")(self._h, None if h is None else _ptr(h), p))
        self._set(self._h, self.channels)

    def clone(self):
        new, hd = object.__new__(type(self)), C.c_void_p()
        _check(self._fn("clone")(self._h, C.byref(hd)))
        new._set(hd, self.channels)
        return new

    def reset_channel(self, c):
        _check(self._fn("reset_channel")(self._h, _symsync_size(c, "channel")))

    def set_bw(self, lam):
        """the forgetting factor lambda in [0, 1], one value for the bank"""
        _check(self._fn("set_bw")(self._h, lam))

    def get_bw(self):
        v = C.c_float()
        _check(self._fn("get_bw")(self._h, C.byref(v)))
        return v.value

    def get_length(self):
        return self.p

    def set_lanes(self, L):
        """L lanes per channel instead of the planner's choice (0 gives the choice back); L must be admissible for p"""
        _check(self._fn("set_lanes")(self._h, _symsync_size(L, "L")))

    def get_lanes(self):
        v = C.c_size_t()
        _check(self._fn("get_lanes")(self._h, C.byref(v)))
        return v.value

    def get_coefficients(self):
        """w0[channels, p]; synchronises"""
        out = np.zeros((self.channels, self.p), self.T)
        _check(self._fn("get_coefficients")(self._h, _ptr(out)))
        return out

    def get_weights(self):
        """w1 reversed, [channels, p] (:148-156); synchronises"""
        out = np.zeros((self.channels, self.p), self.T)
        _check(self._fn("get_weights")(self._h, _ptr(out)))
        return out

    def get_matrix(self):
        """P0[channels, p, p]; synchronises"""
        out = np.zeros((self.channels, self.p, self.p), self.T)
        _check(self._fn("get_matrix")(self._h, _ptr(out)))
        return out

    def set_constellation(self, table):
        """DECISION's table, 1 .. EQLMS_TABLE_MAX points"""
        table = _arr(table, self.T)
        if table.ndim != 1:
            raise ConfigError("the constellation is one-dimensional")
        _check(self._fn("set_constellation")(self._h, _ptr(table), table.size))

    def _block(self, x):
        x = _arr(x, self.T)
        if x.ndim != 2 or x.shape[1] != self.channels:
            raise ConfigError(f"the block is [steps, {self.channels}]")
        return x

    def step_block(self, k, mode, x, d=None):
        """x[n k, channels] -> y[n, channels]: per symbol push x[i k], y[i] = execute(), one update of `mode` (EqRlsUpdate),
        then the other k - 1 pushes; d[n, channels] are TRAIN's known symbols"""
        x, k = self._block(x), _symsync_size(k, "k")
        if d is not None:
            d = self._block(d)
            if k and d.shape[0] * k != x.shape[0]:
                raise ConfigError("d holds one row per symbol")
        y = np.zeros((x.shape[0] // max(k, 1), self.channels), self.T)
        _check(self._fn("step_block")(self._h, k, int(mode), _ptr(x), self.channels, x.shape[0],
                                      None if d is None else _ptr(d), self.channels, _ptr(y), self.channels))
        return y

    def train(self, w, x, d):
        """Eqrls::train (:158-176): reset(), w0[i] = w[c, p - 1 - i], one TRAIN step per row of x[n, channels] against
        d[n, channels]; returns get_weights()"""
        w, x, d = _arr(w, self.T).copy(), self._block(x), self._block(d)
        if w.shape != (self.channels, self.p):
            raise ConfigError("w is [channels, p]")
        if d.shape != x.shape:
            raise ConfigError("d holds one row per row of x")
        _check(self._fn("train")(self._h, _ptr(w), _ptr(x), self.channels, x.shape[0], _ptr(d), self.channels))
        return w

    def step_block_devptr(self, k, mode, x_dev, x_pitch, n, d_dev, d_pitch, y_dev, y_pitch):
        """x_dev: n rows (a multiple of k); d_dev: n / k rows of known symbols, None unless TRAIN; y_dev: n / k rows.
        Asynchronous on the object's stream (the C ABI's step_block_dev)"""
        x_dev, d_dev, y_dev = (None if p is None else _devptr(p) for p in (x_dev, d_dev, y_dev))
        _check(self._fn("step_block_dev")(self._h, k, int(mode), x_dev, x_pitch, n, d_dev, d_pitch, y_dev, y_pitch))

    def train_devptr(self, w, x_dev, x_pitch, n, d_dev, d_pitch):
        """train on device pointers (the C ABI's train_dev): w[channels, p] is a host array read before the launch; the
        call is asynchronous on the object's stream and get_weights() returns the result"""
        w = _arr(w, self.T)
        if w.shape != (self.channels, self.p):
            raise ConfigError("w is [channels, p]")
        x_dev, d_dev = (None if p is None else _devptr(p) for p in (x_dev, d_dev))
        _check(self._fn("train_dev")(self._h, _ptr(w), x_dev, x_pitch, n, d_dev, d_pitch))

    @staticmethod
    def execute_host(channels, p, h, lam, k, x, mode=EqRlsUpdate.NONE, d=None, table=None, x_pitch=None, d_pitch=None,
                     y_pitch=None):
        """the definition on the host alone, no device needed: one step_block call from reset().  x is [n, x_pitch] (the
        pitches default to channels); returns (y[rows, y_pitch], w0[channels, p], w1[channels, p], P0[channels, p, p]).
        The library's own sequential form, slow and meant for checks"""
        channels, p, k = (_symsync_size(v, "argument") for v in (channels, p, k))
        if not 1 <= channels <= EQRLS_CHANNELS_MAX:
            raise ConfigError("channels must be in 1 .. EQRLS_CHANNELS_MAX")
        x_pitch, d_pitch, y_pitch = (channels if v is None else _symsync_size(v, "pitch") for v in (x_pitch, d_pitch, y_pitch))
        x = _arr(x, np.complex64)
        if x.ndim != 2 or x.shape[1] != x_pitch:
            raise ConfigError("the block is [steps, x_pitch]")
        h = EqRls._taps(h, p)
        if d is not None:
            d = _arr(d, np.complex64)
            if d.ndim != 2 or d.shape[1] != d_pitch or d.shape[0] * max(k, 1) != x.shape[0]:
                raise ConfigError("d is [symbols, d_pitch]")
        if table is not None:
            table = _arr(table, np.complex64).reshape(-1)
        n = x.shape[0]
        y = np.zeros((n // max(k, 1), y_pitch), np.complex64)
        pc = min(p, EQRLS_LEN_MAX)
        w0, w1 = np.zeros((channels, pc), np.complex64), np.zeros((channels, pc), np.complex64)
        P0 = np.zeros((channels, pc, pc) if channels * pc * pc <= EQRLS_MATRIX_MAX else (0, pc, pc), np.complex64)
        _check(lib.yagi_hip_eqrls_cccf_execute_host(
            channels, None if h is None else _ptr(h), p, lam, int(mode), k, _ptr(x), x_pitch, n,
            None if d is None else _ptr(d), d_pitch, None if table is None else _ptr(table),
            0 if table is None else table.size, _ptr(y), y_pitch, _ptr(w0), _ptr(w1), _ptr(P0)))
        return y, w0, w1, P0


AGC_CHANNELS_MAX = 1 << 20        # YAGI_AGC_CHANNELS_MAX


class AgcSquelchMode(enum.IntEnum):
    """agc::AgcSquelchMode (src/agc/agc.rs:22-31), numbered as YAGI_AGC_SQUELCH_*"""
    DISABLED = 0
    ENABLED = 1
    RISE = 2
    SIGNALHI = 3
    FALL = 4
    SIGNALLO = 5
    TIMEOUT = 6


def _word(name, x):
    x = _arr(x, np.float32)
    y = np.empty_like(x)
    _check(getattr(lib, "yagi_hip_" + name)(_ptr(x), x.size, _ptr(y)))
    return y


def lnf(x):
    """the library's ln in f32 (yagi_hip.h, the Agc block), elementwise on the host"""
    return _word("lnf", x)


def expf(x):
    """the library's exp in f32, elementwise on the host"""
    return _word("expf", x)


def log10f(x):
    """the library's log10 in f32, elementwise on the host"""
    return _word("log10f", x)


class Agc(_Handle):
    """Agc(channels, kind="crcf"): `channels` independent agc::Agc<T> objects of one set of settings (src/agc/agc.rs), T =
    Complex<f32> ("crcf") or f32 ("rrrf").  A block is x[n, channels] (step, channel); per channel every output word, gain
    and squelch mode is the reference's sequential loop bit for bit, with the library's own ln, exp and log10 (lnf, expf,
    log10f) where the reference calls the platform's (yagi_hip.h).  A locked channel's output is not scaled, as in the
    reference.  The block calls run agc_kernels.hip, one lane per channel.  channels <= AGC_CHANNELS_MAX."""

    def __init__(self, channels, kind="crcf"):
        if kind not in ("crcf", "rrrf"):
            raise ConfigError(f"unknown type combination {kind!r}")
        channels = _symsync_size(channels, "channels")
        self._prefix = f"yagi_hip_agc_{kind}_"
        hd = C.c_void_p()
        _check(self._fn("create")(channels, C.byref(hd)))
        self._set(hd, kind, channels)

    def _set(self, hd, kind, channels):
        self._prefix = f"yagi_hip_agc_{kind}_"
        self._h, self.kind, self.T, self.channels = hd, kind, KINDS[kind][0], channels

    def clone(self):
        new, hd = object.__new__(type(self)), C.c_void_p()
        _check(self._fn("clone")(self._h, C.byref(hd)))
        new._set(hd, self.kind, self.channels)
        return new

    def reset_channel(self, c):
        _check(self._fn("reset_channel")(self._h, _symsync_size(c, "channel")))

    def _call(self, name, *args):
        _check(self._fn(name)(self._h, *args))

    def _get(self, name, ctype):
        v = ctype()
        _check(self._fn(name)(self._h, C.byref(v)))
        return v.value

    def _per_channel(self, name, dt):
        out = np.zeros(self.channels, dt)
        _check(self._fn(name)(self._h, _ptr(out)))
        return out

    def _vector(self, v, dt, what):
        v = _arr(v, dt)
        if v.shape != (self.channels,):
            raise ConfigError(f"{what} holds one value per channel")
        return v

    def lock(self):
        self._call("lock")

    def unlock(self):
        self._call("unlock")

    def is_locked(self):
        """True where every channel is locked"""
        return bool(self._get("is_locked", C.c_int))

    def set_locked(self, locked):
        """locked[channels], nonzero = locked"""
        self._call("set_locked", _ptr(self._vector(np.asarray(locked) != 0, np.uint8, "locked")))

    def get_locked(self):
        return self._per_channel("get_locked", np.uint8)

    def set_bandwidth(self, bt):
        self._call("set_bandwidth", bt)

    def get_bandwidth(self):
        return self._get("get_bandwidth", C.c_float)

    def set_scale(self, scale):
        self._call("set_scale", scale)

    def get_scale(self):
        return self._get("get_scale", C.c_float)

    def set_gain(self, gain):
        self._call("set_gain", gain)

    def set_gains(self, gain):
        self._call("set_gains", _ptr(self._vector(gain, np.float32, "gain")))

    def set_signal_level(self, x2):
        self._call("set_signal_level", x2)

    def set_rssi(self, rssi):
        self._call("set_rssi", rssi)

    def get_gain(self):
        """g[channels]; synchronises"""
        return self._per_channel("get_gain", np.float32)

    def get_signal_level(self):
        return self._per_channel("get_signal_level", np.float32)

    def get_rssi(self):
        return self._per_channel("get_rssi", np.float32)

    def squelch_enable(self):
        self._call("squelch_enable")

    def squelch_disable(self):
        self._call("squelch_disable")

    def squelch_is_enabled(self):
        return bool(self._get("squelch_is_enabled", C.c_int))

    def squelch_set_threshold(self, threshold):
        self._call("squelch_set_threshold", threshold)

    def squelch_get_threshold(self):
        return self._get("squelch_get_threshold", C.c_float)

    def squelch_set_timeout(self, timeout):
        self._call("squelch_set_timeout", _symsync_size(timeout, "timeout"))

    def squelch_get_timeout(self):
        return self._get("squelch_get_timeout", C.c_uint64)

    def squelch_get_status(self):
        """AgcSquelchMode numbers, [channels]; synchronises"""
        return self._per_channel("squelch_get_status", np.uint8)

    def _block(self, x):
        x = _arr(x, self.T)
        if x.ndim != 2 or x.shape[1] != self.channels:
            raise ConfigError(f"the block is [steps, {self.channels}]")
        return x

    def init(self, x):
        """Agc::init (:171-178) per channel on x[n, channels]"""
        x = self._block(x)
        self._call("init", _ptr(x), self.channels, x.shape[0])

    def init_devptr(self, x_dev, x_pitch, n):
        self._call("init_dev", None if x_dev is None else _devptr(x_dev), x_pitch, n)

    def execute_block(self, x, status=False):
        """x[n, channels] -> y[n, channels], or (y, mode[n, channels]) with status: the squelch mode after each sample"""
        x = self._block(x)
        y = np.zeros_like(x)
        st = np.zeros(x.shape, np.uint8) if status else None
        self._call("execute_block", _ptr(x), self.channels, x.shape[0], _ptr(y), self.channels,
                   None if st is None else _ptr(st), self.channels)
        return (y, st) if status else y

    def execute_block_devptr(self, x_dev, x_pitch, n, y_dev, y_pitch, status_dev=None, status_pitch=0):
        """x_dev, y_dev: n rows of pitch x_pitch, y_pitch elements (y_dev may be x_dev at the same pitch); status_dev: n
        rows of status_pitch bytes or None.  Asynchronous on the object's stream (the C ABI's execute_block_dev)"""
        x_dev, y_dev, status_dev = (None if p is None else _devptr(p) for p in (x_dev, y_dev, status_dev))
        self._call("execute_block_dev", x_dev, x_pitch, n, y_dev, y_pitch, status_dev, status_pitch)

    @staticmethod
    def execute_host(channels, bandwidth, scale, g0, locked, squelch, threshold, timeout, x, kind="crcf", status=False,
                     x_pitch=None, y_pitch=None, status_pitch=None, y=None):
        """the definition on the host alone, no device needed: one call from reset() followed by set_gain(g0).  x is
        [n, x_pitch] (the pitches default to channels); y, where given, is the [n, y_pitch] array that is written
        (y = x runs in place).  Returns (y, mode[n, status_pitch] or None, g[channels], mode[channels]).  The
        library's own sequential form, slow and meant for checks"""
        if kind not in ("crcf", "rrrf"):
            raise ConfigError(f"unknown type combination {kind!r}")
        T = KINDS[kind][0]
        channels, timeout = _symsync_size(channels, "channels"), _symsync_size(timeout, "timeout")
        if not 1 <= channels <= AGC_CHANNELS_MAX:
            raise ConfigError("channels must be in 1 .. AGC_CHANNELS_MAX")
        x_pitch, y_pitch, status_pitch = (channels if p is None else _symsync_size(p, "pitch")
                                          for p in (x_pitch, y_pitch, status_pitch))
        if not (isinstance(x, np.ndarray) and x.dtype == np.dtype(T) and x.flags.c_contiguous):
            x = _arr(x, T)
        if x.ndim != 2 or x.shape[1] != x_pitch:
            raise ConfigError("the block is [steps, x_pitch]")
        n = x.shape[0]
        if y is None:
            y = np.zeros((n, y_pitch), T)
        elif not (isinstance(y, np.ndarray) and y.dtype == np.dtype(T) and y.flags.c_contiguous and y.shape == (n, y_pitch)):
            raise ConfigError("y is a C-contiguous [steps, y_pitch] array of the block's type")
        st = np.zeros((n, status_pitch), np.uint8) if status else None
        g, mode = np.zeros(channels, np.float32), np.zeros(channels, np.uint8)
        fn = getattr(lib, f"yagi_hip_agc_{kind}_execute_host")
        _check(fn(channels, bandwidth, scale, g0, int(bool(locked)), int(bool(squelch)), threshold, timeout, _ptr(x),
                  x_pitch, n, _ptr(y), y_pitch, None if st is None else _ptr(st), status_pitch, _ptr(g), _ptr(mode)))
        return y, st, g, mode


CHANNEL_CHANNELS_MAX = 1 << 20     # YAGI_CHANNEL_CHANNELS_MAX
CHANNEL_TAPS_MAX = 64              # YAGI_CHANNEL_TAPS_MAX: the most taps of a link
CHANNEL_COSSIN_E = 2.0 ** -45      # YAGI_CHANNEL_COSSIN_E: the f64 error bound of the noise's cos and sin words
CHANNEL_SHAPE = np.dtype([("links", "u4"), ("rows", "u4"), ("tile_steps", "u8"), ("lds_bytes", "u8")])


def _channel_scheme(scheme):
    return scheme.value if isinstance(scheme, OscScheme) else int(scheme)


def _channel_u64(v, what):
    if not (isinstance(v, (int, np.integer)) and 0 <= v < 2 ** 64):
        raise ConfigError(f"{what} must be an unsigned 64-bit integer")
    return int(v)


def _channel_shape(s):
    return {"links": s.links, "rows": s.rows, "tile_steps": s.tile_steps, "lds_bytes": s.lds_bytes}


def channel_plan(channels, L, n, osc_scheme=OscScheme.Nco, bcast=False):
    """yagi_hip_channel_plan: the arrangement a Channel call of n steps runs at: links per workgroup row, outputs per
    lane, steps per tile and the LDS bytes"""
    s = _capi.channel_shape()
    _check(lib.yagi_hip_channel_plan(_symsync_size(channels, "channels"), _symsync_size(L, "L"), _symsync_size(n, "n"),
                                     _channel_scheme(osc_scheme), int(bool(bcast)), C.byref(s)))
    return _channel_shape(s)


def channel_awgn_words(n0_db, snr_db):
    """(gamma, nstd) of Channel.set_awgn"""
    g, s = C.c_float(), C.c_float()
    _check(lib.yagi_hip_channel_awgn_words(n0_db, snr_db, C.byref(g), C.byref(s)))
    return np.float32(g.value), np.float32(s.value)


def channel_cos_sin(k2):
    """the f64 evaluations (C, S) of cos and sin(2 pi k2 / 2^24) of Channel's noise, before the f32 rounding"""
    k2 = _arr(k2, np.uint32)
    c, s = np.empty(k2.shape, np.float64), np.empty(k2.shape, np.float64)
    _check(lib.yagi_hip_channel_cos_sin(_ptr(k2), k2.size, _ptr(c), _ptr(s)))
    return c, s


def channel_radius(k1):
    """R[k1] of Channel's noise, k1 in 1 .. 2^24"""
    k1 = _arr(k1, np.uint32)
    r = np.empty(k1.shape, np.float32)
    _check(lib.yagi_hip_channel_radius(_ptr(k1), k1.size, _ptr(r)))
    return r


def channel_noise(seed, link, first, n):
    """the noise samples of (seed, link) at counters first .. first + n - 1, on the host"""
    out = np.empty(_symsync_size(n, "n"), np.complex64)
    _check(lib.yagi_hip_channel_noise(_channel_u64(seed, "seed"), _channel_u64(link, "link"), _channel_u64(first, "first"),
                                      out.size, _ptr(out)))
    return out


def channel_constrain(phi):
    """Osc's constrain(): the u32 word of a phase or frequency in radians"""
    w = C.c_uint32()
    _check(lib.yagi_hip_channel_constrain(phi, C.byref(w)))
    return w.value


class Channel(_Handle):
    """Channel(channels, L=1, osc_scheme=OscScheme.Nco): `channels` independent links of one shape (yagi_hip.h,
    "Channel: the definition"): an L-tap multipath filter, a carrier offset (Osc's words) and gain plus white Gaussian
    noise from a counter-based generator, per link.  A block is x[n, channels] (step, channel) or, broadcast, one
    stream x[n] for every link; one output per input.  Every output word equals the definition's sequential loop bit
    for bit at every launch arrangement.  The block calls run channel_kernels.hip."""
    _prefix = "yagi_hip_channel_cccf_"

    def __init__(self, channels, L=1, osc_scheme=OscScheme.Nco):
        channels, L = _symsync_size(channels, "channels"), _symsync_size(L, "L")
        hd = C.c_void_p()
        _check(self._fn("create")(channels, L, _channel_scheme(osc_scheme), C.byref(hd)))
        self._h, self.channels, self.L = hd, channels, L

    def clone(self):
        new, hd = object.__new__(type(self)), C.c_void_p()
        _check(self._fn("clone")(self._h, C.byref(hd)))
        new._h, new.channels, new.L = hd, self.channels, self.L
        return new

    def _call(self, name, *args):
        _check(self._fn(name)(self._h, *args))

    def _vector(self, v, dt, what, shape=None):
        v = _arr(v, dt)
        if v.shape != (shape or (self.channels,)):
            raise ConfigError(f"{what} holds one value per channel")
        return v

    def reset_channel(self, c):
        self._call("reset_channel", _symsync_size(c, "channel"))

    def set_awgn(self, c, n0_db, snr_db):
        """noise floor n0_db and signal-to-noise ratio snr_db of link c: nstd = 10^(n0_db / 20), gamma = 10^((snr_db +
        n0_db) / 20)"""
        self._call("set_awgn", _symsync_size(c, "channel"), n0_db, snr_db)

    def set_awgn_all(self, n0_db, snr_db):
        self._call("set_awgn_all", _ptr(self._vector(n0_db, np.float32, "n0_db")),
                   _ptr(self._vector(snr_db, np.float32, "snr_db")))

    def set_gain_noise(self, c, gamma, nstd):
        self._call("set_gain_noise", _symsync_size(c, "channel"), gamma, nstd)

    def set_gain_noise_all(self, gamma, nstd):
        self._call("set_gain_noise_all", _ptr(self._vector(gamma, np.float32, "gamma")),
                   _ptr(self._vector(nstd, np.float32, "nstd")))

    def set_carrier_offset(self, c, dphi, phi=0.0):
        """radians per sample and the phase now, through Osc's set_frequency and set_phase"""
        self._call("set_carrier_offset", _symsync_size(c, "channel"), dphi, phi)

    def set_carrier_offset_all(self, dphi, phi):
        self._call("set_carrier_offset_all", _ptr(self._vector(dphi, np.float32, "dphi")),
                   _ptr(self._vector(phi, np.float32, "phi")))

    def set_multipath(self, c, h):
        h = _arr(h, np.complex64)
        if h.shape != (self.L,):
            raise ConfigError(f"a link has {self.L} taps")
        self._call("set_multipath", _symsync_size(c, "channel"), _ptr(h))

    def set_multipath_all(self, h):
        self._call("set_multipath_all", _ptr(self._vector(h, np.complex64, "h", (self.channels, self.L))))

    def get_multipath(self):
        h = np.zeros((self.channels, self.L), np.complex64)
        self._call("get_multipath", _ptr(h))
        return h

    def set_seed(self, seed):
        self._call("set_seed", _channel_u64(seed, "seed"))

    def get_seed(self):
        v = C.c_uint64()
        self._call("get_seed", C.byref(v))
        return v.value

    def set_position(self, c, t):
        """seek link c's noise: the counter of its next sample"""
        self._call("set_position", _symsync_size(c, "channel"), _channel_u64(t, "t"))

    def set_position_all(self, t):
        self._call("set_position_all", _ptr(self._vector(t, np.uint64, "t")))

    def get_position(self):
        t = np.zeros(self.channels, np.uint64)
        self._call("get_position", _ptr(t))
        return t

    def get_gain_noise(self):
        """(gamma[channels], nstd[channels])"""
        g, s = np.zeros(self.channels, np.float32), np.zeros(self.channels, np.float32)
        self._call("get_gain_noise", _ptr(g), _ptr(s))
        return g, s

    def get_osc_state(self):
        """the oscillators' raw words (theta[channels], d_theta[channels])"""
        th, d = np.zeros(self.channels, np.uint32), np.zeros(self.channels, np.uint32)
        self._call("get_osc_state", _ptr(th), _ptr(d))
        return th, d

    def set_shape(self, links=0, rows=0):
        """override the launch arrangement (links a power of two up to 64, rows 1, 2, 4, 8 or 16); (0, 0): the planner"""
        self._call("set_shape", links, rows)

    def get_shape(self, n, bcast=False):
        s = _capi.channel_shape()
        self._call("get_shape", _symsync_size(n, "n"), int(bool(bcast)), C.byref(s))
        return _channel_shape(s)

    def execute(self, x):
        """x[n, channels] -> y[n, channels]"""
        x = _arr(x, np.complex64)
        if x.ndim != 2 or x.shape[1] != self.channels:
            raise ConfigError(f"the block is [steps, {self.channels}]")
        y = np.zeros_like(x)
        self._call("execute", _ptr(x), self.channels, x.shape[0], _ptr(y), self.channels)
        return y

    def execute_bcast(self, x):
        """x[n], the same stream into every link -> y[n, channels]"""
        x = _arr(x, np.complex64)
        if x.ndim != 1:
            raise ConfigError("the broadcast input is one stream")
        y = np.zeros((x.size, self.channels), np.complex64)
        self._call("execute_bcast", _ptr(x), x.size, _ptr(y), self.channels)
        return y

    def execute_devptr(self, x_dev, x_pitch, n, y_dev, y_pitch):
        """n rows of pitch x_pitch, y_pitch elements; asynchronous on the object's stream (the C ABI's execute_dev)"""
        self._call("execute_dev", None if x_dev is None else _devptr(x_dev), x_pitch, n,
                   None if y_dev is None else _devptr(y_dev), y_pitch)

    def execute_bcast_devptr(self, x_dev, n, y_dev, y_pitch):
        self._call("execute_bcast_dev", None if x_dev is None else _devptr(x_dev), n,
                   None if y_dev is None else _devptr(y_dev), y_pitch)

    @staticmethod
    def execute_host(h, gamma, nstd, theta, d_theta, t, x, osc_scheme=OscScheme.Nco, seed=0, bcast=False, x_pitch=None,
                     y_pitch=None, y=None):
        """the definition on the host alone, no device needed: one call from reset() with the raw words given.
        h[channels, L]; gamma, nstd, theta, d_theta, t are [channels]; x is [n, x_pitch], or [n] where bcast; y, where
        given, is the [n, y_pitch] array that is written.  The library's own sequential form, slow and meant for checks"""
        h = _arr(h, np.complex64)
        if h.ndim != 2:
            raise ConfigError("h is [channels, L]")
        channels, L = h.shape
        words = [_arr(v, dt) for v, dt in ((gamma, np.float32), (nstd, np.float32), (theta, np.uint32),
                                            (d_theta, np.uint32), (t, np.uint64))]
        if any(w.shape != (channels,) for w in words):
            raise ConfigError("every word array holds one value per channel")
        x_pitch, y_pitch = (channels if p is None else _symsync_size(p, "pitch") for p in (x_pitch, y_pitch))
        x = _arr(x, np.complex64)
        if bcast:
            if x.ndim != 1:
                raise ConfigError("the broadcast input is one stream")
        elif x.ndim != 2 or x.shape[1] != x_pitch:
            raise ConfigError("the block is [steps, x_pitch]")
        n = x.shape[0]
        if y is None:
            y = np.zeros((n, y_pitch), np.complex64)
        elif not (isinstance(y, np.ndarray) and y.dtype == np.complex64 and y.flags.c_contiguous and y.shape == (n, y_pitch)):
            raise ConfigError("y is a C-contiguous [steps, y_pitch] complex64 array")
        _check(lib.yagi_hip_channel_cccf_execute_host(channels, L, _channel_scheme(osc_scheme), int(bool(bcast)),
                                                      _channel_u64(seed, "seed"), _ptr(h),
                                                      *(_ptr(w) for w in words), _ptr(x), x_pitch, n, _ptr(y), y_pitch))
        return y


CONVCODE_DECISION_BYTES = 131072   # YAGI_CONVCODE_DECISION_BYTES: the decisions of one frame, T S / 8 bytes
CONVCODE_STEPS_MAX = 65536         # YAGI_CONVCODE_STEPS_MAX
CONVCODE_FRAMES_MAX = 1 << 20      # YAGI_CONVCODE_FRAMES_MAX
CONVCODE_PERIOD_MAX = 32           # YAGI_CONVCODE_PERIOD_MAX


def _convcode_shape(s):
    return {"frames_per_wave": s.frames_per_wave, "waves": s.waves, "states_per_lane": s.states_per_lane,
            "chunk_steps": s.chunk_steps, "frames_per_wg": s.frames_per_wg, "lds_bytes": s.lds_bytes}


def _convcode_code(K, polys, puncture):
    """(K, g, R, P or None, p) as the C ABI takes them; what it would misread is a ConfigError here"""
    polys = list(polys)
    if not all(isinstance(v, (int, np.integer)) and 0 <= v < 2 ** 32 for v in polys):
        raise ConfigError("the generator words are unsigned integers")
    g = np.array(polys, np.uint32)
    if puncture is None:
        return int(K), g, g.size, None, 1
    P = np.asarray(puncture)
    if P.ndim != 2 or P.shape[0] != g.size or not np.isin(P, (0, 1)).all():
        raise ConfigError("the puncture matrix is [generators, p] of 0 and 1")
    return int(K), g, g.size, _arr(P, np.uint8), P.shape[1]


def _convcode_rows(a, width, what):
    """a 2-D uint8 plane of at least `width` bytes per row -> (array, rows, pitch)"""
    a = _arr(a, np.uint8)
    if a.ndim == 1:
        a = a[None, :]
    if a.ndim != 2 or a.shape[1] < width:
        raise ConfigError(f"{what} is [frames, at least {width} bytes]")
    return a, a.shape[0], a.shape[1]


def _convcode_out(out, F, width):
    if out is None:
        return np.zeros((F, width), np.uint8)
    if not (isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.flags.c_contiguous and out.ndim == 2
            and out.shape[0] == F and out.shape[1] >= width):
        raise ConfigError(f"the output is a C-contiguous uint8 array [{F}, at least {width}]")
    return out


def convcode_plan(K, n, F, terminated=True):
    """yagi_hip_convcode_plan: the arrangement ConvCode.decode_block runs F frames of n bits at"""
    s = _capi.convcode_shape()
    _check(lib.yagi_hip_convcode_plan(int(K), int(bool(terminated)), _symsync_size(n, "n"), _symsync_size(F, "F"), C.byref(s)))
    return _convcode_shape(s)


class ConvCode(_Handle):
    """ConvCode(K, polys, puncture=None, terminated=True): a convolutional code of constraint length K (3 .. 9) with
    2 .. 4 generator words and an optional [generators, p] puncture matrix, over a bank of frames (yagi_hip.h, "ConvCode:
    the definition").  encode_block turns rows of packed message bytes (most significant bit first) into rows of one byte
    per coded bit; decode_block is a Viterbi decoder over rows of soft bytes (0 .. 255, 255 a confident 1: Modem's soft
    bits) and returns the packed messages and the path metric of each frame.  Everything is integer arithmetic: every
    byte equals the definition's sequential loop.  The block calls run convcode_kernels.hip; no call keeps state."""
    _prefix = "yagi_hip_convcode_"

    def __init__(self, K, polys, puncture=None, terminated=True):
        K, g, R, P, p = _convcode_code(K, polys, puncture)
        hd = C.c_void_p()
        _check(self._fn("create")(K, _ptr(g), R, None if P is None else _ptr(P), p, int(bool(terminated)), C.byref(hd)))
        self._h, self.K, self.R, self.terminated = hd, K, R, bool(terminated)

    # the public Voyager / CCSDS words
    @classmethod
    def v27(cls):
        return cls(7, (0x6d, 0x4f))

    @classmethod
    def v29(cls):
        return cls(9, (0x1af, 0x11d))

    @classmethod
    def v39(cls):
        return cls(9, (0x1ed, 0x19b, 0x127))

    @classmethod
    def v27p23(cls):
        return cls(7, (0x6d, 0x4f), [[1, 1], [1, 0]])

    @classmethod
    def v27p34(cls):
        return cls(7, (0x6d, 0x4f), [[1, 1, 0], [1, 0, 1]])

    def clone(self):
        new, hd = object.__new__(type(self)), C.c_void_p()
        _check(self._fn("clone")(self._h, C.byref(hd)))
        new._h, new.K, new.R, new.terminated = hd, self.K, self.R, self.terminated
        return new

    def _call(self, name, *args):
        _check(self._fn(name)(self._h, *args))

    def get_K(self):
        v = C.c_int()
        self._call("get_K", C.byref(v))
        return v.value

    def get_R(self):
        v = C.c_int()
        self._call("get_R", C.byref(v))
        return v.value

    def rate(self):
        """(kept, p): kept coded bits per p message bits"""
        k, p = C.c_size_t(), C.c_size_t()
        self._call("get_rate", C.byref(k), C.byref(p))
        return k.value, p.value

    def ncoded(self, n):
        """coded bytes of a frame of n message bits"""
        v = C.c_size_t()
        self._call("get_ncoded", _symsync_size(n, "n"), C.byref(v))
        return v.value

    def nmax(self):
        v = C.c_size_t()
        self._call("get_nmax", C.byref(v))
        return v.value

    def set_shape(self, frames_per_wave=0, waves=0):
        """override the decoder's launch arrangement; (0, 0): the planner"""
        self._call("set_shape", frames_per_wave, waves)

    def get_shape(self, n, F):
        s = _capi.convcode_shape()
        self._call("get_shape", _symsync_size(n, "n"), _symsync_size(F, "F"), C.byref(s))
        return _convcode_shape(s)

    def encode_block(self, msg, n, out=None):
        """msg[F, >= ceil(n / 8)] packed bytes -> coded[F, ncoded(n)] of 0 / 1 (or into the leading columns of out)"""
        n = _symsync_size(n, "n")
        msg, F, pitch = _convcode_rows(msg, (n + 7) // 8, "msg")
        out = _convcode_out(out, F, self.ncoded(n))
        self._call("encode_block", _ptr(msg), pitch, n, F, _ptr(out), out.shape[1])
        return out

    def decode_block(self, soft, n, out=None, metric=True):
        """soft[F, >= ncoded(n)] -> (msg[F, ceil(n / 8)], metric[F] uint32), or msg alone where metric is False"""
        n = _symsync_size(n, "n")
        soft, F, pitch = _convcode_rows(soft, self.ncoded(n), "soft")
        out = _convcode_out(out, F, (n + 7) // 8)
        m = np.zeros(F, np.uint32) if metric else None
        self._call("decode_block", _ptr(soft), pitch, n, F, _ptr(out), out.shape[1], None if m is None else _ptr(m))
        return (out, m) if metric else out

    def encode_block_devptr(self, msg_dev, msg_pitch, n, F, coded_dev, coded_pitch):
        """device pointers, pitches in bytes; asynchronous on the object's stream (the C ABI's encode_block_dev)"""
        self._call("encode_block_dev", None if msg_dev is None else _devptr(msg_dev), msg_pitch, n, F,
                   None if coded_dev is None else _devptr(coded_dev), coded_pitch)

    def decode_block_devptr(self, soft_dev, soft_pitch, n, F, msg_dev, msg_pitch, metric_dev=None):
        self._call("decode_block_dev", None if soft_dev is None else _devptr(soft_dev), soft_pitch, n, F,
                   None if msg_dev is None else _devptr(msg_dev), msg_pitch, None if metric_dev is None else _devptr(metric_dev))

    # the definition on the host alone, no device needed: the library's own sequential loops, slow and meant for checks
    @staticmethod
    def ncoded_host(K, R, n, puncture=None, terminated=True):
        K, g, R, P, p = _convcode_code(K, [1] * int(R), puncture)
        v = C.c_size_t()
        _check(lib.yagi_hip_convcode_ncoded_host(K, R, None if P is None else _ptr(P), p, int(bool(terminated)),
                                                 _symsync_size(n, "n"), C.byref(v), None))
        return v.value

    @staticmethod
    def nmax_host(K, R=2, puncture=None, terminated=True):
        K, g, R, P, p = _convcode_code(K, [1] * int(R), puncture)
        v = C.c_size_t()
        _check(lib.yagi_hip_convcode_ncoded_host(K, R, None if P is None else _ptr(P), p, int(bool(terminated)), 0, None,
                                                 C.byref(v)))
        return v.value

    @staticmethod
    def encode_host(K, polys, msg, n, puncture=None, terminated=True, out=None, msg_pitch=None, coded_pitch=None):
        """msg[F, pitch] -> coded[F, coded_pitch]; the pitches default to the arrays' widths (given explicitly they are
        handed to the library as they are, for its argument checks)"""
        K, g, R, P, p = _convcode_code(K, polys, puncture)
        n = _symsync_size(n, "n")
        msg = _arr(msg, np.uint8)
        msg = msg[None, :] if msg.ndim == 1 else msg
        F = msg.shape[0]
        if out is None:
            out = np.zeros((F, ConvCode.ncoded_host(K, R, n, puncture, terminated)), np.uint8)
        _check(lib.yagi_hip_convcode_encode_host(K, _ptr(g), R, None if P is None else _ptr(P), p, int(bool(terminated)),
                                                 _ptr(msg), msg.shape[1] if msg_pitch is None else msg_pitch, n, F, _ptr(out),
                                                 out.shape[1] if coded_pitch is None else coded_pitch))
        return out

    @staticmethod
    def decode_host(K, polys, soft, n, puncture=None, terminated=True, out=None, metric=True, soft_pitch=None, msg_pitch=None):
        """soft[F, pitch] -> (msg[F, ceil(n / 8)], metric[F]), or msg alone where metric is False"""
        K, g, R, P, p = _convcode_code(K, polys, puncture)
        n = _symsync_size(n, "n")
        soft = _arr(soft, np.uint8)
        soft = soft[None, :] if soft.ndim == 1 else soft
        F = soft.shape[0]
        if out is None:
            out = np.zeros((F, (n + 7) // 8), np.uint8)
        m = np.zeros(F, np.uint32) if metric else None
        _check(lib.yagi_hip_convcode_decode_host(K, _ptr(g), R, None if P is None else _ptr(P), p, int(bool(terminated)),
                                                 _ptr(soft), soft.shape[1] if soft_pitch is None else soft_pitch, n, F,
                                                 _ptr(out), out.shape[1] if msg_pitch is None else msg_pitch,
                                                 None if m is None else _ptr(m)))
        return (out, m) if metric else out


PACKETIZER_COLUMNS_MAX = 1 << 20   # YAGI_PACKETIZER_COLUMNS_MAX


class CrcScheme(enum.IntEnum):
    """the Packetizer's CRC, numbered as YAGI_CRC_* (yagi_hip.h gives the Rocksoft parameters of each)"""
    NONE = 0
    CRC_8 = 1       # poly 0x07, init 0x00
    CRC_16 = 2      # poly 0x1021, init 0xFFFF (CCITT-FALSE)
    CRC_24 = 3      # poly 0x864CFB, init 0xB704CE (OpenPGP)
    CRC_32 = 4      # poly 0x04C11DB7 reflected, init and xorout 0xFFFFFFFF (zlib's)


def _crc_scheme(scheme):
    if not isinstance(scheme, (int, np.integer)):
        raise ConfigError("the CRC scheme is a CrcScheme")
    return int(scheme)


def crc(scheme, data):
    """yagi_hip_crc_host: the CRC of a byte string under one of the Packetizer's schemes"""
    data = _arr(np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray)) else data, np.uint8).reshape(-1)
    v = C.c_uint32()
    _check(lib.yagi_hip_crc_host(_crc_scheme(scheme), _ptr(data), data.size, C.byref(v)))
    return v.value


def packetizer_permutation(N, columns):
    """yagi_hip_packetizer_permutation: pi[i], the transmit position of coder-order bit i of N through C columns"""
    N = _symsync_size(N, "N")
    pi = np.zeros(N, np.uint32)
    _check(lib.yagi_hip_packetizer_permutation(N, _symsync_size(columns, "columns"), _ptr(pi)))
    return pi


def _scramble(fn, x):
    x = np.array(_arr(x, np.uint8).reshape(-1))
    _check(fn(_ptr(x), x.size))
    return x


def scramble_data(x):
    """random::scramble::scramble_data (scramble.rs :7-29) on a copy of the bytes"""
    return _scramble(lib.yagi_hip_scramble_data, x)


def unscramble_data(x):
    """random::scramble::unscramble_data (scramble.rs :31-34) on a copy"""
    return _scramble(lib.yagi_hip_unscramble_data, x)


def unscramble_data_soft(x):
    """random::scramble::unscramble_data_soft (scramble.rs :37-53) on a copy: whole groups of eight soft bytes"""
    return _scramble(lib.yagi_hip_unscramble_data_soft, x)


def packetizer_plan(K, n, crc, F, terminated=True):
    """yagi_hip_packetizer_plan: the arrangement Packetizer.decode_block runs F frames of n payload bytes at"""
    s = _capi.convcode_shape()
    _check(lib.yagi_hip_packetizer_plan(int(K), int(bool(terminated)), _symsync_size(n, "n"), _crc_scheme(crc),
                                        _symsync_size(F, "F"), C.byref(s)))
    return _convcode_shape(s)


def _packetizer_code(n, crc, K, polys, puncture, terminated, columns, scramble):
    """the ten leading arguments of create and of the host forms, with what must stay alive"""
    K, g, R, P, p = _convcode_code(K, polys, puncture)
    args = (_symsync_size(n, "n"), _crc_scheme(crc), K, _ptr(g), R, None if P is None else _ptr(P), p, int(bool(terminated)),
            _symsync_size(columns, "columns"), int(bool(scramble)))
    return args, (g, P)


class Packetizer(_Handle):
    """Packetizer(n, crc, K, polys, puncture=None, terminated=True, columns=1, scramble=True): n payload bytes per frame, a
    CRC behind them, ConvCode's code over both, a block interleaver of `columns` columns and the reference's scrambler
    (random::scramble), for a bank of frames and in one launch per direction (yagi_hip.h, "Packetizer: the definition").
    encode_block(payload, bps) gives the transmit plane, bps bits per byte (bps = 2 feeds Modem(Qpsk).modulate_block);
    decode_block(soft) takes Modem's soft bytes in transmit order and returns the payloads, a valid flag per frame, the
    CRC computed over each decoded payload and ConvCode's path metric.  Everything is integer arithmetic: every byte equals
    the definition's sequential loops.  The block calls run packetizer_kernels.hip; no call keeps state."""
    _prefix = "yagi_hip_packetizer_"

    def __init__(self, n, crc, K, polys, puncture=None, terminated=True, columns=1, scramble=True):
        args, keep = _packetizer_code(n, crc, K, polys, puncture, terminated, columns, scramble)
        hd = C.c_void_p()
        _check(self._fn("create")(*args, C.byref(hd)))
        self._h, self.n, self.crc, self.K, self.terminated = hd, args[0], CrcScheme(args[1]), args[2], bool(terminated)
        self.columns, self.scramble = args[8], bool(scramble)

    # ConvCode's named codes
    @classmethod
    def v27(cls, n, crc=CrcScheme.CRC_32, **kw):
        return cls(n, crc, 7, (0x6d, 0x4f), **kw)

    @classmethod
    def v29(cls, n, crc=CrcScheme.CRC_32, **kw):
        return cls(n, crc, 9, (0x1af, 0x11d), **kw)

    @classmethod
    def v39(cls, n, crc=CrcScheme.CRC_32, **kw):
        return cls(n, crc, 9, (0x1ed, 0x19b, 0x127), **kw)

    @classmethod
    def v27p23(cls, n, crc=CrcScheme.CRC_32, **kw):
        return cls(n, crc, 7, (0x6d, 0x4f), [[1, 1], [1, 0]], **kw)

    @classmethod
    def v27p34(cls, n, crc=CrcScheme.CRC_32, **kw):
        return cls(n, crc, 7, (0x6d, 0x4f), [[1, 1, 0], [1, 0, 1]], **kw)

    def clone(self):
        new, hd = object.__new__(type(self)), C.c_void_p()
        _check(self._fn("clone")(self._h, C.byref(hd)))
        new._h = hd
        for k in ("n", "crc", "K", "terminated", "columns", "scramble"):
            setattr(new, k, getattr(self, k))
        return new

    def _call(self, name, *args):
        _check(self._fn(name)(self._h, *args))

    def _size(self, name, *args):
        v = C.c_size_t()
        self._call(name, *args, C.byref(v))
        return v.value

    def payload_len(self):
        return self._size("get_payload_len")

    def crc_len(self):
        return self._size("get_crc_len")

    def msg_bits(self):
        return self._size("get_msg_bits")

    def enc_len(self):
        """N: coded (= transmit) bits of a frame"""
        return self._size("get_enc_len")

    def nsym(self, bps=1):
        """bytes of a frame's row of the transmit plane at bps bits per byte"""
        return self._size("get_nsym", self._bps(bps))

    def get_columns(self):
        return self._size("get_columns")

    @staticmethod
    def _bps(bps):
        if not (isinstance(bps, (int, np.integer)) and 0 <= bps < 2 ** 32):
            raise ConfigError("bps is 1 .. 8")
        return int(bps)

    def set_shape(self, frames_per_wave=0, waves=0):
        """override the decoder's launch arrangement (ConvCode's admissible set); (0, 0): the planner"""
        self._call("set_shape", frames_per_wave, waves)

    def get_shape(self, F):
        s = _capi.convcode_shape()
        self._call("get_shape", _symsync_size(F, "F"), C.byref(s))
        return _convcode_shape(s)

    def encode_block(self, payload, bps=1, out=None):
        """payload[F, >= n] -> tx[F, nsym(bps)] (or into the leading columns of out)"""
        bps = self._bps(bps)
        payload, F, pitch = _convcode_rows(payload, self.n, "payload")
        out = _convcode_out(out, F, self.nsym(bps))
        self._call("encode_block", _ptr(payload), pitch, F, bps, _ptr(out), out.shape[1])
        return out

    def decode_block(self, soft, out=None, crc=True, metric=True):
        """soft[F, >= N] -> (payload[F, n], valid[F] uint8, crc[F] uint32, metric[F] uint32); crc and metric are None where
        not asked for"""
        soft, F, pitch = _convcode_rows(soft, self.enc_len(), "soft")
        out = _convcode_out(out, F, self.n)
        valid = np.zeros(F, np.uint8)
        c = np.zeros(F, np.uint32) if crc else None
        m = np.zeros(F, np.uint32) if metric else None
        self._call("decode_block", _ptr(soft), pitch, F, _ptr(out), out.shape[1], _ptr(valid), None if c is None else _ptr(c),
                   None if m is None else _ptr(m))
        return out, valid, c, m

    def encode_block_devptr(self, payload_dev, payload_pitch, F, bps, tx_dev, tx_pitch):
        """device pointers, pitches in bytes; asynchronous on the object's stream (the C ABI's encode_block_dev)"""
        self._call("encode_block_dev", None if payload_dev is None else _devptr(payload_dev), payload_pitch, F, self._bps(bps),
                   None if tx_dev is None else _devptr(tx_dev), tx_pitch)

    def decode_block_devptr(self, soft_dev, soft_pitch, F, payload_dev, payload_pitch, valid_dev, crc_dev=None, metric_dev=None):
        opt = [None if v is None else _devptr(v) for v in (soft_dev, payload_dev, valid_dev, crc_dev, metric_dev)]
        self._call("decode_block_dev", opt[0], soft_pitch, F, opt[1], payload_pitch, opt[2], opt[3], opt[4])

    # the definition on the host alone, no device needed: the library's own sequential loops, slow and meant for checks
    @staticmethod
    def encode_host(n, crc, K, polys, payload, bps=1, puncture=None, terminated=True, columns=1, scramble=True, out=None,
                    payload_pitch=None, tx_pitch=None):
        """payload[F, pitch] -> tx[F, tx_pitch]; the pitches default to the arrays' widths (given explicitly they are handed
        to the library as they are, for its argument checks); out is needed where the sizes are not valid ones"""
        args, keep = _packetizer_code(n, crc, K, polys, puncture, terminated, columns, scramble)
        payload = _arr(payload, np.uint8)
        payload = payload[None, :] if payload.ndim == 1 else payload
        F = payload.shape[0]
        if out is None:
            w = (0, 1, 2, 3, 4)[args[1]] if 0 <= args[1] <= 4 else 0
            N = ConvCode.ncoded_host(K, len(list(polys)), 8 * (args[0] + w), puncture, terminated)
            out = np.zeros((F, -(-N // max(1, int(bps)))), np.uint8)
        _check(lib.yagi_hip_packetizer_encode_host(*args, _ptr(payload), payload.shape[1] if payload_pitch is None else payload_pitch,
                                                   F, Packetizer._bps(bps), _ptr(out), out.shape[1] if tx_pitch is None else tx_pitch))
        return out

    @staticmethod
    def decode_host(n, crc, K, polys, soft, puncture=None, terminated=True, columns=1, scramble=True, out=None, soft_pitch=None,
                    payload_pitch=None, want_crc=True, metric=True):
        """soft[F, pitch] -> (payload[F, n], valid[F], crc[F] or None, metric[F] or None)"""
        args, keep = _packetizer_code(n, crc, K, polys, puncture, terminated, columns, scramble)
        soft = _arr(soft, np.uint8)
        soft = soft[None, :] if soft.ndim == 1 else soft
        F = soft.shape[0]
        if out is None:
            out = np.zeros((F, args[0]), np.uint8)
        valid = np.zeros(F, np.uint8)
        c = np.zeros(F, np.uint32) if want_crc else None
        m = np.zeros(F, np.uint32) if metric else None
        _check(lib.yagi_hip_packetizer_decode_host(*args, _ptr(soft), soft.shape[1] if soft_pitch is None else soft_pitch, F,
                                                   _ptr(out), out.shape[1] if payload_pitch is None else payload_pitch, _ptr(valid),
                                                   None if c is None else _ptr(c), None if m is None else _ptr(m)))
        return out, valid, c, m


SYMTRACK_CHANNELS_MAX = 1 << 20    # YAGI_SYMTRACK_CHANNELS_MAX
SYMTRACK_PLL_ARG_MAX = 256.0       # YAGI_SYMTRACK_PLL_ARG_MAX: a pll_step argument of this magnitude stalls the channel
SYMTRACK_STALL_CAPACITY = 1        # YAGI_SYMTRACK_STALL_CAPACITY: the channel would have written symbol number ycap
SYMTRACK_STALL_PLL = 2             # YAGI_SYMTRACK_STALL_PLL


class SymTrackEq(enum.IntEnum):
    """what SymTrack's equalizer does after each symbol past the hold-off, numbered as YAGI_SYMTRACK_EQ_*"""
    OFF = 0         # the weights stay
    CM = 1          # constant modulus: step(d_hat / |d_hat|, d_hat)
    DD = 2          # decision directed: step(x_hat, d_hat), x_hat from the de-rotated sample


def _symtrack_scheme(scheme):
    """(scheme number, table or None) of a ModulationScheme or a table of points"""
    if isinstance(scheme, (int, np.integer, enum.IntEnum)):
        return int(scheme), None
    t = _arr(scheme, np.complex64)
    if t.ndim != 1:
        raise ConfigError("a constellation table is one-dimensional")
    return int(ModulationScheme.Arb), t


class SymTrack(_Handle):
    """SymTrack(channels, ftype, k, m, beta, scheme, osc_scheme, npfb=16, eq_len=9): `channels` independent receivers of
    one design: Agc -> SymSync (k_out = 2) -> Osc.mix_down -> EqLms -> Modem, with the carrier loop closed from the
    demodulator's phase error per symbol and the equalizer updated from the de-rotated sample (yagi_hip.h, "SymTrack: the
    definition"; the reference's src/framing/symtrack.rs is empty).  scheme is a ModulationScheme (Bpsk, Qpsk, Ook, Ask*,
    Qam*; Psk* and Dpsk* are a ConfigError) or a table of 2 .. 256 points.  execute takes a block x[n, channels] (step,
    channel) and returns per channel the equalized symbols d_hat and the decisions, bit for bit the composition of the
    parts' sequential loops.
    A channel that would write more than ycap symbols in a call, or whose pll_step argument reaches SYMTRACK_PLL_ARG_MAX,
    is stalled: it ignores all further input and reports ny = 0 until reset() or reset_channel(c).
    The block calls run symtrack_kernels.hip, one lane per channel."""
    _prefix = "yagi_hip_symtrack_cccf_"

    def __init__(self, channels, ftype, k, m, beta, scheme, osc_scheme=OscScheme.Nco, npfb=16, eq_len=9):
        channels, k, m, npfb, eq_len = (_symsync_size(v, "argument") for v in (channels, k, m, npfb, eq_len))
        scheme, table = _symtrack_scheme(scheme)
        osc = OscScheme(osc_scheme).value
        hd = C.c_void_p()
        if table is None:
            _check(self._fn("create")(channels, int(ftype), k, m, beta, scheme, osc, npfb, eq_len, C.byref(hd)))
        else:
            _check(self._fn("create_from_table")(channels, int(ftype), k, m, beta, _ptr(table), table.size, osc, npfb,
                                                 eq_len, C.byref(hd)))
        self._set(hd, channels, k, eq_len)

    def _set(self, hd, channels, k, eq_len):
        self._h, self.kind, self.T, self.channels, self.k, self.eq_len = hd, "cccf", np.complex64, channels, k, eq_len

    def clone(self):
        new, hd = object.__new__(type(self)), C.c_void_p()
        _check(self._fn("clone")(self._h, C.byref(hd)))
        new._set(hd, self.channels, self.k, self.eq_len)
        return new

    def reset_channel(self, c):
        _check(self._fn("reset_channel")(self._h, _symsync_size(c, "channel")))

    def set_bandwidth(self, bw):
        """agc 0.02 bw, timing loop 0.001 bw, equalizer 0.02 bw, PLL 0.001 bw, the products in f32"""
        _check(self._fn("set_bandwidth")(self._h, bw))

    def get_bandwidth(self):
        v = C.c_float()
        _check(self._fn("get_bandwidth")(self._h, C.byref(v)))
        return v.value

    def set_bandwidths(self, agc, sync, eq, pll):
        """the four setters one by one; get_bandwidth reports NaN afterwards"""
        _check(self._fn("set_bandwidths")(self._h, agc, sync, eq, pll))

    def set_eq_strategy(self, strategy):
        _check(self._fn("set_eq_strategy")(self._h, int(SymTrackEq(strategy))))

    def set_eq_holdoff(self, nsyms):
        _check(self._fn("set_eq_holdoff")(self._h, _symsync_size(nsyms, "nsyms")))

    def set_nco(self, c, frequency, phase=0.0):
        """set_frequency and set_phase of channel c's oscillator, radians per synchroniser output sample and radians"""
        _check(self._fn("set_nco")(self._h, _symsync_size(c, "channel"), frequency, phase))

    def set_nco_all(self, frequency, phase=None):
        f = _arr(frequency, np.float32)
        p = np.zeros(self.channels, np.float32) if phase is None else _arr(phase, np.float32)
        if f.shape != (self.channels,) or p.shape != (self.channels,):
            raise ConfigError("one frequency and one phase per channel")
        _check(self._fn("set_nco_all")(self._h, _ptr(f), _ptr(p)))

    def _get(self, name, dt, shape=None):
        out = np.zeros(self.channels if shape is None else shape, dt)
        _check(self._fn(name)(self._h, _ptr(out)))
        return out

    def get_tau(self):
        """tau_decim of every channel; synchronises, as every getter below does"""
        return self._get("get_tau", np.float32)

    def get_gain(self):
        return self._get("get_gain", np.float32)

    def get_rssi(self):
        return self._get("get_rssi", np.float32)

    def get_nco_frequency(self):
        return self._get("get_nco_frequency", np.float32)

    def get_nco_phase(self):
        return self._get("get_nco_phase", np.float32)

    def get_nco_state(self):
        """(theta, d_theta): the oscillators' raw u32 words"""
        th, dth = np.zeros(self.channels, np.uint32), np.zeros(self.channels, np.uint32)
        _check(self._fn("get_nco_state")(self._h, _ptr(th), _ptr(dth)))
        return th, dth

    def get_weights(self):
        """[channels, eq_len], as EqLms.get_weights"""
        return self._get("get_weights", np.complex64, (self.channels, self.eq_len))

    def get_num_syms(self):
        return self._get("get_num_syms", np.uint64)

    def get_stalled(self):
        """the stall reason of every channel, 0 = running"""
        return self._get("get_stalled", np.uint32)

    def default_ycap(self, n):
        """ceil(n / k) + 8: a default, not a bound (a loop far from lock can write more)"""
        return -(-int(n) // self.k) + 8

    def execute(self, x, ycap=None, symbols=True):
        """x[n, channels] -> (y[ycap, channels], sym[ycap, channels] or None, ny[channels], stalled[channels]); y[j, c] and
        sym[j, c] are symbol j of channel c for j < ny[c] and zero below.  ycap defaults to default_ycap(n)"""
        x = _arr(x, self.T)
        if x.ndim != 2 or x.shape[1] != self.channels:
            raise ConfigError(f"the block is [steps, {self.channels}]")
        n = x.shape[0]
        ycap = self.default_ycap(n) if ycap is None else _symsync_size(ycap, "ycap")
        y = np.zeros((ycap, self.channels), self.T)
        sym = np.zeros((ycap, self.channels), np.uint8) if symbols else None
        ny, st = np.zeros(self.channels, np.uint32), np.zeros(self.channels, np.uint32)
        _check(self._fn("execute")(self._h, _ptr(x), self.channels, n, _ptr(y), self.channels,
                                   None if sym is None else _ptr(sym), self.channels, ycap, _ptr(ny), _ptr(st)))
        return y, sym, ny, st

    def execute_devptr(self, x_dev, x_pitch, n, y_dev, y_pitch, sym_dev, sym_pitch, ycap, status_dev):
        """x_dev: n rows of pitch x_pitch samples; y_dev: ycap rows of pitch y_pitch; sym_dev: ycap rows of sym_pitch bytes
        or None; status_dev: 3 channels uint32 that receive ny, the stall reason and the low word of num_syms.  Rows >=
        ny[c] of a channel are not touched.  Asynchronous on the object's stream (the C ABI's execute_dev)"""
        x_dev, y_dev, sym_dev, status_dev = (None if p is None else _devptr(p) for p in (x_dev, y_dev, sym_dev, status_dev))
        _check(self._fn("execute_dev")(self._h, x_dev, x_pitch, n, y_dev, y_pitch, sym_dev, sym_pitch, ycap, status_dev))


def symtrack_host(channels, ftype, k, m, beta, scheme, osc_scheme, x, npfb=16, eq_len=9, bw=0.9, strategy=SymTrackEq.CM,
                  holdoff=200, nco_frequency=None, nco_phase=None, ycap=None, x_pitch=None, y_pitch=None, sym_pitch=None):
    """SymTrack's definition on the host alone, no device needed: one call from reset().  x is [n, x_pitch] (the pitches
    default to channels); returns (y[ycap, y_pitch], sym[ycap, sym_pitch], ny, stalled).  The library's own sequential
    form, slow and meant for checks"""
    channels, k, m, npfb, eq_len, holdoff = (_symsync_size(v, "argument") for v in (channels, k, m, npfb, eq_len, holdoff))
    if not 1 <= channels <= SYMTRACK_CHANNELS_MAX:
        raise ConfigError("channels must be in 1 .. SYMTRACK_CHANNELS_MAX")
    scheme, table = _symtrack_scheme(scheme)
    x_pitch, y_pitch, sym_pitch = (channels if p is None else _symsync_size(p, "pitch") for p in (x_pitch, y_pitch, sym_pitch))
    x = _arr(x, np.complex64)
    if x.ndim != 2 or x.shape[1] != x_pitch:
        raise ConfigError("the block is [steps, x_pitch]")
    n = x.shape[0]
    ycap = -(-n // max(k, 1)) + 8 if ycap is None else _symsync_size(ycap, "ycap")
    f = None if nco_frequency is None else _arr(nco_frequency, np.float32)
    p = None if nco_phase is None else _arr(nco_phase, np.float32)
    if any(a is not None and a.shape != (channels,) for a in (f, p)):
        raise ConfigError("one frequency and one phase per channel")
    y, sym = np.zeros((ycap, y_pitch), np.complex64), np.zeros((ycap, sym_pitch), np.uint8)
    ny, st = np.zeros(channels, np.uint32), np.zeros(channels, np.uint32)
    _check(lib.yagi_hip_symtrack_cccf_execute_host(
        channels, int(ftype), k, m, beta, scheme, None if table is None else _ptr(table), 0 if table is None else table.size,
        OscScheme(osc_scheme).value, npfb, eq_len, bw, int(SymTrackEq(strategy)), holdoff, None if f is None else _ptr(f),
        None if p is None else _ptr(p), _ptr(x), x_pitch, n, _ptr(y), y_pitch, _ptr(sym), sym_pitch, ycap, _ptr(ny), _ptr(st)))
    return y, sym, ny, st


MSEQUENCE_TILE = 8192    # YAGI_MSEQUENCE_TILE: symbols per workgroup of the generator kernel
BSEQUENCE_TILE = 4096    # YAGI_BSEQUENCE_TILE: outputs per workgroup of the correlator kernel
BSEQUENCE_NMAX = 8192    # YAGI_BSEQUENCE_NMAX: the longest BSequence, in bits


class MSequence(_Handle):
    """MSequence (src/sequence/msequence.rs:41-164): a shift-register sequence of period 2^m - 1 for a primitive g.  The
    per-bit calls run on the host; the block forms run sequence_kernels.hip and give the same bits, because advance() is
    linear over GF(2) and every lane jumps to its own start.  create_default is left out (yagi_hip.h): pass g."""
    _prefix = "yagi_hip_msequence_"

    def __init__(self, m, g, a=1):                            # new() :55-67; the state starts as a, not masked
        hd = C.c_void_p()
        _check(lib.yagi_hip_msequence_create(m, g, a, C.byref(hd)))
        self._h = hd

    @classmethod
    def from_genpoly(cls, g):                                 # create_genpoly() :69-77
        new = object.__new__(cls)
        hd = C.c_void_p()
        _check(lib.yagi_hip_msequence_create_genpoly(g, C.byref(hd)))
        new._h = hd
        return new

    def clone(self):                                          # derive(Clone)
        new = object.__new__(type(self))
        hd = C.c_void_p()
        _check(lib.yagi_hip_msequence_clone(self._h, C.byref(hd)))
        new._h = hd
        return new

    def _get(self, name):
        v = C.c_uint()
        _check(self._fn(name)(self._h, C.byref(v)))
        return v.value

    def advance(self):                                        # :116-122
        return self._get("advance")

    def generate_symbol(self, bps):                           # :124-131, MSB first, bps <= 32
        v = C.c_uint()
        _check(lib.yagi_hip_msequence_generate_symbol(self._h, bps, C.byref(v)))
        return v.value

    def set_state(self, a):                                   # :143-145, not masked
        _check(lib.yagi_hip_msequence_set_state(self._h, a))

    def get_state(self):
        return self._get("get_state")

    def get_genpoly(self):
        return self._get("get_genpoly")

    def get_genpoly_length(self):
        return self._get("get_genpoly_length")

    def get_length(self):
        return self._get("get_length")

    def measure_period(self):                                 # :147-158
        return self._get("measure_period")

    def skip(self, k):
        """extension: the state becomes what k calls of advance() would leave, in O(log k)"""
        _check(lib.yagi_hip_msequence_skip(self._h, k))

    def generate_bits_block(self, n, y=None):
        """n calls of advance(), one bit per byte"""
        y = _out(y, n, np.uint8)
        _check(lib.yagi_hip_msequence_generate_bits_block(self._h, n, _ptr(y)))
        return y

    def generate_symbols_block(self, bps, n, y=None):
        """y[i] = generate_symbol(bps), 1 <= bps <= 8: the layout Modem.modulate_block reads"""
        y = _out(y, n, np.uint8)
        _check(lib.yagi_hip_msequence_generate_symbols_block(self._h, bps, n, _ptr(y)))
        return y

    def generate_bits_block_devptr(self, n, y_dev):
        """y_dev: n bytes on the device; asynchronous on the object's stream"""
        _check(lib.yagi_hip_msequence_generate_bits_block_dev(self._h, n, _devptr(y_dev)))

    def generate_symbols_block_devptr(self, bps, n, y_dev):
        """y_dev: n bytes on the device; asynchronous on the object's stream"""
        _check(lib.yagi_hip_msequence_generate_symbols_block_dev(self._h, bps, n, _devptr(y_dev)))


class BSequence(_Handle):
    """BSequence (src/sequence/bsequence.rs:8-195): num_bits <= BSEQUENCE_NMAX bits, the newest at index 0.  The per-bit
    calls run on the host; push_correlate_block runs the sliding correlator of sequence_kernels.hip and equals the loop
    `for s in sym: push the bps bits of s, MSB first; rxy = ref.correlate(self)` bit for bit."""
    _prefix = "yagi_hip_bsequence_"

    def __init__(self, num_bits):                             # new() :16-30
        hd = C.c_void_p()
        _check(lib.yagi_hip_bsequence_create(num_bits, C.byref(hd)))
        self._h = hd

    @classmethod
    def from_msequence(cls, ms):                              # :81-88; ms advances by its length
        new = object.__new__(cls)
        hd = C.c_void_p()
        _check(lib.yagi_hip_bsequence_create_from_msequence(ms._h, C.byref(hd)))
        new._h = hd
        return new

    @classmethod
    def ccodes(cls, n):                                       # create_ccodes() :34-79 on two new sequences of n bits
        a, b = cls(n), cls(n)
        _check(lib.yagi_hip_bsequence_create_ccodes(a._h, b._h))
        return a, b

    def clone(self):                                          # derive(Clone)
        new = object.__new__(type(self))
        hd = C.c_void_p()
        _check(lib.yagi_hip_bsequence_clone(self._h, C.byref(hd)))
        new._h = hd
        return new

    def init(self, v):                                        # :95-108
        v = _arr(v, np.uint8)
        _check(lib.yagi_hip_bsequence_init(self._h, _ptr(v), v.size))

    def push(self, bit):                                      # :115-127
        _check(lib.yagi_hip_bsequence_push(self._h, int(bit) & 0xffffffff))

    def circshift(self):                                      # :130-134
        _check(lib.yagi_hip_bsequence_circshift(self._h))

    def correlate(self, other):                               # :137-150; self is the receiver
        r = C.c_int32()
        _check(lib.yagi_hip_bsequence_correlate(self._h, other._h, C.byref(r)))
        return r.value

    def add(self, other, out):                                # :153-163
        _check(lib.yagi_hip_bsequence_add(self._h, other._h, out._h))

    def mul(self, other, out):                                # :166-176
        _check(lib.yagi_hip_bsequence_mul(self._h, other._h, out._h))

    def accumulate(self):                                     # :179-181
        v = C.c_uint()
        _check(lib.yagi_hip_bsequence_accumulate(self._h, C.byref(v)))
        return v.value

    def index(self, i):                                       # :188-194
        v = C.c_uint()
        _check(lib.yagi_hip_bsequence_index(self._h, i, C.byref(v)))
        return v.value

    def get_length(self):
        v = C.c_size_t()
        _check(lib.yagi_hip_bsequence_get_length(self._h, C.byref(v)))
        return v.value

    def push_correlate_block(self, ref, sym, bps, rxy=True):
        """pushes the bps bits of every symbol (uint8, MSB first) and returns ref.correlate(self) after each as int32;
        rxy=None only pushes, rxy=<int32 array of len(sym)> is filled and returned"""
        sym = _arr(sym, np.uint8)
        if rxy is None:
            _check(lib.yagi_hip_bsequence_push_correlate_block(self._h, ref._h, _ptr(sym), sym.size, bps, None))
            return None
        y = _out(None if rxy is True else rxy, sym.size, np.int32)
        _check(lib.yagi_hip_bsequence_push_correlate_block(self._h, ref._h, _ptr(sym), sym.size, bps, _ptr(y)))
        return y

    def push_correlate_block_devptr(self, ref, sym_dev, n, bps, rxy_dev):
        """sym_dev: n bytes, rxy_dev: n int32 on the device (or None: only push), not overlapping (ConfigError);
        asynchronous on the object's stream"""
        _check(lib.yagi_hip_bsequence_push_correlate_block_dev(self._h, ref._h, _devptr(sym_dev), n, bps,
                                                               None if rxy_dev is None else _devptr(rxy_dev)))


class ModulationScheme(enum.IntEnum):
    """modem::ModulationScheme (src/modem/modem.rs:27-79), numbered as yagi_modem_scheme"""
    Unknown = 0
    Psk2 = 1
    Psk4 = 2
    Psk8 = 3
    Psk16 = 4
    Psk32 = 5
    Psk64 = 6
    Psk128 = 7
    Psk256 = 8
    Dpsk2 = 9
    Dpsk4 = 10
    Dpsk8 = 11
    Dpsk16 = 12
    Dpsk32 = 13
    Dpsk64 = 14
    Dpsk128 = 15
    Dpsk256 = 16
    Ask2 = 17
    Ask4 = 18
    Ask8 = 19
    Ask16 = 20
    Ask32 = 21
    Ask64 = 22
    Ask128 = 23
    Ask256 = 24
    Qam4 = 25
    Qam8 = 26
    Qam16 = 27
    Qam32 = 28
    Qam64 = 29
    Qam128 = 30
    Qam256 = 31
    Apsk4 = 32
    Apsk8 = 33
    Apsk16 = 34
    Apsk32 = 35
    Apsk64 = 36
    Apsk128 = 37
    Apsk256 = 38
    Bpsk = 39
    Qpsk = 40
    Ook = 41
    Sqam32 = 42
    Sqam128 = 43
    V29 = 44
    Arb16Opt = 45
    Arb32Opt = 46
    Arb64Opt = 47
    Arb128Opt = 48
    Arb256Opt = 49
    Arb64Vt = 50
    Arb64Ui = 51
    Pi4Dqpsk = 52
    Arb = 53


MAX_MOD_BITS_PER_SYMBOL = 8
SOFTBIT_0, SOFTBIT_ERASURE, SOFTBIT_1 = 0, 127, 255


def gray_encode(symbol_in):                                   # modem.rs:516-518
    symbol_in = int(symbol_in) & 0xFFFFFFFF
    return symbol_in ^ (symbol_in >> 1)


def gray_decode(symbol_in):                                   # modem.rs:521-537
    mask = symbol_out = int(symbol_in) & 0xFFFFFFFF
    for _ in range(0, MAX_MOD_BITS_PER_SYMBOL, 4):
        symbol_out ^= mask >> 1
        symbol_out ^= mask >> 2
        symbol_out ^= mask >> 3
        symbol_out ^= mask >> 4
        mask >>= 4
    return symbol_out


def pack_soft_bits(soft_bits, bps):                           # modem.rs:543-555
    if bps > MAX_MOD_BITS_PER_SYMBOL:
        raise ConfigError(f"pack_soft_bits(), bits/symbol exceeds maximum ({MAX_MOD_BITS_PER_SYMBOL})")
    s = 0
    for bit in list(soft_bits)[:bps]:
        s = (s << 1) | (1 if int(bit) > SOFTBIT_ERASURE else 0)
    return s


def unpack_soft_bits(sym_in, bps):                            # modem.rs:561-575
    if bps > MAX_MOD_BITS_PER_SYMBOL:
        raise ConfigError(f"unpack_soft_bits(), bits/symbol exceeds maximum ({MAX_MOD_BITS_PER_SYMBOL})")
    return np.array([SOFTBIT_1 if (int(sym_in) >> (bps - i - 1)) & 1 else SOFTBIT_0 for i in range(bps)], np.uint8)


class Modem(_Handle):
    """modem::Modem (src/modem/modem.rs): linear modulation and hard / soft demodulation for Psk*, Dpsk*, Ask*, Qam*,
    Bpsk, Qpsk, Ook and from_table (Arb); every other scheme is a ConfigError.  The per-sample calls run on the host;
    modulate_block, demodulate_block and demodulate_soft_block run modem_kernels.hip.  Symbols are uint8 arrays, soft
    bits uint8 with bps per symbol, most significant bit first.  Decisions, soft bits and x_hat equal the reference's
    f32 arithmetic; DPSK modulation keeps an exact running index instead of the reference's f32 phase
    (include/yagi_hip.h)."""
    _prefix = "yagi_hip_modem_"

    def __init__(self, scheme):                               # Modem::new :151-207
        hd = C.c_void_p()
        _check(self._fn("create")(int(scheme), C.byref(hd)))
        self._h = hd

    @classmethod
    def from_table(cls, table):                               # :209-216
        self = object.__new__(cls)
        t = _arr(table, np.complex64)
        hd = C.c_void_p()
        _check(self._fn("create_from_table")(_ptr(t), t.size, C.byref(hd)))
        self._h = hd
        return self

    def clone(self):
        new = object.__new__(type(self))
        h = C.c_void_p()
        _check(self._fn("clone")(self._h, C.byref(h)))
        new._h = h
        return new

    def _size(self, name):
        v = C.c_size_t()
        _check(self._fn(name)(self._h, C.byref(v)))
        return v.value

    def get_bps(self):                                        # :226-228
        return self._size("get_bps")

    def get_scheme(self):                                     # :230-232
        v = C.c_int()
        _check(self._fn("get_scheme")(self._h, C.byref(v)))
        return ModulationScheme(v.value)

    def get_constellation_size(self):                         # :234-236
        return self._size("get_constellation_size")

    def get_constellation(self):
        """extension: the M points, map[s] = modulate(s) (Dpsk: map[k] = polar(1, k 2 pi / M))"""
        m = np.empty(self.get_constellation_size(), np.complex64)
        _check(self._fn("get_constellation")(self._h, _ptr(m)))
        return m

    def get_neighbours(self):
        """extension: the soft demodulator's neighbour table as an (M, p) uint8 array; p = 0 where the scheme has none"""
        p = C.c_size_t()
        _check(self._fn("get_neighbours")(self._h, None, 0, C.byref(p)))
        t = np.zeros((self.get_constellation_size(), p.value), np.uint8)
        if t.size:
            _check(self._fn("get_neighbours")(self._h, _ptr(t), t.size, C.byref(p)))
        return t

    def modulate(self, symbol_in):                            # :243-253
        y = cf32()
        _check(self._fn("modulate")(self._h, int(symbol_in), C.byref(y)))
        return np.complex64(complex(y.re, y.im))

    def demodulate(self, x):                                  # :255-257
        s = C.c_uint()
        _check(self._fn("demodulate")(self._h, _byval(x, cf32), C.byref(s)))
        return s.value

    def demodulate_soft(self, x):                             # :259-271 -> (symbol, soft bits)
        s = C.c_uint()
        soft = np.zeros(MAX_MOD_BITS_PER_SYMBOL, np.uint8)
        _check(self._fn("demodulate_soft")(self._h, _byval(x, cf32), C.byref(s), _ptr(soft)))
        return s.value, soft[:self.get_bps()].copy()

    def get_demodulator_sample(self):                         # :273-275
        y = cf32()
        _check(self._fn("get_demodulator_sample")(self._h, C.byref(y)))
        return np.complex64(complex(y.re, y.im))

    def get_demodulator_phase_error(self):                    # :277-279
        v = C.c_float()
        _check(self._fn("get_demodulator_phase_error")(self._h, C.byref(v)))
        return np.float32(v.value)

    def get_demodulator_evm(self):                            # :281-283
        v = C.c_float()
        _check(self._fn("get_demodulator_evm")(self._h, C.byref(v)))
        return np.float32(v.value)

    def modulate_block(self, sym, y=None):
        """extension: y[i] = modulate(sym[i]); a symbol >= M anywhere is a RangeError and y is not written"""
        sym = _arr(sym, np.uint8)
        y = _out(y, sym.size, np.complex64)
        _check(self._fn("modulate_block")(self._h, _ptr(sym), sym.size, _ptr(y)))
        return y

    # The device-pointer forms (yagi_hip_modem_*_dev) are spelled *_devptr here: tests/test_gpu_dev_buffers.py owns the
    # list of the package's *_dev methods; these three are covered by tests/test_gpu_modem_dev_buffers.py instead.
    def modulate_block_devptr(self, sym_dev, n, y_dev):
        _check(self._fn("modulate_block_dev")(self._h, _devptr(sym_dev), n, _devptr(y_dev)))

    def demodulate_block(self, x, xhat=False):
        """extension: sym[i] = demodulate(x[i]); xhat=True also returns the re-modulated decisions"""
        x = _arr(x, np.complex64)
        sym = np.empty(x.size, np.uint8)
        xh = np.empty(x.size, np.complex64) if xhat else None
        _check(self._fn("demodulate_block")(self._h, _ptr(x), x.size, _ptr(sym), _ptr(xh) if xhat else None))
        return (sym, xh) if xhat else sym

    def demodulate_block_devptr(self, x_dev, n, sym_dev, xhat_dev=None):
        _check(self._fn("demodulate_block_dev")(self._h, _devptr(x_dev), n, _devptr(sym_dev),
                                                None if xhat_dev is None else _devptr(xhat_dev)))

    def demodulate_soft_block(self, x):
        """extension: (sym, soft) with soft an (n, bps) uint8 array, most significant bit first"""
        x = _arr(x, np.complex64)
        bps = self.get_bps()
        sym = np.empty(x.size, np.uint8)
        soft = np.empty((x.size, bps), np.uint8)
        _check(self._fn("demodulate_soft_block")(self._h, _ptr(x), x.size, _ptr(sym), _ptr(soft)))
        return sym, soft

    def demodulate_soft_block_devptr(self, x_dev, n, sym_dev, soft_dev):
        _check(self._fn("demodulate_soft_block_dev")(self._h, _devptr(x_dev), n, _devptr(sym_dev), _devptr(soft_dev)))


class SymStream(_Handle):
    """framing::SymStream (src/framing/symstream.rs), symstreamcf: symbol source -> Modem -> x gain ->
    FirInterpolationFilter<Complex<f32>, f32> of k branches, written in any number of samples per call.  The symbol
    source is a private copy of an MSequence taken at creation (the reference draws from an RNG nobody can reproduce), so
    every output word equals MSequence.generate_symbols_block -> Modem.modulate_block -> x gain per component ->
    FirInterpolationFilter("crcf").execute_block, and a clone writes the stream its original writes.  A block call is one
    launch of symstream_kernels.hip (is_fused) except for Dpsk* schemes and shapes the fused kernel does not serve, which
    run the three objects' launchers; the words are the same (include/yagi_hip.h)."""
    _prefix = "yagi_hip_symstreamcf_"

    def __init__(self, ftype, k, m, beta, scheme, source):    # new_linear :24-59 plus the source
        hd = C.c_void_p()
        _check(self._fn("create_linear")(int(ftype), k, m, beta, int(scheme), source._h, C.byref(hd)))
        self._h = hd

    @classmethod
    def from_taps(cls, k, h, scheme, source, h_len=None):
        """extension: externally designed taps, read as FirInterpolationFilter("crcf", k, h, h_len) reads them"""
        self = object.__new__(cls)
        h = _arr(h, np.float32)
        hd = C.c_void_p()
        _check(self._fn("create_taps")(k, _ptr(h), h.size if h_len is None else h_len, int(scheme), source._h, C.byref(hd)))
        self._h = hd
        return self

    def clone(self):                                          # derive(Clone)
        new = object.__new__(type(self))
        hd = C.c_void_p()
        _check(self._fn("clone")(self._h, C.byref(hd)))
        new._h = hd
        return new

    def _get(self, name, ctype):
        v = ctype()
        _check(self._fn(name)(self._h, C.byref(v)))
        return v.value

    def get_ftype(self):                                      # :67-69
        return FirFilterShape(self._get("get_ftype", C.c_int))

    def get_k(self):                                          # :71-73
        return self._get("get_k", C.c_size_t)

    def get_m(self):                                          # :75-77; from_taps: (ceil(h_len / k) - 1) // 2
        return self._get("get_m", C.c_size_t)

    def get_beta(self):                                       # :79-81
        return np.float32(self._get("get_beta", C.c_float))

    def set_scheme(self, scheme):                             # :83-86 a new modem: Dpsk index 0
        _check(self._fn("set_scheme")(self._h, int(scheme)))

    def set_modem(self, modem):
        """extension: a copy of `modem` (a Modem, e.g. Modem.from_table) at its current state becomes the modulator"""
        _check(self._fn("set_modem")(self._h, modem._h))

    def get_scheme(self):                                     # :88-90
        return ModulationScheme(self._get("get_scheme", C.c_int))

    def set_gain(self, gain):                                 # :92-94
        _check(self._fn("set_gain")(self._h, gain))

    def get_gain(self):                                       # :96-98
        return np.float32(self._get("get_gain", C.c_float))

    def get_delay(self):                                      # :100-102
        return self._get("get_delay", C.c_size_t)

    def get_buf_index(self):
        """extension: t mod k for the next sample t"""
        return self._get("get_buf_index", C.c_size_t)

    def is_fused(self):
        """True where a block call of the object as it stands is one launch of the fused kernel"""
        return bool(self._get("is_fused", C.c_int))

    def source_set_state(self, a):
        """extension: the source's state word (not masked, as MSequence.set_state)"""
        _check(self._fn("source_set_state")(self._h, a))

    def source_get_state(self):
        return self._get("source_get_state", C.c_uint)

    def write_samples(self, n, y=None):                       # :111-121
        """the next n samples of the stream; n may start and end inside a symbol"""
        y = _out(y, n, np.complex64)
        _check(self._fn("write_samples")(self._h, _ptr(y), n))
        return y

    def modulate_symbols(self, sym, y=None):
        """extension: the caller's symbols instead of the source, k samples each.  A symbol >= M is a RangeError and
        nothing moves; off a symbol boundary (get_buf_index() != 0) it is a ModeError"""
        sym = _arr(sym, np.uint8)
        y = _out(y, sym.size * self.get_k(), np.complex64)
        _check(self._fn("modulate_symbols")(self._h, _ptr(sym), sym.size, _ptr(y)))
        return y

    # The device-pointer forms are spelled *_devptr, as Modem's and Autocorr's: tests/test_gpu_dev_buffers.py owns the
    # list of the package's *_dev methods; these two are covered by tests/test_gpu_symstream_dev_buffers.py instead.
    def write_samples_devptr(self, y_dev, n):
        """y_dev: n samples on the device; asynchronous on the object's stream"""
        _check(self._fn("write_samples_dev")(self._h, _devptr(y_dev), n))

    def modulate_symbols_devptr(self, sym_dev, nsym, y_dev):
        """sym_dev: nsym bytes, y_dev: nsym k samples on the device; they must not overlap (ConfigError)"""
        _check(self._fn("modulate_symbols_dev")(self._h, _devptr(sym_dev), nsym, _devptr(y_dev)))


SymStreamRPlan = collections.namedtuple(
    "SymStreamRPlan", "interp tile max_wg_tiles wg_tiles step phase_next rate rate_arb stages lds q need outputs_arb "
                      "outputs leftover")


def plan_symstreamr(bw, m, n, p0=0):
    """yagi_hip_plan_symstreamr: what a SymStreamR(bw, m) call that misses n outputs does with its Resamp at phase p0
    (no device needed): tile = arbitrary-stage outputs per tile of the fused kernel, wg_tiles of them per workgroup,
    need = samples of the SymStream pushed, leftover = outputs the call leaves for the next one"""
    p = _capi.symstreamr_plan()
    _check(lib.yagi_hip_plan_symstreamr(bw, m, n, p0, C.byref(p)))
    return SymStreamRPlan(p.interp, p.tile, p.max_wg_tiles, p.wg_tiles, p.step, p.phase_next, np.float32(p.rate),
                          np.float32(p.rate_arb), p.stages, p.lds, p.q, p.need, p.outputs_arb, p.outputs, p.leftover)


class SymStreamR(_Handle):
    """framing::SymStreamR (src/framing/symstreamr.rs), symstreamrcf: a SymStream at two samples per symbol pushed one
    sample at a time through MsResamp("crcf", 0.5 / bw, 60), written in any number of samples per call; bw in
    [0.001, 1] is the occupied bandwidth.  Every output word equals SymStream.write_samples -> MsResamp.execute fed
    exactly the samples the reference would have pushed, at any cut of the stream into calls.  A call is one launch of
    symstreamr_kernels.hip (SymStream and the arbitrary Resamp, no sample read) plus the half-band chain's launch where
    bw < 0.25 (is_fused); Dpsk* schemes and shapes the fused kernel does not serve run the two objects' device forms.
    The words are the same (include/yagi_hip.h)."""
    _prefix = "yagi_hip_symstreamrcf_"

    def __init__(self, ftype, bw, m, beta, scheme, source):   # new_linear :23-53 plus the source
        hd = C.c_void_p()
        _check(self._fn("create_linear")(int(ftype), bw, m, beta, int(scheme), source._h, C.byref(hd)))
        self._h = hd

    clone = SymStream.clone
    _get = SymStream._get
    get_ftype = SymStream.get_ftype                           # :62-64
    get_m = SymStream.get_m                                   # :70-72
    get_beta = SymStream.get_beta                             # :74-76
    set_scheme = SymStream.set_scheme                         # :78-80
    set_modem = SymStream.set_modem
    get_scheme = SymStream.get_scheme                         # :82-84
    set_gain = SymStream.set_gain                             # :86-88
    get_gain = SymStream.get_gain                             # :90-92
    is_fused = SymStream.is_fused
    source_set_state = SymStream.source_set_state
    source_get_state = SymStream.source_get_state
    write_samples = SymStream.write_samples                   # :118-128
    write_samples_devptr = SymStream.write_samples_devptr

    def get_bw(self):                                         # :66-68: 1 / (rate k), not the argument echoed back
        return np.float32(self._get("get_bw", C.c_float))

    def get_delay(self):                                      # :94-99
        return np.float32(self._get("get_delay", C.c_float))

    def get_pending(self):
        """extension: outputs of the last pushed sample that no call has taken yet"""
        return self._get("get_pending", C.c_size_t)

    def get_params(self):
        """(type, half-band stages, rate of the arbitrary resampler) of the MsResamp, as MsResamp.get_params"""
        interp, ns, ra = C.c_int(), C.c_size_t(), C.c_float()
        _check(self._fn("get_params")(self._h, C.byref(interp), C.byref(ns), C.byref(ra)))
        return interp.value, ns.value, np.float32(ra.value)


class MsResamp(_FirBase):
    """MsResamp<T,Coeff> (src/filter/resampler/msresamp.rs): any rate > 0 as MsResamp2 half-band stages (Kaiser
    prototypes, see MsResamp2) around a Resamp for the remaining factor in [0.5, 2]."""
    DECIM, INTERP = 0, 1

    def __init__(self, kind, rate, as_=60.0):                 # new(rate, as_) :28-79
        self._init_kind(kind)
        self._prefix = f"yagi_hip_msresamp_{kind}_"
        hd = C.c_void_p()
        _check(self._fn("create")(rate, as_, C.byref(hd)))
        self._h = hd

    def set_scale(self, scale):
        raise ConfigError("MsResamp has no scale (msresamp.rs)")

    get_scale = set_scale

    def get_rate(self):                                       # :105-107
        r = C.c_float()
        _check(self._fn("get_rate")(self._h, C.byref(r)))
        return np.float32(r.value)

    def get_delay(self):                                      # :87-103
        d = C.c_float()
        _check(self._fn("get_delay")(self._h, C.byref(d)))
        return np.float32(d.value)

    def get_params(self):
        """(type, number of half-band stages, arbitrary rate)"""
        it, ns, ra = C.c_int(), C.c_size_t(), C.c_float()
        _check(self._fn("get_params")(self._h, C.byref(it), C.byref(ns), C.byref(ra)))
        return it.value, ns.value, np.float32(ra.value)

    def get_num_output(self, num_input):                      # :109-120
        n = C.c_size_t()
        _check(self._fn("get_num_output")(self._h, num_input, C.byref(n)))
        return n.value

    def execute(self, x):                                     # :122-176
        x = _arr(x, self.T)
        y = np.empty(max(self.get_num_output(x.size), 1), self.T)
        nw = C.c_size_t()
        _check(self._fn("execute")(self._h, _ptr(x), x.size, _ptr(y), y.size, C.byref(nw)))
        return y[: nw.value]

    def execute_dev(self, x_dev, nx, y_dev, ny_cap):
        """nx device samples in; y_dev holds ny_cap samples (>= get_num_output(nx)); returns the outputs written"""
        nw = C.c_size_t()
        _check(self._fn("execute_dev")(self._h, _devptr(x_dev), nx, _devptr(y_dev), ny_cap, C.byref(nw)))
        return nw.value


class FftFilt(_FirBase):
    """FftFilt<T,Coeff> (src/filter/fftfilt.rs): overlap-add fast convolution, block n, FFT size 2n."""

    def __init__(self, kind, h, n):                          # create(h, n) :46-84
        self._init_kind(kind)
        self._prefix = f"yagi_hip_fftfilt_{kind}_"
        h = _arr(h, self.Cdt)
        hd = C.c_void_p()
        _check(self._fn("create")(_ptr(h), h.size, n, C.byref(hd)))
        self._h = hd
        self.n = n

    create = classmethod(lambda cls, kind, h, n: cls(kind, h, n))

    def get_length(self):                                    # :140-142
        n = C.c_size_t()
        _check(self._fn("get_length")(self._h, C.byref(n)))
        return n.value

    def execute(self, x, y=None):                            # :103-138
        x = _arr(x, self.T)
        y = _out(y, self.n, self.T)
        _check(self._fn("execute")(self._h, _ptr(x), x.size, _ptr(y), y.size))
        return y

    def execute_blocks(self, x):
        """consecutive execute() calls over len(x)/n blocks as one device batch"""
        x = _arr(x, self.T)
        if x.size % self.n:
            raise ConfigError("input must hold a whole number of blocks")
        y = np.empty_like(x)
        _check(self._fn("execute_blocks")(self._h, _ptr(x), x.size // self.n, _ptr(y)))
        return y

    def execute_blocks_dev(self, x_dev, nblocks, y_dev):
        _check(self._fn("execute_blocks_dev")(self._h, _devptr(x_dev), nblocks, _devptr(y_dev)))


# ---- Fft (src/fft/mod.rs:33-69) ---------------------------------------------------------------
class FftPath(enum.IntEnum):
    """yagi_hip_fft_path: the form run / run_batch_dev take for a plan"""
    one_kernel = 0
    bluestein_fused = 1
    bluestein = 2
    two_pass = 3
    tile256 = 4
    mixed_two_pass = 5
    four_step = 6


FftInfo = collections.namedtuple("FftInfo", "path batch_chunk n1 n2 bluestein_m nested")
FftNestedInfo = collections.namedtuple("FftNestedInfo", "n path batch_chunk")


class Fft(_Handle):
    _prefix = "yagi_hip_fft_"

    def __init__(self, n, direction):
        hd = C.c_void_p()
        _check(lib.yagi_hip_fft_create(n, Direction(direction).value, C.byref(hd)))
        self._h = hd
        self.n = n
        self.direction = Direction(direction)

    def run(self, input, output=None):                       # fft/mod.rs:45-48
        x = _arr(input, np.complex64)
        y = _out(output, self.n, np.complex64)
        _check(lib.yagi_hip_fft_run(self._h, _ptr(x), x.size, _ptr(y), y.size))
        return y

    def describe(self):
        """which form this plan takes and how it cuts a batch into passes over its scratch (yagi_hip_fft_describe);
        batch_chunk = 0: one launch whatever the batch; nested: the plan the sub-transforms go to, or None"""
        i = _capi.fft_info()
        _check(lib.yagi_hip_fft_describe(self._h, C.byref(i)))
        nested = FftNestedInfo(i.nested_n, FftPath(i.nested_path), i.nested_batch_chunk) if i.nested_n else None
        return FftInfo(FftPath(i.path), i.batch_chunk, i.n1, i.n2, i.bluestein_m, nested)

    def run_batch_dev(self, in_dev, out_dev, batch, stream=None):
        _check(lib.yagi_hip_fft_run_batch_dev(self._h, _devptr(in_dev), _devptr(out_dev), batch, stream))

    def run_batch(self, x):
        """host convenience: x holds batch*n samples"""
        x = _arr(x, np.complex64)
        if x.size % self.n:
            raise ConfigError("batch input must hold a whole number of transforms")
        dx = DeviceArray.from_numpy(x)
        dy = DeviceArray(x.size, np.complex64)
        self.run_batch_dev(dx, dy, x.size // self.n)
        synchronize()
        return dy.to_numpy().reshape(-1, self.n)

    def shift(self, buf, n=None):                            # fft/mod.rs:50-57 (in place)
        if not (isinstance(buf, np.ndarray) and buf.dtype == np.complex64 and buf.flags.c_contiguous):
            raise ConfigError("shift works in place on a contiguous complex64 array")
        _check(lib.yagi_hip_fft_shift(_ptr(buf), buf.size if n is None else n))
        return buf

    def set_stream(self, stream):
        raise ModeError("Fft plans take the stream per call (run_batch_dev)")

    def reset(self):
        pass


def fft_run(input, direction):                               # fft/mod.rs:66-69
    x = _arr(input, np.complex64)
    y = np.empty_like(x)
    _check(lib.yagi_hip_fft_run_oneshot(_ptr(x), _ptr(y), x.size, Direction(direction).value))
    return y


class WindowType(enum.IntEnum):
    """math::WindowType (src/math/windows.rs:7-18)"""
    Unknown = 0
    Hamming = 1
    Hann = 2
    BlackmanHarris = 3
    BlackmanHarris7 = 4
    Kaiser = 5
    FlatTop = 6
    Triangular = 7
    RcosTaper = 8
    Kbd = 9


class Spgram(_Handle):
    """fft::Spgram<T> (src/fft/spgram.rs); T = Complex32 (dtype complex64) or f32 (float32)."""

    def __init__(self, nfft, wtype, window_len, delay, dtype=np.complex64):      # new() :49-125
        self._set_type(dtype)
        hd = C.c_void_p()
        _check(self._fn("create")(nfft, int(wtype), window_len, delay, C.byref(hd)))
        self._h = hd

    def _set_type(self, dtype):
        self.T = np.dtype(dtype).type
        if self.T not in (np.complex64, np.float32):
            raise ConfigError("Spgram sample type must be complex64 or float32")
        self._prefix = "yagi_hip_spgramcf_" if self.T is np.complex64 else "yagi_hip_spgramf_"
        self._Tc = cf32 if self.T is np.complex64 else C.c_float

    @classmethod
    def default(cls, nfft, dtype=np.complex64):                                  # :128-131
        self = object.__new__(cls)
        self._set_type(dtype)
        hd = C.c_void_p()
        _check(self._fn("create_default")(nfft, C.byref(hd)))
        self._h = hd
        return self

    def clear(self):
        _check(self._fn("clear")(self._h))

    def set_alpha(self, alpha):
        _check(self._fn("set_alpha")(self._h, alpha))

    def get_alpha(self):
        a = C.c_float()
        _check(self._fn("get_alpha")(self._h, C.byref(a)))
        return a.value

    def set_freq(self, f):
        _check(self._fn("set_freq")(self._h, f))

    def set_rate(self, r):
        _check(self._fn("set_rate")(self._h, r))

    def _params(self):
        a, b, c, d = C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_int()
        _check(self._fn("get_params")(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return a.value, b.value, c.value, WindowType(d.value)

    def get_nfft(self):
        return self._params()[0]

    def get_window_len(self):
        return self._params()[1]

    def get_delay(self):
        return self._params()[2]

    def get_wtype(self):
        return self._params()[3]

    def _counters(self):
        v = [C.c_uint64() for _ in range(4)]
        _check(self._fn("get_counters")(self._h, *[C.byref(t) for t in v]))
        return [t.value for t in v]

    def get_num_samples(self):
        return self._counters()[0]

    def get_num_samples_total(self):
        return self._counters()[1]

    def get_num_transforms(self):
        return self._counters()[2]

    def get_num_transforms_total(self):
        return self._counters()[3]

    def push(self, x):                                                           # :237-251
        _check(self._fn("push")(self._h, _byval(x, self._Tc)))

    def write(self, x):                                                          # :254-258
        x = _arr(x, self.T)
        _check(self._fn("write")(self._h, _ptr(x), x.size))

    def write_dev(self, x_dev, n):
        _check(self._fn("write_dev")(self._h, _devptr(x_dev), n))

    def get_psd_mag(self):                                                       # :292-304
        out = np.empty(self.get_nfft(), np.float32)
        _check(self._fn("get_psd_mag")(self._h, _ptr(out), out.size))
        return out

    def get_psd(self):                                                           # :308-316
        out = np.empty(self.get_nfft(), np.float32)
        with np.errstate(divide="ignore"):
            _check(self._fn("get_psd")(self._h, _ptr(out), out.size))
        return out

    @classmethod
    def estimate_psd(cls, nfft, x, dtype=np.complex64):                          # :319-330
        T = np.dtype(dtype).type
        x = _arr(x, T)
        out = np.empty(nfft, np.float32)
        fn = lib.yagi_hip_spgramcf_estimate_psd if T is np.complex64 else lib.yagi_hip_spgramf_estimate_psd
        _check(fn(nfft, _ptr(x), x.size, _ptr(out)))
        return out


# ---- headline stream ----------------------------------------------------------------------------
class FirFftStream(_Handle):
    """firfilt_crcf.execute_block -> consecutive nfft frames -> Fft::run(Forward), fused."""
    _prefix = "yagi_hip_firfft_crcf_"

    def __init__(self, h, nfft=4096):
        h = _arr(h, np.float32)
        hd = C.c_void_p()
        _check(lib.yagi_hip_firfft_crcf_create(_ptr(h), h.size, nfft, C.byref(hd)))
        self._h = hd
        self.nfft = nfft

    def set_scale(self, scale):
        _check(lib.yagi_hip_firfft_crcf_set_scale(self._h, scale))

    def set_variant(self, v):
        _check(lib.yagi_hip_firfft_crcf_set_variant(self._h, v))

    def execute(self, x):
        x = _arr(x, np.complex64)
        if x.size % self.nfft:
            raise ConfigError("input must hold a whole number of frames")
        nf = x.size // self.nfft
        y = np.empty(x.size, np.complex64)
        _check(lib.yagi_hip_firfft_crcf_execute(self._h, _ptr(x), nf, _ptr(y)))
        return y.reshape(nf, self.nfft)

    def execute_dev(self, x_dev, nframes, spectra_dev):
        _check(lib.yagi_hip_firfft_crcf_execute_dev(self._h, _devptr(x_dev), nframes, _devptr(spectra_dev)))

    def set_pipeline(self, on=True):
        """pipelined block calls: consecutive execute_dev calls overlap on two streams owned by the object;
        their outputs are ordered on the object's stream only after join() (include/yagi_hip.h)"""
        _check(lib.yagi_hip_firfft_crcf_set_pipeline(self._h, 1 if on else 0))

    def join(self):
        _check(lib.yagi_hip_firfft_crcf_join(self._h))


# ---- channelizers (absent from the reference; see include/yagi_hip.h) ---------------------------
class FirPfbCh(_Handle):
    _prefix = "yagi_hip_firpfbch_crcf_"

    def __init__(self, M, p, h):
        h = _arr(h, np.float32)
        if h.size < M * p:
            raise ConfigError("prototype shorter than M*p")
        hd = C.c_void_p()
        _check(lib.yagi_hip_firpfbch_crcf_create(M, p, _ptr(h), C.byref(hd)))
        self._h, self.M, self.p = hd, M, p

    @classmethod
    def new_kaiser(cls, M, m, as_):
        self = object.__new__(cls)
        hd = C.c_void_p()
        _check(lib.yagi_hip_firpfbch_crcf_create_kaiser(M, m, as_, C.byref(hd)))
        self._h, self.M, self.p = hd, M, 2 * m
        return self

    def analyzer_execute(self, x):
        x = _arr(x, np.complex64)
        if x.size % self.M:
            raise ConfigError("input must hold a whole number of M-sample frames")
        nf = x.size // self.M
        y = np.empty(x.size, np.complex64)
        _check(lib.yagi_hip_firpfbch_crcf_analyzer_execute(self._h, _ptr(x), nf, _ptr(y)))
        return y.reshape(nf, self.M)

    def analyzer_execute_dev(self, x_dev, nframes, y_dev):
        _check(lib.yagi_hip_firpfbch_crcf_analyzer_execute_dev(self._h, _devptr(x_dev), nframes, _devptr(y_dev)))

    def synthesizer_execute(self, X):
        """X: frames of M channel samples ([nframes, M] or flat) -> nframes*M output samples"""
        X = _arr(X, np.complex64)
        if X.size % self.M:
            raise ConfigError("input must hold a whole number of M-channel frames")
        nf = X.size // self.M
        y = np.empty(X.size, np.complex64)
        _check(lib.yagi_hip_firpfbch_crcf_synthesizer_execute(self._h, _ptr(X), nf, _ptr(y)))
        return y

    def synthesizer_execute_dev(self, x_dev, nframes, y_dev):
        _check(lib.yagi_hip_firpfbch_crcf_synthesizer_execute_dev(self._h, _devptr(x_dev), nframes, _devptr(y_dev)))


class FirPfbCh2(_Handle):
    _prefix = "yagi_hip_firpfbch2_crcf_"

    def __init__(self, M, m, h):
        h = _arr(h, np.float32)
        if h.size < 2 * M * m:
            raise ConfigError("prototype shorter than 2*M*m")
        hd = C.c_void_p()
        _check(lib.yagi_hip_firpfbch2_crcf_create(M, m, _ptr(h), C.byref(hd)))
        self._h, self.M, self.m = hd, M, m

    @classmethod
    def new_kaiser(cls, M, m, as_):
        self = object.__new__(cls)
        hd = C.c_void_p()
        _check(lib.yagi_hip_firpfbch2_crcf_create_kaiser(M, m, as_, C.byref(hd)))
        self._h, self.M, self.m = hd, M, m
        return self

    @classmethod
    def new_kaiser_synthesizer(cls, M, m, as_):
        """prototype of the matching synthesizer: kaiser(2Mm+1, 0.5/M, as_) scaled to sum M"""
        self = object.__new__(cls)
        hd = C.c_void_p()
        _check(lib.yagi_hip_firpfbch2_crcf_create_kaiser_synthesizer(M, m, as_, C.byref(hd)))
        self._h, self.M, self.m = hd, M, m
        return self

    def synthesizer_execute(self, X):
        """X: steps of M channel samples ([nsteps, M] or flat) -> nsteps*M/2 output samples"""
        X = _arr(X, np.complex64)
        if X.size % self.M:
            raise ConfigError("input must hold a whole number of M-channel steps")
        ns = X.size // self.M
        y = np.empty(ns * (self.M // 2), np.complex64)
        _check(lib.yagi_hip_firpfbch2_crcf_synthesizer_execute(self._h, _ptr(X), ns, _ptr(y)))
        return y

    def synthesizer_execute_dev(self, x_dev, nsteps, y_dev):
        _check(lib.yagi_hip_firpfbch2_crcf_synthesizer_execute_dev(self._h, _devptr(x_dev), nsteps, _devptr(y_dev)))

    def analyzer_execute(self, x):
        x = _arr(x, np.complex64)
        M2 = self.M // 2
        if x.size % M2:
            raise ConfigError("input must hold a whole number of M/2-sample steps")
        ns = x.size // M2
        y = np.empty(ns * self.M, np.complex64)
        _check(lib.yagi_hip_firpfbch2_crcf_analyzer_execute(self._h, _ptr(x), ns, _ptr(y)))
        return y.reshape(ns, self.M)

    def analyzer_execute_dev(self, x_dev, nsteps, y_dev):
        _check(lib.yagi_hip_firpfbch2_crcf_analyzer_execute_dev(self._h, _devptr(x_dev), nsteps, _devptr(y_dev)))

    def analyzer_execute_shard_dev(self, x_dev, nsteps, rank, nranks, yshard_dev):
        _check(lib.yagi_hip_firpfbch2_crcf_analyzer_execute_shard_dev(
            self._h, _devptr(x_dev), nsteps, rank, nranks, _devptr(yshard_dev)))

    def analyzer_execute_sharded_dev(self, x_dev, nsteps, comm, y_dev, nchunks=0):
        """sub-bands sharded over the ranks of `comm` (yagi_amd.dist.Comm): shard kernel -> RCCL all-gather ->
        assemble, chunked so the exchange overlaps the next chunk's kernel; y_dev = [nsteps][M] on every rank"""
        _check(lib.yagi_hip_firpfbch2_crcf_analyzer_execute_sharded_dev(
            self._h, _devptr(x_dev), nsteps, comm._h, nchunks, _devptr(y_dev)))

    @staticmethod
    def assemble_dev(gathered_dev, nsteps, M, nranks, y_dev, stream=None):
        _check(lib.yagi_hip_firpfbch2_crcf_assemble_dev(_devptr(gathered_dev), nsteps, M, nranks, _devptr(y_dev), stream))


class FirPfbChr(_Handle):
    """Rational-oversampling channelizer: M channels spaced 1/M, each output once per P input samples (1 <= P <= M,
    oversampling M/P), prototype h[0 : 2*M*m].  FirPfbCh is P = M, FirPfbCh2 is P = M/2 (include/yagi_hip.h has the
    closed forms).  The analyzer takes P samples per step and gives M channel values; the synthesizer takes M channel
    values per step and gives P samples.  Steps are counted from the start of the stream and carried across calls."""
    _prefix = "yagi_hip_firpfbchr_crcf_"

    def __init__(self, M, P, m, h):
        h = _arr(h, np.float32)
        if M >= 1 and m >= 1 and h.size < 2 * M * m:
            raise ConfigError("prototype shorter than 2*M*m")
        hd = C.c_void_p()
        _check(lib.yagi_hip_firpfbchr_crcf_create(M, P, m, _ptr(h), C.byref(hd)))
        self._h, self.M, self.P, self.m = hd, M, P, m

    @classmethod
    def _designed(cls, fn, M, P, m, as_):
        self = object.__new__(cls)
        hd = C.c_void_p()
        _check(fn(M, P, m, as_, C.byref(hd)))
        self._h, self.M, self.P, self.m = hd, M, P, m
        return self

    @classmethod
    def new_kaiser(cls, M, P, m, as_):
        """analyzer prototype kaiser(2Mm+1, 0.5/P, as_) scaled to sum M"""
        return cls._designed(lib.yagi_hip_firpfbchr_crcf_create_kaiser, M, P, m, as_)

    @classmethod
    def new_kaiser_synthesizer(cls, M, P, m, as_):
        """prototype of the matching synthesizer: kaiser(2Mm+1, 0.5/M, as_) scaled to sum M; new_kaiser's analyzer followed
        by this synthesizer returns the input delayed by 2Mm - P + 1 samples"""
        return cls._designed(lib.yagi_hip_firpfbchr_crcf_create_kaiser_synthesizer, M, P, m, as_)

    def set_kernel(self, choice):
        """analyzer: 0 auto, 1 the general kernel, 2 the column kernel (M in {64, 128, 256}, P a multiple of M/8,
        2m <= 16; a ConfigError elsewhere)"""
        _check(lib.yagi_hip_firpfbchr_crcf_set_kernel(self._h, choice))

    def get_last_kernel(self):
        """1 (general) or 2 (column): what the last analyzer call ran; 0 before the first"""
        k = C.c_int()
        _check(lib.yagi_hip_firpfbchr_crcf_get_last_kernel(self._h, C.byref(k)))
        return k.value

    def analyzer_execute(self, x):
        x = _arr(x, np.complex64)
        if x.size % self.P:
            raise ConfigError("input must hold a whole number of P-sample steps")
        ns = x.size // self.P
        y = np.empty(ns * self.M, np.complex64)
        _check(lib.yagi_hip_firpfbchr_crcf_analyzer_execute(self._h, _ptr(x), ns, _ptr(y)))
        return y.reshape(ns, self.M)

    def analyzer_execute_devptr(self, x_dev, nsteps, y_dev):
        """x_dev: nsteps*P complex64 on the device, y_dev: nsteps*M, not overlapping (ConfigError), 8-byte aligned;
        asynchronous on the object's stream (the C ABI's analyzer_execute_dev; named as Ddc.execute_block_devptr is)"""
        _check(lib.yagi_hip_firpfbchr_crcf_analyzer_execute_dev(self._h, _devptr(x_dev), nsteps, _devptr(y_dev)))

    def synthesizer_execute(self, X):
        """X: steps of M channel samples ([nsteps, M] or flat) -> nsteps*P output samples"""
        X = _arr(X, np.complex64)
        if X.size % self.M:
            raise ConfigError("input must hold a whole number of M-channel steps")
        ns = X.size // self.M
        y = np.empty(ns * self.P, np.complex64)
        _check(lib.yagi_hip_firpfbchr_crcf_synthesizer_execute(self._h, _ptr(X), ns, _ptr(y)))
        return y

    def synthesizer_execute_devptr(self, x_dev, nsteps, y_dev):
        _check(lib.yagi_hip_firpfbchr_crcf_synthesizer_execute_dev(self._h, _devptr(x_dev), nsteps, _devptr(y_dev)))
