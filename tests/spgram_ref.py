"""fft::Spgram in f64 from index arithmetic (a helper, not a conftest): where every transform of a sequence of calls
lies in the stream, what weight the recurrence gives it in the final estimate, and the estimate itself.

Operations (tuples): ("write", n) -- also spelled ("write_dev", n) and ("push", n), which differ only in how a test drives
the device object -- ("clear",), ("reset",), ("set_alpha", a).  The writes consume one stream x in order.

  positions   the timer is `delay` after reset and after clear, so transform k (k = 1, 2, ..) since then ends on sample
              c + k delay - 1, c = samples written before that clear.  A frame is the wlen newest samples times the
              taper, zero padded to nfft; the buffer survives clear and is zeroed by reset, so samples before the last
              reset (the `origin` of a frame) and before the stream read as zero.
  recurrence  psd = |X|^2 for the first transform after a clear, then psd = gamma psd + alpha |X|^2 with the object's
              f32 alpha and gamma = f32(1 - f32(alpha)); accumulate mode is alpha = gamma = 1.  In closed form frame j
              carries the weight c_j prod_{i > j} gamma_i, c_j = 1 for a first frame and alpha_j otherwise.
  output      get_psd_mag: bins rotated by nfft / 2, max(psd, f32(1e-12)) * scale, scale = 1 / max(1, transforms since
              the clear) in accumulate mode and 0 otherwise (the reference's quirk), in f64.

Only frames that hold a non-zero sample are transformed: an all-zero frame adds nothing (and is the multiply by gamma
the weights already contain), so a stream of a few bursts costs a few transforms whatever its length.  model_f32 is the
same pipeline with every stage rounded to f32 in the reference's order (oracle.Spgram statement by statement): the
yardstick for the device's rounding error."""
import collections

import numpy as np

Geometry = collections.namedtuple("Geometry", "nfft wlen delay wtype")
Schedule = collections.namedtuple(
    "Schedule", "end origin alpha gamma first call live0 accumulate nsamples num_samples num_samples_total "
                "num_transforms num_transforms_total call_frames")
PSD_MIN = np.float32(1e-12)
WRITES = ("write", "write_dev", "push")


def taper(oracle, g):
    """the f32 taper, normalised as oracle.Spgram does (window_fn, unit energy summed in f32)"""
    return np.asarray(oracle.Spgram(g.nfft, int(g.wtype), g.wlen, g.delay).w, np.float32)


def schedule(g, ops):
    """every transform of the calls: last sample index, origin, f32 alpha / gamma (as f64), first-after-clear flag and
    the index of the op that ran it; live0 = first transform since the last clear; call_frames = (op index, first
    transform, count) per writing op"""
    pos = origin = ns = 0
    timer, nt, ntt, nst = g.delay, 0, 0, 0
    acc, a32, g32 = True, np.float32(1.0), np.float32(1.0)
    live0 = at_reset = 0
    end, org, al, ga, fi, ca, calls = [], [], [], [], [], [], []
    for i, op in enumerate(ops):
        if op[0] in WRITES:
            n = int(op[1])
            k = (n - timer) // g.delay + 1 if n >= timer else 0
            if k:
                e = pos + timer - 1 + g.delay * np.arange(k, dtype=np.int64)
                first = np.zeros(k, bool)
                first[0] = nt == 0
                end.append(e)
                org.append(np.full(k, origin, np.int64))
                al.append(np.full(k, float(a32)))
                ga.append(np.full(k, float(g32)))
                fi.append(first)
                ca.append(np.full(k, i, np.int64))
            calls.append((i, ntt, k))
            timer = timer - n if n < timer else g.delay - (n - timer) % g.delay
            pos, ns, nst, nt, ntt = pos + n, ns + n, nst + n, nt + k, ntt + k
        elif op[0] == "clear" or op[0] == "reset":
            timer, nt, ns, live0 = g.delay, 0, 0, ntt
            if op[0] == "reset":
                origin, nst, at_reset = pos, 0, ntt
        elif op[0] == "set_alpha":
            acc = op[1] == -1.0
            a32 = np.float32(1.0 if acc else op[1])
            g32 = np.float32(1.0) if acc else np.float32(np.float32(1.0) - a32)
        else:
            raise ValueError(op)
    cat = lambda v, dt: np.concatenate(v) if v else np.zeros(0, dt)
    return Schedule(cat(end, np.int64), cat(org, np.int64), cat(al, float), cat(ga, float), cat(fi, bool),
                    cat(ca, np.int64), live0, acc, pos, ns, nst, nt, ntt - at_reset, calls)


def frame_end(g, j):
    """last sample of transform j (0-based) of a stream with no clear or reset"""
    return g.delay * (j + 1) - 1


def weights(s):
    """weight of every live transform in the final estimate (f64)"""
    coef = np.where(s.first[s.live0:], 1.0, s.alpha[s.live0:])
    gam = s.gamma[s.live0:]
    tail = np.ones(len(gam))
    if len(gam) > 1:
        tail[:-1] = np.cumprod(gam[::-1])[::-1][1:]
    return coef * tail


def _nonzero_frames(g, x, end, origin):
    nzc = np.concatenate([[0], np.cumsum(x != 0)])
    lo = np.maximum(np.maximum(end - (g.wlen - 1), origin), 0)
    hi = np.minimum(end + 1, len(x))
    return np.flatnonzero(nzc[np.maximum(hi, lo)] - nzc[lo] > 0)


def _frames(g, x, end, origin):
    """[len(end), wlen] samples of the frames, zero outside [origin, len(x))"""
    idx = end[:, None] - (g.wlen - 1) + np.arange(g.wlen)[None, :]
    ok = (idx >= origin[:, None]) & (idx >= 0) & (idx < len(x))
    return np.where(ok, x[np.clip(idx, 0, len(x) - 1)], 0)


def _scale(s):
    return 1.0 / max(1, s.num_transforms) if s.accumulate else 0.0


def _rot(nfft):
    return (np.arange(nfft) + nfft // 2) % nfft


def spgram_ref(g, w, x, ops, mutation=None, sched=None):
    """get_psd_mag() after `ops` in f64; w = taper(oracle, g).  mutation = (kind, j) changes live transform j:
    "shift" (its frame one sample later), "drop", "twice", "swap" (its weight with that of its successor, or of its
    predecessor for the last one).  sched = schedule(g, ops) if the caller has it.  Returns (psd_mag, schedule)."""
    s = sched if sched is not None else schedule(g, ops)
    x = np.asarray(x)
    assert len(x) >= s.nsamples
    x = x[:s.nsamples]
    end, origin, wt = s.end[s.live0:].copy(), s.origin[s.live0:], weights(s)
    if mutation is not None:
        kind, j = mutation
        j -= s.live0
        assert 0 <= j < len(end)
        if kind == "shift":
            end[j] += 1
        elif kind == "drop":
            wt[j] = 0.0
        elif kind == "twice":
            wt[j] *= 2.0
        elif kind == "swap":
            o = j + 1 if j + 1 < len(end) else j - 1
            wt[j], wt[o] = wt[o], wt[j]
        else:
            raise ValueError(kind)
    psd = np.zeros(g.nfft)
    nz = _nonzero_frames(g, x, end, origin)
    w64 = np.asarray(w, np.float64)
    for a in range(0, len(nz), 256):
        k = nz[a:a + 256]
        t = _frames(g, x, end[k], origin[k]).astype(np.complex128) * w64[None, :]
        f = np.fft.fft(t, n=g.nfft, axis=1)
        psd += wt[k] @ (f.real * f.real + f.imag * f.imag)
    return np.maximum(psd[_rot(g.nfft)], float(PSD_MIN)) * _scale(s), s


def model_f32(g, w, x, ops):
    """the same calls with every stage rounded to f32 as the reference does: tapered frame to complex64, spectrum to
    complex64, |X|^2 and the recurrence in float32, one transform after the other"""
    s = schedule(g, ops)
    x = np.asarray(x)[:s.nsamples]
    x = x.astype(np.complex64 if np.iscomplexobj(x) else np.float32)
    end, origin = s.end[s.live0:], s.origin[s.live0:]
    first = s.first[s.live0:]
    al, ga = s.alpha[s.live0:].astype(np.float32), s.gamma[s.live0:].astype(np.float32)
    w = np.asarray(w, np.float32)
    psd = np.zeros(g.nfft, np.float32)
    nz = _nonzero_frames(g, x, end, origin)
    prev = 0
    for j in list(nz) + [len(end)]:
        # the all-zero transforms prev .. j - 1: psd = gamma psd (+ alpha 0); a first one sets psd = 0
        if j > prev and np.any(first[prev:j]):
            psd[:] = 0
        if j > prev and psd.any() and np.any(ga[prev:j] != 1):
            for i in range(prev, j):
                np.multiply(psd, ga[i], out=psd)
        if j == len(end):
            break
        t = np.zeros(g.nfft, np.complex64)
        t[:g.wlen] = (_frames(g, x, end[j:j + 1], origin[j:j + 1])[0] * w).astype(np.complex64)
        f = np.fft.fft(t.astype(np.complex128)).astype(np.complex64)
        mag = (f.real * f.real + f.imag * f.imag).astype(np.float32)
        psd = mag if first[j] else (ga[j] * psd + al[j] * mag).astype(np.float32)
        prev = j + 1
    scale = np.float32(_scale(s))
    return (np.fmax(psd[_rot(g.nfft)], PSD_MIN) * scale).astype(np.float32)


def burst_len(g):
    return max(2, g.wlen // 2)


def sparse_stream(dtype, g, frames_of_interest, seed, ops=None, n=None, gains=None):
    """a stream that is zero except for one burst per listed transform (at most 8): burst_len(g) samples of unit noise
    (real for float32) that end on the transform's last sample, +8 on the first of them.  A burst is clipped to the
    stream and then scaled to the energy of a whole one, with the +8 on its first kept sample: the first transform of a
    stream holds `delay` samples under the taper's tail and would otherwise vanish beside the others.  Bursts add where
    they overlap; gains = an amplitude per burst, in the order of the sorted transforms.  The transforms are numbered
    over `ops` (all of them, erased ones included), or over one uninterrupted stream of n samples when ops is None."""
    frames = sorted(set(int(j) for j in frames_of_interest))
    assert 1 <= len(frames) <= 8, frames
    if ops is not None:
        s = schedule(g, ops)
        ends, n = s.end[frames], s.nsamples
    else:
        ends = np.array([frame_end(g, j) for j in frames])
    rng = np.random.default_rng(seed)
    cplx = np.dtype(dtype) == np.complex64
    x = np.zeros(n, np.complex128 if cplx else np.float64)
    L = burst_len(g)
    gains = np.ones(len(frames)) if gains is None else np.asarray(gains, float)
    for e, gain in zip(ends, gains):
        b = rng.standard_normal(L) + (1j * rng.standard_normal(L) if cplx else 0.0)
        if cplx:
            b = b * np.sqrt(0.5)
        lo = int(e) - L + 1
        a, z = max(lo, 0), min(int(e) + 1, n)
        b = b[a - lo:z - lo] * np.sqrt(L / (z - a))
        b[0] += 8.0 * np.sqrt(L / (z - a))
        x[a:z] += gain * b
    return x.astype(dtype)
