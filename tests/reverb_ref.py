"""The reverb's rule restated (include/gansynth_hip.h, DESIGN.md "Reverb"), shared by tests/test_reverb_cpu.py and tests/test_reverb_gpu.py
(a plain helper module: no test lives here).

    y[r][t] = dry * x[r][t] + wet * sum over k in [0, m) of h[rh][k] * x[r][t - k],   t in [0, n + m - 1),   rh = r or 0 (shared)

`convolve` is that sum in float64 (by a float64 FFT over the whole row: its own error, about 1e-16 of the scale, is nine orders below the
bound).  `convolve_f32` is the SAME partitioned overlap-save algorithm the kernel runs -- blocks of B new samples, 2B-point real transforms,
the products summed over the partitions in ascending order -- with scipy.fft on float32 arrays, which computes in single precision (pocketfft):
an honest fp32 evaluation by another factorisation.  The bound is set by it, not by the kernel:

    e = max over t of |y - ref| / max over t of A[t],   A = |dry| |x| + |wet| (|h| conv |x|)   (float64, per row)
    a case's tolerance = 4 * e(convolve_f32) on that case

(the factor covers a radix-2 factorisation with table twiddles against pocketfft's and another summation order).  E_F32 below holds e(convolve_f32) of
every case of the GPU test, measured once with this file and written down: the code under test never sets its own bound.
"""
import numpy as np
import scipy.fft

from tests import synth_ref as SRF

B = 2048                      # GS_FFTCONV_BLOCK
SIZES = [(5, 1), (B - 1, 2), (B, B), (B + 1, B + 1), (5 * B + 17, 3 * B + 5), (2 * B + 3, 6 * B - 1)]   # (n, m)
ROWS = [(1, 1), (2, 1), (2, 2)]                                                                         # (rows, ir_rows)
DELAYS = [0, 1, B - 1, B, B + 1, 2 * B + 3]
DRY, WET = float(np.float32(0.7)), float(np.float32(0.45))   # (the fp32 values the kernel is handed: the reference uses the same)


def draw(n, m, rows, ir_rows, seed=None):
    """The fixed draw of a case: x [rows, n] uniform in (-1, 1), h [ir_rows, m] Gaussian under a decay to -60 dB at its end (a room's
    shape: the taps a reverb has) over sqrt(min(m, 1000)), which keeps a row's 2-norm near 1 without making a single tap +-1 (with m = 1
    a unit-norm tap and dyadic dry / wet make every operation exact, and the bound of that case collapses to the reference's own 1e-17).  fp32."""
    rng = np.random.default_rng(1000003 * n + 101 * m + 7 * rows + ir_rows if seed is None else seed)
    x = (rng.random((rows, n)) * 2 - 1).astype(np.float32)
    h = rng.standard_normal((ir_rows, m)) * 10.0 ** (-3.0 * np.arange(m) / m)
    h /= np.sqrt(min(m, 1000))
    return x, h.astype(np.float32)


def _rows(x, h):
    x, h = np.atleast_2d(np.asarray(x)), np.atleast_2d(np.asarray(h))
    assert h.shape[0] in (1, x.shape[0])
    return x, h


def convolve(x, h, dry, wet):
    """The definition in float64: -> [rows, n + m - 1]."""
    x, h = _rows(x, h)
    n, m = x.shape[1], h.shape[1]
    size = scipy.fft.next_fast_len(n + m - 1, real=True)
    out = np.empty((x.shape[0], n + m - 1))
    for r in range(x.shape[0]):
        hr = h[r if h.shape[0] > 1 else 0].astype(np.float64)
        y = scipy.fft.irfft(scipy.fft.rfft(x[r].astype(np.float64), size) * scipy.fft.rfft(hr, size), size)[:n + m - 1]
        out[r] = wet * y
        out[r, :n] += dry * x[r].astype(np.float64)
    return out


def scale(x, h, dry, wet):
    """A = |dry| |x| + |wet| (|h| conv |x|) in float64: what the error of a sample is measured against."""
    return convolve(np.abs(_rows(x, h)[0]), np.abs(_rows(x, h)[1]), abs(dry), abs(wet))


def convolve_f32(x, h, dry, wet, block=B):
    """The kernel's algorithm in single precision by scipy.fft (float32 in, complex64 out): -> [rows, n + m - 1] fp32."""
    x, h = _rows(x, h)
    x, h = x.astype(np.float32), h.astype(np.float32)
    n, m = x.shape[1], h.shape[1]
    n_out = n + m - 1
    parts, blocks = -(-m // block), -(-n_out // block)
    out = np.zeros((x.shape[0], blocks * block), dtype=np.float32)
    for r in range(x.shape[0]):
        hr = np.zeros(parts * block, dtype=np.float32)
        hr[:m] = h[r if h.shape[0] > 1 else 0]
        spectra = [scipy.fft.rfft(np.concatenate([hr[p * block:(p + 1) * block], np.zeros(block, dtype=np.float32)])) for p in range(parts)]
        assert spectra[0].dtype == np.complex64
        padded = np.zeros((blocks + 1) * block, dtype=np.float32)     # padded[block + t] = x[t]
        padded[block:block + n] = x[r]
        segments = [scipy.fft.rfft(padded[j * block:(j + 2) * block]) for j in range(blocks)]
        for j in range(blocks):
            acc = np.zeros(block + 1, dtype=np.complex64)
            for p in range(min(j, parts - 1) + 1):
                acc = acc + segments[j - p] * spectra[p]
            y = scipy.fft.irfft(acc, 2 * block)[block:]
            assert y.dtype == np.float32
            out[r, j * block:(j + 1) * block] = np.float32(wet) * y + np.float32(dry) * padded[(j + 1) * block:(j + 2) * block]
    return out[:, :n_out]


def error(y, ref, a):
    """e of the module's docstring, the largest over the rows."""
    y, ref, a = np.atleast_2d(y).astype(np.float64), np.atleast_2d(ref), np.atleast_2d(a)
    return float(max(np.abs(y[r] - ref[r]).max() / a[r].max() for r in range(ref.shape[0])))


def finish(y, normalize):
    """y [rows, n] fp32 -> (peak fp32, out [rows, n] fp32, pcm int16 [n, rows], or [n] for one row): tests/stereo_ref.py::finish's rule --
    ONE peak over all rows, the correctly rounded quotient when `normalize` and peak > 1, gs_summary_audio_s16's PCM."""
    y = np.atleast_2d(np.asarray(y, dtype=np.float32))
    peak = np.float32(np.abs(y).max())
    out = y
    if normalize and peak > 1:
        out = (y.astype(np.float64) / np.float64(peak)).astype(np.float32)
    pcm = SRF.pcm16(out)
    return peak, out, (pcm[0] if y.shape[0] == 1 else np.ascontiguousarray(pcm.T))


def design_impulse(rate, rt60, channels=1, seed=0, predelay=0.0):
    """gansynth_amd.reverb.design_impulse restated: -> [channels, m] fp32."""
    pre = int(np.floor(predelay * rate + 0.5))
    length = int(np.ceil(rt60 * rate))
    g = np.random.Generator(np.random.PCG64(seed)).standard_normal((channels, length))
    h = np.zeros((channels, pre + length))
    h[:, pre:] = g * 10.0 ** (-3.0 * np.arange(length) / (rt60 * rate))
    return (h / np.sqrt((h * h).sum(axis=1)).max()).astype(np.float32)


def cases():
    """Every (n, m, rows, ir_rows) of the GPU test's accuracy cases."""
    return [(n, m, rows, ir_rows) for n, m in SIZES for rows, ir_rows in ROWS]


# e(convolve_f32) of every case at (DRY, WET), measured once with this file (scipy's pocketfft) and rounded up in the fourth digit; DESIGN.md
# "Reverb" quotes them.  tests/test_reverb_cpu.py holds the restatement to these figures, tests/test_reverb_gpu.py the kernel to 4 times them.
E_F32 = {(5, 1, 1, 1): 3.878e-08, (5, 1, 2, 1): 5.134e-08, (5, 1, 2, 2): 6.057e-08,
         (2047, 2, 1, 1): 8.136e-08, (2047, 2, 2, 1): 1.359e-07, (2047, 2, 2, 2): 1.258e-07,
         (2048, 2048, 1, 1): 3.220e-08, (2048, 2048, 2, 1): 3.400e-08, (2048, 2048, 2, 2): 4.208e-08,
         (2049, 2049, 1, 1): 3.619e-08, (2049, 2049, 2, 1): 3.784e-08, (2049, 2049, 2, 2): 3.492e-08,
         (10257, 6149, 1, 1): 3.272e-08, (10257, 6149, 2, 1): 2.851e-08, (10257, 6149, 2, 2): 2.764e-08,
         (4099, 12287, 1, 1): 2.183e-08, (4099, 12287, 2, 1): 2.637e-08, (4099, 12287, 2, 2): 2.283e-08}
FACTOR = 4.0


def tolerance(case):
    """The bound on e for the kernel on `case` = (n, m, rows, ir_rows)."""
    return FACTOR * E_F32[case]
