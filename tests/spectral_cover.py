"""The cover of the spectral kernels (gansynth_amd/csrc/spectral.hip, spectral_wave.hip), shared by tests/test_spectral_cover_cpu.py and
tests/test_spectral_cover_gpu.py:

  route()        the decision of csrc/spectral_route.h restated from the geometry (the library is NOT asked: the CPU test holds the two
                 against each other), kernels_of() the kernel instantiations a route launches, KERNELS every instantiation compiled
  CASES          the smallest shapes that enter each branch, with the route each of them names
  references     oracle.spectral_np in float64 (the inverse with the float32-built pinv, as tests/test_spectral_gpu.py does), a plain
                 dense-matrix variant for caller-supplied mel matrices, and one-defect variants for the sensitivity test
  conditioning   if_conditioning / near_branch / check_if / check_branch_bins / wrap2 (tests/test_spectral_gpu.py imports them)
  runners        ctypes calls of the entry points with a caller-chosen mel matrix, workspace size and dtype (GPU only)

Run as a script (`python tests/spectral_cover.py FILE.npz`) it is the child of the knob test: the measurement knobs are read once per
process, so each knob runs in a fresh interpreter on the inputs and float64 references the parent saved, and prints its worst ratios."""
import collections
import ctypes
import functools
import itertools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import spectral_np as S  # noqa: E402

F32, BF16 = 0, 1
OVERLAP = 0.75
SW_WAVES = 12                             # waves per block of the wave-per-frame kernels
SW_SHAPE = (1, 1, 2, 2, 3, 3, 4, 6)       # mel run lengths per 128-column block the wave kernel's gather is unrolled for
FWD_GENERIC, FWD_WAVE = 0, 1
GEMM_NONE, GEMM_F32_64, GEMM_F32_128, GEMM_SPLIT_ALL, GEMM_SPLIT_TWO, GEMM_WIDE_256 = range(6)
ISTFT_NONE, ISTFT_WAVE_OLA, ISTFT_WAVE_FRAMES, ISTFT_BLOCK_FFT = range(4)
SAMPLE_RATES = (8000, 16000, 22050, 44100, 48000)

# tolerances: the project's own, from tests/test_spectral_gpu.py
TOL_MAG = 1e-5          # magnitude, of the example maximum
TOL_MEL = 3e-4          # mel magnitude in the linear domain, of the example maximum, everywhere
TOL_LOG = 1e-3          # log-mel, on the bins above LOUD of the maximum
TOL_IF = 1e-3           # IF on the well-conditioned bins (check_if)
TOL_WAVE = 1e-4         # inverse, of the peak
MIN_CORR = 0.999999
LOUD = 1e-3
BF16_REL = 2.0 ** -8    # one round-to-nearest of an 8-bit mantissa: |error| <= 2^-8 |value|
PAD_LOG_MEL = (np.log(1e-6) + 3.76) / 10.05

# ------------------------------------------------------------------------------------------------------------ knobs
DEFAULT_KNOBS = dict(generic=0, fp32_gemm=0, mag_6terms=0, gemm_256=0, gemm_kb=4, gemm_kb3=2, block_fft=0, separate_ola=0)
# (environment variable, value, the knob struct it gives)
KNOB_SETTINGS = [
    ("GS_INVERSE_FP32_GEMM", "1", dict(fp32_gemm=1)),
    ("GS_INVERSE_MAG_6TERMS", "1", dict(mag_6terms=1)),
    ("GS_INVERSE_GEMM_256", "1", dict(gemm_256=1)),
    ("GS_INVERSE_GEMM_KB", "2", dict(gemm_kb=2)),
    ("GS_INVERSE_GEMM_KB3", "4", dict(gemm_kb3=4)),
    ("GS_INVERSE_BLOCK_FFT", "1", dict(block_fft=1)),
    ("GS_INVERSE_SEPARATE_OLA", "1", dict(separate_ola=1)),
    ("GS_SPECTRAL_GENERIC", "1", dict(generic=1)),
]
KNOB_NAMES = [k for k, _, _ in KNOB_SETTINGS]


def knobs(**kw):
    return dict(DEFAULT_KNOBS, **kw)


def knobs_unset():
    return not any(k in os.environ for k in KNOB_NAMES)


# ------------------------------------------------------------------------------------------------------------ geometry and route
def geometry(time_steps, nbins):
    """frame_length, frame_step, num_samples (spectral_ops.py:50-53)."""
    frame_length = 2 * nbins
    frame_step = int((1.0 - OVERLAP) * frame_length)
    return frame_length, frame_step, frame_step * (time_steps - 1) + frame_length


@functools.lru_cache(maxsize=None)
def mel_matrix(nbins, sample_rate):
    return np.ascontiguousarray(S.linear_to_mel_weight_matrix(nbins, nbins, sample_rate, 0.0, sample_rate / 2.0, np.float32))


@functools.lru_cache(maxsize=None)
def mel_pinv(nbins, sample_rate):
    return np.ascontiguousarray(S.pinv(mel_matrix(nbins, sample_rate)))


def mel_digest(mel):
    """(non-zeros of the fullest column, every column's non-zeros within 8 consecutive bins, longest such span per 128-column block)."""
    nz = mel != 0
    maxnz = max(1, int(nz.sum(0).max()))
    if mel.shape[0] != 1024:
        return maxnz, False, (0,) * 8
    first = np.where(nz.any(0), nz.argmax(0), 0)
    last = np.where(nz.any(0), mel.shape[0] - 1 - nz[::-1].argmax(0), -1)
    span = last - first + 1
    if span.max() > 8:
        return maxnz, False, (0,) * 8
    return maxnz, True, tuple(max(1, int(span[128 * j:128 * (j + 1)].max())) for j in range(8))


def runs_per_example(batch, time_steps):
    runs = max(1, min(-(-256 * SW_WAVES // batch), time_steps))
    return runs - runs % SW_WAVES if runs >= SW_WAVES else runs


ROUTE_FIELDS = ("fwd_workspace_bytes", "fwd_kind", "maxnz", "mz", "mel_cnt", "runs", "q", "rem", "exchange", "span_examples", "gemm_kind",
                "gemm_launches", "gemm_nj", "gemm_np", "gemm_kb", "istft_kind")


def route(time_steps, nbins, mel, has_pinv, batch, wave_len, front_pad, ws_bytes=None, k=DEFAULT_KNOBS, digest=None):
    """What the library runs, from the geometry (ws_bytes None: the workspace its own query asks for; digest: mel_digest(mel), if at hand)."""
    frame_length, frame_step, _ = geometry(time_steps, nbins)
    maxnz, one_run, cnt = mel_digest(mel) if digest is None else digest
    if maxnz <= 8:
        maxnz += maxnz & 1
    r = dict(maxnz=maxnz, mz=maxnz if maxnz <= 8 else 0, mel_cnt=cnt, runs=0, q=0, rem=0, exchange=0, span_examples=0, gemm_kind=GEMM_NONE,
             gemm_launches=0, gemm_nj=(0, 0), gemm_np=(0, 0), gemm_kb=(0, 0), istft_kind=ISTFT_NONE)
    wave = nbins == 1024 and not k["generic"] and one_run and cnt == SW_SHAPE
    r["fwd_kind"] = FWD_WAVE if wave else FWD_GENERIC
    if wave:
        runs = runs_per_example(batch, time_steps)
        need = batch * runs * 4096
        r.update(runs=runs, q=time_steps // runs, rem=time_steps % runs, span_examples=int(runs < SW_WAVES), fwd_workspace_bytes=need,
                 exchange=int(runs % SW_WAVES == 0 and (ws_bytes is None or ws_bytes >= need)))
    else:
        r["fwd_workspace_bytes"] = batch * time_steps * nbins * 4
    if not has_pinv:
        return r
    rows = batch * time_steps
    split = (2 * rows) % 128 == 0 and nbins % 128 == 0 and not k["fp32_gemm"]
    two = split and rows % 128 == 0 and not k["mag_6terms"]
    if split and k["gemm_256"] and nbins % 256 == 0:
        launches = [(4, 2, 2), (4, 3, 2)] if two else [(4, 3, 2)]
        r["gemm_kind"] = GEMM_WIDE_256
    elif two:
        launches = [(2, 2, 4 if k["gemm_kb"] == 4 else 2), (2, 3, 4 if k["gemm_kb3"] == 4 else 2)]
        r["gemm_kind"] = GEMM_SPLIT_TWO
    elif split:
        launches = [(2, 3, 2)]
        r["gemm_kind"] = GEMM_SPLIT_ALL
    else:
        launches = [(0, 0, 0)]
        r["gemm_kind"] = GEMM_F32_128 if (2 * rows) % 128 == 0 and nbins % 128 == 0 else GEMM_F32_64
    launches = launches + [(0, 0, 0)] * (2 - len(launches))
    r.update(gemm_launches=sum(1 for l in launches if l != (0, 0, 0)) or 1, gemm_nj=tuple(l[0] for l in launches),
             gemm_np=tuple(l[1] for l in launches), gemm_kb=tuple(l[2] for l in launches))
    ola_ok = frame_length == 2048 and frame_step == 512 and time_steps >= 3 * SW_WAVES and wave_len % 2 == 0 and front_pad % 2 == 0
    if wave and not k["block_fft"] and not k["separate_ola"] and ola_ok:
        r["istft_kind"] = ISTFT_WAVE_OLA
    elif wave and not k["block_fft"]:
        r["istft_kind"] = ISTFT_WAVE_FRAMES
    else:
        r["istft_kind"] = ISTFT_BLOCK_FFT
    return r


def lib_routes(lib, time_steps, nbins, mel, has_pinv, batch, count, wave_len, front_pad, ws_bytes=0, k=DEFAULT_KNOBS, dtype=F32):
    """gs_spectral_route for the batch sizes batch .. batch + count - 1: the array of GsSpectralRoute (k None: this process's environment)."""
    from gansynth_amd import _lib
    frame_length, frame_step, _ = geometry(time_steps, nbins)
    ks = None if k is None else ctypes.byref(_lib.GsSpectralKnobs(**k))
    out = (_lib.GsSpectralRoute * count)()
    _lib.check(lib.gs_spectral_route(frame_length, frame_step, time_steps, mel.ctypes.data, int(has_pinv), batch, count, wave_len, front_pad, dtype, ws_bytes,
                                     ks, out), "gs_spectral_route")
    return out


def route_dict(out):
    assert out.reserved == 0
    return {f: (tuple(getattr(out, f)) if f.startswith(("mel_cnt", "gemm_n", "gemm_kb")) else int(getattr(out, f))) for f in ROUTE_FIELDS}


def lib_route(lib, time_steps, nbins, mel, has_pinv, batch, wave_len, front_pad, ws_bytes=None, k=DEFAULT_KNOBS, dtype=F32):
    """gs_spectral_route as a dict of ROUTE_FIELDS (ws_bytes None: the workspace its own answer asks for)."""
    if ws_bytes is None:
        ws_bytes = lib_routes(lib, time_steps, nbins, mel, has_pinv, batch, 1, wave_len, front_pad, 0, k, dtype)[0].fwd_workspace_bytes
    return route_dict(lib_routes(lib, time_steps, nbins, mel, has_pinv, batch, 1, wave_len, front_pad, ws_bytes, k, dtype)[0])


def route_row(r):
    """A route (dict of ROUTE_FIELDS) as the int32 words of GsSpectralRoute."""
    need = r["fwd_workspace_bytes"]
    return (need & 0xffffffff, need >> 32, r["fwd_kind"], r["maxnz"], r["mz"]) + tuple(r["mel_cnt"]) + (
        r["runs"], r["q"], r["rem"], r["exchange"], r["span_examples"], r["gemm_kind"], r["gemm_launches"]) + tuple(r["gemm_nj"]) + tuple(r["gemm_np"]) + tuple(
        r["gemm_kb"]) + (r["istft_kind"], 0)


# every kernel instantiation of the two .hip files (their hipLaunchKernelGGL sites), by name
_T = ("f32", "bf16")
KERNELS = (["stft_kernel<f32,0,0>", "mel_project_kernel", "if_unwrap_kernel<f32,0>"]
           + [f"stft_kernel<{t},1,{mz}>" for t in _T for mz in (0, 2, 4, 6, 8)]
           + [f"if_unwrap_kernel<{t},1>" for t in _T] + [f"inv_prep_kernel<{t}>" for t in _T]
           + [f"gemm_bf16x6_kernel<{nj},{np_},{kb}>" for nj, np_, kb in ((4, 2, 2), (4, 3, 2), (2, 2, 4), (2, 2, 2), (2, 3, 4), (2, 3, 2))]
           + ["gemm_f32_128_kernel", "gemm_f32_kernel", "istft_kernel", "overlap_add_kernel", "istft_wave_kernel<false>", "istft_wave_kernel<true>"]
           + [f"stft_wave_kernel<{t},1>" for t in _T] + ["stft_wave_kernel<f32,0>"])
# reachable only with a measurement knob set: tests/test_spectral_cover_gpu.py::test_knob_routes runs them
KNOB_ONLY = {"gemm_f32_128_kernel": "GS_INVERSE_FP32_GEMM", "gemm_bf16x6_kernel<4,2,2>": "GS_INVERSE_GEMM_256", "gemm_bf16x6_kernel<4,3,2>": "GS_INVERSE_GEMM_256",
             "gemm_bf16x6_kernel<2,2,2>": "GS_INVERSE_GEMM_KB", "gemm_bf16x6_kernel<2,3,4>": "GS_INVERSE_GEMM_KB3"}
# route values reachable only with a knob
KNOB_ONLY_VALUES = {("gemm_kind", GEMM_F32_128): "GS_INVERSE_FP32_GEMM", ("gemm_kind", GEMM_WIDE_256): "GS_INVERSE_GEMM_256"}


def kernels_of(r, dtype, entry):
    """The kernels one entry point launches under route r: entry "fused" (gs_stft_mel_if_fwd), "stft" (gs_stft_fwd), "mel_project",
    "if_unwrap", "inverse" (gs_mel_if_to_waveform)."""
    t = _T[dtype]
    if entry == "fused":
        return {f"stft_wave_kernel<{t},1>"} if r["fwd_kind"] == FWD_WAVE else {f"stft_kernel<{t},1,{r['mz']}>", f"if_unwrap_kernel<{t},1>"}
    if entry == "stft":
        return {"stft_wave_kernel<f32,0>"} if r["fwd_kind"] == FWD_WAVE else {"stft_kernel<f32,0,0>"}
    if entry == "mel_project":
        return {"mel_project_kernel"}
    if entry == "if_unwrap":
        return {"if_unwrap_kernel<f32,0>"}
    assert entry == "inverse" and r["gemm_kind"] != GEMM_NONE
    out = {f"inv_prep_kernel<{t}>"}
    if r["gemm_kind"] in (GEMM_F32_64, GEMM_F32_128):
        out.add("gemm_f32_kernel" if r["gemm_kind"] == GEMM_F32_64 else "gemm_f32_128_kernel")
    else:
        out |= {f"gemm_bf16x6_kernel<{r['gemm_nj'][i]},{r['gemm_np'][i]},{r['gemm_kb'][i]}>" for i in range(r["gemm_launches"])}
    out |= {ISTFT_WAVE_OLA: {"istft_wave_kernel<true>"}, ISTFT_WAVE_FRAMES: {"istft_wave_kernel<false>", "overlap_add_kernel"},
            ISTFT_BLOCK_FFT: {"istft_kernel", "overlap_add_kernel"}}[r["istft_kind"]]
    return out


# ------------------------------------------------------------------------------------------------------------ cases
# name, [T, H], sample rate (0: caller-supplied mel matrix `mel`), batch, waveform_length, rows compared with the oracle (None: all),
# fwd / inv: the dtypes of the fused forward / the inverse that run, expect: the route the case is there for
Case = collections.namedtuple("Case", "name time_steps nbins sample_rate batch wave_len rows fwd inv expect mel tone seed")


def _case(name, shape, sample_rate, batch, wave_len, expect, rows=None, fwd=(F32, BF16), inv=(F32,), mel=None, tone=False, seed=0):
    return Case(name, shape[0], shape[1], sample_rate, batch, wave_len, rows, tuple(fwd), tuple(inv), expect, mel, tone, seed)


def _custom_mel(kind):
    """Caller-supplied 64 x 64 mel matrices: "two" = two taps per column (ELL width 2); "eleven" = even columns with eleven taps in two
    separate runs (six + five, ELL width 11: the run-time-width kernel), odd columns with three.  No tap on the last linear bin: the Nyquist
    bin of a real signal is real, its phase sits ON the atan2 branch cut."""
    mel = np.zeros((64, 64), np.float32)
    for m in range(64):
        if kind == "two":
            mel[min(m, 61), m], mel[min(m, 61) + 1, m] = 0.625, 0.375
        elif m % 2 == 0:
            for j in range(6):
                mel[m % 46 + j, m] = 0.05 + 0.03125 * j
            for j in range(5):
                mel[m % 46 + 12 + j, m] = 0.25 - 0.03125 * j
        else:
            mel[m % 30, m], mel[m % 30 + 7, m], mel[m % 30 + 30, m] = 0.5, 0.25, 0.125
    assert not mel[63].any()
    return mel


# front_pad = num_samples - wave_len takes the values 0, odd, even, and more than one hop
CASES = [
    # forward and inverse, generic path
    _case("g64_8k_b3", [16, 64], 8000, 3, 608, dict(fwd_kind=FWD_GENERIC, mz=4, gemm_kind=GEMM_F32_64, istft_kind=ISTFT_BLOCK_FFT), seed=11),          # pad 0; GEMM N = 64
    _case("g128_16k_b3", [16, 128], 16000, 3, 1201, dict(fwd_kind=FWD_GENERIC, mz=6, gemm_kind=GEMM_F32_64, istft_kind=ISTFT_BLOCK_FFT), seed=12),      # pad 15; ragged M = 96
    _case("g128_16k_b4", [16, 128], 16000, 4, 886, dict(fwd_kind=FWD_GENERIC, mz=6, gemm_kind=GEMM_SPLIT_ALL, gemm_kb=(2, 0)), seed=13),             # pad 330: two padding frames
    _case("g128_16k_b8", [16, 128], 16000, 8, 1200, dict(fwd_kind=FWD_GENERIC, mz=6, gemm_kind=GEMM_SPLIT_TWO, gemm_kb=(4, 2)), seed=14),             # pad 16; KB = 4 at H = 128
    _case("g128_44k_b4", [32, 128], 44100, 4, 2239, dict(fwd_kind=FWD_GENERIC, mz=8, gemm_kind=GEMM_SPLIT_TWO), seed=15),                              # pad 1
    _case("g512_22k_b2", [27, 512], 22050, 2, 7000, dict(fwd_kind=FWD_GENERIC, gemm_kind=GEMM_F32_64, istft_kind=ISTFT_BLOCK_FFT), seed=16),           # pad 680; T % 8 != 0
    _case("g1024_8k_b2", [32, 1024], 8000, 2, 16000, dict(fwd_kind=FWD_GENERIC, mel_cnt=(1, 2, 2, 2, 3, 3, 4, 5), gemm_kind=GEMM_SPLIT_ALL, istft_kind=ISTFT_BLOCK_FFT), seed=17),
    _case("c64_two_b2", [9, 64], 0, 2, 371, dict(fwd_kind=FWD_GENERIC, mz=2, maxnz=2), inv=(), mel="two", seed=18),                                    # pad 13
    _case("c64_eleven_b2", [9, 64], 0, 2, 371, dict(fwd_kind=FWD_GENERIC, mz=0, maxnz=11), inv=(), mel="eleven", seed=19),
    # forward, wave path (1024 bins at 16 kHz)
    _case("w8_b5", [8, 1024], 16000, 5, 5632, dict(fwd_kind=FWD_WAVE, runs=8, q=1, rem=0, exchange=0, span_examples=1), fwd=(F32,), inv=(), seed=21),      # pad 0; 40 runs in 4 blocks
    _case("w16_b300", [16, 1024], 16000, 300, 9128, dict(fwd_kind=FWD_WAVE, runs=11, q=1, rem=5, exchange=0, span_examples=1), rows=(0, 150, 299), fwd=(F32,), inv=(), seed=22),
    _case("w16_b257", [16, 1024], 16000, 257, 9727, dict(fwd_kind=FWD_WAVE, runs=12, q=1, rem=4, exchange=1, span_examples=0), rows=(0, 256), fwd=(F32,), inv=(), seed=23),   # pad 1
    _case("w32_b3", [32, 1024], 16000, 3, 15320, dict(fwd_kind=FWD_WAVE, runs=24, q=1, rem=8, exchange=1), fwd=(F32, BF16), inv=(), tone=True, seed=24),    # pad 2600: two padding frames; row 2: two tones
    _case("w32_b200", [32, 1024], 16000, 200, 17918, dict(fwd_kind=FWD_WAVE, runs=12, q=2, rem=8, exchange=1), rows=(0, 199), fwd=(F32,), inv=(), seed=27),   # pad 2; two frames per run
    _case("w37_b2", [37, 1024], 16000, 2, 20000, dict(fwd_kind=FWD_WAVE, runs=36, q=1, rem=1, exchange=1), fwd=(F32,), inv=(), seed=25),                    # pad 480
    _case("w128_b1", [128, 1024], 16000, 1, 64000, dict(fwd_kind=FWD_WAVE, runs=120, q=1, rem=8, exchange=1), fwd=(F32,), inv=(), seed=26),                 # pad 3072
    # inverse, wave path
    _case("i32_b2", [32, 1024], 16000, 2, 16000, dict(istft_kind=ISTFT_WAVE_FRAMES, gemm_kind=GEMM_SPLIT_ALL), fwd=(), seed=31),                       # T < 36
    _case("i36_b2", [36, 1024], 16000, 2, 19000, dict(istft_kind=ISTFT_WAVE_OLA, gemm_kind=GEMM_F32_64), fwd=(), inv=(F32, BF16), seed=32),            # three frames per run; N = 1024
    _case("i40_b2", [40, 1024], 16000, 2, 21000, dict(istft_kind=ISTFT_WAVE_OLA, gemm_kind=GEMM_F32_64), fwd=(), seed=33),                             # T % 12 = 4
    _case("i64_b2", [64, 1024], 16000, 2, 32000, dict(istft_kind=ISTFT_WAVE_OLA, gemm_kind=GEMM_SPLIT_TWO, gemm_kb=(4, 2)), fwd=(), inv=(F32, BF16), seed=34),
    _case("i64_odd_b2", [64, 1024], 16000, 2, 31999, dict(istft_kind=ISTFT_WAVE_FRAMES, gemm_kind=GEMM_SPLIT_TWO), fwd=(), seed=35),                   # odd length leaves the OLA route
    _case("i64_pad0_b2", [64, 1024], 16000, 2, 34304, dict(istft_kind=ISTFT_WAVE_OLA, gemm_kind=GEMM_SPLIT_TWO), fwd=(), seed=36),
]
BY_NAME = {c.name: c for c in CASES}
KNOB_CASE = "i64_b2"          # every knob runs on it (GS_SPECTRAL_GENERIC also forward)
STAGEWISE = ("c64_two_b2", "c64_eleven_b2", "w32_b3")   # gs_stft_fwd (and, on the custom matrices, gs_mel_project / gs_if_unwrap) run on these


def case_mel(c):
    return _custom_mel(c.mel) if c.mel else mel_matrix(c.nbins, c.sample_rate)


def front_pad(c):
    return geometry(c.time_steps, c.nbins)[2] - c.wave_len


def case_route(c, ws_bytes=None, k=DEFAULT_KNOBS):
    return route(c.time_steps, c.nbins, case_mel(c), bool(c.inv) or c.name == KNOB_CASE, c.batch, c.wave_len, front_pad(c), ws_bytes, k)


def case_lib_route(lib, c, ws_bytes=None, k=DEFAULT_KNOBS):
    return lib_route(lib, c.time_steps, c.nbins, case_mel(c), bool(c.inv) or c.name == KNOB_CASE, c.batch, c.wave_len, front_pad(c), ws_bytes, k)


def case_kernels(c):
    """Every kernel the GPU test of case c launches."""
    r, out = case_route(c), set()
    for dt in c.fwd:
        out |= kernels_of(r, dt, "fused")
    for dt in c.inv:
        out |= kernels_of(r, dt, "inverse")
    if c.name in STAGEWISE:
        out |= kernels_of(r, F32, "stft")
        if c.mel:
            out |= kernels_of(r, F32, "mel_project") | kernels_of(r, F32, "if_unwrap")
    return out


def params(c):
    return dict(waveform_length=c.wave_len, sample_rate=c.sample_rate, spectrogram_shape=[c.time_steps, c.nbins], overlap=OVERLAP)


@functools.lru_cache(maxsize=None)
def _waves(name):
    c = BY_NAME[name]
    w = np.clip(np.random.default_rng(4000 + c.seed).normal(0.0, 0.1, (c.batch, c.wave_len)), -1, 1).astype(np.float32)
    if c.tone:   # the last row: two tones, a sparse spectrum (handled as tests/test_spectral_gpu.py handles its tone)
        t = np.arange(c.wave_len) / float(c.sample_rate)
        w[-1] = (0.5 * np.sin(2 * np.pi * 440.0 * t) + 0.25 * np.sin(2 * np.pi * 880.0 * t)).astype(np.float32)
    w.setflags(write=False)
    return w


def waves(c):
    return _waves(c.name)


def ref_rows(c):
    return tuple(range(c.batch)) if c.rows is None else c.rows


def padding_frames(c):
    """Frames that lie entirely inside the front padding."""
    frame_length, frame_step, _ = geometry(c.time_steps, c.nbins)
    return [t for t in range(c.time_steps) if t * frame_step + frame_length <= front_pad(c)]


# ------------------------------------------------------------------------------------------------------------ references
def stages_dense(waveforms, wave_len, time_steps, nbins, mel, dtype=np.float64):
    """oracle.spectral_np.convert_to_spectrogram_stages with a caller-supplied dense mel matrix."""
    frame_length, frame_step, num_samples = geometry(time_steps, nbins)
    x = np.pad(np.asarray(waveforms, dtype=dtype), [[0, 0], [num_samples - wave_len, 0]])
    s = S.stft(x, frame_length, frame_step, dtype)[..., 1:]
    mag, phase, mel = np.abs(s).astype(dtype), np.angle(s).astype(dtype), np.asarray(mel, dtype)
    mel_mag, mel_phase = (mag @ mel).astype(dtype), (phase @ mel).astype(dtype)
    dt = np.dtype(dtype).type
    log_mel = (np.log(mel_mag + dt(1.0e-6)) - dt(-3.76)) / dt(10.05)
    return dict(stft=s, magnitude=mag, phase=phase, mel=mel, mel_magnitude=mel_mag, mel_phase=mel_phase, log_mel=log_mel.astype(dtype),
                mel_if=S.instantaneous_frequency(mel_phase, axis=-2).astype(dtype))


def linear_mel64(c):
    """The float64 mel matrix of case c's reference: the oracle's own float64 build, or the caller-supplied matrix widened."""
    if c.mel:
        return case_mel(c).astype(np.float64)
    return S.linear_to_mel_weight_matrix(c.nbins, c.nbins, c.sample_rate, 0.0, c.sample_rate / 2.0, np.float64)


def stages(c, w, dtype=np.float64, mel=None):
    if c.mel or mel is not None:
        return stages_dense(w, c.wave_len, c.time_steps, c.nbins, case_mel(c) if mel is None else mel, dtype)
    return S.convert_to_spectrogram_stages(w, **params(c), dtype=dtype)


@functools.lru_cache(maxsize=None)
def _forward_reference(name):
    c = BY_NAME[name]
    st64 = stages(c, waves(c)[list(ref_rows(c))])
    on_cut, branch = if_conditioning(st64)
    return st64, on_cut, branch


def forward_reference(c):
    """(float64 stages of the rows ref_rows(c), on_cut, branch), computed once per process."""
    return _forward_reference(c.name)


def bf16_round(x, truncate=False):
    """float32 -> bf16 -> float32 on the host: round-to-nearest-even, or the defect: truncation."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    if not truncate:
        u = u + (np.uint32(0x7fff) + ((u >> np.uint32(16)) & np.uint32(1)))
    return (u & np.uint32(0xffff0000)).view(np.float32)


@functools.lru_cache(maxsize=None)
def _inverse_inputs(name):
    c = BY_NAME[name]
    lm, mi = S.convert_to_spectrogram(waves(c), **params(c))     # float32: what the forward kernels hand the inverse ones
    return lm, mi


def inverse_inputs(c, dtype=F32, truncate=False):
    lm, mi = _inverse_inputs(c.name)
    return (lm, mi) if dtype == F32 else (bf16_round(lm, truncate), bf16_round(mi, truncate))


def inverse_reference(c, lm, mi, drop_overlap=None, zero_rows_from=None):
    """float64 evaluation with the float32-built pinv(mel), from the values the kernel is given.  One-defect variants:
    drop_overlap (example, frame, segment): that frame's contribution to output hop `segment` is left out;
    zero_rows_from r: rows r.. of the stacked [mel_mag; mel_phase] @ pinv product stay zero (a GEMM row block never written)."""
    pinv = mel_pinv(c.nbins, c.sample_rate).astype(np.float64)
    frame_length, frame_step, num_samples = geometry(c.time_steps, c.nbins)
    mel_mag = np.exp(np.asarray(lm, np.float64) * 10.05 - 3.76)
    mel_phase = np.cumsum(np.asarray(mi, np.float64) * np.pi, axis=-2)
    stacked = np.concatenate([mel_mag.reshape(-1, c.nbins), mel_phase.reshape(-1, c.nbins)]) @ pinv
    if zero_rows_from is not None:
        stacked[zero_rows_from:] = 0.0
    rows = c.batch * c.time_steps
    mag, phase = stacked[:rows].reshape(mel_mag.shape), stacked[rows:].reshape(mel_mag.shape)
    s = np.pad(mag * (np.cos(phase) + 1j * np.sin(phase)), [[0, 0], [0, 0], [1, 0]])
    frames = np.fft.irfft(s, n=frame_length, axis=-1) * S.inverse_stft_window(frame_length, frame_step, np.float64)
    out = np.zeros((c.batch, num_samples))
    for i in range(c.time_steps):
        out[:, i * frame_step:i * frame_step + frame_length] += frames[:, i]
    if drop_overlap is not None:
        b, f, seg = drop_overlap
        lo = seg * frame_step
        assert 0 <= lo - f * frame_step < frame_length
        out[b, lo:lo + frame_step] -= frames[b, f, lo - f * frame_step:lo - f * frame_step + frame_step]
    return out[:, num_samples - c.wave_len:]


# ------------------------------------------------------------------------------------------------------------ conditioning
def wrap2(d):
    """An IF difference modulo 2 (a +-pi branch flip is a 2.0 jump) -- only applied to bins PROVEN ill-conditioned, see
    if_conditioning."""
    return (d + 1.0) % 2.0 - 1.0


def if_conditioning(st64, margin=1e-3, cut=1e-4):
    """Where the reference's IF (spectral_ops.py:21-44) is discontinuous in its input, from the float64 oracle:
      on_cut[b,t,m]  the wrapped phase difference sits within `margin` rad of +-pi: wrap() may take either branch (IF = +-1);
      branch[b,t,m]  a linear bin feeding mel column m has |arg X| within `cut` of pi at frame t or t-1 (with magnitude): atan2
                     may return +pi or -pi there, which moves the mel phase by 2 pi w -- NOT a multiple of 2 pi.
    Everything else is well conditioned and must agree plainly."""
    ph = st64["mel_phase"]
    d = np.diff(ph, axis=-2)
    md = np.mod(d + np.pi, 2 * np.pi) - np.pi
    on_cut = np.zeros(ph.shape, bool)
    on_cut[:, 1:] = np.pi - np.abs(md) < margin
    near = near_branch(st64, cut)
    hit = (near.astype(np.float64) @ (st64["mel"] != 0).astype(np.float64)) > 0          # [b, t, m]
    branch = hit.copy()
    branch[:, 1:] |= hit[:, :-1]
    return on_cut, branch


def near_branch(st64, cut=1e-4):
    """[b, t, k]: linear bin k of frame t (with magnitude) has |arg X| within `cut` of pi -- atan2 may land on either side."""
    lin, mag = st64["phase"], st64["magnitude"]
    return (np.pi - np.abs(lin) < cut) & (mag > 1e-6 * mag.max())


def check_branch_bins(got, ref, st64, b, branch, where=None, tol=2e-3):
    """The bins check_if leaves out are not unchecked: where a linear bin k sits on the atan2 branch cut at frame t or t - 1, the mel
    phase of column m moves by +-2 pi w[k, m] (w = the mel weight) and IF = wrap(p[t] - p[t-1]) / pi by +-2 w[k, m] modulo 2.  Every
    such bin must equal the oracle's value up to a signed sum of those quanta over the (few) hit bins of its column."""
    where = np.ones(ref.shape, bool) if where is None else where
    near, mel = near_branch(st64)[b], st64["mel"]
    ts, ms = np.nonzero(branch & where)
    worst = 0.0
    for t, m in zip(ts, ms):
        ks = [k for k in np.nonzero(mel[:, m])[0] if near[t, k] or (t > 0 and near[t - 1, k])]
        quanta = [2.0 * float(mel[k, m]) for k in ks]
        # a bin on the cut at t AND t - 1 may flip at either frame or both: coefficients -2 .. 2 per hit bin (columns have <= 6 non-zeros)
        best = min(abs(float(wrap2(np.float64(got[t, m] - ref[t, m] - sum(c * q for c, q in zip(cs, quanta))))))
                   for cs in itertools.product((-2, -1, 0, 1, 2), repeat=len(quanta)))
        worst = max(worst, best)
        assert best < tol, (b, t, m, float(got[t, m]), float(ref[t, m]), quanta)
    return len(ts), worst


def check_if(got, ref, on_cut, branch, where=None, tol=1e-3, max_branch=2e-3, extra=None):
    """IF parity: plain on the well-conditioned bins, modulo 2 on the branch cut of wrap(), nothing on atan2 branch hits; the
    ill-conditioned sets must stay the small sets they are.  `extra` (an array like ref, optional): added to tol per bin (a storage format's
    rounding)."""
    where = np.ones(ref.shape, bool) if where is None else where
    tol = tol if extra is None else tol + extra
    plain = where & ~on_cut & ~branch
    assert (np.abs(got - ref) < tol)[plain].all(), np.abs(got - ref)[plain].max()
    worst = (np.abs(got - ref) / tol)[plain].max()
    cut = where & on_cut & ~branch
    if cut.any():
        assert (np.abs(wrap2(got - ref)) < tol)[cut].all()
    assert on_cut[where].mean() < 2e-3 and branch[where].mean() < max_branch, (on_cut[where].mean(), branch[where].mean())
    return float(worst)


def conditioning_shares(c):
    """(on-cut share, atan2-branch share) of each reference row of case c, over the bins its IF check covers."""
    st64, on_cut, branch = forward_reference(c)
    out = []
    for i in range(len(ref_rows(c))):
        where = if_where(c, st64, i)
        out.append((float(on_cut[i][where].mean()), float(branch[i][where].mean())))
    return out


def is_tone_row(c, i):
    return c.tone and ref_rows(c)[i] == c.batch - 1


def if_where(c, st64, i):
    """The bins of reference row i whose IF is compared: all of them for noise; for the tone row the bins that carry signal at t and t - 1."""
    ref = st64["mel_magnitude"][i]
    if not is_tone_row(c, i):
        return np.ones(ref.shape, bool)
    loud = ref > LOUD * ref.max()
    prev_loud = loud.copy()
    prev_loud[1:] &= loud[:-1]
    return prev_loud


def compare_forward(c, lm, mi, dtype=F32, ref=None):
    """Images (log-mel lm, IF mi: float arrays [rows, T, H], the rows ref_rows(c)) against the float64 reference: worst error / tolerance per
    family.  Asserts every one of them."""
    st64, on_cut, branch = forward_reference(c) if ref is None else ref
    out = dict(mel=0.0, log=0.0, IF=0.0, branch_bins=0, pad=0.0)
    pads = padding_frames(c)
    for i in range(lm.shape[0]):
        ref_mel, ref_log, ref_if = st64["mel_magnitude"][i], st64["log_mel"][i], st64["mel_if"][i]
        loud = ref_mel > LOUD * ref_mel.max()
        if dtype == F32:   # (a bf16 log-mel carries 2^-8 x 10.05 = 4 % in the linear domain: only the image itself is compared there)
            out["mel"] = max(out["mel"], float(np.abs(np.exp(lm[i] * 10.05 - 3.76) - 1e-6 - ref_mel).max() / (TOL_MEL * ref_mel.max())))
        extra_log = BF16_REL * np.abs(ref_log) if dtype == BF16 else 0.0
        extra_if = BF16_REL * np.abs(ref_if) if dtype == BF16 else None
        out["log"] = max(out["log"], float((np.abs(lm[i] - ref_log) / (TOL_LOG + extra_log))[loud].max()))
        where = if_where(c, st64, i)
        out["IF"] = max(out["IF"], check_if(mi[i], ref_if, on_cut[i], branch[i], where=where, tol=TOL_IF, max_branch=3e-2 if is_tone_row(c, i) else 2e-3,
                                            extra=extra_if))
        n, _ = check_branch_bins(mi[i], ref_if, st64, i, branch[i] & ~on_cut[i], where=where, tol=2e-3 + (BF16_REL if dtype == BF16 else 0.0))
        out["branch_bins"] += n
        if pads:
            exact = PAD_LOG_MEL if dtype == F32 else float(bf16_round(np.float32([PAD_LOG_MEL]))[0])
            out["pad"] = max(out["pad"], float(np.abs(lm[i][pads] - exact).max() / 1e-6))
            assert np.all(mi[i][pads] == 0), "IF of a padding frame"
    assert out["mel"] < 1.0 and out["log"] < 1.0 and out["IF"] < 1.0 and out["pad"] <= 1.0, (c.name, dtype, out)
    return out


def compare_inverse(got, ref64):
    """Waveforms [b, n] against the float64 reference: (worst error / tolerance, least correlation).  Asserts both."""
    worst, corr = 0.0, 1.0
    for a, b in zip(np.asarray(got, np.float64), ref64):
        worst = max(worst, float(np.abs(a - b).max() / np.abs(b).max() / TOL_WAVE))
        corr = min(corr, float(S.cross_correlation(a, b)))
    assert worst < 1.0 and corr > MIN_CORR, (worst, corr)
    return worst, corr


# ------------------------------------------------------------------------------------------------------------ runners (GPU)
class Plan(object):
    """gs_spectral_plan_create with a caller-chosen mel matrix (and its pinv)."""

    def __init__(self, c, with_inverse=False):
        from gansynth_amd import _lib, kernels
        self.lib, self.case = kernels.get().lib, c
        self.mel = np.ascontiguousarray(case_mel(c))
        self.pinv = mel_pinv(c.nbins, c.sample_rate) if with_inverse else None
        frame_length, frame_step, _ = geometry(c.time_steps, c.nbins)
        self.handle = ctypes.c_void_p()
        _lib.check(self.lib.gs_spectral_plan_create(ctypes.byref(self.handle), frame_length, frame_step, c.time_steps, self.mel.ctypes.data,
                                                    self.pinv.ctypes.data if with_inverse else None), "gs_spectral_plan_create")

    def close(self):
        if self.handle:
            self.lib.gs_spectral_plan_destroy(self.handle)
            self.handle = None

    __del__ = close


def _torch_dtype(dtype):
    import torch
    return torch.float32 if dtype == F32 else torch.bfloat16


def _stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def run_fused(plan, w, dtype=F32, ws_bytes=None):
    """gs_stft_mel_if_fwd -> images [b, T, H, 2] (ws_bytes None: what the workspace query asks for)."""
    import torch
    from gansynth_amd import _lib
    c = plan.case
    x = torch.from_numpy(np.array(w, np.float32)).cuda().contiguous()   # (a copy: the cached inputs are read-only)
    images = torch.empty((x.shape[0], c.time_steps, c.nbins, 2), dtype=_torch_dtype(dtype), device="cuda")
    nbytes = plan.lib.gs_stft_mel_if_workspace_bytes(plan.handle, x.shape[0]) if ws_bytes is None else ws_bytes
    ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device="cuda")
    _lib.check(plan.lib.gs_stft_mel_if_fwd(plan.handle, x.data_ptr(), x.shape[0], x.shape[1], front_pad(c), images.data_ptr(), dtype, ws.data_ptr(), nbytes,
                                           _stream()), "gs_stft_mel_if_fwd")
    torch.cuda.synchronize()
    return images


def run_stft(plan, w):
    import torch
    from gansynth_amd import _lib
    c = plan.case
    x = torch.from_numpy(np.array(w, np.float32)).cuda().contiguous()   # (a copy: the cached inputs are read-only)
    mag = torch.empty((x.shape[0], c.time_steps, c.nbins), dtype=torch.float32, device="cuda")
    ph = torch.empty_like(mag)
    _lib.check(plan.lib.gs_stft_fwd(plan.handle, x.data_ptr(), x.shape[0], x.shape[1], front_pad(c), mag.data_ptr(), ph.data_ptr(), _stream()), "gs_stft_fwd")
    torch.cuda.synchronize()
    return mag.cpu().numpy(), ph.cpu().numpy()


def run_mel_project(plan, x):
    import torch
    from gansynth_amd import _lib
    x = torch.as_tensor(np.ascontiguousarray(x, np.float32)).cuda()
    out = torch.empty_like(x)
    _lib.check(plan.lib.gs_mel_project(plan.handle, x.data_ptr(), out.data_ptr(), x.numel() // plan.case.nbins, _stream()), "gs_mel_project")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def run_if_unwrap(plan, mel_phase):
    import torch
    from gansynth_amd import _lib
    x = torch.as_tensor(np.ascontiguousarray(mel_phase, np.float32)).cuda()
    out = torch.empty_like(x)
    _lib.check(plan.lib.gs_if_unwrap(plan.handle, x.data_ptr(), out.data_ptr(), x.shape[0], _stream()), "gs_if_unwrap")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def run_inverse(plan, lm, mi, dtype=F32):
    """gs_mel_if_to_waveform on images built from (lm, mi) [b, T, H] in `dtype` -> waveforms [b, wave_len] (numpy)."""
    import torch
    from gansynth_amd import _lib
    c = plan.case
    images = torch.stack([torch.as_tensor(np.asarray(lm)), torch.as_tensor(np.asarray(mi))], dim=-1).to(_torch_dtype(dtype)).cuda().contiguous()   # [b][T][H][2]
    batch = images.shape[0]
    wave = torch.empty((batch, c.wave_len), dtype=torch.float32, device="cuda")
    nbytes = plan.lib.gs_mel_if_to_waveform_workspace_bytes(plan.handle, batch)
    ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device="cuda")
    _lib.check(plan.lib.gs_mel_if_to_waveform(plan.handle, images.data_ptr(), batch, c.wave_len, front_pad(c), wave.data_ptr(), dtype, ws.data_ptr(),
                                              ws.numel(), _stream()), "gs_mel_if_to_waveform")
    torch.cuda.synchronize()
    return wave.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------ the knob test's child
def save_knob_inputs(path):
    """What a child needs: the case's waveforms, its forward reference (the generic forward route) and the inverse inputs and reference."""
    c = BY_NAME[KNOB_CASE]
    lm, mi = inverse_inputs(c)
    st64, on_cut, branch = forward_reference(c)
    np.savez(path, lm=lm, mi=mi, ref64=inverse_reference(c, lm, mi), on_cut=on_cut, branch=branch,
             **{"st_" + k: st64[k] for k in ("magnitude", "phase", "mel", "mel_magnitude", "mel_phase", "log_mel", "mel_if")})


def knob_child(path):
    """Runs the knob case under this process's environment: inverse always, the fused forward too when GS_SPECTRAL_GENERIC is set.  Prints
    one JSON line: the route the library took (asked with the environment's knobs) and the worst ratios."""
    from gansynth_amd import kernels
    d = np.load(path)
    c = BY_NAME[KNOB_CASE]
    lib = kernels.get().lib
    out = dict(route=case_lib_route(lib, c, k=None))
    plan = Plan(c, with_inverse=True)
    out["inverse"], out["corr"] = compare_inverse(run_inverse(plan, d["lm"], d["mi"]), d["ref64"])
    if "GS_SPECTRAL_GENERIC" in os.environ:
        img = run_fused(plan, waves(c)).float().cpu().numpy()
        st64 = {k[3:]: d[k] for k in d.files if k.startswith("st_")}
        out["forward"] = compare_forward(c, img[..., 0], img[..., 1], ref=(st64, d["on_cut"], d["branch"]))
    plan.close()
    print(json.dumps(out))


if __name__ == "__main__":
    knob_child(sys.argv[1])
