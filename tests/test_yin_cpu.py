"""CPU: the rules of gansynth_amd/pitch.py through the float64 restatement (tests/yin_ref.py) on the synthetic notes -- the parameter choice and
its stability under the fp32 bound of the difference function --, note_statistics / summarize on hand-made arrays, every refusal of the gs_yin
entries (no launch) and of the Python layers, and the driver's flag.  Every figure is printed before it is asserted."""
import functools

import numpy as np
import pytest
import torch

from tests import yin_ref as R

PITCHES = list(range(24, 85))


@functools.lru_cache(maxsize=None)
def _picked(pitch):
    """(lag, period, aperiodicity, ambiguous, power) of the pitch's synthetic note, all float64 rules."""
    d, power = R.synthetic_tracks(pitch)
    return R.pick(d) + (power,)


def test_the_restatement_recovers_the_synthetic_notes():
    """One note per pitch 24 .. 84 as dataset.synthetic_nsynth_input_fn makes it (seed 0), production parameters: all 245 frames voiced and the
    median within 10 cents of the label.  This test carries the parameter choice (W 1024, L 512, hop 256, tau_min 8, threshold 0.15)."""
    cents, voiced, jitter = {}, {}, {}
    for p in PITCHES:
        _, period, aper, _, power = _picked(p)
        assert period.shape == (245,)
        cents[p], jitter[p], voiced[p] = R.note(period, aper, power, p)
    worst = max(PITCHES, key=lambda p: abs(cents[p]))
    low = max((p for p in PITCHES if p <= 72), key=lambda p: abs(cents[p]))
    print(f"worst |median cents| {abs(cents[worst]):.3f} at pitch {worst}; up to pitch 72: {abs(cents[low]):.3f} at {low}; fewest voiced frames "
          f"{min(voiced.values())}; largest jitter {max(jitter.values()):.3f} cents")
    assert all(v == 245 for v in voiced.values())
    assert all(abs(c) < 10.0 for c in cents.values())


def test_the_pick_is_stable_under_the_fp32_bound():
    """Every d of those notes perturbed by a uniform relative error of (W + 8) 2^-24, what gs_yin_difference may be off by: at most 0.1 % of the
    frames change their lag and no note's median moves by 0.01 cent."""
    rng = np.random.default_rng(2002)
    bound = R.dist_bound(R.WINDOW)
    changed, total, moved = 0, 0, 0.0
    for p in PITCHES:
        d, power = R.synthetic_tracks(p)
        lag, period, aper, _, _ = _picked(p)
        lag2, period2, aper2, _ = R.pick(d * (1.0 + rng.uniform(-bound, bound, d.shape)))
        changed += int((lag != lag2).sum())
        total += lag.size
        moved = max(moved, abs(R.note(period2, aper2, power, p)[0] - R.note(period, aper, power, p)[0]))
    print(f"{changed} frames of {total} changed their lag (cap {0.001 * total:.1f}); the largest move of a note's median {moved:.5f} cent")
    assert total == 61 * 245 and changed <= 0.001 * total
    assert moved < 0.01


# ----------------------------------------------------------------------------------------------------------------- the entries' refusals
def _lib():
    from gansynth_amd import _lib as L
    return L.load()


P = 0x10000   # (never dereferenced: the argument checks come first)
GOOD = dict(ldx=64000, rows=2, n=64000, W=1024, L=512, hop=256, tau_min=8)


def _difference(lib, x=P, d=P, power=P, **kw):
    a = dict(GOOD, **kw)
    return lib.gs_yin_difference(x, a["ldx"], a["rows"], a["n"], a["W"], a["L"], a["hop"], d, power, None)


def _track(lib, x=P, lag=P, period=P, aper=P, power=P, **kw):
    a = dict(GOOD, **kw)
    return lib.gs_yin_track(x, a["ldx"], a["rows"], a["n"], a["W"], a["L"], a["hop"], a["tau_min"], 0.15, lag, period, aper, power, None)


def _pick(lib, d=P, lag=P, period=P, aper=P, F=245, **kw):
    a = dict(GOOD, **kw)
    return lib.gs_yin_pick(d, a["rows"], F, a["L"], a["tau_min"], 0.15, lag, period, aper, None)


def test_entry_point_refusals_without_gpu():
    """Every limit of the header, at each entry that has the argument: -1, a message that names the argument, and nothing dereferenced (the
    pointers are not mapped) or launched (there is no device)."""
    lib = _lib()
    frame_cases = [(dict(rows=0), b"rows"), (dict(rows=-3), b"rows"), (dict(hop=0), b"hop"), (dict(hop=-1), b"hop"), (dict(L=1025), b"L must be"),
                   (dict(L=3, tau_min=2), b"L must be"), (dict(W=511), b"W must be"), (dict(W=4097), b"W must be"), (dict(n=1535), b"n 1535 is below W + L"),
                   (dict(ldx=63999), b"ldx"), (dict(rows=2 ** 40), b"rows")]
    for entry, name in ((_difference, b"yin_difference"), (_track, b"yin_track")):
        for kw, message in frame_cases:
            assert entry(lib, **kw) == -1, (name, kw)
            assert message in lib.gs_last_error() and name in lib.gs_last_error(), (name, kw, lib.gs_last_error())
        assert entry(lib, x=None) == -1 and b"null pointer" in lib.gs_last_error()
        assert entry(lib, x=P + 2) == -1 and b"misaligned" in lib.gs_last_error()
        assert entry(lib, power=None) == -1 and b"null pointer" in lib.gs_last_error()
    pick_cases = [(dict(tau_min=1), b"tau_min"), (dict(tau_min=0), b"tau_min"), (dict(tau_min=8, L=9), b"L must be"), (dict(L=1025), b"L must be")]
    for entry, name in ((_pick, b"yin_pick"), (_track, b"yin_track")):
        for kw, message in pick_cases:
            assert entry(lib, **kw) == -1, (name, kw)
            assert message in lib.gs_last_error() and name in lib.gs_last_error(), (name, kw, lib.gs_last_error())
        assert entry(lib, period=P + 4) == -1 and b"misaligned" in lib.gs_last_error()
        assert entry(lib, lag=None) == -1 and b"null pointer" in lib.gs_last_error()
    assert _pick(lib, tau_min=511) == -1 and b"L must be" in lib.gs_last_error()               # tau_min + 2 <= L
    assert _pick(lib, rows=0) == -1 and b"rows" in lib.gs_last_error()
    assert _pick(lib, F=0) == -1 and b"F must be" in lib.gs_last_error()
    assert _pick(lib, d=None) == -1 and b"null pointer" in lib.gs_last_error()
    assert _difference(lib, d=None) == -1 and b"null pointer" in lib.gs_last_error()


def test_frames_without_gpu():
    lib = _lib()
    W, L, hop = 1024, 512, 256
    assert lib.gs_yin_frames(W + L - 1, W, L, hop) == 0 and b"n 1535 is below W + L" in lib.gs_last_error()
    assert lib.gs_yin_frames(W + L, W, L, hop) == 1
    assert lib.gs_yin_frames(W + L + hop - 1, W, L, hop) == 1
    assert lib.gs_yin_frames(W + L + hop, W, L, hop) == 2
    assert lib.gs_yin_frames(64000, W, L, hop) == 245 == R.frames(64000, W, L, hop)
    for n, w, l, h in ((48, 32, 16, 8), (1000, 100, 37, 33), (2307, 257, 129, 1), (1200, 1024, 124, 7), (6000, 4096, 1024, 512)):
        assert lib.gs_yin_frames(n, w, l, h) == R.frames(n, w, l, h) >= 1
    for args, message in (((64000, W, L, 0), b"hop"), ((64000, W, 1025, hop), b"L must be"), ((64000, 4097, L, hop), b"W must be"),
                          ((64000, 256, L, hop), b"W must be"), ((64000, W, 3, hop), b"L must be")):
        assert lib.gs_yin_frames(*args) == 0 and message in lib.gs_last_error(), (args, lib.gs_last_error())


def test_python_layer_refusals_without_gpu():
    from gansynth_amd import kernels, metrics, pitch, spectral_ops
    x = torch.zeros(3, 64000)
    assert kernels.yin_frames(64000, 1024, 512, 256) == 245
    assert kernels.yin_difference_shapes(x, 1024, 512, 256) == (3, 64000, 245)
    assert kernels.yin_track_shapes(x, 1024, 512, 256, 8, 0.15) == (3, 64000, 245)
    assert kernels.yin_track_shapes(torch.zeros(3, 64003)[:, :64000], 1024, 512, 256, 8, 0.15) == (3, 64000, 245)      # row slack is welcome
    assert kernels.yin_pick_shapes(torch.zeros(3, 245, 512), 8, 0.15) == (3, 245, 512)
    for bad, message in ((dict(lags=1025), "lags must be in"), (dict(window=511), "window must be in"), (dict(window=4097), "window must be in"),
                         (dict(hop=0), "hop must be positive"), (dict(hop=2.5), "hop must be an integer"), (dict(tau_min=1), "tau_min must be at least 2"),
                         (dict(tau_min=511), "lags must be in \\[tau_min \\+ 2"), (dict(threshold="a"), "threshold must be a number")):
        args = dict(dict(window=1024, lags=512, hop=256, tau_min=8, threshold=0.15), **bad)
        with pytest.raises(ValueError, match=message):
            kernels.yin_track_shapes(x, **args)
        with pytest.raises(ValueError, match=message):
            pitch.track(x, **args)
    with pytest.raises(ValueError, match="shorter than window \\+ lags"):
        kernels.yin_difference_shapes(torch.zeros(2, 1535), 1024, 512, 256)
    for bad in (torch.zeros(64000, dtype=torch.float64)[None], torch.zeros(0, 64000), torch.zeros(2, 3, 4), "x"):
        with pytest.raises(ValueError, match="yin_difference: x must be"):
            kernels.yin_difference_shapes(bad, 1024, 512, 256)
    for bad in (torch.zeros(3, 245, 512)[:, :, :100], torch.zeros(3, 512), torch.zeros(3, 245, 512, dtype=torch.float64)):
        with pytest.raises(ValueError, match="yin_pick: d must be"):
            kernels.yin_pick_shapes(bad, 8, 0.15)
    with pytest.raises(ValueError, match="waveforms must be a tensor"):
        pitch.track(np.zeros((2, 64000), dtype=np.float32))
    with pytest.raises(ValueError, match="waveforms must be a non-empty"):
        metrics.f0_pitch_accuracy_device(np.zeros(64000, dtype=np.float32), [60])
    with pytest.raises(ValueError, match="2 pitches for 3 notes"):
        metrics.f0_pitch_accuracy_device(x, [60, 61])
    with pytest.raises(ValueError, match="shorter than window"):
        metrics.f0_pitch_accuracy_device(torch.zeros(2, 100), [60, 61])
    with pytest.raises(ValueError, match="sample_rate must be positive"):
        spectral_ops.estimate_f0(x, sample_rate=0)


def test_the_driver_refuses_f0_without_evaluate():
    import gan_synth_main as main
    assert main.parser.parse_args(["--evaluate", "--f0"]).f0 and not main.parser.parse_args(["--evaluate"]).f0
    with pytest.raises(SystemExit, match="--f0 applies to --evaluate only"):
        main.main(main.parser.parse_args(["--f0", "--generate"]))


# ----------------------------------------------------------------------------------------------------------------- rule 5
def _period_for(cents, pitch, rate=16000.0):
    """The period of a tone `cents` above the label."""
    return rate / (R.label_frequency(pitch) * 2.0 ** (cents / 1200.0))


def test_note_statistics_and_summarize_on_hand_made_arrays():
    from gansynth_amd import pitch
    frames = 6
    pitches = [60, 60, 48, 72, 69, 64]
    period, aper, power = np.zeros((6, frames)), np.full((6, frames), 0.01), np.ones((6, frames))
    period[0] = [_period_for(c, 60) for c in (-4.0, -2.0, 0.0, 2.0, 4.0, 6.0)]          # in tune: median 1, std of the six values
    period[1] = 2.0 * _period_for(3.0, 60)                                               # an octave low: -1197 cents, accurate in chroma only
    period[2] = _period_for(5.0, 48)
    aper[2] = 0.15                                                                       # not UNDER the threshold: unvoiced
    period[3] = [_period_for(c, 72) for c in (10.0, 10.0, 10.0, 700.0, 700.0, 700.0)]
    power[3] = [1.0, 0.5, 0.2, 1.0e-4, 0.9e-4, 0.0]                                     # the gate is strict: 1e-4 of the largest is out
    period[4] = [_period_for(c, 69) for c in (30.0, 80.0, 80.0, 80.0, 80.0, 80.0)]
    aper[4] = [0.1, 0.2, 0.3, 0.15, 1.0, 0.5]                                           # a lone voiced frame: median 30, jitter 0
    period[5] = _period_for(70.0, 64)                                                    # voiced, 70 cents sharp: in neither count
    stats = pitch.note_statistics(period, aper, power, pitches)
    print(stats)
    assert stats.voiced.tolist() == [6, 6, 0, 3, 1, 6] and stats.voiced.dtype == np.int64
    want0 = np.array([-4.0, -2.0, 0.0, 2.0, 4.0, 6.0])
    assert abs(stats.cents[0] - 1.0) < 1e-9 and abs(stats.jitter[0] - want0.std()) < 1e-9
    assert abs(stats.cents[1] - (3.0 - 1200.0)) < 1e-9 and stats.jitter[1] < 1e-9
    assert np.isnan(stats.cents[2]) and np.isnan(stats.jitter[2])
    assert abs(stats.cents[3] - 10.0) < 1e-9 and stats.jitter[3] < 1e-9
    assert abs(stats.cents[4] - 30.0) < 1e-9 and stats.jitter[4] == 0.0
    assert abs(stats.cents[5] - 70.0) < 1e-9
    for i in range(6):                                                                   # the restatement, note by note
        c, j, v = R.note(period[i], aper[i], power[i], pitches[i])
        assert v == stats.voiced[i] and (np.isnan(c) if v == 0 else (abs(c - stats.cents[i]) < 1e-9 and abs(j - stats.jitter[i]) < 1e-9))
    figures = pitch.summarize(stats.cents, stats.jitter)
    print(figures)
    assert set(figures) == {"f0_pitch_accuracy", "f0_chroma_accuracy", "f0_median_abs_cents", "f0_jitter_cents", "f0_voiced_fraction"}
    assert figures["f0_pitch_accuracy"] == 3 / 6 and figures["f0_chroma_accuracy"] == 4 / 6 and figures["f0_voiced_fraction"] == 5 / 6
    assert abs(figures["f0_median_abs_cents"] - 10.0) < 1e-9                             # the median of 1, 10, 30
    assert abs(figures["f0_jitter_cents"] - want0.std() / 3.0) < 1e-9
    assert pitch.fold_cents([3.0 - 1200.0, 650.0, -600.0, 599.0]).tolist() == pytest.approx([3.0, -550.0, -600.0, 599.0])
    none = pitch.summarize([np.nan, 300.0], [np.nan, 1.0])
    assert none["f0_pitch_accuracy"] == 0.0 and none["f0_voiced_fraction"] == 0.5 and np.isnan(none["f0_median_abs_cents"]) and np.isnan(none["f0_jitter_cents"])
    with pytest.raises(ValueError, match="must be \\[notes, frames\\] alike"):
        pitch.note_statistics(period, aper[:, :3], power, pitches)
    with pytest.raises(ValueError, match="non-empty vectors alike"):
        pitch.summarize([], [])
    # tensors are taken as they are
    again = pitch.note_statistics(torch.from_numpy(period), torch.from_numpy(aper), torch.from_numpy(power), pitches)
    assert np.array_equal(again.voiced, stats.voiced)
