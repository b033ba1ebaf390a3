"""CPU: the loudness meter without a device -- the K-weighting coefficients against the table of BS.1770, gs_loudness_design against
loudness.k_weighting and against tests/loudness_ref.py, the descriptor's matrix powers (the library's chunking restated in numpy agrees with
scipy's sequential filter), the closed forms of EBU Tech 3341 within its +-0.1 LU, the gating's edge cases, the scaling law, every refusal of
the entry points, of kernels.loudness_shapes, of gansynth_amd/loudness.py and of the driver's flags by its message, and the hop and
workspace queries against their formulas."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import loudness_ref as R


def _design(rate):
    from gansynth_amd import _lib
    d = _lib.GsLoudness()
    assert _lib.load().gs_loudness_design(rate, ctypes.byref(d)) == 0, _lib.load().gs_last_error()
    return d


# --------------------------------------------------------------------------------------------------------------------- the design
def test_coefficients_at_48k_are_the_table_of_bs1770():
    from gansynth_amd import loudness
    (b1, a1), (b2, a2), hop = loudness.k_weighting(48000)
    assert hop == 4800
    for got, want in ((b1, R.TABLE_48K[0][0]), (a1, R.TABLE_48K[0][1]), (b2, R.TABLE_48K[1][0]), (a2, R.TABLE_48K[1][1])):
        assert got.dtype == np.float64 and np.abs(got - np.array(want)).max() <= 1e-12, (got, want)
    for got, want in zip(R.coefficients(48000), R.TABLE_48K):          # the restatement's own arithmetic too
        assert np.abs(got[0] - np.array(want[0])).max() <= 1e-12 and np.abs(got[1] - np.array(want[1])).max() <= 1e-12


@pytest.mark.parametrize("rate", [16000, 44100, 48000, 8000, 192000, 22050])
def test_design_matches_k_weighting_and_the_restatement(rate):
    from gansynth_amd import loudness
    d = _design(rate)
    (b1, a1), (b2, a2), hop = loudness.k_weighting(rate)
    for got, want in ((b1, d.b1), (a1, d.a1), (b2, d.b2), (a2, d.a2)):
        assert np.array_equal(got.view(np.uint64), np.array(want, dtype=np.float64).view(np.uint64))          # bit for bit
    assert hop == d.hop == R.hop_of(rate) == math.floor(0.1 * rate + 0.5) and abs(hop - 0.1 * rate) <= 0.5
    for got, want in zip(((b1, a1), (b2, a2)), R.coefficients(rate)):   # another tan and another power: a few ulp
        assert np.abs(got[0] - want[0]).max() <= 1e-14 and np.abs(got[1] - want[1]).max() <= 1e-14
    # the chunking: odd chunks (a conflict-free LDS stride), at most 256 lanes, the last lane's rest
    assert d.chunk == (-(-hop // 256)) | 1 and d.chunk % 2 == 1 and d.lanes == -(-hop // d.chunk) <= 256
    assert d.rem == hop - (d.lanes - 1) * d.chunk and 1 <= d.rem <= d.chunk and d.reserved == 0
    # the matrix powers against numpy's: A applied to a state is one silent sample of both sections
    A = np.array([[-a1[1], 1, 0, 0], [-a1[2], 0, 0, 0], [b2[1] - a2[1] * b2[0], 0, -a2[1], 1], [b2[2] - a2[2] * b2[0], 0, -a2[2], 0]])
    s = np.array([[0.3, -0.2, 0.7, 0.1]])
    assert np.allclose(R._run(((b1, a1), (b2, a2)), np.zeros((1, 1)), s)[1][0], A @ s[0], rtol=0, atol=1e-15)
    # (absolute: a state is of the size of the samples, so what counts is the error against 1, not against an entry that has decayed to
    #  1e-39.  The high-pass's two poles nearly coincide (Q = 0.5003: an eigenvector condition of about 1e4), so two orders of multiplying
    #  A^e out differ by about e * 2^-53 * 1e4 of an entry -- 6e-10 at e = 608, where the entries reach 29; one sample more or fewer changes
    #  A^chunk by 5e-3 of its entries.  1e-7 tells the two apart.  The test after this one holds the powers to what they are for.)
    cp, hp, rp = (np.array(m).reshape(-1, 4, 4) for m in (d.chunk_pow, d.hop_pow, d.rem_pow))
    for k in range(8):
        for got, e in ((cp[k], d.chunk << k), (hp[k], hop << k)):
            want = np.linalg.matrix_power(A, e)
            assert np.abs(got - want).max() <= 1e-7 * max(1.0, np.abs(want).max()), (k, e)
    assert np.abs(rp[0] - np.linalg.matrix_power(A, d.rem)).max() <= 1e-7 * max(1.0, np.abs(rp[0]).max())


@pytest.mark.parametrize("rate,hops", [(16000, 300), (44100, 7), (48000, 9), (8000, 5), (192000, 3)])
def test_the_descriptor_carries_the_states_of_the_sequential_filter(rate, hops):
    """The library's chunking, restated with the descriptor's numbers (tests/loudness_ref.py chunked_f64: 300 hops cross a tile of the
    carry), against scipy's filter on noise over a DC offset: float64 against float64."""
    from gansynth_amd import loudness
    d = _design(rate)
    coef = loudness.k_weighting(rate)[:2]
    cp, hp, rp = (np.array(m).reshape(-1, 4, 4) for m in (d.chunk_pow, d.hop_pow, d.rem_pow))
    g = np.random.default_rng(rate)
    x = (g.uniform(-0.25, 0.25, hops * d.hop + 17) + 0.6).astype(np.float32)
    got = R.chunked_f64(x, coef, d.hop, d.chunk, cp, hp, rp[0])
    e = R.error(got[None], R.energy_f64(x, rate))
    print(f"rate {rate}: chunked float64 against lfilter {e:.3g}")
    assert e <= 1e-9


# --------------------------------------------------------------------------------------------------------------------- the rule
def _tone(freq, dbfs, seconds, rate=48000):
    return (10.0 ** (dbfs / 20.0)) * np.sin(2 * np.pi * freq * np.arange(int(seconds * rate)) / rate)


def _lufs(x, rate=48000):
    from gansynth_amd import loudness
    return loudness.integrated(R.energy_f64(x, rate), R.hop_of(rate))


def test_closed_forms_within_the_meter_tolerance():
    one = _lufs(np.stack([_tone(997, 0, 20), np.zeros(20 * 48000)]))
    both = _lufs(np.stack([_tone(1000, -23, 20)] * 2))
    seq = np.concatenate([_tone(1000, -36, 10), _tone(1000, -23, 60), _tone(1000, -36, 10)])
    gated = _lufs(np.stack([seq, seq]))
    print(f"997 Hz 0 dBFS one channel {one:.4f} (-3.01), 1 kHz -23 dBFS both {both:.4f} (-23.0), -36 / -23 / -36 gated {gated:.4f} (-23.0)")
    assert abs(one + 3.01) <= 0.1 and abs(one + 3.0103) <= 1e-3
    assert abs(both + 23.0) <= 0.1 and abs(gated + 23.0) <= 0.1
    assert abs(one - R.lufs_of(np.stack([_tone(997, 0, 20), np.zeros(20 * 48000)]), 48000)) <= 1e-9     # loudness.integrated and the restatement's


def test_gating_edge_cases():
    from gansynth_amd import loudness
    assert loudness.integrated(np.zeros((2, 50)), 4800) == -math.inf                        # silence
    assert loudness.integrated(np.full((1, 3), 100.0), 4800) == -math.inf                   # fewer than 4 hops
    assert loudness.integrated(np.zeros((2, 0)), 4800) == -math.inf
    assert loudness.integrated(np.full(50, 4800 * 1e-9), 4800) == -math.inf                 # -90.7 LUFS: under the absolute gate
    assert math.isfinite(loudness.integrated(np.full(4, 100.0), 4800))
    for bad in (np.nan, np.inf):
        e = np.full((2, 10), 5.0)
        e[1, 7] = bad
        with pytest.raises(ValueError, match="not all finite"):
            loudness.integrated(e, 4800)
    with pytest.raises(ValueError, match="negative"):
        loudness.integrated(np.array([1.0, -1.0, 1.0, 1.0]), 4800)
    with pytest.raises(ValueError, match="hop a positive integer"):
        loudness.integrated(np.ones(8), 0)
    # the relative gate: a quiet passage (20 LU down) does not pull the result down
    e = np.concatenate([np.full(100, 4800 * 1e-2), np.full(100, 4800 * 1e-4)])
    kept = [1e-2] * 97 + [(3e-2 + 1e-4) / 4, (2e-2 + 2e-4) / 4, (1e-2 + 3e-4) / 4]           # the loud blocks and the three that straddle the change
    assert abs(loudness.integrated(e, 4800) - (-0.691 + 10 * math.log10(sum(kept) / 100))) <= 1e-9
    assert abs(loudness.integrated(e, 4800) - (-0.691 - 20.0)) <= 0.1
    assert abs(R.integrated(e, 4800) - loudness.integrated(e, 4800)) <= 1e-12


@pytest.mark.parametrize("g", [0.01, 0.5, 3.0])
def test_scaling_moves_the_loudness_by_20_log10(g):
    rng = np.random.default_rng(5)
    n = 6 * 48000
    env = np.where(np.arange(n) < 3 * 48000, 1.0, 0.45)                      # two levels 6.9 LU apart: both above the relative gate
    x = rng.uniform(-0.3, 0.3, (2, n)) * env
    e = R.energy_f64(x, 48000)
    margin = R.gate_margin(e, 4800)
    assert margin > 0.5, margin
    assert R.gate_margin(R.energy_f64(g * x, 48000), 4800) > 0.5
    assert abs(_lufs(g * x) - _lufs(x) - 20 * math.log10(g)) <= 1e-9


# --------------------------------------------------------------------------------------------------------------------- refusals
def test_loudness_shapes_refusals_name_the_argument():
    from gansynth_amd import kernels
    x = torch.zeros(2, 100)
    assert kernels.loudness_shapes(x, 48000) == (2, 100) and kernels.loudness_shapes(x[0], 16000) == (1, 100)
    assert kernels.loudness_shapes(x, np.int64(44100)) == (2, 100)
    for bad in (torch.zeros(3, 100), ):
        with pytest.raises(ValueError, match="1 or 2 rows"):
            kernels.loudness_shapes(bad, 48000)
    for bad in (torch.zeros(2, 100, dtype=torch.float64), torch.zeros(2, 0), torch.zeros(1, 2, 100), np.zeros(100, dtype=np.float32), None):
        with pytest.raises(ValueError, match="x must be a non-empty fp32"):
            kernels.loudness_shapes(bad, 48000)
    for bad in (7999, 192001, 0, -48000, 48000.0, True, None, "48000"):
        with pytest.raises(ValueError, match="rate must be an integer"):
            kernels.loudness_shapes(x, bad)
    with pytest.raises(ValueError, match="rate must be an integer"):     # refused before a device is asked for
        kernels.loudness_energy(x, 500)


def test_loudness_module_refusals():
    from gansynth_amd import loudness
    with pytest.raises(ValueError, match="rate must be in"):
        loudness.k_weighting(7999)
    with pytest.raises(ValueError, match="rate must be in"):
        loudness.k_weighting(192001)
    with pytest.raises(ValueError, match="rate must be an integer"):
        loudness.k_weighting(48000.0)
    for fn, extra in ((loudness.measure, (48000,)), (loudness.apply, (48000, -23.0))):
        for bad in (torch.zeros(3, 100), torch.zeros(2, 100, dtype=torch.float64), torch.zeros(0), torch.zeros(1, 1, 5), None):
            with pytest.raises(ValueError, match=r"clip must be \[n\] or \[2, n\] fp32"):
                fn(bad, *extra)
    for bad in (math.nan, math.inf, None, "loud", True):
        with pytest.raises(ValueError, match="target_lufs must be a finite number"):
            loudness.apply(torch.zeros(2, 100), 48000, bad)
    with pytest.raises(ValueError, match="ceiling_db must not be above 0"):     # the limiter's own checks, before any measurement
        loudness.apply(torch.zeros(2, 100), 48000, -23.0, ceiling_db=1.0)
    with pytest.raises(ValueError, match="lookahead_seconds"):
        loudness.apply(torch.zeros(2, 100), 48000, -23.0, lookahead_seconds=1.0)


def test_hop_and_workspace_queries_without_gpu():
    from gansynth_amd import _lib
    lib = _lib.load()
    for rate in (8000, 16000, 44100, 48000, 192000):
        d = _design(rate)
        hop = math.floor(0.1 * rate + 0.5)
        for n in (1, hop - 1, hop, hop + 1, 4 * hop + 1, 60 * rate, 1 << 40):
            hops = n // hop
            assert lib.gs_loudness_hops(ctypes.byref(d), n) == hops, (rate, n)
            for rows in (1, 2):
                assert lib.gs_loudness_workspace_bytes(ctypes.byref(d), rows, n) == rows * max(hops, 1) * 64, (rate, n, rows)
        for rows, n in ((0, 100), (3, 100), (-1, 100), (1, 0), (2, -5), (1, (1 << 40) + 1)):
            assert lib.gs_loudness_workspace_bytes(ctypes.byref(d), rows, n) == 0, (rows, n)
        for n in (0, -1, (1 << 40) + 1):
            assert lib.gs_loudness_hops(ctypes.byref(d), n) == -1 and b"n must be in" in lib.gs_last_error()
    bad = _design(48000)
    bad.hop = 4801
    assert lib.gs_loudness_hops(ctypes.byref(bad), 100000) == -1 and b"does not follow from its rate" in lib.gs_last_error()
    assert lib.gs_loudness_workspace_bytes(ctypes.byref(bad), 1, 100000) == 0
    assert lib.gs_loudness_hops(None, 100000) == -1 and lib.gs_loudness_workspace_bytes(None, 1, 100000) == 0


def test_gs_loudness_refusals_without_gpu():
    """Every GS_ERR_ARG case of include/gansynth_hip.h, with its message; nothing is dereferenced or launched."""
    from gansynth_amd import _lib
    lib = _lib.load()
    for rate in (7999, 192001, 0, -48000):
        assert lib.gs_loudness_design(rate, ctypes.byref(_lib.GsLoudness())) == -1 and b"rate must be in [8000, 192000]" in lib.gs_last_error()
    assert lib.gs_loudness_design(48000, None) == -1 and b"null descriptor" in lib.gs_last_error()
    X, E, WS = 0x100000, 0x200000, 0x300000
    n = 4800 * 5 + 7
    good = dict(x=X, rows=2, n=n, row_stride=n, energy=E, energy_stride=5, ws=WS, ws_bytes=2 * 5 * 64)
    order = ("x", "rows", "n", "row_stride", "energy", "energy_stride", "ws", "ws_bytes")
    bad = [(dict(rows=0), b"rows must be 1 or 2"), (dict(rows=3), b"rows must be 1 or 2"), (dict(n=0), b"n must be in"), (dict(n=-4), b"n must be in"),
           (dict(n=(1 << 40) + 1, row_stride=1 << 41), b"n must be in"),
           (dict(row_stride=n - 1), b"row_stride 24006 is below n 24007"), (dict(energy_stride=4), b"energy_stride 4 is below the 5 hops"),
           (dict(x=None), b"null pointer"), (dict(energy=None), b"null pointer"), (dict(x=X + 2), b"misaligned"), (dict(energy=E + 1), b"misaligned"),
           (dict(ws=None), b"workspace too small or misaligned"), (dict(ws=WS + 8), b"workspace too small or misaligned"),
           (dict(ws_bytes=639), b"workspace too small or misaligned (639 bytes, need 640)")]
    d = _design(48000)
    for change, message in bad:
        a = dict(good, **change)
        assert lib.gs_loudness(ctypes.byref(d), *[a[k] for k in order], None) == -1, change
        assert message in lib.gs_last_error(), (change, lib.gs_last_error())
    # a descriptor that does not follow from its rate: any number of it
    assert lib.gs_loudness(None, *[good[k] for k in order], None) == -1 and b"does not follow from its rate" in lib.gs_last_error()
    for field, value in (("rate", 44100), ("hop", 4799), ("chunk", 21), ("lanes", 252), ("rem", 11), ("reserved", 1)):
        t = _design(48000)
        setattr(t, field, value)
        assert lib.gs_loudness(ctypes.byref(t), *[good[k] for k in order], None) == -1, field
        assert b"does not follow from its rate" in lib.gs_last_error(), field
    for field, index in (("b1", 0), ("a1", 2), ("b2", 1), ("a2", 1), ("rem_pow", 5)):
        t = _design(48000)
        getattr(t, field)[index] = np.nextafter(getattr(t, field)[index], 10.0)
        assert lib.gs_loudness(ctypes.byref(t), *[good[k] for k in order], None) == -1 and b"does not follow" in lib.gs_last_error(), field
    for field in ("chunk_pow", "hop_pow"):
        t = _design(48000)
        getattr(t, field)[7][15] = 1e-3
        assert lib.gs_loudness(ctypes.byref(t), *[good[k] for k in order], None) == -1 and b"does not follow" in lib.gs_last_error(), field
    t = _design(48000)
    t.rate = 7000
    assert lib.gs_loudness(ctypes.byref(t), *[good[k] for k in order], None) == -1 and b"does not follow" in lib.gs_last_error()
    # fewer samples than a hop: accepted, nothing to launch (no device is needed to say so)
    short = dict(good, n=4799, row_stride=4799, energy_stride=0, ws_bytes=128)
    assert lib.gs_loudness(ctypes.byref(d), *[short[k] for k in order], None) == 0


# ------------------------------------------------------------------------------------------------------------------ the driver
def test_driver_flags():
    import gan_synth_main as main
    args = main.parser.parse_args(["--synthesize", "score.mid"])
    assert args.loudness is None and main.check_loudness_args(args) is False and main.check_loudness_args(main.parser.parse_args([])) is False
    args = main.parser.parse_args(["--synthesize", "a.mid", "--loudness", "-16"])
    assert args.loudness == -16.0 and main.check_loudness_args(args) is True and main.check_limit_args(args) is False
    args = main.parser.parse_args(["--synthesize", "a.mid", "--loudness", "-23", "--limit", "-2", "--limit_lookahead", "0.01"])
    assert main.check_loudness_args(args) is True and main.check_limit_args(args) is True
    args = main.parser.parse_args(["--synthesize", "a.mid", "--loudness", "0", "--limit_lookahead", "0.01"])     # the look-ahead without --limit
    assert main.check_limit_args(args) is False and main.check_loudness_args(args) is True
    bad = [(["--synthesize", "a.mid", "--loudness", "nan"], "finite target in LUFS"), (["--synthesize", "a.mid", "--loudness", "inf"], "finite target in LUFS"),
           (["--synthesize", "a.mid", "--loudness=-inf"], "finite target in LUFS"), (["--synthesize", "a.mid", "--loudness", "0.5"], "at most 0"),
           (["--generate", "--loudness", "-16"], "--loudness applies to --synthesize only"),
           (["--synthesize", "a.mid", "--loudness", "-16", "--limit_drive", "9"], "the level is set by --loudness"),
           (["--synthesize", "a.mid", "--loudness", "-16", "--limit", "-1", "--limit_drive", "0"], "the level is set by --loudness"),
           (["--synthesize", "a.mid", "--loudness", "-16", "--limit_lookahead", "-0.001"], "--limit_lookahead must be a non-negative number of seconds"),
           (["--synthesize", "a.mid", "--loudness", "-16", "--limit_lookahead", "nan"], "--limit_lookahead must be a non-negative number of seconds")]
    for argv, message in bad:
        with pytest.raises(SystemExit, match=message):
            main.check_loudness_args(main.parser.parse_args(argv))
    # the limiter's own messages stay as they were, with and without --loudness
    with pytest.raises(SystemExit, match="--limit_drive and --limit_lookahead need --limit"):
        main.check_limit_args(main.parser.parse_args(["--synthesize", "a.mid", "--limit_lookahead", "0.01"]))
    with pytest.raises(SystemExit, match="--limit takes a ceiling in dBFS, at most 0"):
        main.check_limit_args(main.parser.parse_args(["--synthesize", "a.mid", "--loudness", "-16", "--limit", "0.5"]))
    with pytest.raises(SystemExit, match="--loudness applies to --synthesize only"):     # main refuses before it touches a device
        main.main(main.parser.parse_args(["--generate", "--loudness", "-16"]))
    with pytest.raises(SystemExit):
        main.parser.parse_args(["--loudness", "loud"])
