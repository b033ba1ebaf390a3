"""CPU: the cases of tests/test_spectral_cover_gpu.py exist and mean something (no GPU: gs_spectral_route is host arithmetic).

Route: gs_spectral_route agrees with tests/spectral_cover.py's restatement on every case and on a grid (batch 1..320, T in {3..40, 64, 128}, the
five bin counts, five sample rates, every knob).  Reachability: every compiled kernel instantiation and every value of every route field the
library produces on that grid is produced by a case -- or is listed as reachable through a knob only, and then by the knob case under that
knob; every case takes the route it names.  Conditioning: the float64 oracle alone stays inside the caps check_if puts on the bins it leaves to
the modulo rule.  Sensitivity: a reference with one defect per family lies at least ten tolerances from the true one."""
import ctypes

import numpy as np
import pytest

from tests import spectral_cover as C

GRID_T = tuple(range(3, 41)) + (64, 128)
GRID_BINS = (64, 128, 256, 512, 1024)
GRID_BATCHES = 320
ALL_KNOBS = [C.DEFAULT_KNOBS] + [C.knobs(**k) for _, _, k in C.KNOB_SETTINGS]


@pytest.fixture(scope="module")
def lib():
    from gansynth_amd import _lib
    assert (C.F32, C.BF16) == (_lib.GS_F32, _lib.GS_BF16)
    assert (C.FWD_GENERIC, C.FWD_WAVE) == (_lib.SPEC_FWD_GENERIC, _lib.SPEC_FWD_WAVE)
    assert (C.GEMM_NONE, C.GEMM_F32_64, C.GEMM_F32_128, C.GEMM_SPLIT_ALL, C.GEMM_SPLIT_TWO, C.GEMM_WIDE_256) == (
        _lib.SPEC_GEMM_NONE, _lib.SPEC_GEMM_F32_64, _lib.SPEC_GEMM_F32_128, _lib.SPEC_GEMM_SPLIT_ALL, _lib.SPEC_GEMM_SPLIT_TWO, _lib.SPEC_GEMM_WIDE_256)
    assert (C.ISTFT_NONE, C.ISTFT_WAVE_OLA, C.ISTFT_WAVE_FRAMES, C.ISTFT_BLOCK_FFT) == (
        _lib.SPEC_ISTFT_NONE, _lib.SPEC_ISTFT_WAVE_OLA, _lib.SPEC_ISTFT_WAVE_FRAMES, _lib.SPEC_ISTFT_BLOCK_FFT)
    assert ctypes.sizeof(_lib.GsSpectralRoute) == 4 * len(C.route_row(C.case_route(C.CASES[0]))) and ctypes.sizeof(_lib.GsSpectralKnobs) == 32
    assert sorted(f for f, _ in _lib.GsSpectralKnobs._fields_) == sorted(C.DEFAULT_KNOBS)
    assert C.knobs_unset(), "the cases name the routes of the default knobs"
    return _lib.load()


def _grid_pad(time_steps):
    """front_pad over the grid: 0, odd, even, and more than a hop (of the shortest frame), by T."""
    return (0, 1, 16, 49)[time_steps % 4]


@pytest.fixture(scope="module")
def grid(lib):
    """{route row (int32 words): one (T, bins, sample rate, batch, knobs index)} over the grid, after holding the library's answer against the
    restatement at every point."""
    seen, points = {}, 0
    for nbins in GRID_BINS:
        for sr in C.SAMPLE_RATES:
            mel = C.mel_matrix(nbins, sr)
            digest = C.mel_digest(mel)
            for time_steps in GRID_T:
                pad = _grid_pad(time_steps)
                wave_len = C.geometry(time_steps, nbins)[2] - pad
                for ki, k in enumerate(ALL_KNOBS):
                    for ws in ((None, 0) if ki == 0 and nbins == 1024 else (None,)):   # (the workspace only matters to the wave path's exchange)
                        big = 1 << 40
                        got = np.frombuffer(C.lib_routes(lib, time_steps, nbins, mel, True, 1, GRID_BATCHES, wave_len, pad, big if ws is None else ws, k),
                                            np.int32).reshape(GRID_BATCHES, -1)
                        rows = [C.route_row(C.route(time_steps, nbins, mel, True, b, wave_len, pad, ws, k, digest=digest)) for b in range(1, GRID_BATCHES + 1)]
                        want = np.array(rows, np.int64).astype(np.int32)
                        bad = np.nonzero((got != want).any(1))[0]
                        assert bad.size == 0, (time_steps, nbins, sr, int(bad[0]) + 1, k, got[bad[0]].tolist(), want[bad[0]].tolist())
                        points += GRID_BATCHES
                        for b, row in enumerate(rows):
                            seen.setdefault(row[2:], (time_steps, nbins, sr, b + 1, ki))
    print(f"{points} grid points, {len(seen)} distinct routes")
    return seen


def test_route_agrees_with_the_restatement_on_every_case(lib):
    for c in C.CASES:
        for ws in (None, 0):
            for k in ALL_KNOBS:
                assert C.case_lib_route(lib, c, ws, k) == C.case_route(c, ws, k), (c.name, ws, k)
    # the query refuses what the plan refuses, and answers for the environment when no knob struct is given
    from gansynth_amd import _lib
    out = _lib.GsSpectralRoute()
    mel = C.mel_matrix(64, 8000)
    assert lib.gs_spectral_route(96, 24, 8, mel.ctypes.data, 0, 1, 1, 100, 0, C.F32, 0, None, out) == -1 and b"frame_length" in lib.gs_last_error()
    assert lib.gs_spectral_route(128, 32, 8, None, 0, 1, 1, 100, 0, C.F32, 0, None, out) == -1
    assert lib.gs_spectral_route(128, 32, 8, mel.ctypes.data, 0, 0, 1, 100, 0, C.F32, 0, None, out) == -1
    assert lib.gs_spectral_route(128, 32, 8, mel.ctypes.data, 0, 1, 1, 100, 0, 7, 0, None, out) == -1 and b"dtype" in lib.gs_last_error()
    c = C.BY_NAME[C.KNOB_CASE]
    assert C.case_lib_route(lib, c, k=None) == C.case_route(c)


def _classes(r):
    """The values of a route the kernels branch on, as (field, value) pairs (runs / q / rem by the branches they select)."""
    out = {("fwd_kind", r["fwd_kind"]), ("mz", r["mz"]), ("gemm_kind", r["gemm_kind"]), ("istft_kind", r["istft_kind"]), ("gemm_launches", r["gemm_launches"])}
    out |= {("gemm_launch", (r["gemm_nj"][i], r["gemm_np"][i], r["gemm_kb"][i])) for i in range(r["gemm_launches"])}
    if r["fwd_kind"] == C.FWD_WAVE:
        out |= {("exchange", r["exchange"]), ("span_examples", r["span_examples"]), ("rem", "0" if r["rem"] == 0 else ">0"), ("q", "1" if r["q"] == 1 else ">1")}
    return out


def _row_route(row):
    """route_row without its first two words, back to the fields _classes reads."""
    return dict(fwd_kind=row[0], maxnz=row[1], mz=row[2], mel_cnt=row[3:11], runs=row[11], q=row[12], rem=row[13], exchange=row[14], span_examples=row[15],
                gemm_kind=row[16], gemm_launches=row[17], gemm_nj=row[18:20], gemm_np=row[20:22], gemm_kb=row[22:24], istft_kind=row[24])


def test_every_kernel_and_every_route_value_has_a_case(lib, grid):
    assert len(C.KERNELS) == 32 == len(set(C.KERNELS))
    knob_case = C.BY_NAME[C.KNOB_CASE]
    by_case = {c.name: C.case_kernels(c) for c in C.CASES}
    reached = set().union(*by_case.values())
    missing = [k for k in C.KERNELS if k not in reached and k not in C.KNOB_ONLY]
    assert not missing, f"compiled, but no case runs them under the default knobs: {missing}"
    assert reached <= set(C.KERNELS) and not (reached & set(C.KNOB_ONLY)), sorted(reached & set(C.KNOB_ONLY))
    by_knob = {}
    for env, _, k in C.KNOB_SETTINGS:
        r = C.case_route(knob_case, k=C.knobs(**k))
        assert r != C.case_route(knob_case), f"{env} changes nothing on the knob case"
        by_knob[env] = C.kernels_of(r, C.F32, "inverse") | (C.kernels_of(r, C.F32, "fused") if env == "GS_SPECTRAL_GENERIC" else set())
    for kernel, env in C.KNOB_ONLY.items():
        assert kernel in by_knob[env], (kernel, env)
    # route values: what the library produces anywhere on the grid against what the cases (and the knob case under each knob) produce
    produced = set()
    for row in grid:
        produced |= _classes(_row_route(row))
    for c in C.CASES:   # (the custom matrices are not on the grid)
        produced |= _classes(C.case_lib_route(lib, c))
    covered = set()
    for c in C.CASES:
        r = C.case_route(c)
        for f, v in c.expect.items():
            assert r[f] == v, (c.name, f, r[f], v)
        covered |= _classes(r) | (_classes(C.case_route(c, ws_bytes=0)) if c.name == "w32_b3" else set())
    knob_covered = set()
    for env, _, k in C.KNOB_SETTINGS:
        knob_covered |= _classes(C.case_route(knob_case, k=C.knobs(**k)))
    left = produced - covered
    assert left <= knob_covered, sorted(left - knob_covered, key=str)
    assert {(f, v) for f, v in left if f == "gemm_kind"} == set(C.KNOB_ONLY_VALUES), left
    print(f"{len(reached)} kernels by {len(C.CASES)} cases, {len(C.KNOB_ONLY)} by knobs; route values only knobs reach: {sorted(left, key=str)}")


FORWARD = [c.name for c in C.CASES if c.fwd] + [C.KNOB_CASE]


@pytest.mark.parametrize("name", FORWARD)
def test_the_oracle_alone_stays_inside_the_conditioning_caps(name):
    c = C.BY_NAME[name]
    for i, (on_cut, branch) in enumerate(C.conditioning_shares(c)):
        assert on_cut < 2e-3 and branch < (3e-2 if C.is_tone_row(c, i) else 2e-3), (name, i, on_cut, branch)
    st64, _, _ = C.forward_reference(c)
    assert st64["log_mel"].dtype == np.float64 and st64["mel_if"].shape == (len(C.ref_rows(c)), c.time_steps, c.nbins)
    assert len(C.padding_frames(c)) == max(0, (C.front_pad(c) - 2 * c.nbins) // (c.nbins // 2) + 1)


def test_dense_variant_is_the_oracle():
    c = C.BY_NAME["g128_16k_b3"]
    a = C.stages(c, C.waves(c))
    b = C.stages(c, C.waves(c), mel=C.linear_mel64(c))
    for k in ("magnitude", "mel_magnitude", "log_mel", "mel_if"):
        assert np.array_equal(a[k], b[k]), k


# ------------------------------------------------------------------------------------------------------------ sensitivity
def test_a_frame_from_the_neighbouring_run_is_ten_tolerances_away():
    """The IF of a run's first frame differenced against the frame BEFORE the neighbouring run's last one (t0 - 2 instead of t0 - 1), at every
    run boundary of the case with two-frame and one-frame runs."""
    c = C.BY_NAME["w32_b3"]
    r = C.case_route(c)
    st64, on_cut, branch = C.forward_reference(c)
    ph, ref = st64["mel_phase"], st64["mel_if"]
    least = None
    for run in range(1, r["runs"]):
        t0 = run * r["q"] + min(run, r["rem"])
        if t0 < 2 or t0 - 1 in C.padding_frames(c):
            continue
        d = ph[:, t0] - ph[:, t0 - 2]
        bad = (np.mod(d + np.pi, 2 * np.pi) - np.pi) / np.pi
        plain = ~on_cut[:, t0] & ~branch[:, t0]
        moved = float(np.abs(C.wrap2(bad - ref[:, t0]))[plain].max() / C.TOL_IF)
        least = moved if least is None else min(least, moved)
    assert least is not None and least >= 10, least
    print(f"wrong lead frame: least visible {least:.3g} tolerances")


def test_a_dropped_mel_tap_is_ten_tolerances_away():
    """The last tap of the fullest mel column dropped (the eight-wide matrix; and the eleven-wide caller-supplied one)."""
    for name in ("g128_44k_b4", "c64_eleven_b2"):
        c = C.BY_NAME[name]
        mel = C.case_mel(c)
        m = int((mel != 0).sum(0).argmax())
        k = int(np.nonzero(mel[:, m])[0][-1])
        taps = int((mel[:, m] != 0).sum())
        assert (taps + (taps & 1) if taps <= 8 else taps) == C.case_route(c)["maxnz"]   # (widths up to 8 are padded to even)
        mel64 = C.linear_mel64(c).copy()
        mel64[k, m] = 0
        good = C.forward_reference(c)[0]
        bad = C.stages(c, C.waves(c), mel=mel64)
        lin = np.abs(bad["mel_magnitude"] - good["mel_magnitude"]).max(axis=(1, 2)) / (C.TOL_MEL * good["mel_magnitude"].max(axis=(1, 2)))
        log = np.abs(bad["log_mel"] - good["log_mel"])[..., m].max() / C.TOL_LOG
        # (the linear-domain check, 3e-4 of the maximum everywhere, is the one that sees a light tap ten times over; the log check sees it too)
        assert lin.min() >= 10 and log > 1, (name, m, k, lin, log)
        print(f"{name}: tap {k} of column {m} dropped: {lin.min():.3g} (linear) / {log:.3g} (log) tolerances")


def test_a_dropped_overlap_and_an_unwritten_row_block_are_ten_tolerances_away():
    c = C.BY_NAME["i64_b2"]
    lm, mi = C.inverse_inputs(c)
    good = C.inverse_reference(c, lm, mi)
    bad = C.inverse_reference(c, lm, mi, drop_overlap=(1, 20, 22))     # one of the four frames over output hop 22 of example 1
    moved = np.abs(bad - good)[1].max() / np.abs(good[1]).max() / C.TOL_WAVE
    assert moved >= 10 and np.array_equal(bad[0], good[0]), moved
    c2 = C.BY_NAME["g128_16k_b3"]                                       # 96 stacked rows: the second 64-row block is ragged
    assert 2 * c2.batch * c2.time_steps == 96
    lm2, mi2 = C.inverse_inputs(c2)
    good2 = C.inverse_reference(c2, lm2, mi2)
    bad2 = C.inverse_reference(c2, lm2, mi2, zero_rows_from=64)
    moved2 = min(np.abs(bad2 - good2)[b].max() / np.abs(good2[b]).max() / C.TOL_WAVE for b in (1, 2))   # (rows 64.. are the phases of examples 1 and 2)
    assert moved2 >= 10, moved2
    print(f"dropped overlap {moved:.3g}, unwritten row block {moved2:.3g} tolerances")


def test_bf16_truncation_is_told_from_rounding():
    """Inverse: the reference starts from the widened bf16 values, and one started from TRUNCATED values lies ten tolerances away (the IF is
    summed over time before cos / sin).  Forward: the image tolerance 1e-3 + 2^-8 |ref| admits every round-to-nearest (error <= 2^-8 |ref|) and
    a truncation (error up to 2^-7 |ref|) exceeds it where |ref| > 0.26 -- by less than a factor 2, by construction: a one-ulp defect cannot be
    ten tolerances of a half-ulp bound away."""
    c = C.BY_NAME["i64_b2"]
    assert C.BF16 in c.inv
    lm, mi = C.inverse_inputs(c, C.BF16)
    lt, mt = C.inverse_inputs(c, C.BF16, truncate=True)
    assert np.abs(lm - C.inverse_inputs(c)[0]).max() <= C.BF16_REL * np.abs(lm).max()
    good, bad = C.inverse_reference(c, lm, mi), C.inverse_reference(c, lt, mt)
    moved = min(np.abs(bad - good)[b].max() / np.abs(good[b]).max() / C.TOL_WAVE for b in range(c.batch))
    assert moved >= 10, moved
    f = C.BY_NAME["w32_b3"]
    ref = C.forward_reference(f)[0]["mel_if"][0]
    as32 = ref.astype(np.float32)
    rne = np.abs(C.bf16_round(as32) - ref) / (C.TOL_IF + C.BF16_REL * np.abs(ref))
    trunc = np.abs(C.bf16_round(as32, truncate=True) - ref) / (C.TOL_IF + C.BF16_REL * np.abs(ref))
    assert rne.max() < 1.0 < trunc.max(), (rne.max(), trunc.max())
    print(f"truncated bf16 input: {moved:.3g} tolerances (inverse); forward image {trunc.max():.3g} against {rne.max():.3g} rounded")
