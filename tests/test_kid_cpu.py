"""CPU: the rules of gansynth_amd/kid.py on hand-made and statistical cases through the restatement (tests/kid_ref.py) and the package's own host
functions (kid.estimate, kid.draw_subsets), every refusal of the Python layers (kernels.kid_sums_shapes, kid, metrics.kernel_inception_distance_
device, the driver's --kid) and the argument checks and host arithmetic of the gs_kid entries -- no device is touched.  Every figure is printed
before it is asserted."""
import argparse

import numpy as np
import pytest
import torch

from tests import kid_ref as DR


def _features(rng, rows, d, shift=0.0):
    return (np.abs(rng.normal(0.5, 0.2, (rows, d))) + shift).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------- the rules
def test_the_hand_example():
    """d = 1, x = {1, 2}, y = {0, 3}: k(1, 2) = 3^3 = 27 both ways, Sxx = 54; k(0, 3) = 1 both ways, Syy = 2; k(1, 0) + k(1, 3) + k(2, 0) + k(2, 3) =
    1 + 64 + 1 + 343 = 409; KID = 54 / 2 + 2 / 2 - 2 * 409 / 4 = -176.5: negative, and nothing clamps it."""
    from gansynth_amd import kid
    x, y = np.array([[1.0], [2.0]], dtype=np.float32), np.array([[0.0], [3.0]], dtype=np.float32)
    s, terms = DR.three_sums(x, y)
    print("sums", s.tolist(), "bound terms", terms.tolist(), "KID", DR.estimate(s, 2, 2))
    assert s.tolist() == [54.0, 2.0, 409.0] and terms.tolist() == [54.0, 2.0, 409.0]       # (non-negative inputs: the bound term is the sum)
    assert DR.estimate(s, 2, 2) == -176.5
    assert kid.estimate([54.0, 2.0, 409.0], 2, 2) == -176.5 and kid.estimate(np.array([[54.0, 2.0, 409.0]] * 2), 2, 2).tolist() == [-176.5, -176.5]
    got = DR.figures(x, y, subsets=2, subset_size=1000, seed=0)                             # size clips to 2: every subset is the whole of both sets
    assert got["kid"] == -176.5 and got["size"] == 2 and got["subset_kids"].tolist() == [-176.5, -176.5]
    assert (got["subset_mean"], got["subset_std"]) == (-176.5, 0.0)


def test_a_set_against_a_permutation_of_itself_and_against_itself():
    """y a permutation of x: the pairs of Syy are the pairs of Sxx, and Sxy holds every i != j pair once and the n pairs of a row with itself:
    Sxy = Sxx + sum_i k(x_i, x_i).  Only the index excludes: against ITSELF the same holds.  The estimate is then 2 Sxx / (n (n - 1)) - 2 Sxy / n^2."""
    from gansynth_amd import kid
    rng = np.random.default_rng(1)
    x = _features(rng, 37, 12)
    own = (np.einsum("ic,ic->i", x.astype(DR.LD), x.astype(DR.LD)) / 12 + 1) ** 3
    for y, what in ((x[rng.permutation(37)], "a permutation"), (x, "itself")):
        s, _ = DR.three_sums(x, y)
        print(f"{what}: Sxx {s[0]!r} Syy {s[1]!r} Sxy {s[2]!r}; Sxx + own pairs {s[0] + own.sum()!r}")
        assert abs(s[1] - s[0]) <= 1e-17 * s[0] and abs(s[2] - (s[0] + own.sum())) <= 1e-17 * s[2]
        want = 2 * s[0] / (37 * 36) - 2 * s[2] / 37 ** 2
        assert abs(DR.estimate(s, 37, 37) - want) <= 1e-17 * s[0] / (37 * 36)
        assert abs(kid.estimate(s.astype(np.float64), 37, 37) - float(want)) <= 8 * DR.U * float(s[0]) / (37 * 36)
        assert DR.estimate(s, 37, 37) < 0        # the own pairs are the largest of their rows: against itself the estimate is negative


def test_unbiased_on_one_distribution_and_positive_on_a_shift():
    """64 trials of two seeded draws of ONE distribution: the mean estimate lies within three standard errors of 0 (a biased estimator's would
    not: the V-statistic's bias here is many standard errors).  With the second set shifted by 0.2 it is positive by many."""
    from gansynth_amd import kid
    same, biased, shifted = [], [], []
    for trial in range(64):
        rng = np.random.default_rng(1000 + trial)
        x, y = _features(rng, 24, 16), _features(rng, 24, 16)
        s, _ = DR.three_sums(x, y)
        same.append(kid.estimate(s.astype(np.float64), 24, 24))
        assert same[-1] == float(DR.estimate(s.astype(np.float64), 24, 24))
        own = sum(float((np.einsum("ic,ic->i", t.astype(np.float64), t.astype(np.float64)) / 16 + 1).__pow__(3).sum()) for t in (x, y))
        biased.append((float(s[0] + s[1]) + own) / 24 ** 2 - 2 * float(s[2]) / 24 ** 2)
        s2, _ = DR.three_sums(x, y + np.float32(0.2))
        shifted.append(kid.estimate(s2.astype(np.float64), 24, 24))
    same, biased, shifted = np.array(same), np.array(biased), np.array(shifted)
    se, se_shifted = same.std(ddof=1) / 8, shifted.std(ddof=1) / 8
    print(f"one distribution: mean {same.mean():.3e}, standard error {se:.3e} ({same.mean() / se:.2f} of them); {int((same < 0).sum())} of 64 negative; "
          f"the biased form: {biased.mean() / (biased.std(ddof=1) / 8):.1f} standard errors; shifted: mean {shifted.mean():.3e}, {shifted.mean() / se_shifted:.1f} standard errors")
    assert abs(same.mean()) <= 3 * se and (same < 0).any() and (same > 0).any()
    assert biased.mean() > 10 * biased.std(ddof=1) / 8
    assert shifted.mean() > 20 * se_shifted and (shifted > 0).all()


def test_draw_subsets_follows_the_stated_sequence():
    from gansynth_amd import kid
    xi, yi = kid.draw_subsets(50, 40, 5, 16, seed=7)
    rng = np.random.default_rng(7)
    for s in range(5):
        assert xi[s].tolist() == rng.choice(50, 16, replace=False).tolist() and yi[s].tolist() == rng.choice(40, 16, replace=False).tolist()
    want = DR.draw_subsets(50, 40, 5, 16, 7)
    assert xi.dtype == np.int32 and yi.dtype == np.int32 and np.array_equal(xi, want[0]) and np.array_equal(yi, want[1])
    assert all(len(set(row.tolist())) == 16 for row in list(xi) + list(yi)) and xi.max() < 50 and yi.max() < 40 and min(xi.min(), yi.min()) >= 0
    xi, yi = kid.draw_subsets(50, 12, 3, 1000, seed=0)                                      # clipped to the smaller set: a permutation of it
    assert xi.shape == yi.shape == (3, 12) and all(sorted(row.tolist()) == list(range(12)) for row in yi)
    assert not np.array_equal(kid.draw_subsets(50, 40, 2, 16, seed=1)[0], kid.draw_subsets(50, 40, 2, 16, seed=2)[0])
    empty = kid.draw_subsets(50, 40, 0, 16)
    assert empty[0].shape == empty[1].shape == (0, 16)


# ------------------------------------------------------------------------------------------------------------- Python layers
def _raises(fn, *args, match, **kw):
    with pytest.raises(ValueError, match=match):
        fn(*args, **kw)


def test_host_refusals_name_the_argument():
    from gansynth_amd import kernels, kid, metrics
    x = np.zeros((10, 6), dtype=np.float32)
    for fn, what in ((kid.figures, "kid"), (metrics.kernel_inception_distance_device, "kernel_inception_distance_device")):
        _raises(fn, x[:1], x, match=f"{what}: real must have at least 2 rows \\(got 1\\)")
        _raises(fn, x, x[:1], match=f"{what}: fake must have at least 2 rows \\(got 1\\)")
        _raises(fn, x, x[:, :5], match=f"{what}: real and fake differ in width \\(6 and 5\\)")
        _raises(fn, x[0], x, match="real must be a \\[rows, columns\\] matrix")
        for bad in (-1, 1.5, None, True):
            _raises(fn, x, x, subsets=bad, match="subsets must be an integer >= 0")
        for bad in (1, 0, -3, 2.0):
            _raises(fn, x, x, subset_size=bad, match="subset_size must be an integer >= 2")
    _raises(metrics.kernel_inception_distance_device, [[0.0]], x, match="real_features must be a")
    assert kid.check_sets(x, x[:7], 100, 1000) == 7 and kid.check_sets(x, x, 0, 4) == 4
    _raises(kid.draw_subsets, 1, 5, 2, 2, match="draw_subsets: n must be an integer >= 2")
    _raises(kid.draw_subsets, 5, 1, 2, 2, match="draw_subsets: m must be an integer >= 2")
    _raises(kid.draw_subsets, 5, 5, -1, 2, match="draw_subsets: subsets must be an integer >= 0")
    _raises(kid.draw_subsets, 5, 5, 2, 1, match="draw_subsets: subset_size must be an integer >= 2")
    _raises(kid.estimate, [1.0, 2.0], 3, 3, match="estimate: sums must end in the three sums")
    _raises(kid.estimate, [1.0, 2.0, 3.0], 1, 3, match="estimate: n must be an integer >= 2")
    assert kid.KidResult._fields == ("kid", "subset_mean", "subset_std", "subset_kids", "sums", "subset_sums", "size")
    # kernels.kid_sums: the shapes and the lists, before a device is asked for
    a, b = torch.zeros(10, 6), torch.zeros(7, 6)
    good = np.tile(np.arange(5), (3, 1))
    assert kernels.kid_sums_shapes(a, b) == (10, 7, 6, 0, 0) and kernels.kid_sums_shapes(a, b, good, torch.from_numpy(good)) == (10, 7, 6, 3, 5)
    assert kernels.kid_sums_shapes(torch.zeros(10, 9)[:, :6], b, good.astype(np.int32), good) == (10, 7, 6, 3, 5)   # row slack is welcome
    for bad in (np.zeros((10, 6), dtype=np.float32), torch.zeros(10), torch.zeros(10, 6, dtype=torch.float64), torch.zeros(0, 6)):
        _raises(kernels.kid_sums_shapes, bad, b, match="kid_sums: x must be")
    for bad in (torch.zeros(7, 5), torch.zeros(7, 6, dtype=torch.float16), None):
        _raises(kernels.kid_sums_shapes, a, bad, match="kid_sums: y must be")
    _raises(kernels.kid_sums_shapes, a[:1], b, match="kid_sums: x must have at least 2 rows \\(got 1\\)")
    _raises(kernels.kid_sums_shapes, a, b[:1], match="kid_sums: y must have at least 2 rows \\(got 1\\)")
    _raises(kernels.kid_sums_shapes, a, b, good, None, match="kid_sums: yi must be a \\[subsets, size\\] integer")
    _raises(kernels.kid_sums_shapes, a, b, None, good, match="kid_sums: xi must be a \\[subsets, size\\] integer")
    for bad in (good.astype(np.float32), good[0], good[:0], good.tolist()):
        _raises(kernels.kid_sums_shapes, a, b, bad, good, match="kid_sums: xi must be a \\[subsets, size\\] integer")
    _raises(kernels.kid_sums_shapes, a, b, good[:, :1], good[:, :1], match="kid_sums: xi holds subsets of size 1: size must be at least 2")
    _raises(kernels.kid_sums_shapes, a, b, good, good[:2], match="kid_sums: xi and yi differ in shape")
    _raises(kernels.kid_sums_shapes, a, b, good + 6, good, match="kid_sums: xi holds an index outside its set of 10 rows \\(10\\)")
    _raises(kernels.kid_sums_shapes, a, b, good, good + 3, match="kid_sums: yi holds an index outside its set of 7 rows \\(7\\)")
    _raises(kernels.kid_sums_shapes, a, b, good - 1, good, match="kid_sums: xi holds an index outside its set of 10 rows \\(-1\\)")
    wide = np.tile(np.arange(8) % 7, (2, 1))
    _raises(kernels.kid_sums_shapes, a, b, wide, wide, match="kid_sums: xi holds subsets of size 8, above the smaller set's 7 rows")
    _raises(kernels.kid_sums, a, torch.zeros(7, 5), match="y must be")                      # the wrapper refuses before a device is asked for
    _raises(kernels.kid_sums, a, b, good + 6, good, match="index outside its set")


def test_the_driver_refuses_kid_without_a_classifier():
    import gan_synth_main as main
    good = dict(evaluate=True, kid=True, kid_subsets=100, kid_subset_size=1000, classifier="pitch_classifier.pb")
    assert main.check_kid_args(argparse.Namespace(**good)) is True
    assert main.check_kid_args(argparse.Namespace(**dict(good, kid=False))) is False
    assert main.check_kid_args(main.parser.parse_args(["--evaluate", "--kid", "--kid_subsets", "0", "--kid_subset_size", "50"])) is True
    defaults = main.parser.parse_args([])
    assert defaults.kid is False and (defaults.kid_subsets, defaults.kid_subset_size) == (100, 1000)
    for change, message in ((dict(classifier="none"), "--kid needs the pitch classifier"), (dict(classifier="None"), "--kid needs the pitch classifier"),
                            (dict(evaluate=False), "--kid applies to --evaluate only"), (dict(kid_subsets=-1), "--kid_subsets must not be negative"),
                            (dict(kid_subset_size=1), "--kid_subset_size must be at least 2"), (dict(kid=False, kid_subsets=5), "need --kid"),
                            (dict(kid=False, kid_subset_size=5), "need --kid")):
        with pytest.raises(SystemExit, match=message):
            main.check_kid_args(argparse.Namespace(**dict(good, **change)))
    with pytest.raises(SystemExit, match="--kid needs the pitch classifier"):       # main() itself: refused before anything is loaded
        main.main(main.parser.parse_args(["--evaluate", "--kid", "--classifier", "none"]))
    assert all(flag in main.__doc__ for flag in ("--kid", "--kid_subsets", "--kid_subset_size"))


# ------------------------------------------------------------------------------------------------------------- the C entries
def _tiles(rx, ry):
    tx, ty = -(-rx // 128), -(-ry // 128)
    return tx * (tx + 1) // 2 + ty * (ty + 1) // 2 + tx * ty


def test_workspace_arithmetic():
    from gansynth_amd import _lib
    lib = _lib.load()
    assert (_lib.KID_TILE, _lib.KID_MAX_ROWS, _lib.KID_MAX_SUBSETS) == (128, 2 ** 21, 65535)
    # 50 000 rows a side: 391 tiles a side, 76 636 a triangle, 152 881 the square: 306 153 doubles
    by_hand = [((50000, 50000, 0, 0), 306153), ((2, 2, 0, 0), 3), ((128, 129, 0, 0), 1 + 3 + 2), ((5000, 3000, 100, 1000), 100 * (36 + 36 + 64)),
               ((547, 291, 3, 257), 3 * (6 + 6 + 9)), ((2 ** 21, 2 ** 21, 0, 0), 2 ** 14 * (2 ** 14 + 1) + 2 ** 28)]
    for (n, m, subsets, size), doubles in by_hand:
        got = lib.gs_kid_workspace_bytes(n, m, 512, subsets, size)
        print(f"n {n} m {m} subsets {subsets} size {size}: {got} bytes, by hand {doubles} doubles")
        assert got == -(-8 * doubles // 16) * 16 == -(-8 * max(subsets, 1) * (_tiles(size, size) if subsets else _tiles(n, m)) // 16) * 16
    rng = np.random.default_rng(3)
    for _ in range(300):
        n, m, d = int(rng.integers(2, 400000)), int(rng.integers(2, 400000)), int(rng.integers(1, 1200))
        subsets = int(rng.integers(0, 200))
        size = int(rng.integers(2, min(n, m) + 1)) if subsets else 0
        want = 8 * max(subsets, 1) * (_tiles(size, size) if subsets else _tiles(n, m))
        assert lib.gs_kid_workspace_bytes(n, m, d, subsets, size) == -(-want // 16) * 16, (n, m, subsets, size)
    for n, m, d, subsets, size in ((1, 4, 4, 0, 0), (4, 1, 4, 0, 0), (0, 4, 4, 0, 0), (2 ** 21 + 1, 4, 4, 0, 0), (4, 2 ** 21 + 1, 4, 0, 0), (10, 10, 0, 0, 0),
                                   (10, 10, -3, 0, 0), (10, 10, 2 ** 20 + 1, 0, 0), (10, 10, 4, -1, 0), (10, 10, 4, 65536, 4), (10, 10, 4, 0, 4), (10, 10, 4, 2, 0),
                                   (10, 10, 4, 2, 1), (10, 8, 4, 2, 9), (8, 10, 4, 2, 9)):
        assert lib.gs_kid_workspace_bytes(n, m, d, subsets, size) == 0, (n, m, d, subsets, size)


def test_abi_refusals():
    """Dummy pointers: the argument checks come first, nothing is dereferenced or launched; every message names its argument."""
    from gansynth_amd import _lib
    lib = _lib.load()
    P, n, m, d = 0x10000, 5000, 3000, 24

    def call(a):
        return lib.gs_kid_sums(a["x"], a["ldx"], a["n"], a["y"], a["ldy"], a["m"], a["d"], a["xi"], a["yi"], a["subsets"], a["size"], a["out"], a["ws"],
                               a["ws_bytes"], None)

    full = dict(x=P, ldx=d, n=n, y=P, ldy=d, m=m, d=d, xi=None, yi=None, subsets=0, size=0, out=P, ws=P, ws_bytes=int(lib.gs_kid_workspace_bytes(n, m, d, 0, 0)))
    batch = dict(full, xi=P, yi=P, subsets=7, size=300, ws_bytes=int(lib.gs_kid_workspace_bytes(n, m, d, 7, 300)))
    assert full["ws_bytes"] > 16 and batch["ws_bytes"] > 16
    shared = [(dict(d=0, ldx=0, ldy=0), b"d must be"), (dict(d=-2), b"d must be"), (dict(d=2 ** 20 + 1, ldx=2 ** 20 + 1, ldy=2 ** 20 + 1), b"d must be"),
              (dict(n=1), b"n must be in"), (dict(n=0), b"n must be in"), (dict(n=2 ** 21 + 1), b"n must be in"), (dict(m=1), b"m must be in"),
              (dict(m=-5), b"m must be in"), (dict(m=2 ** 21 + 1), b"m must be in"), (dict(ldx=d - 1), b"ldx"), (dict(ldy=d - 1), b"ldy"),
              (dict(subsets=-1), b"subsets must be in"), (dict(subsets=65536), b"subsets must be in"),
              (dict(x=None), b"null pointer"), (dict(y=None), b"null pointer"), (dict(out=None), b"null pointer"), (dict(x=P + 2), b"misaligned"),
              (dict(y=P + 1), b"misaligned"), (dict(out=P + 4), b"misaligned"), (dict(ws=None), b"workspace"), (dict(ws=P + 8), b"workspace"),
              (dict(ws_bytes=15), b"workspace"), (dict(ws_bytes=0), b"workspace")]
    cases = [(full, shared + [(dict(xi=P), b"xi and yi must be NULL"), (dict(yi=P), b"xi and yi must be NULL"), (dict(size=300), b"size must be 0"),
                              (dict(ws_bytes=full["ws_bytes"] - 1), b"workspace")]),
             (batch, shared + [(dict(xi=None), b"xi and yi are required"), (dict(yi=None), b"xi and yi are required"), (dict(xi=P + 2), b"misaligned"),
                               (dict(yi=P + 1), b"misaligned"), (dict(size=1), b"size must be in"), (dict(size=0), b"size must be in"),
                               (dict(size=m + 1), b"size must be in"), (dict(ws_bytes=batch["ws_bytes"] - 1), b"workspace"),
                               (dict(subsets=8), b"workspace")])]
    for good, changes in cases:
        for change, message in changes:
            assert call(dict(good, **change)) == -1, change
            print(change, "->", lib.gs_last_error().decode())
            assert message in lib.gs_last_error() and b"kid_sums" in lib.gs_last_error(), (change, lib.gs_last_error())
