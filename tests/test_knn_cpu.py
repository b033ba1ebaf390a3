"""CPU: the rules of gansynth_amd/manifold.py on hand-made cases through the restatement (tests/knn_ref.py), every refusal of the Python layers
(kernels.knn_*_shapes, manifold, metrics.precision_recall_device, the driver's --prd) and the argument checks and host arithmetic of the gs_knn
entries -- no device is touched.  Every figure is printed before it is asserted."""
import argparse

import numpy as np
import pytest
import torch

from tests import knn_ref as NR

REAL = np.array([[0.0], [1.0], [2.0], [10.0]], dtype=np.float32)
FAKE = np.array([[0.5], [3.5], [20.0]], dtype=np.float32)


# ------------------------------------------------------------------------------------------------------------- the rules
def test_the_hand_example():
    """real = {0, 1, 2, 10}, fake = {0.5, 3.5, 20}, k = 1.  Real radii^2 1, 1, 1, 64: 0.5 lies in the balls of 0 and 1, 3.5 in that of 10 (42.25 <=
    64), 20 in none (100 > 64): precision 2/3, density 3 / (1 * 3).  Nearest fake of every real row: 0.25, 0.25, 2.25, 42.25 against 1, 1, 1, 64:
    coverage 3/4.  Fake radii^2 9, 9, 272.25: 0, 1, 2 lie in the ball of 0.5 (1 and 2 also in that of 3.5), 10 in that of 20 (100 <= 272.25): recall 1."""
    got = NR.figures(REAL, FAKE, 1)
    print({key: (value.tolist() if hasattr(value, "tolist") else value) for key, value in got.items()})
    assert got["real_radii"].tolist() == [1.0, 1.0, 1.0, 64.0] and got["fake_radii"].tolist() == [9.0, 9.0, 272.25]
    assert got["fake_counts"].tolist() == [2, 1, 0] and got["real_counts"].tolist() == [1, 2, 2, 1]
    assert got["coverage_minima"].tolist() == [0.25, 0.25, 2.25, 42.25]
    assert (got["precision"], got["density"], got["coverage"], got["recall"]) == (2 / 3, 1.0, 3 / 4, 1.0)
    single = NR.figures(REAL, FAKE, 1, np.float32)             # (every number of the example is exact in fp32)
    assert all(single[key] == got[key] for key in ("precision", "recall", "density", "coverage"))


def test_far_apart_sets_and_a_set_against_itself():
    rng = np.random.default_rng(0)
    a, centres = NR.clustered(40, 5, rng)
    b = NR.clustered(30, 5, rng, centres)[0] + np.float32(1000.0)
    far = NR.figures(a, b, 3)
    print("far apart:", {key: far[key] for key in ("precision", "recall", "density", "coverage")})
    assert (far["precision"], far["recall"], far["density"], far["coverage"]) == (0.0, 0.0, 0.0, 0.0)
    same = NR.figures(a, a, 3)
    print("against itself:", {key: same[key] for key in ("precision", "recall", "density", "coverage")})
    assert (same["precision"], same["recall"], same["coverage"]) == (1.0, 1.0, 1.0)
    assert same["density"] >= 4 / 3 and (same["fake_counts"] >= 1).all()   # every ball holds its own row and at least 3 others: 4 M pairs over 3 M
    # the restatement's own edges: +inf where the candidates run out, a NaN radius admits nothing, +inf everything
    assert NR.kth(a[:2], a[:2], 3, True)[0].tolist()[1:] == [np.inf, np.inf] and NR.kth(a[:2], a[:2], 1, True)[0, 0] > 0
    assert NR.within(a, a[:3], [np.nan, np.inf, 0.0]).tolist() == [1, 1, 2] + [1] * 37
    assert NR.ambiguous_pairs(a[:3], a[:3], NR.kth(a[:3], a[:3], 1, True)[:, 0], 5).sum() >= 3


# ------------------------------------------------------------------------------------------------------------- Python layers
def _raises(fn, *args, match, **kw):
    with pytest.raises(ValueError, match=match):
        fn(*args, **kw)


def test_shapes_refusals_name_the_argument():
    from gansynth_amd import kernels
    a, b, r = torch.zeros(10, 6), torch.zeros(7, 6), torch.zeros(7)
    assert kernels.knn_kth_shapes(a, b, 3) == (10, 7, 6) and kernels.knn_kth_shapes(a, a, 8) == (10, 10, 6)
    assert kernels.knn_kth_shapes(torch.zeros(10, 9)[:, :6], b, 1) == (10, 7, 6)            # row slack is welcome
    assert kernels.knn_within_shapes(a, b, r) == (10, 7, 6)
    for bad in (np.zeros((10, 6), dtype=np.float32), torch.zeros(10), torch.zeros(10, 6, dtype=torch.float64), torch.zeros(0, 6)):
        _raises(kernels.knn_kth_shapes, bad, b, 3, match="knn_kth: a must be")
        _raises(kernels.knn_within_shapes, bad, b, r, match="knn_within: q must be")
    for bad in (torch.zeros(7, 5), torch.zeros(6), torch.zeros(7, 6, dtype=torch.float16), torch.zeros(0, 6), None):
        _raises(kernels.knn_kth_shapes, a, bad, 3, match="knn_kth: b must be")
        _raises(kernels.knn_within_shapes, a, bad, r, match="knn_within: ref must be")
    for bad in (0, 9, -1, 2.0, None, True):
        _raises(kernels.knn_kth_shapes, a, b, bad, match="knn_kth: k must be an integer in \\[1, 8\\]")
    for bad in (torch.zeros(6), torch.zeros(7, dtype=torch.float64), torch.zeros(7, 1), torch.zeros(14)[::2], [0.0] * 7):
        _raises(kernels.knn_within_shapes, a, b, bad, match="knn_within: radius2 must be")
    wide = torch.zeros(1, 2 ** 20 + 1)
    _raises(kernels.knn_kth_shapes, wide, wide, 1, match="knn_kth: a must have at most 1048576 columns")
    _raises(kernels.knn_within_shapes, wide, wide, torch.zeros(1), match="knn_within: q must have at most 1048576 columns")
    # the wrappers refuse before a device is asked for
    _raises(kernels.knn_kth, a, torch.zeros(7, 5), 3, match="b must be")
    _raises(kernels.knn_kth, a, b, 9, match="k must be")
    _raises(kernels.knn_within, a, b, r[:6], match="radius2 must be")


def test_manifold_and_metrics_refuse_on_the_host():
    from gansynth_amd import manifold, metrics
    x = np.zeros((10, 6), dtype=np.float32)
    for fn, what in ((manifold.figures, "manifold"), (metrics.precision_recall_device, "precision_recall_device")):
        _raises(fn, x[:3], x, 3, match=f"{what}: real must have at least k \\+ 1 = 4 rows \\(got 3\\)")
        _raises(fn, x, x[:3], 3, match=f"{what}: fake must have at least k \\+ 1 = 4 rows \\(got 3\\)")
        _raises(fn, torch.zeros(2, 6), torch.zeros(9, 6), 2, match="real must have at least k \\+ 1 = 3 rows")
        _raises(fn, x, x[:, :5], 3, match=f"{what}: real and fake differ in width \\(6 and 5\\)")
        _raises(fn, x[0], x, 3, match="real must be a \\[rows, columns\\] matrix")
        for bad in (0, 9, 1.5):
            _raises(fn, x, x, bad, match="k must be an integer in \\[1, 8\\]")
    _raises(metrics.precision_recall_device, [[0.0]], x, match="real_features must be a")
    assert manifold.ManifoldResult._fields[:4] == ("precision", "recall", "density", "coverage")


def test_the_driver_refuses_prd_without_a_classifier():
    import gan_synth_main as main
    good = dict(evaluate=True, prd=True, prd_k=3, classifier="pitch_classifier.pb")
    assert main.check_prd_args(argparse.Namespace(**good)) is True
    assert main.check_prd_args(argparse.Namespace(**dict(good, prd=False))) is False
    assert main.check_prd_args(main.parser.parse_args(["--evaluate", "--prd", "--prd_k", "5"])) is True
    assert main.parser.parse_args([]).prd is False and main.parser.parse_args([]).prd_k == 3
    for change, message in ((dict(classifier="none"), "--prd needs the pitch classifier"), (dict(classifier="None"), "--prd needs the pitch classifier"),
                            (dict(evaluate=False), "--prd applies to --evaluate only"), (dict(prd_k=0), "--prd_k must be in"), (dict(prd_k=9), "--prd_k must be in"),
                            (dict(prd=False, prd_k=5), "--prd_k needs --prd")):
        with pytest.raises(SystemExit, match=message):
            main.check_prd_args(argparse.Namespace(**dict(good, **change)))
    with pytest.raises(SystemExit, match="--prd needs the pitch classifier"):       # main() itself: refused before a device is asked for
        main.main(main.parser.parse_args(["--evaluate", "--prd", "--classifier", "none"]))
    assert "--prd" in main.__doc__ and "--prd_k" in main.__doc__


# ------------------------------------------------------------------------------------------------------------- the C entries
def test_slices_and_workspace_arithmetic():
    from gansynth_amd import _lib
    lib = _lib.load()
    assert (_lib.KNN_MAX_K, _lib.KNN_BLOCKS, _lib.KNN_MIN_SLICE_ROWS) == (8, 3072, 256)
    # 8192 rows: 32 tiles, 96 slices wanted, 86 rows each -> the floor of 256: 32 slices, 1024 blocks on 256 CUs
    by_hand = [((8192, 8192), 32), ((50000, 50000), 16), ((289205, 289205), 3), ((2 ** 20, 64), 1), ((2 ** 20, 2 ** 20), 1), ((2, 2), 1), ((5, 547), 3),
               ((1, 2 ** 31 - 1), 3072)]
    for (n, m), want in by_hand:
        got = lib.gs_knn_slices(n, m, 512)
        print(f"n {n} m {m}: library {got} slices, restatement {NR.slices(n, m)}, by hand {want}; workspace at k = 3: {lib.gs_knn_workspace_bytes(n, m, 512, 3)}")
        assert got == NR.slices(n, m) == want
        assert lib.gs_knn_workspace_bytes(n, m, 512, 3) == NR.workspace_bytes(n, m, 3) == (16 if want == 1 else -(-4 * want * n * 3 // 16) * 16)
    assert lib.gs_knn_slices(8192, 8192, 512) > 1 and lib.gs_knn_slices(2 ** 20, 64, 512) == 1
    assert lib.gs_knn_workspace_bytes(8192, 8192, 512, 3) > lib.gs_knn_workspace_bytes(8192, 4096, 512, 3) > lib.gs_knn_workspace_bytes(8192, 256, 512, 3)
    rng = np.random.default_rng(2)
    for _ in range(300):
        n, m, d, k = int(rng.integers(1, 400000)), int(rng.integers(1, 400000)), int(rng.integers(1, 1200)), int(rng.integers(1, 9))
        assert lib.gs_knn_slices(n, m, d) == NR.slices(n, m), (n, m)
        assert lib.gs_knn_workspace_bytes(n, m, d, k) == NR.workspace_bytes(n, m, k), (n, m, k)
    for n, m, d, k in ((0, 4, 4, 2), (-1, 4, 4, 2), (2 ** 31, 4, 4, 2), (4, 0, 4, 2), (4, 2 ** 31, 4, 2), (10, 10, 0, 2), (10, 10, -3, 2), (10, 10, 2 ** 20 + 1, 2),
                       (10, 10, 4, 0), (10, 10, 4, 9)):
        assert lib.gs_knn_workspace_bytes(n, m, d, k) == 0, (n, m, d, k)
        assert k in (0, 9) or lib.gs_knn_slices(n, m, d) == 0, (n, m, d)


def test_abi_refusals():
    """Dummy pointers: the argument checks come first, nothing is dereferenced or launched; every message names its argument."""
    from gansynth_amd import _lib
    lib = _lib.load()
    P, n, m, d, k = 0x10000, 5000, 3000, 24, 3
    ws = int(lib.gs_knn_workspace_bytes(n, m, d, k))
    assert ws > 16 and int(lib.gs_knn_workspace_bytes(n, m, d, 1)) > 16
    good = dict(a=P, lda=d, n=n, b=P, ldb=d, m=m, d=d, k=k, out=P, radius2=P, ws=P, ws_bytes=ws)

    def kth(a):
        return lib.gs_knn_kth(a["a"], a["lda"], a["n"], a["b"], a["ldb"], a["m"], a["d"], a["k"], 1, a["out"], a["ws"], a["ws_bytes"], None)

    def within(a):
        return lib.gs_knn_within(a["a"], a["lda"], a["n"], a["b"], a["ldb"], a["m"], a["d"], a["radius2"], a["out"], a["ws"], a["ws_bytes"], None)

    shape = [(dict(d=0, lda=0, ldb=0), b"d must be"), (dict(d=-2), b"d must be"), (dict(d=2 ** 20 + 1, lda=2 ** 20 + 1, ldb=2 ** 20 + 1), b"d must be"),
             (dict(n=0), b"n must be in"), (dict(n=2 ** 31), b"n must be in"), (dict(m=0), b"m must be in"), (dict(m=-5), b"m must be in"), (dict(m=2 ** 31), b"m must be in")]
    pointers = [(dict(a=None), b"null pointer"), (dict(b=None), b"null pointer"), (dict(out=None), b"null pointer"), (dict(a=P + 2), b"misaligned"),
                (dict(b=P + 1), b"misaligned"), (dict(out=P + 3), b"misaligned"), (dict(ws=None), b"workspace"), (dict(ws=P + 8), b"workspace"),
                (dict(ws_bytes=15), b"workspace"), (dict(ws_bytes=0), b"workspace")]
    for entry, name, extra in ((kth, b"knn_kth", [(dict(k=0), b"k must be in"), (dict(k=9), b"k must be in"), (dict(k=-1), b"k must be in"), (dict(lda=d - 1), b"lda"),
                                                  (dict(ldb=d - 1), b"ldb"), (dict(ws_bytes=ws - 1), b"workspace")]),
                               (within, b"knn_within", [(dict(lda=d - 1), b"ldq"), (dict(ldb=d - 1), b"ldr"), (dict(radius2=None), b"null pointer"),
                                                        (dict(radius2=P + 2), b"misaligned"), (dict(ws_bytes=int(lib.gs_knn_workspace_bytes(n, m, d, 1)) - 1), b"workspace")])):
        for change, message in shape + pointers + extra:
            assert entry(dict(good, **change)) == -1, (name, change)
            print(name.decode(), change, "->", lib.gs_last_error().decode())
            assert message in lib.gs_last_error() and name in lib.gs_last_error(), (change, lib.gs_last_error())
