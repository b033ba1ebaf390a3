"""CPU: the host rules of gansynth_amd/kmeans.py (pick_next, relocate_empty) and metrics.jensen_shannon_divergence against the restatement
(tests/kmeans_ref.py) on hand-made cases, every *_shapes refusal of the Python layer, and the argument checks and workspace arithmetic of the
four gs_kmeans entries -- no device is touched.  Every figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

from tests import kmeans_ref as KR


# ------------------------------------------------------------------------------------------------------------- host rules
PICKS = [
    ("plain", [1.0, 2.0, 3.0, 4.0], 0.25, 1),               # running 1 3 6 10, target 2.5: the first sum above it is row 1
    ("on a boundary", [1.0, 2.0, 3.0, 4.0], 0.3, 2),        # target 3.0 = the running sum at row 1: "exceeds" moves on to row 2
    ("u = 0", [0.0, 0.0, 5.0, 1.0], 0.0, 2),                # rows of zero distance (centres already picked) are never drawn
    ("all zero", [0.0, 0.0, 0.0], 0.7, 2),                  # nothing exceeds 0: clamped to the last row
    ("u just below 1", [2.0, 0.0, 2.0, 0.0], 1.0 - 2.0 ** -53, 2),
    ("one row", [3.0], 0.5, 0),
]


@pytest.mark.parametrize("name,dist,u,want", PICKS, ids=[p[0] for p in PICKS])
def test_pick_next(name, dist, u, want):
    from gansynth_amd import kmeans
    dist = np.asarray(dist, dtype=np.float32)
    got, ref = kmeans.pick_next(dist, u), KR.pick_next(dist, u)
    print(f"{name}: package {got}, restatement {ref}, by hand {want}")
    assert got == ref == want


def test_pick_next_on_random_draws():
    from gansynth_amd import kmeans
    rng = np.random.default_rng(3)
    for _ in range(200):
        dist = (rng.random(rng.integers(1, 40)) * (rng.random() < 0.8)).astype(np.float32)
        dist[rng.random(len(dist)) < 0.3] = 0.0
        u = rng.random()
        assert kmeans.pick_next(dist, u) == KR.pick_next(dist, u), (dist, u)


RELOCATIONS = [
    ("none empty", [2, 1, 3], [0.5, 0.1, 0.9, 0.2, 0.3, 0.4], []),
    ("one empty", [3, 0, 3], [0.5, 0.1, 0.9, 0.2, 0.3, 0.4], [(1, 2)]),
    ("two empty", [0, 6, 0], [0.5, 0.1, 0.9, 0.2, 0.3, 0.4], [(0, 2), (2, 0)]),
    ("ties", [0, 4, 0, 2], [0.7, 0.9, 0.9, 0.7, 0.9, 0.1], [(0, 1), (2, 2)]),       # the lowest index first, a taken row not again
    ("all distances zero", [0, 0, 5], [0.0, 0.0, 0.0, 0.0, 0.0], [(0, 0), (1, 1)]),
]


@pytest.mark.parametrize("name,counts,dist,want", RELOCATIONS, ids=[r[0] for r in RELOCATIONS])
def test_relocate_empty(name, counts, dist, want):
    from gansynth_amd import kmeans
    got, ref = kmeans.relocate_empty(np.asarray(counts), np.asarray(dist, dtype=np.float32)), KR.relocate(counts, np.asarray(dist, dtype=np.float32))
    print(f"{name}: package {got}, restatement {ref}")
    assert got == ref == want
    with pytest.raises(ValueError, match="empty clusters"):
        kmeans.relocate_empty(np.zeros(4, dtype=np.int64), np.ones(3, dtype=np.float32))


def test_jensen_shannon_divergence():
    from gansynth_amd import metrics
    p = np.array([0.1, 0.2, 0.3, 0.4])
    cases = [("identical", p, p, 0.0), ("disjoint", [0.5, 0.5, 0.0, 0.0], [0.0, 0.0, 0.25, 0.75], np.log(2.0)),
             # a zero bin: p = (1/2, 1/2, 0), q = (1/2, 0, 1/2), m = (1/2, 1/4, 1/4): each KL is (1/2) ln 2
             ("a zero bin", [0.5, 0.5, 0.0], [0.5, 0.0, 0.5], 0.5 * np.log(2.0)),
             ("both zero in a bin", [1.0, 0.0], [1.0, 0.0], 0.0)]
    for name, a, b, want in cases:
        got, ref = float(metrics.jensen_shannon_divergence(a, b)), KR.jsd(a, b)
        print(f"{name}: package {got!r}, restatement {ref!r}, by hand {want!r}")
        assert abs(got - want) <= 1e-15 and abs(ref - want) <= 1e-15
    rng = np.random.default_rng(5)
    a, b = rng.dirichlet(np.ones(50)), rng.dirichlet(np.ones(50))
    assert abs(float(metrics.jensen_shannon_divergence(a, b)) - KR.jsd(a, b)) <= 1e-15
    assert float(metrics.jensen_shannon_divergence(a, b)) == float(metrics.jensen_shannon_divergence(b, a))   # symmetric
    assert metrics.jensen_shannon_divergence(np.stack([a, b]), np.stack([b, b])).shape == (2,)


def test_the_restatement_on_a_case_by_hand():
    """Two clusters on a line: the restatement's own rules, checked by hand, and the package's host rules on the same case."""
    from gansynth_amd import kmeans
    x = np.array([[0.0], [1.0], [10.0], [11.0], [100.0]], dtype=np.float32)
    labels, inertia, iterations, centres = KR.lloyd(x, x[[0, 1]], 300)
    # from centres 0, 1: {0} | {1, 10, 11, 100} -> 0, 30.5 -> {0, 1, 10, 11} | {100} -> 5.5, 100 -> unchanged: two updates
    assert labels.tolist() == [0, 0, 0, 0, 1] and iterations == 2 and centres[:, 0].tolist() == [5.5, 100.0]
    assert inertia == 5.5 ** 2 + 4.5 ** 2 + 4.5 ** 2 + 5.5 ** 2
    log = []
    labels, _, _, centres = KR.lloyd(x, np.array([[0.5], [1e6]]), 300, log=log)   # the far centre empties: it takes row 4, the farthest
    assert log == [[(1, 4)]] and labels.tolist() == [0, 0, 0, 0, 1]
    first = KR.assign(x, np.array([[0.5], [1e6]]))[1]         # the distances of that first assign: the package relocates the same row
    assert kmeans.relocate_empty([5, 0], first.astype(np.float32)) == log[0]
    assert kmeans.pick_next(first.astype(np.float32), 0.5) == KR.pick_next(first.astype(np.float32), 0.5) == 4
    assert KR.assign(np.array([[1.0], [3.0]]), np.array([[2.0], [2.0], [0.0]]))[0].tolist() == [0, 0]   # ties: the lowest index
    assert KR.dist_bound(512) == 520 * 2.0 ** -24


# ------------------------------------------------------------------------------------------------------------- Python layer
def _raises(fn, *args, match):
    with pytest.raises(ValueError, match=match):
        fn(*args)


def test_shapes_refusals_name_the_argument():
    from gansynth_amd import kernels
    x, c = torch.zeros(10, 6), torch.zeros(3, 6)
    lab, dist = torch.zeros(10, dtype=torch.int32), torch.zeros(10)
    assert kernels.kmeans_assign_shapes(x, c) == (10, 6, 3) and kernels.kmeans_assign_shapes(x, c, lab) == (10, 6, 3)
    assert kernels.kmeans_assign_shapes(torch.zeros(10, 9)[:, :6], c) == (10, 6, 3)          # row slack is welcome
    assert kernels.kmeans_update_shapes(x, lab, c) == (10, 6, 3) and kernels.kmeans_inertia_shapes(x, c, lab) == (10, 6, 3)
    assert kernels.kmeans_mindist_shapes(x, c[0]) == (10, 6) and kernels.kmeans_mindist_shapes(x, c[0], dist) == (10, 6)
    for bad in (np.zeros((10, 6), dtype=np.float32), torch.zeros(10), torch.zeros(10, 6, dtype=torch.float64), torch.zeros(0, 6)):
        _raises(kernels.kmeans_assign_shapes, bad, c, match="kmeans_assign: x must be")
        _raises(kernels.kmeans_update_shapes, bad, lab, c, match="kmeans_update: x must be")
        _raises(kernels.kmeans_inertia_shapes, bad, c, lab, match="kmeans_inertia: x must be")
        _raises(kernels.kmeans_mindist_shapes, bad, c[0], match="kmeans_mindist: x must be")
    for bad in (torch.zeros(3, 5), torch.zeros(6), torch.zeros(3, 6, dtype=torch.float16), torch.zeros(0, 6), None):
        _raises(kernels.kmeans_assign_shapes, x, bad, match="kmeans_assign: centres must be")
        _raises(kernels.kmeans_update_shapes, x, lab, bad, match="kmeans_update: centres must be")
        _raises(kernels.kmeans_inertia_shapes, x, bad, lab, match="kmeans_inertia: centres must be")
    _raises(kernels.kmeans_assign_shapes, x, torch.zeros(257, 6), match="kmeans_assign: centres must have at most 256 rows")
    _raises(kernels.kmeans_update_shapes, x, lab, torch.zeros(257, 6), match="kmeans_update: centres must have at most 256 rows")
    _raises(kernels.kmeans_update_shapes, x, lab, torch.zeros(3, 12)[:, ::2], match="kmeans_update: centres must be contiguous")
    for bad in (torch.zeros(10, dtype=torch.int64), torch.zeros(9, dtype=torch.int32), torch.zeros(20, dtype=torch.int32)[::2], [0] * 10):
        _raises(kernels.kmeans_assign_shapes, x, c, bad, match="kmeans_assign: labels must be")
        _raises(kernels.kmeans_update_shapes, x, bad, c, match="kmeans_update: labels must be")
        _raises(kernels.kmeans_inertia_shapes, x, c, bad, match="kmeans_inertia: labels must be")
    for bad in (torch.zeros(5), torch.zeros(1, 6), torch.zeros(6, dtype=torch.float64), torch.zeros(12)[::2]):
        _raises(kernels.kmeans_mindist_shapes, x, bad, match="kmeans_mindist: centre must be")
    for bad in (torch.zeros(9), torch.zeros(10, dtype=torch.float64), torch.zeros(10, 1)):
        _raises(kernels.kmeans_mindist_shapes, x, c[0], bad, match="kmeans_mindist: dist must be")
    wide = torch.zeros(1, 2 ** 20 + 1)                        # one column more than update's grid takes
    _raises(kernels.kmeans_assign_shapes, wide, wide, match="kmeans_assign: x must have at most 1048576 columns")
    _raises(kernels.kmeans_mindist_shapes, wide, wide[0], match="kmeans_mindist: x must have at most 1048576 columns")
    # the wrappers refuse before a device is asked for
    _raises(kernels.kmeans_inertia, x, c, lab[:9], match="labels must be")
    _raises(kernels.kmeans_assign, x, torch.zeros(3, 5), match="centres must be")
    _raises(kernels.kmeans_update, x, lab[:9], c, match="labels must be")
    _raises(kernels.kmeans_mindist, x, c, match="centre must be")


def test_kmeans_refuses_bad_arguments_on_the_host():
    from gansynth_amd import kmeans
    for bad in (np.zeros(5), np.zeros((0, 4)), torch.zeros(2, 3, 4)):
        _raises(kmeans.to_device, bad, match="kmeans: x must be a non-empty")


# ------------------------------------------------------------------------------------------------------------- the C entries
def test_workspace_arithmetic():
    from gansynth_amd import _lib
    lib = _lib.load()
    assert (_lib.KMEANS_MAX_K, _lib.KMEANS_TILE, _lib.KMEANS_MAX_SLICES) == (KR.MAX_K, KR.TILE, KR.MAX_SLICES)
    by_hand = [((289205, 512, 50), 4 * 256 * 50 * 513),      # 2048 / 8 = 256 slices of 1130 rows (the last one shorter)
               ((1, 1, 1), 16), ((64, 64, 1), 272),          # one slice: 4 * 65 = 260 -> 272
               ((100000, 1, 256), 4 * 511 * 256 * 2),        # s0 = 512: slices of ceil(100000 / 512) = 196 rows, 511 of them cover 100000
               ((2 ** 31 - 1, 1, 1), 12 * 2 ** 23)]          # the assign partials outweigh 512 slices * 8 bytes
    for (n, d, k), want in by_hand:
        got = lib.gs_kmeans_workspace_bytes(n, d, k)
        print(f"n {n} d {d} k {k}: library {got}, restatement {KR.workspace_bytes(n, d, k)}, by hand {want}")
        assert got == KR.workspace_bytes(n, d, k) == want
    rng = np.random.default_rng(1)
    for _ in range(300):
        n, d, k = int(rng.integers(1, 400000)), int(rng.integers(1, 1200)), int(rng.integers(1, 257))
        assert lib.gs_kmeans_workspace_bytes(n, d, k) == KR.workspace_bytes(n, d, k), (n, d, k)
    for n, d, k in ((0, 4, 2), (-1, 4, 2), (2 ** 31, 4, 2), (10, 0, 2), (10, -3, 2), (10, 2 ** 20 + 1, 2), (10, 4, 0), (10, 4, 257)):
        assert lib.gs_kmeans_workspace_bytes(n, d, k) == 0, (n, d, k)


def test_abi_refusals():
    """Dummy pointers: the argument checks come first, nothing is dereferenced or launched; every message names its argument."""
    from gansynth_amd import _lib
    lib = _lib.load()
    P, n, d, k = 0x10000, 5000, 24, 7
    ws = int(lib.gs_kmeans_workspace_bytes(n, d, k))
    good = dict(x=P, ldx=d, n=n, d=d, c=P, k=k, labels=P, dist=P, changed=P, inertia=P, counts=P, ws=P, ws_bytes=ws, first=1)

    def assign(a):
        return lib.gs_kmeans_assign(a["x"], a["ldx"], a["n"], a["d"], a["c"], a["k"], a["labels"], a["dist"], a["changed"], a["inertia"], a["ws"], a["ws_bytes"], None)

    def update(a):
        return lib.gs_kmeans_update(a["x"], a["ldx"], a["n"], a["d"], a["labels"], a["k"], a["c"], a["counts"], a["ws"], a["ws_bytes"], None)

    def inertia(a):
        return lib.gs_kmeans_inertia(a["x"], a["ldx"], a["n"], a["d"], a["c"], a["k"], a["labels"], a["inertia"], a["ws"], a["ws_bytes"], None)

    def mindist(a):
        return lib.gs_kmeans_mindist(a["x"], a["ldx"], a["n"], a["d"], a["c"], a["dist"], a["first"], None)

    shape = [(dict(k=0), b"k must be in"), (dict(k=257), b"k must be in"), (dict(k=-1), b"k must be in"), (dict(d=0, ldx=0), b"d must be"),
             (dict(d=-2), b"d must be"), (dict(d=2 ** 20 + 1, ldx=2 ** 20 + 1), b"d must be"), (dict(n=0), b"n must be in"), (dict(n=2 ** 31), b"n must be in"), (dict(ldx=d - 1), b"ldx")]
    both = [(dict(x=None), b"null pointer"), (dict(c=None), b"null pointer"), (dict(labels=None), b"null pointer"), (dict(x=P + 2), b"misaligned"),
            (dict(ws=None), b"workspace"), (dict(ws=P + 8), b"workspace"), (dict(ws_bytes=ws - 1), b"workspace"), (dict(ws_bytes=0), b"workspace")]
    for entry, name, extra in ((assign, b"kmeans_assign", both + [(dict(inertia=P + 4), b"misaligned"), (dict(dist=P + 1), b"misaligned")]),
                               (update, b"kmeans_update", both + [(dict(counts=None), b"null pointer")]),
                               (inertia, b"kmeans_inertia", both + [(dict(inertia=None), b"null pointer"), (dict(inertia=P + 4), b"misaligned")]),
                               (mindist, b"kmeans_mindist", [(dict(x=None), b"null pointer"), (dict(c=None), b"null pointer"), (dict(dist=None), b"null pointer"),
                                                             (dict(dist=P + 2), b"misaligned")])):
        for change, message in shape + extra:
            if entry is mindist and "k" in change:
                continue
            assert entry(dict(good, **change)) == -1, (name, change)
            print(name.decode(), change, "->", lib.gs_last_error().decode())
            assert message in lib.gs_last_error() and name in lib.gs_last_error(), (change, lib.gs_last_error())
