"""GANSynth's sample-quality metrics on host arrays (float64), with the reference's semantics (metrics.py:6-63):
softmax, KL divergence, inception score, Frechet distance between two feature sets, the two-proportion z-test and the number of
statistically different bins (NDB) of a k-means partition of the real features.  num_different_bins_device is NDB with the partition made on
the device (kmeans.py: this project's own clustering rules, no scikit-learn), beside the Jensen-Shannon divergence of the bin proportions.
precision_recall_device is precision, recall, density and coverage from k-nearest-neighbour radii on the device (manifold.py).
f0_pitch_accuracy_device is pitch accuracy from the audio itself, a YIN f0 tracker on the device (pitch.py)."""
import numpy as np
import scipy.linalg
import scipy.stats


def softmax(logits, axis=-1):
    z = np.asarray(logits, dtype=np.float64)
    e = np.exp(z - z.max(axis=axis, keepdims=True))
    return e / e.sum(axis=axis, keepdims=True)


def kl_divergence(p, q, axis=-1):
    """sum p log(p / q), a zero p contributing nothing."""
    p, q = np.asarray(p, dtype=np.float64), np.asarray(q, dtype=np.float64)
    zero = p == 0.0
    return np.sum(np.where(zero, 0.0, p * np.log(np.where(zero, 1.0, p) / np.where(zero, 1.0, q))), axis=axis)


def inception_score(logits):
    """exp(E_x KL(p(y|x) || p(y))), p(y) the mean of the class posteriors over the set."""
    p = softmax(logits)
    return float(np.exp(np.mean(kl_divergence(p, p.mean(axis=0, keepdims=True)))))


def frechet_inception_distance(real_features, fake_features):
    """|mu_r - mu_f|^2 + tr(S_r + S_f - 2 (S_r S_f)^(1/2)), sample covariances (N - 1).  A square root whose diagonal keeps an
    imaginary part beyond 1e-3 is refused, as the reference refuses it."""
    a, b = np.asarray(real_features, dtype=np.float64), np.asarray(fake_features, dtype=np.float64)
    mu_a, mu_b = a.mean(axis=0), b.mean(axis=0)
    cov_a, cov_b = np.cov(a, rowvar=False), np.cov(b, rowvar=False)
    root = scipy.linalg.sqrtm(cov_a @ cov_b)
    if np.iscomplexobj(root):
        if not np.allclose(np.diagonal(root).imag, 0.0, atol=1.0e-3):
            raise ValueError(f"Imaginary component {np.max(np.abs(root.imag))}")
        root = root.real
    return float(np.sum((mu_a - mu_b) ** 2) + np.trace(cov_a + cov_b - 2.0 * root))


def binomial_proportion_test(p, m, q, n, significance_level):
    """Two-proportion z-test per bin with the pooled standard error: True where proportions p (of m draws) and q (of n) differ.
    As in the reference (metrics.py:33-38) the statistic is (pooled - q) / se, the pooled proportion standing in for p -- not the
    textbook (p - q) / se, which is (m + n) / m times larger -- so that num_different_bins counts the bins the reference counts."""
    p, q = np.asarray(p, dtype=np.float64), np.asarray(q, dtype=np.float64)
    pooled = (p * m + q * n) / (m + n)
    se = np.sqrt(pooled * (1.0 - pooled) * (1.0 / m + 1.0 / n))
    with np.errstate(divide="ignore", invalid="ignore"):
        z = (pooled - q) / se
    return scipy.stats.norm.cdf(-np.abs(z)) * 2.0 < significance_level


def num_different_bins(real_features, fake_features, num_bins=50, significance_level=0.05, random_state=None):
    """NDB: k-means (scikit-learn) on the real features, each fake feature to its nearest centre, then the bins whose two proportions
    differ significantly.  Raises ImportError without scikit-learn."""
    from sklearn import cluster
    real, fake = np.asarray(real_features, dtype=np.float64), np.asarray(fake_features, dtype=np.float64)
    km = cluster.KMeans(n_clusters=num_bins, random_state=random_state, n_init=10).fit(real)
    real_counts = np.bincount(km.labels_, minlength=num_bins)
    real_prop = real_counts / real_counts.sum()
    c = km.cluster_centers_
    d = (fake ** 2).sum(axis=1, keepdims=True) - 2.0 * fake @ c.T + (c ** 2).sum(axis=1)[None, :]
    fake_counts = np.bincount(np.argmin(d, axis=1), minlength=num_bins)
    fake_prop = fake_counts / fake_counts.sum()
    return int(np.count_nonzero(binomial_proportion_test(real_prop, len(real), fake_prop, len(fake), significance_level)))


def jensen_shannon_divergence(p, q, axis=-1):
    """(KL(p || m) + KL(q || m)) / 2 with m = (p + q) / 2, in nats and float64: 0 for identical, ln 2 for disjoint distributions.  A bin that is
    zero in p (or q) contributes nothing to its term, as in kl_divergence; m is zero only where both are."""
    p, q = np.asarray(p, dtype=np.float64), np.asarray(q, dtype=np.float64)
    m = 0.5 * (p + q)
    return 0.5 * kl_divergence(p, m, axis=axis) + 0.5 * kl_divergence(q, m, axis=axis)


def num_different_bins_device(real_features, fake_features, num_bins=50, significance_level=0.05, seed=0, n_init=10, details=None):
    """NDB without scikit-learn: kmeans.kmeans (this project's own, stated rules; HIP kernels) on the real features, whose labels give the real
    counts; one kmeans_assign of the fake features to its centres gives the fake counts; then binomial_proportion_test as in num_different_bins.
    `details` (a dict) receives real_counts, fake_counts, inertia and jsd, the Jensen-Shannon divergence of the two bin proportions."""
    from . import kernels, kmeans
    real, fake = kmeans.to_device(real_features, "real_features"), kmeans.to_device(fake_features, "fake_features")
    if real.shape[1] != fake.shape[1]:
        raise ValueError(f"num_different_bins_device: real and fake features differ in width ({real.shape[1]} and {fake.shape[1]})")
    result = kmeans.kmeans(real, num_bins, seed=seed, n_init=n_init)
    real_counts = np.asarray(result.counts, dtype=np.int64)
    fake_labels = kernels.kmeans_assign(fake.to(real.device), result.centres, want_dist=False)[0]
    fake_counts = np.bincount(fake_labels.cpu().numpy(), minlength=num_bins).astype(np.int64)
    real_prop, fake_prop = real_counts / real_counts.sum(), fake_counts / fake_counts.sum()
    if details is not None:
        details.update(real_counts=real_counts, fake_counts=fake_counts, inertia=result.inertia, jsd=float(jensen_shannon_divergence(real_prop, fake_prop)))
    return int(np.count_nonzero(binomial_proportion_test(real_prop, len(real), fake_prop, len(fake), significance_level)))


def precision_recall_device(real_features, fake_features, k=3, details=None):
    """Improved precision and recall (Kynkaanniemi et al. 2019) and density and coverage (Naeem et al. 2020) of two feature sets [rows, columns]
    (numpy or torch): manifold.figures (this project's own, stated rules; HIP kernels, no distance matrix) -> dict(precision=, recall=, density=,
    coverage=).  `details` (a dict) receives real_radii and fake_radii (the squared k-NN radii, fp32), fake_counts and real_counts (int32: the balls
    of the other set every row lies in) and coverage_minima (fp32: every real row's squared distance to its nearest fake row)."""
    from . import kmeans, manifold
    for name, t in (("real_features", real_features), ("fake_features", fake_features)):
        if not hasattr(t, "shape"):
            raise ValueError(f"precision_recall_device: {name} must be a [rows, columns] array or tensor (got {type(t).__name__})")
    manifold.check_sets(real_features, fake_features, k, "precision_recall_device")   # (before a device is asked for)
    real = kmeans.to_device(real_features, "real_features")
    fake = kmeans.to_device(fake_features, "fake_features").to(real.device)
    result = manifold.figures(real, fake, k)
    if details is not None:
        details.update(real_radii=result.real_radii, fake_radii=result.fake_radii, fake_counts=result.fake_counts, real_counts=result.real_counts,
                       coverage_minima=result.coverage_minima)
    return dict(precision=result.precision, recall=result.recall, density=result.density, coverage=result.coverage)


def kernel_inception_distance_device(real_features, fake_features, subsets=100, subset_size=1000, seed=0, details=None):
    """The kernel inception distance (Binkowski et al. 2018) of two feature sets [rows, columns] (numpy or torch): kid.figures (this project's
    own, stated rules; an fp64 matrix-core HIP kernel, no Gram matrix) -> dict(kernel_inception_distance=, the unbiased estimate over all rows,
    kernel_inception_distance_subset_mean=, kernel_inception_distance_subset_std=, its mean and population standard deviation over `subsets`
    seeded subsets of min(subset_size, rows) rows a side; NaN with subsets = 0).  `details` (a dict) receives subset_kids (one estimate a
    subset), sums (Sxx, Syy, Sxy of the full sets), subset_sums and size."""
    from . import kid, kmeans
    for name, t in (("real_features", real_features), ("fake_features", fake_features)):
        if not hasattr(t, "shape"):
            raise ValueError(f"kernel_inception_distance_device: {name} must be a [rows, columns] array or tensor (got {type(t).__name__})")
    kid.check_sets(real_features, fake_features, subsets, subset_size, "kernel_inception_distance_device")   # (before a device is asked for)
    real = kmeans.to_device(real_features, "real_features")
    fake = kmeans.to_device(fake_features, "fake_features").to(real.device)
    result = kid.figures(real, fake, subsets, subset_size, seed)
    if details is not None:
        details.update(subset_kids=result.subset_kids, sums=result.sums, subset_sums=result.subset_sums, size=result.size)
    return dict(kernel_inception_distance=result.kid, kernel_inception_distance_subset_mean=result.subset_mean,
                kernel_inception_distance_subset_std=result.subset_std)


def sliced_wasserstein_distance_device(real_images, fake_images, seed=0, details=None, batch_size=None):
    """The sliced Wasserstein distance between Laplacian-pyramid patches of two image sets [n, 2, h, w] (tensors or arrays, fp32 or bf16; the
    same n): swd.SlicedWasserstein (this project's own, stated rules; HIP kernels, no classifier) -> the mean over the levels of
    1e3 * mean |sort(A) - sort(B)|.  `details` (a dict) receives levels (one float a level, finest first), sizes ("HxW" a level) and n.
    `batch_size`: the sets are added that many images at a time, in order -- the corner draws follow the batches, so this reproduces an
    accumulator that was fed the same batches; None: all at once."""
    import torch
    from . import kernels, swd
    sets = []
    for name, images in (("real_images", real_images), ("fake_images", fake_images)):
        t = images if isinstance(images, torch.Tensor) else torch.from_numpy(np.array(images))   # (a copy: torch does not wrap a read-only array quietly)
        if t.dim() != 4 or t.shape[0] == 0:
            raise ValueError(f"sliced_wasserstein_distance_device: {name} must be a non-empty [n, 2, h, w] set (got {tuple(t.shape)})")
        sets.append(t)
    if sets[0].shape != sets[1].shape:
        raise ValueError(f"sliced_wasserstein_distance_device: the sets differ in shape ({tuple(sets[0].shape)} and {tuple(sets[1].shape)})")
    acc = swd.SlicedWasserstein(sets[0].shape, seed=seed)
    n = sets[0].shape[0]
    step = n if batch_size is None else int(batch_size)
    if step < 1:
        raise ValueError(f"sliced_wasserstein_distance_device: batch_size must be positive (got {batch_size})")
    on_hip = isinstance(kernels.get(), kernels.HipKernels)   # (a host without a device fails here, with the library's message)
    device = torch.device("cuda") if on_hip and not sets[0].is_cuda else sets[0].device
    for at in range(0, n, step):
        acc.add(*(t[at:at + step].to(device) for t in sets))
    out = acc.result()
    if details is not None:
        details.update(levels=out["levels"], sizes=out["sizes"], n=out["n"])
    return out["mean"]


def f0_pitch_accuracy_device(waveforms, pitches, details=None):
    """Pitch accuracy of notes from their AUDIO, without a classifier: waveforms [notes, n] (a tensor or array, fp32, 16 kHz) tracked by
    pitch.track (this project's own, stated rules: a YIN tracker on HIP kernels, production parameters) and judged against `pitches` [notes]
    (MIDI numbers) by pitch.note_statistics -> pitch.summarize's dict: f0_pitch_accuracy, f0_chroma_accuracy, f0_median_abs_cents,
    f0_jitter_cents and f0_voiced_fraction.  `details` (a dict) receives the per-note cents and jitter (NaN: unvoiced) and voiced (frames).
    YIN is not perfect on real instruments: read a generated set's figures against those of the real set."""
    import torch
    from . import kernels, pitch
    t = waveforms if isinstance(waveforms, torch.Tensor) else torch.from_numpy(np.array(waveforms, dtype=np.float32))
    if t.dim() != 2 or t.shape[0] == 0:
        raise ValueError(f"f0_pitch_accuracy_device: waveforms must be a non-empty [notes, samples] set (got {tuple(t.shape)})")
    pitches = np.asarray(pitches, dtype=np.float64).reshape(-1)
    if pitches.shape[0] != t.shape[0]:
        raise ValueError(f"f0_pitch_accuracy_device: {pitches.shape[0]} pitches for {t.shape[0]} notes")
    kernels.yin_track_shapes(t.float(), pitch.WINDOW, pitch.LAGS, pitch.HOP, pitch.TAU_MIN, pitch.THRESHOLD)   # (before a device is asked for)
    on_hip = isinstance(kernels.get(), kernels.HipKernels)   # (a host without a device fails here, with the library's message)
    if on_hip and not t.is_cuda:
        t = t.cuda()
    tracked = pitch.track(t)
    stats = pitch.note_statistics(tracked.period, tracked.aperiodicity, tracked.power, pitches)
    if details is not None:
        details.update(cents=stats.cents, jitter=stats.jitter, voiced=stats.voiced)
    return pitch.summarize(stats.cents, stats.jitter)
