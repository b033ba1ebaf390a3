"""The averaged generator restated in float64 (tests/test_ema_cpu.py, tests/test_ema_gpu.py): tf.train.ExponentialMovingAverage with
`num_updates`, shadow -= (shadow - w) * (1 - decay_t), decay_t = min(decay, (1 + t) / (10 + t)).  Nothing here imports the package."""
import numpy as np
import torch


def one_minus(decay, t):
    """1 - decay_t behind the generator's t-th Adam step: float64 arithmetic, rounded to fp32 ONCE (the value the kernel is handed),
    returned as float64."""
    decay_t = min(float(decay), (1.0 + float(t)) / (10.0 + float(t)))
    return float(np.float32(1.0 - decay_t))


def recurrence(snapshots, decay):
    """snapshots[0]: the initial weights; snapshots[t]: the weights after the generator's t-th step.  -> the float64 shadow after the last."""
    shadow = snapshots[0].detach().double().cpu().clone()
    for t, w in enumerate(snapshots[1:], start=1):
        shadow = shadow - (shadow - w.detach().double().cpu()) * one_minus(decay, t)
    return shadow


def step(shadow, w, om):
    """One update in float64 from fp32 operands (numpy); `om` is the fp32 scalar the kernel multiplies by."""
    s, w = np.asarray(shadow, dtype=np.float64), np.asarray(w, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return s - (s - w) * float(np.float32(om))


def bound(n, snapshots):
    """5 * n * 2^-24 * M, M the largest magnitude in any snapshot.  One step makes at most three roundings -- the difference, the product,
    the sum -- whose absolute sum is at most 2^-24 (|s'| + 2 om |w - s|) <= 5 * 2^-24 * M; the recurrence multiplies an inherited error by
    decay_t <= 1; an FMA only removes a rounding."""
    m = max(float(s.detach().abs().max()) for s in snapshots)
    return 5.0 * n * 2.0 ** -24 * m, m


def check_recurrence(snapshots, shadow, decay, named_ranges, what=""):
    """The trainer's shadow against the float64 recurrence within bound(), and the two non-vacuity conditions: the weights moved by at least
    100 bounds (median over the variables' elements), and the shadow is more than a bound away from both the first and the last snapshot
    on more than half of the elements of the variables that received a gradient.  `named_ranges`: [(offset, numel)] of the variables
    inside the flat buffer (the padding between them is excluded).  Prints every figure before it asserts."""
    n = len(snapshots) - 1
    tol, m = bound(n, snapshots)
    ref = recurrence(snapshots, decay)
    got = shadow.detach().double().cpu()
    err = float((got - ref).abs().max())
    first, last = snapshots[0].detach().double().cpu(), snapshots[-1].detach().double().cpu()
    keep = torch.zeros(first.numel(), dtype=torch.bool)
    moved = torch.zeros(first.numel(), dtype=torch.bool)
    for off, cnt in named_ranges:
        keep[off:off + cnt] = True
        if bool((first[off:off + cnt] != last[off:off + cnt]).any()):
            moved[off:off + cnt] = True
    drift = float((last - first).abs()[keep].median())
    apart = ((got - first).abs() > tol) & ((got - last).abs() > tol)
    share = float(apart[moved].double().mean()) if bool(moved.any()) else 0.0
    print(f"ema recurrence {what}: n = {n}, M = {m:.4g}, bound = {tol:.4g}, worst error = {err:.4g} ({err / tol:.3f} bounds), "
          f"median |w_n - w_0| = {drift:.4g} ({drift / tol:.1f} bounds), shadow apart from both ends on {share:.3f} of "
          f"{int(moved.sum())} elements with a gradient")
    assert bool(torch.isfinite(got).all())
    assert drift >= 100.0 * tol, f"{what}: the weights moved by {drift:.3g} (median), under 100 x the bound {tol:.3g}: the check would be vacuous"
    assert share > 0.5, f"{what}: the shadow is within the bound of an end point on {1 - share:.3f} of the elements"
    assert err <= tol, f"{what}: the shadow is {err:.4g} from the float64 recurrence, bound {tol:.4g}"
    # the padding between the variables is zero in both buffers and stays zero
    assert float(got[~keep].abs().max() if bool((~keep).any()) else 0.0) == 0.0
    return err, tol
