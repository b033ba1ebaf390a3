"""The element-wise bound of the conv, dense and weight-gradient covers (tests/igemm_cover.py, thin_cover.py, dense_cover.py, wgrad_cover.py) -- a
plain helper module: no fixtures, no collection hooks.

Every element i of a result is held to a bound derived from the arithmetic of a GEMM-like kernel, not to one number per tensor:

  mag_i = |alpha| sum_k |a_k| |w_k| + |bias_i| (+ |gw0_i| of an accumulating gradient, + |addend_i|), times the mask factor where there is one:
          the map itself on the absolute values of the operands as stored.  It is a scale, not a reference: the covers evaluate it in fp32 on
          the CPU (never through the library under test) and it enters inflated by 1 + 1e-3.
  F_i   = min((K + e) u mag_i, ceiling * max |ref|)           the fp32 part
          K: the most products any element sums; u = 2^-24; e = 3 (alpha, the bias or accumulate add, one fold), + 1 for a leaky-relu slope or
          a mask factor, + 2 for a tanh mask 1 - m^2.  (K + e) u bounds a sum of K products in fp32 in ANY order and through any
          split-and-fold, so nothing here knows a kernel's loop structure.  Leaky relu and tanh are 1-Lipschitz: a forward activation carries
          the bound through; a forward tanh adds 2^-20 |ref_i| (fast_tanh of gs_common.h: <= 5e-7 relative, and one rounding).
          The `ceiling` (16 times the worst max-norm ratio measured on the MI355X, rounded up to a power of ten, never above the suite's own)
          keeps long reductions no weaker than the max-norm assertion these covers made before.
  an fp32 result:                                |got_i - ref_i| <= F_i
  a bf16 result rounded r times on the way out:  |got_i - ref_i| <= r 2^-8 (|ref_i| + F_i) + F_i

No element is left out: `measure` compares every one and says how many it compared.
"""
import math
from collections import namedtuple

import torch

U = 2.0 ** -24              # unit round-off of fp32; v_mfma_f32_*_f32 is a k-ordered fmaf chain
U_BF16_MFMA = 2.0 ** -24    # v_mfma_f32_32x32x16_bf16: decided by the measurement recorded in tests/igemm_cover.py's docstring
BF16_STEP = 2.0 ** -8       # a value rounded to bf16 (8 significant bits) is within 2^-8 of its own size, whichever way it was rounded
INFLATE = 1.0 + 1e-3        # mag is evaluated in fp32
E_BASE = 3                  # alpha, the bias / accumulate add, one fold
TANH_FWD = 2.0 ** -20       # fast_tanh and the rounding behind it, relative
SEEDS = tuple(range(12))    # of the measurement: every case of at most SMALL_MACS reference multiply-adds at each, the others at SEEDS[0]
SMALL_MACS = 5e7
SEED_STRIDE = 1000          # seed s of a case: the case's own seed + SEED_STRIDE * s (seed 0 is the case as it always ran)

Measure = namedtuple("Measure", "ratio worst over compared message")


def seeds_for(macs):
    return SEEDS if macs <= SMALL_MACS else SEEDS[:1]


def ceiling_rule(measured, suite):
    """16 times the worst measured ratio, rounded up to a power of ten, never above the suite's own."""
    return min(suite, 10.0 ** math.ceil(math.log10(16.0 * measured) - 1e-12))


def fp32_part(ref, mag, K, e, ceiling, u=U, tanh_fwd=False):
    """F_i.  mag None: the ceiling part alone (a composite reference)."""
    ref = ref.double()
    f = torch.full_like(ref, ceiling * float(ref.abs().max()))
    if mag is not None:
        assert mag.shape == ref.shape and K >= 1 and e >= E_BASE, (tuple(mag.shape), tuple(ref.shape), K, e)
        f = torch.minimum((K + e) * u * INFLATE * mag.double(), f)
    return f + TANH_FWD * ref.abs() if tanh_fwd else f


def bound(ref, mag, K, e, ceiling, roundings=0, u=U, tanh_fwd=False):
    """The bound of every element of a result: fp32 (roundings = 0) or bf16 rounded `roundings` times."""
    f = fp32_part(ref, mag, K, e, ceiling, u, tanh_fwd)
    return roundings * BF16_STEP * (ref.double().abs() + f) + f if roundings else f


def never_weaker(old_tolerance, ceiling, roundings, tanh_fwd=False):
    """Whether the bound, at its largest (F_i = ceiling * max |ref| (+ tanh), |ref_i| = max |ref|), stays under old_tolerance * max |ref|."""
    f = ceiling + (TANH_FWD if tanh_fwd else 0.0)
    return (roundings * BF16_STEP * (1.0 + f) + f if roundings else f) <= old_tolerance


def measure(tag, got, ref, bnd, mag=None):
    """Every element of `got` against its bound: Measure(max error over max |ref|, worst err / bound, elements over, elements compared, message
    naming the worst element)."""
    got, ref, bnd = got.detach().double().cpu(), ref.detach().double().cpu(), bnd.double()
    assert got.shape == ref.shape == bnd.shape, (tag, tuple(got.shape), tuple(ref.shape), tuple(bnd.shape))
    assert bool(torch.isfinite(ref).all()) and bool((bnd >= 0).all()), tag
    err = (got - ref).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    q = torch.where(bnd > 0, err / bnd.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    over, compared = int((q > 1).sum()), q.numel()
    ratio = float(err.max()) / (float(ref.abs().max()) + 1e-300)
    i = int(q.reshape(-1).argmax())
    idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), q.shape)) if q.dim() else ()
    at = lambda t: float(t.reshape(-1)[i])   # noqa: E731
    message = (f"{tag}: {over} of {compared} elements over the bound; worst err / bound {at(q):.3g} at {idx}: got {at(got):.9g} ref {at(ref):.9g} "
               f"bound {at(bnd):.3g} mag {'-' if mag is None else format(at(mag.double()), '.3g')}; max error over max |ref| {ratio:.3e}")
    return Measure(ratio, float(q.max()), over, compared, message)


def hold(prefix, tag, got, ref, bnd, mag=None, worst=None, family=None):
    """measure, printed (`<prefix> <tag> ratio ... err/bound ...`), noted in `worst` under `family`, then asserted: every element compared,
    every element inside."""
    m = measure(tag, got, ref, bnd, mag)
    print(f"{prefix} {tag} ratio {m.ratio:.3e} err/bound {m.worst:.3f}")
    if worst is not None:
        worst.note(family, m, got.dtype != torch.bfloat16)
    assert m.compared == ref.numel() and m.over == 0, m.message
    return m


class Worst(object):
    """The worst max-norm ratio (fp32 results: the `measured` column of a cover's table) and the worst err / bound per family, over whatever ran."""
    def __init__(self):
        self.rows = {}

    def note(self, family, m, fp32_result):
        row = self.rows.setdefault(family, [0.0, 0.0, 0.0, 0.0, 0])   # ratio and err / bound of fp32 results, of bf16 results, comparisons
        at = 0 if fp32_result else 2
        row[at], row[at + 1], row[4] = max(row[at], m.ratio), max(row[at + 1], m.worst), row[4] + 1

    def merge(self, rows):
        for family, other in rows.items():
            row = self.rows.setdefault(family, [0.0, 0.0, 0.0, 0.0, 0])
            row[:4] = [max(a, b) for a, b in zip(row[:4], other[:4])]
            row[4] += other[4]

    def report(self, prefix, ceilings):
        for family in sorted(self.rows):
            r32, q32, r16, q16, n = self.rows[family]
            measured, suite, here = ceilings.get(family, (None, None, None))
            print(f"{prefix}-WORST {family} fp32 results: ratio {r32:.3e} err/bound {q32:.3f}; bf16 results: ratio {r16:.3e} err/bound {q16:.3f}; "
                  f"{n} comparisons; table: measured {measured} suite {suite} here {here}")


def table_lines(ceilings):
    """The `family, measured, suite, here` table of a cover's docstring, line by line, from its CEILINGS."""
    return [f"    {family:<18}{measured:<12.1e}{suite:<8g}{here:g}" for family, (measured, suite, here) in ceilings.items()]


def check_table(doc, ceilings):
    """The docstring's table and the constants are the same thing, and every ceiling is what the rule gives for its measurement."""
    for line in table_lines(ceilings):
        assert line in doc.splitlines(), line
    for family, (measured, suite, here) in ceilings.items():
        assert here == ceiling_rule(measured, suite) <= suite, (family, measured, suite, here)


class Gap(object):
    """The gap between the max-norm assertion the covers made before and the element-wise bound, written down: a mutant result that passes the
    old assertion (ratio <= old tolerance) must fail the new one (some element over its bound) at every case where it is evaluated.  A case at
    which the old assertion already catches the mutant is left out and counted; at least half of the evaluated cases must remain."""
    def __init__(self, names):
        self.evaluated, self.kept = {n: 0 for n in names}, {n: 0 for n in names}

    def check(self, name, tag, got, ref, bnd, old_tolerance):
        if got is None:   # (the mutation touches no element of this case: there is no mutant to evaluate)
            return None
        self.evaluated[name] += 1
        m = measure(f"{name} {tag}", got, ref, bnd)
        if m.ratio > old_tolerance:
            return None
        self.kept[name] += 1
        assert m.over > 0, f"passes the old assertion and the new one: {m.message}"
        return m

    def close(self, need_half=None):
        print("mutants kept (passing the old assertion, failing the new one) of evaluated: "
              + ", ".join(f"{n} {self.kept[n]}/{self.evaluated[n]}" for n in self.evaluated))
        for n in (self.evaluated if need_half is None else need_half):
            assert self.evaluated[n] > 0 and 2 * self.kept[n] >= self.evaluated[n], (n, self.kept[n], self.evaluated[n])


# ------------------------------------------------------------------------------------------- mutants: results that are subtly wrong
def bf16_rne(t):
    return t.float().bfloat16().double()


def bf16_truncate(t):
    """Round towards zero to bf16: the low 16 bits of the fp32 pattern dropped."""
    bits = t.float().contiguous().view(torch.int32)
    return (bits & -65536).view(torch.float32).double()


def fold_through_bf16(part0, part1):
    """M1: the reduction in two parts, each rounded to bf16 before the last add (a fold through a bf16 workspace)."""
    return bf16_rne(part0) + bf16_rne(part1)


def scale_small(ref, factor=1.0 + 2.0 ** -6, below=0.05):
    """M5: every element with |ref_i| < 0.05 max |ref| scaled by 1 + 2^-6; None where there is no such element but zeros."""
    ref = ref.double()
    small = ref.abs() < below * ref.abs().max()
    return torch.where(small, ref * factor, ref) if bool((small & (ref != 0)).any()) else None


def stored_as(t, bf16):
    """A mutant's float64 result as the kernel would store it (round to nearest even); None stays None."""
    return None if t is None else (bf16_rne(t) if bf16 else t.float())
