"""Sliced Wasserstein distance between Laplacian-pyramid patches of real and generated images (the metric of the progressive-GAN paper, under
rules of this project's own: include/gansynth_hip.h, DESIGN.md "SWD on the device"; tests/swd_ref.py restates them in float64 numpy).  It
needs no classifier.  Every array-sized step is a HIP kernel (kernels.swd_*); the host draws the patch corners and the directions.

    acc = SlicedWasserstein((128, 1024), seed=0)
    for real, fake in batches:          # [b, 2, 128, 1024] each, fp32 or bf16, on the device
        acc.add(real, fake)             # the images are not kept: 128 descriptors of 98 floats an image and level are
    out = acc.result()                  # {"levels": [one float a level, finest first], "sizes": ["128x1024", ...], "mean": ..., "n": images}
"""
import numpy as np
import torch

from . import _lib, kernels

PATCHES, PATCH, DESC = _lib.SWD_PATCHES, 7, _lib.SWD_DESC
REPEATS, DIRECTIONS = 4, 128


def directions(seed):
    """[98, 4 * 128] fp32: four draws of standard_normal((98, 128)) from Generator(PCG64(seed + 2)), every column scaled to unit length in
    float64 and rounded once to fp32."""
    rng = np.random.Generator(np.random.PCG64(seed + 2))
    out = []
    for _ in range(REPEATS):
        d = rng.standard_normal((DESC, DIRECTIONS))
        out.append((d / np.sqrt((d * d).sum(axis=0, keepdims=True))).astype(np.float32))
    return np.concatenate(out, axis=1)


def draw_corners(rng, b, h, w, levels):
    """The top-left corners of a batch of b images: per level, ascending, integers(0, h_l - 6, (b, 128)) then integers(0, w_l - 6, (b, 128)).
    -> [(ys, xs)] of int32 [b * 128] a level."""
    out = []
    for l in range(levels):
        ys = rng.integers(0, (h >> l) - PATCH + 1, (b, PATCHES))
        xs = rng.integers(0, (w >> l) - PATCH + 1, (b, PATCHES))
        out.append((ys.reshape(-1).astype(np.int32), xs.reshape(-1).astype(np.int32)))
    return out


class SlicedWasserstein(object):
    """The streaming accumulator: `shape` is (h, w) or an image tensor's [.., h, w]; the real set draws its corners from PCG64(seed), the
    fake set from PCG64(seed + 1), the directions come from PCG64(seed + 2)."""

    def __init__(self, shape, seed=0):
        self.h, self.w = (int(s) for s in tuple(shape)[-2:])
        self.levels = kernels.swd_levels(self.h, self.w)
        if self.levels == 0:
            raise ValueError(f"SlicedWasserstein: images of {self.h} x {self.w} have no level (both sides at least 16 and at most {_lib.SWD_MAX_SIDE}, "
                             f"every halved size even)")
        self.seed = int(seed)
        self.rngs = [np.random.Generator(np.random.PCG64(self.seed + s)) for s in (0, 1)]
        self.dirs = directions(self.seed)
        self.desc = [[None] * self.levels for _ in (0, 1)]   # [set][level]: fp32 [capacity, 98] on the device
        self.n = 0                                            # images a set

    def sizes(self):
        return [f"{self.h >> l}x{self.w >> l}" for l in range(self.levels)]

    def _room(self, s, l, rows, device):
        """The descriptor buffer of set s, level l with room for `rows` rows: doubled (and copied) when it is full."""
        buf = self.desc[s][l]
        if buf is None or buf.shape[0] < rows:
            grown = torch.empty((min(max(rows, 2 * (0 if buf is None else buf.shape[0])), _lib.SWD_MAX_N), DESC), dtype=torch.float32, device=device)
            if buf is not None:
                grown[:self.n * PATCHES].copy_(buf[:self.n * PATCHES])
            self.desc[s][l] = buf = grown
        return buf

    def add(self, real_batch, fake_batch):
        """A batch of real and as many fake images, [b, 2, h, w] each."""
        shapes = [kernels.swd_pyramid_shapes(t) for t in (real_batch, fake_batch)]
        if shapes[0] != shapes[1] or shapes[0][1:3] != (self.h, self.w):
            raise ValueError(f"SlicedWasserstein.add: the batches must both be [b, 2, {self.h}, {self.w}] (got {tuple(real_batch.shape)} and {tuple(fake_batch.shape)})")
        b = shapes[0][0]
        rows = (self.n + b) * PATCHES
        if rows > _lib.SWD_MAX_N:
            raise ValueError(f"SlicedWasserstein.add: at most {_lib.SWD_MAX_N // PATCHES} images a set ({_lib.SWD_MAX_N} descriptors: the sort's limit)")
        K = kernels.get()
        for s, batch in enumerate((real_batch, fake_batch)):
            corners = draw_corners(self.rngs[s], b, self.h, self.w, self.levels)
            for l, level in enumerate(K.swd_pyramid(batch)):
                ys, xs = (torch.from_numpy(c).to(batch.device) for c in corners[l])
                K.swd_patches(level, ys, xs, self._room(s, l, rows, batch.device), self.n * PATCHES)
        self.n += b

    def result(self):
        """-> {"levels": [1e3 * mean |sort(A) - sort(B)| a level, finest first], "sizes", "mean", "n"}."""
        if self.n == 0:
            raise ValueError("SlicedWasserstein.result: no batch was added")
        K = kernels.get()
        rows = self.n * PATCHES
        dirs = torch.from_numpy(self.dirs).to(self.desc[0][0].device)
        values = []
        for l in range(self.levels):
            sorted_sets = []
            for s in (0, 1):
                desc = self.desc[s][l][:rows]
                moments = K.swd_moments(desc)
                std = moments.cpu().numpy()[[3, 7]]
                if not (std > 0).all():
                    raise ValueError(f"SlicedWasserstein.result: level {self.sizes()[l]} of the {'real' if s == 0 else 'fake'} set has a channel of "
                                     f"standard deviation 0 (constant images cannot be normalised)")
                sorted_sets.append(K.swd_sort(K.swd_project(desc, moments, dirs)))
            total = float(K.swd_l1(sorted_sets[0], sorted_sets[1]).item())
            values.append(total / (rows * self.dirs.shape[1]) * 1e3)
        return dict(levels=values, sizes=self.sizes(), mean=float(np.mean(values)), n=self.n)
