"""What the sliced Wasserstein distance costs on the device ("SWD on the device").

    python scripts/bench_swd.py [--repeats 10] [--images 8192] [--batch 64] [--out profiles/swd_bench.json]

The evaluation's own shapes: `images` real and as many generated 2 x 128 x 1024 bf16 images in batches of `batch`, so 128 * images descriptor
rows a set and level (2^20 at 8192) and 512 sorted columns of that length.  Every stage on preallocated buffers with HIP events around each
call, next to a torch restatement on the same device in the same process, in alternating blocks:
  pyramid   gs_swd_pyramid of one batch             | reflect padding, F.conv2d (stride 2), zero stuffing and F.conv2d, a subtraction, per level
  patches   gs_swd_patches of the batch's finest level | advanced indexing
  moments   gs_swd_moments of a full descriptor buffer | sums of the float64 copy
  project   gs_swd_project to 512 directions        | ((desc - mean) / std) @ dirs, transposed and made contiguous
  sort      gs_swd_sort of the [512, rows] projection | torch.sort(dim=1)
  l1        gs_swd_l1 of two such buffers           | (a - b).abs().sum(dtype=float64)
Reported: median / min / max device ms of each, the bytes (and for the projection the flops) the stage needs from its shapes, its rate and its
share of the measured HBM copy rate or of the fp32 vector peak of the datasheet -- whichever bounds it --, the sort's passes and bytes a
pass, whether the device results equal torch's, and the wall time (host clock, synchronised) of the whole metric: `images / batch` calls of
SlicedWasserstein.add on one resident batch, then result().  Needs a GPU; prints one JSON object.
"""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BYTES_PER_S = 6.29e12        # float4 copy, measured (8.0e12 by the datasheet)
VECTOR_FLOPS = 157.3e12          # fp32 vector peak of the datasheet
H, W, DIRS = 128, 1024, 512


def timed(fn, repeats):
    pairs = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        pairs.append((e0, e1))
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in pairs]


def stats(ms):
    ms = sorted(ms)
    return dict(median=ms[len(ms) // 2], min=ms[0], max=ms[-1])


def torch_pyramid(x, levels):
    """The rules with library convolutions: x [b, 2, h, w] fp32 -> the Laplacian levels."""
    k = torch.tensor([1.0, 4.0, 6.0, 4.0, 1.0], device=x.device)
    kernel = (torch.outer(k, k) / 256.0).expand(2, 1, 5, 5).contiguous()
    g, out = x, []
    for _ in range(levels - 1):
        down = F.conv2d(F.pad(g, (2, 2, 2, 2), mode="reflect"), kernel, stride=2, groups=2)
        stuffed = torch.zeros_like(g)
        stuffed[:, :, ::2, ::2] = down
        out.append(g - F.conv2d(F.pad(stuffed, (2, 2, 2, 2), mode="reflect"), 4.0 * kernel, groups=2))
        g = down
    return out + [g]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--images", type=int, default=8192)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_swd.py measures on the GPU: no device found")
    from gansynth_amd import _lib, kernels, swd
    torch.cuda.set_device(0)
    K = kernels.get()
    b, rows = args.batch, args.images * 128
    levels = kernels.swd_levels(H, W)
    g = torch.Generator("cuda").manual_seed(0)
    images = torch.randn(b, 2, H, W, device="cuda", generator=g).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    held = {}

    # ---- the per-batch stages
    def pyramid():
        held["levels"] = K.swd_pyramid(images)

    def t_pyramid():
        held["t_levels"] = torch_pyramid(images.float(), levels)

    pyramid()
    t_pyramid()
    fine = held["levels"][0]
    ys = torch.randint(0, H - 6, (b * 128,), device="cuda", generator=g, dtype=torch.int32)
    xs = torch.randint(0, W - 6, (b * 128,), device="cuda", generator=g, dtype=torch.int32)
    batch_desc = torch.empty(b * 128, 98, device="cuda")
    image_index = torch.arange(b, device="cuda").repeat_interleave(128)[:, None, None, None]
    channel = torch.arange(2, device="cuda")[None, :, None, None]
    dy, dx = torch.arange(7, device="cuda")[None, None, :, None], torch.arange(7, device="cuda")[None, None, None, :]

    def patches():
        K.swd_patches(fine, ys, xs, batch_desc, 0)

    def t_patches():
        held["t_desc"] = fine[image_index, ys.long()[:, None, None, None] + dy, xs.long()[:, None, None, None] + dx, channel].reshape(b * 128, 98)

    # ---- the final stages, at the full length
    desc = torch.randn(rows, 98, device="cuda", generator=g) * 0.5 + 0.1
    dirs = torch.from_numpy(swd.directions(0)).cuda()
    moments_out = torch.empty(8, dtype=torch.float64, device="cuda")
    ws_m = kernels._ws(K.lib.gs_swd_workspace_bytes(_lib.SWD_STAGE_MOMENTS, rows, 0, 0), desc.device)
    proj = torch.empty(DIRS, rows, device="cuda")
    ws_s = kernels._ws(K.lib.gs_swd_workspace_bytes(_lib.SWD_STAGE_SORT, DIRS, rows, 0), desc.device)
    ws_l = kernels._ws(K.lib.gs_swd_workspace_bytes(_lib.SWD_STAGE_L1, DIRS, rows, 0), desc.device)
    l1_out = torch.empty(1, dtype=torch.float64, device="cuda")
    unsorted = torch.randn(DIRS, rows, device="cuda", generator=g)
    work, other = torch.empty_like(unsorted), torch.sort(torch.randn(DIRS, rows, device="cuda", generator=g), dim=1).values

    def moments():
        _lib.check(K.lib.gs_swd_moments(desc.data_ptr(), rows, moments_out.data_ptr(), ws_m.data_ptr(), ws_m.numel(), kernels._stream()), "gs_swd_moments")

    def t_moments():
        d = desc.view(rows, 2, 49).double()
        held["t_moments"] = (d.sum(dim=(0, 2)), (d * d).sum(dim=(0, 2)))

    def project():
        _lib.check(K.lib.gs_swd_project(desc.data_ptr(), rows, moments_out.data_ptr(), dirs.data_ptr(), DIRS, proj.data_ptr(), kernels._stream()), "gs_swd_project")

    def t_project():
        m = moments_out.float()
        mean, std = m[[2, 6]].repeat_interleave(49), m[[3, 7]].repeat_interleave(49)
        held["t_proj"] = (((desc - mean) / std) @ dirs).t().contiguous()

    def sort():   # (the copy that restores the unsorted input is timed on its own and subtracted)
        work.copy_(unsorted)
        _lib.check(K.lib.gs_swd_sort(work.data_ptr(), DIRS, rows, ws_s.data_ptr(), ws_s.numel(), kernels._stream()), "gs_swd_sort")

    def copy_only():
        work.copy_(unsorted)

    def t_sort():
        held["t_sorted"] = torch.sort(unsorted, dim=1).values

    def l1():
        _lib.check(K.lib.gs_swd_l1(work.data_ptr(), other.data_ptr(), DIRS, rows, l1_out.data_ptr(), ws_l.data_ptr(), ws_l.numel(), kernels._stream()), "gs_swd_l1")

    def t_l1():
        held["t_l1"] = (work - other).abs().sum(dtype=torch.float64)

    fns = dict(pyramid=pyramid, torch_pyramid=t_pyramid, patches=patches, torch_patches=t_patches, moments=moments, torch_moments=t_moments, project=project,
               torch_project=t_project, sort=sort, copy_only=copy_only, torch_sort=t_sort, l1=l1, torch_l1=t_l1)
    for _ in range(2):
        for fn in fns.values():
            fn()
    sort()   # (copy_only left the unsorted values in `work`)
    torch.cuda.synchronize()
    agree = dict(
        pyramid_largest_difference=max(float((a.permute(0, 3, 1, 2) - t).abs().max()) for a, t in zip(held["levels"], held["t_levels"])),
        patches_equal=bool(torch.equal(batch_desc, held["t_desc"])),
        moments_largest_relative_difference=float(((moments_out[[0, 4]] - held["t_moments"][0]) / held["t_moments"][0]).abs().max()),
        project_largest_difference=float((proj - held["t_proj"]).abs().max()),
        sort_equal=bool(torch.equal(work, held["t_sorted"])),
        l1_relative_difference=float(((l1_out[0] - held["t_l1"]) / held["t_l1"]).abs()))
    held.pop("t_proj")
    ms = {name: [] for name in fns}
    for _ in range(5):   # alternating blocks: other work shares the machine
        for name, fn in fns.items():
            ms[name] += timed(fn, max(args.repeats // 5, 1))
    result = dict(repeats=args.repeats, images=args.images, batch=b, rows=rows, directions=DIRS, hbm_bytes_per_s=HBM_BYTES_PER_S, vector_flops=VECTOR_FLOPS,
                  agreement_with_torch=agree)
    for name in fns:
        result[name + "_ms"] = stats(ms[name])
    sort_ms = result["sort_ms"]["median"] - result["copy_only_ms"]["median"]
    passes = 0
    run = _lib.SWD_SORT_TILE
    while run < rows:
        passes, run = passes + 1, run * 2
    level_px = [b * (H >> l) * (W >> l) * 2 for l in range(levels)]
    need = dict(pyramid=2.0 * level_px[0] + 4.0 * sum(level_px),          # the bf16 images once, every fp32 level once
                patches=2.0 * 4 * b * 128 * 98, moments=4.0 * rows * 98, project=4.0 * rows * (98 + DIRS), sort=2.0 * 4 * DIRS * rows * (passes + 1),
                l1=2.0 * 4 * DIRS * rows)
    times = dict(pyramid=result["pyramid_ms"]["median"], patches=result["patches_ms"]["median"], moments=result["moments_ms"]["median"],
                 project=result["project_ms"]["median"], sort=sort_ms, l1=result["l1_ms"]["median"])
    result["sort_without_copy_ms"] = sort_ms
    result["sort_passes"] = dict(tile_sorts=1, merge_passes=passes, bytes_a_pass=2.0 * 4 * DIRS * rows)
    for name, nbytes in need.items():
        result[name + "_bytes"] = nbytes
        result[name + "_tb_per_s"] = nbytes / times[name] / 1e9
        result[name + "_fraction_of_hbm_roof"] = nbytes / HBM_BYTES_PER_S * 1e3 / times[name]
    flops = 2.0 * 98 * DIRS * rows
    result.update(project_flops=flops, project_tflops=flops / times["project"] / 1e9, project_fraction_of_vector_peak=flops / VECTOR_FLOPS * 1e3 / times["project"],
                  project_bound="vector" if flops / VECTOR_FLOPS > need["project"] / HBM_BYTES_PER_S else "hbm")
    del desc, proj, unsorted, work, other, ws_s, held

    # ---- the whole metric
    fake = (1.2 * torch.randn(b, 2, H, W, device="cuda", generator=g) + 0.1).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    wall = []
    for _ in range(2):   # (the second: nothing left to load or allocate for the first time)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        acc = swd.SlicedWasserstein((H, W), seed=0)
        for _ in range(args.images // b):
            acc.add(images, fake)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        out = acc.result()
        torch.cuda.synchronize()
        wall.append(dict(add_s=t1 - t0, result_s=time.perf_counter() - t1))
        del acc
    result.update(metric_wall=wall, metric=out)
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
