"""What the k-nearest-neighbour radii and the cover counts of precision / recall / density / coverage cost on the device ("Precision
and recall on the device").

    python scripts/bench_knn.py [--repeats 10] [--out profiles/knn_bench.json]

Two sizes: n = m = 8192 and n = m = 50000 rows of d = 512 columns, k = 3; a seeded Gaussian mixture with a common offset (as the classifier's
post-ReLU features have).  For each, on the same device in the same process and alternating:
  gs_knn_kth of the set against itself (the radii) and gs_knn_within of a second set against those radii -- the entries on preallocated
  buffers, HIP events around every call --
  next to a torch restatement of the same results in the GEMM form: torch.cdist (|x|^2 - 2 x.y + |y|^2 through a matrix product), row-chunked
  so that its matrix fits, then topk / a compare and a sum.
Reported per size: median / min / max device ms of each, the entries as a share of the fp32 vector peak of the datasheet from 3 n m d flops, the
slice count, the largest relative deviation of the device's radii and of torch's from float64 radii (torch.cdist in float64, the direct form),
the rows whose count differs between the two, and the wall time of metrics.precision_recall_device (host clock, the features already on the
device) on real and fake sets of that size.  Needs a GPU; prints one JSON object.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VECTOR_FLOPS = 157.3e12          # fp32 vector peak of the datasheet
SIZES = [(8192, 512, 3), (50000, 512, 3)]
CHUNK = 4096                     # rows of the torch restatement's distance matrix at a time


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


def mixture(n, d, seed, means=None):
    g = torch.Generator("cuda").manual_seed(seed)
    if means is None:
        means = 4.0 + 0.75 * torch.randn(50, d, device="cuda", generator=g)
    comp = torch.randint(0, len(means), (n,), device="cuda", generator=g)
    return means[comp] + torch.randn(n, d, device="cuda", generator=g), means


def torch_radii(x, k, dtype=torch.float32, mode="use_mm_for_euclid_dist"):
    """R_k of every row by torch: cdist a chunk of rows at a time, the diagonal out, topk; squared."""
    out = torch.empty(len(x), dtype=dtype, device=x.device)
    xx = x.to(dtype)
    # (the direct form launches a block per pair: its grid holds 2^23 pairs at a time here, under the 2^32 threads a launch may have)
    chunk = CHUNK if mode == "use_mm_for_euclid_dist" else max(1, (1 << 23) // len(x))
    for at in range(0, len(x), chunk):
        dist = torch.cdist(xx[at:at + chunk], xx, compute_mode=mode)
        rows = torch.arange(dist.shape[0], device=x.device)
        dist[rows, rows + at] = float("inf")
        out[at:at + chunk] = dist.topk(k, dim=1, largest=False).values[:, k - 1] ** 2
    return out


def torch_within(q, ref, radius2):
    out = torch.empty(len(q), dtype=torch.int32, device=q.device)
    for at in range(0, len(q), CHUNK):
        out[at:at + CHUNK] = (torch.cdist(q[at:at + CHUNK], ref, compute_mode="use_mm_for_euclid_dist") ** 2 <= radius2[None, :]).sum(dim=1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_knn.py measures on the GPU: no device found")
    from gansynth_amd import _lib, kernels, metrics
    torch.cuda.set_device(0)
    K = kernels.get()
    cases = []
    for n, d, k in SIZES:
        x, means = mixture(n, d, 0)
        fake = mixture(n, d, 2, means)[0] + 0.05
        out = torch.empty(n, k, device="cuda")
        count = torch.empty(n, dtype=torch.int32, device="cuda")
        ws_bytes = int(K.lib.gs_knn_workspace_bytes(n, n, d, k))
        ws = torch.empty(max(ws_bytes, 256), dtype=torch.uint8, device="cuda")
        held = {}

        def kth():
            _lib.check(K.lib.gs_knn_kth(x.data_ptr(), d, n, x.data_ptr(), d, n, d, k, 1, out.data_ptr(), ws.data_ptr(), ws.numel(), kernels._stream()), "gs_knn_kth")

        kth()
        radius2 = out[:, k - 1].contiguous()

        def within():
            _lib.check(K.lib.gs_knn_within(fake.data_ptr(), d, n, x.data_ptr(), d, n, d, radius2.data_ptr(), count.data_ptr(), ws.data_ptr(), ws.numel(),
                                           kernels._stream()), "gs_knn_within")

        def torch_kth():
            held["radii"] = torch_radii(x, k)

        def torch_count():
            held["count"] = torch_within(fake, x, radius2)

        fns = dict(kth=kth, within=within, torch_kth=torch_kth, torch_within=torch_count)
        for _ in range(2):
            for fn in fns.values():
                fn()
        torch.cuda.synchronize()
        print(f"n {n}: warmed up, float64 radii ...", file=sys.stderr, flush=True)
        exact = torch_radii(x, k, torch.float64, "donot_use_mm_for_euclid_dist")
        case = dict(n=n, m=n, d=d, k=k, slices=int(K.lib.gs_knn_slices(n, n, d)), workspace_bytes=ws_bytes,
                    largest_relative_deviation_from_float64_radii=dict(device=float(((radius2.double() - exact).abs() / exact).max()),
                                                                       torch_gemm=float(((held["radii"].double() - exact).abs() / exact).max())),
                    rows_whose_count_differs_from_torch=int((count != held["count"]).sum()))
        del exact
        ms = {name: [] for name in fns}
        for block in range(5):   # alternating blocks: other work shares the machine
            for name, fn in fns.items():
                ms[name] += timed(fn, max(args.repeats // 5, 1))
            print(f"n {n}: block {block} timed", file=sys.stderr, flush=True)
        for name in fns:
            case[name + "_ms"] = stats(ms[name])
        flops = 3.0 * n * n * d
        for name in ("kth", "within"):
            case[name + "_tflops"] = flops / case[name + "_ms"]["median"] / 1e9
            case[name + "_fraction_of_vector_peak"] = flops / VECTOR_FLOPS * 1e3 / case[name + "_ms"]["median"]
        case["flops"] = flops
        wall = []
        for _ in range(2):   # (the second: nothing left to load or allocate for the first time)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            figures = metrics.precision_recall_device(x, fake, k=k)
            torch.cuda.synchronize()
            wall.append(time.perf_counter() - t0)
        case.update(precision_recall_wall_s=wall, figures=figures,
                    fastest=dict(kth="device" if case["kth_ms"]["median"] <= case["torch_kth_ms"]["median"] else "torch",
                                 within="device" if case["within_ms"]["median"] <= case["torch_within_ms"]["median"] else "torch"))
        cases.append(case)
        del x, fake, held
        torch.cuda.empty_cache()
    result = dict(repeats=args.repeats, vector_flops=VECTOR_FLOPS, cases=cases)
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
