"""What the k-means of the NDB metric costs on the device ("NDB on the device").

    python scripts/bench_kmeans.py [--repeats 20] [--out profiles/kmeans_bench.json]

Two sizes of (rows, columns, centres): the NSynth training split's features (289205, 512, 50) and (4096, 512, 50); a seeded Gaussian mixture
with a common offset, the centres 50 of its rows.  For each, on the same device in the same process and alternating:
  gs_kmeans_assign as Lloyd's loop calls it (labels, distances, the moved-label count), gs_kmeans_update, one Lloyd iteration (both) and
  gs_kmeans_inertia (once at the end of a run) -- the entries on preallocated buffers, HIP events around every call --
  next to a torch restatement: torch.cdist(compute_mode="donot_use_mm_for_euclid_dist") and argmin; index_add_, bincount and a division;
  and, when scikit-learn imports, one Lloyd iteration of sklearn.cluster.KMeans (algorithm="lloyd", 16 threads) on the host: the difference
  of fits with max_iter 4 and 1 from the same centres over the difference of their n_iter_ (a fit also stops when no label moved, whatever
  tol is: the iterations each fit really ran are recorded beside the figure), the median of 15 such pairs; `from_minima` is the same quotient of the fastest fit of either kind.
Reported per size: median / min / max device ms of each, assign as a share of the fp32 vector peak of the datasheet from 3 n k d flops,
update as a share of the measured HBM copy rate from 4 n d bytes, the largest label disagreement with torch, and the wall time of
metrics.num_different_bins_device (host clock, the features already on the device, ten restarts) on real and fake sets of that size.
Needs a GPU; prints one JSON object.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BYTES_PER_S = 6.29e12        # float4 copy, measured (8.0e12 by the datasheet)
VECTOR_FLOPS = 157.3e12          # fp32 vector peak of the datasheet
SIZES = [(289205, 512, 50), (4096, 512, 50)]
HOST_THREADS = 16
SKLEARN_ITERS, SKLEARN_REPEATS = (1, 4), 15  # max_iter of the two fits whose difference is timed (few: the small size converges in five or six)


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


def mixture(n, d, k, seed):
    g = torch.Generator("cuda").manual_seed(seed)
    means = 4.0 + 0.75 * torch.randn(k, d, device="cuda", generator=g)
    comp = torch.randint(0, k, (n,), device="cuda", generator=g)
    return means[comp] + torch.randn(n, d, device="cuda", generator=g)


def sklearn_iteration_ms(x, centres):
    try:
        from sklearn.cluster import KMeans
        from threadpoolctl import threadpool_limits
    except ImportError:
        return None
    k = len(centres)

    def fit(iters):   # -> (ms, the iterations it really ran: Lloyd also stops when no label moved, whatever tol is)
        t0 = time.perf_counter()
        model = KMeans(n_clusters=k, init=centres, n_init=1, max_iter=iters, tol=0.0, algorithm="lloyd").fit(x)
        return (time.perf_counter() - t0) * 1e3, int(model.n_iter_)
    import warnings
    with threadpool_limits(limits=HOST_THREADS), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        fit(1)
        per, ran, longs, shorts = [], set(), [], []
        for _ in range(SKLEARN_REPEATS):
            (long_ms, long_iters), (short_ms, short_iters) = fit(SKLEARN_ITERS[1]), fit(SKLEARN_ITERS[0])
            ran.add((short_iters, long_iters))
            longs.append(long_ms)
            shorts.append(short_ms)
            if long_iters > short_iters:
                per.append((long_ms - short_ms) / (long_iters - short_iters))
    if not per or len(ran) != 1:   # (the same data and init every time: the fits must agree on their iterations)
        return None
    per.sort()
    short_iters, long_iters = next(iter(ran))
    return dict(median=per[len(per) // 2], min=per[0], max=per[-1], from_minima=(min(longs) - min(shorts)) / (long_iters - short_iters),
                threads=HOST_THREADS, max_iter=list(SKLEARN_ITERS), n_iter=[short_iters, long_iters])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_kmeans.py measures on the GPU: no device found")
    from gansynth_amd import _lib, kernels, metrics
    torch.cuda.set_device(0)
    K = kernels.get()
    cases = []
    for n, d, k in SIZES:
        x = mixture(n, d, k, 0)
        centres0 = x[torch.randperm(n, device="cuda", generator=torch.Generator("cuda").manual_seed(1))[:k]].contiguous()
        centres = centres0.clone()
        labels = torch.zeros(n, dtype=torch.int32, device="cuda")
        dist = torch.empty(n, device="cuda")
        changed, inertia = torch.empty(1, dtype=torch.int32, device="cuda"), torch.empty(1, dtype=torch.float64, device="cuda")
        counts = torch.empty(k, dtype=torch.int32, device="cuda")
        ws_bytes = int(K.lib.gs_kmeans_workspace_bytes(n, d, k))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")

        def assign():   # as Lloyd's loop calls it: labels, distances, the moved-label count
            _lib.check(K.lib.gs_kmeans_assign(x.data_ptr(), d, n, d, centres0.data_ptr(), k, labels.data_ptr(), dist.data_ptr(), changed.data_ptr(),
                                              None, ws.data_ptr(), ws_bytes, kernels._stream()), "gs_kmeans_assign")

        def inertia_of_labels():   # the end of a run: the inertia of the final labels in double (one read of x)
            _lib.check(K.lib.gs_kmeans_inertia(x.data_ptr(), d, n, d, centres0.data_ptr(), k, labels.data_ptr(), inertia.data_ptr(), ws.data_ptr(), ws_bytes,
                                               kernels._stream()), "gs_kmeans_inertia")

        def update():
            _lib.check(K.lib.gs_kmeans_update(x.data_ptr(), d, n, d, labels.data_ptr(), k, centres.data_ptr(), counts.data_ptr(), ws.data_ptr(), ws_bytes,
                                              kernels._stream()), "gs_kmeans_update")

        def iteration():
            assign()
            update()

        held = {}

        def torch_assign():
            held["labels"] = torch.cdist(x, centres0, compute_mode="donot_use_mm_for_euclid_dist").argmin(dim=1)

        def torch_update():
            sums = torch.zeros(k, d, device="cuda").index_add_(0, held["labels"], x)
            held["centres"] = sums / torch.bincount(held["labels"], minlength=k).clamp(min=1)[:, None]

        def torch_iteration():
            torch_assign()
            torch_update()

        fns = dict(assign=assign, inertia=inertia_of_labels, update=update, iteration=iteration, torch_assign=torch_assign, torch_update=torch_update,
                   torch_iteration=torch_iteration)
        for _ in range(3):
            for fn in fns.values():
                fn()
        torch.cuda.synchronize()
        disagree = int((labels.long() != held["labels"]).sum())
        centre_difference = float((centres - held["centres"]).abs().max())
        ms = {name: [] for name in fns}
        for _ in range(5):   # alternating blocks: other work shares the machine
            for name, fn in fns.items():
                ms[name] += timed(fn, max(args.repeats // 5, 1))
        case = dict(n=n, d=d, k=k, workspace_bytes=ws_bytes, labels_differing_from_torch=disagree, largest_centre_difference_from_torch=centre_difference)
        for name in fns:
            case[name + "_ms"] = stats(ms[name])
        flops, nbytes = 3.0 * n * k * d, 4.0 * n * d
        case.update(assign_flops=flops, assign_tflops=flops / case["assign_ms"]["median"] / 1e9,
                    assign_fraction_of_vector_peak=flops / VECTOR_FLOPS * 1e3 / case["assign_ms"]["median"],
                    inertia_tb_per_s=nbytes / case["inertia_ms"]["median"] / 1e9,
                    update_bytes=nbytes, update_tb_per_s=nbytes / case["update_ms"]["median"] / 1e9,
                    update_fraction_of_hbm_roof=nbytes / HBM_BYTES_PER_S * 1e3 / case["update_ms"]["median"],
                    sklearn_iteration_host_ms=sklearn_iteration_ms(x.cpu().numpy(), centres0.cpu().numpy()))
        fake = mixture(n, d, k, 2) + 0.05
        wall = []
        for _ in range(2):   # (the second: nothing left to load or allocate for the first time)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            details = {}
            ndb = metrics.num_different_bins_device(x, fake, num_bins=k, details=details)
            torch.cuda.synchronize()
            wall.append(time.perf_counter() - t0)
        case.update(ndb_wall_s=wall, ndb=ndb, ndb_jsd=details["jsd"], ndb_inertia=details["inertia"])
        three = dict(device=case["iteration_ms"]["median"], torch=case["torch_iteration_ms"]["median"])
        if case["sklearn_iteration_host_ms"] is not None:
            three["sklearn"] = case["sklearn_iteration_host_ms"]["median"]
        case["fastest_iteration"] = min(three, key=three.get)
        cases.append(case)
        del x, fake, held
    result = dict(repeats=args.repeats, hbm_bytes_per_s=HBM_BYTES_PER_S, vector_flops=VECTOR_FLOPS, cases=cases)
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
