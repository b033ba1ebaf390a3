"""What the three kernel sums of the kernel inception distance cost on the device ("KID on the device").

    python scripts/bench_kid.py [--repeats 10] [--out profiles/kid_bench.json]

d = 512 columns, a seeded Gaussian mixture with a common offset (as the classifier's post-ReLU features have), the second set shifted a little.
  * The full sets at n = m = 4096, 8192 and 50000 rows, and 100 subsets of 1000 rows a side of the 50000: gs_kid_sums on preallocated buffers,
    HIP events around every call,
  * next to a torch float64 restatement of the same sums -- torch.matmul in float64 (the BLAS's fp64 matrix-core path), the cubic, the sum, the
    diagonal taken off the symmetric ones; row-chunked so that its Gram block fits; the subsets gathered first -- on the same device in the same
    process and alternating.
  * The fp64 matrix-core roof: a register-only probe loop (no memory traffic: every wave of a grid that fills the part issues independent
    v_mfma_f64_16x16x4_f64 back to back), compiled here with hipcc.  The datasheet's 78.6 TFLOP/s is quoted beside it, unverified.
Reported per case: median / min / max device ms of each, their ratio, the entry's FLOP/s -- 2 d flops a pair, the pairs it has to visit: the
upper triangles with their diagonals and the rectangle -- and that as a share of the probed roof, the largest relative deviation of the three
sums from torch's; and the wall time metrics.kernel_inception_distance_device (what --kid adds to an evaluation: host arrays in, figures out)
takes at every size.  Needs a GPU and hipcc; prints one JSON object.
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DATASHEET_FP64_MATRIX_FLOPS = 78.6e12   # quoted, unverified
SIZES = [4096, 8192, 50000]
D = 512
SUBSETS, SUBSET_SIZE = 100, 1000
CHUNK = 4096                            # rows of the torch restatement's Gram block at a time

PROBE_SOURCE = r"""
#include <hip/hip_runtime.h>
typedef double f64x4 __attribute__((ext_vector_type(4)));
// every wave: 8 independent accumulators, `iters` rounds of 8 MFMAs, operands in registers; the sum leaves the wave so that nothing is dropped
__global__ __launch_bounds__(256) void probe(double* out, int iters, double a, double b) {
    f64x4 acc[8];
    for (int i = 0; i < 8; ++i) acc[i] = f64x4{0.0, 0.0, 0.0, 0.0};
    const double x = a + threadIdx.x, y = b + blockIdx.x;
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(x, y, acc[i], 0, 0, 0);
    }
    double s = 0.0;
    for (int i = 0; i < 8; ++i) s += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
    out[(size_t)blockIdx.x * blockDim.x + threadIdx.x] = s;
}
extern "C" int probe_launch(double* out, int blocks, int iters, void* stream) {
    hipLaunchKernelGGL(probe, dim3(blocks), dim3(256), 0, (hipStream_t)stream, out, iters, 1.0, 2.0);
    return (int)hipGetLastError();
}
"""


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


def torch_sum(a, b, same):
    """sum over the pairs of (a.b / d + 1)^3 in float64, a chunk of rows at a time; with `same` without the pairs of a row with itself."""
    d = a.shape[1]
    total = torch.zeros((), dtype=torch.float64, device=a.device)
    for at in range(0, len(a), CHUNK):
        t = torch.matmul(a[at:at + CHUNK], b.T) / d + 1.0
        k = t * t * t
        total += k.sum()
        if same:
            total -= k.diagonal(at).sum()
    return total


def torch_sums(x, y, xi=None, yi=None):
    """-> [S, 3] float64: the restatement of gs_kid_sums."""
    x64, y64 = x.double(), y.double()
    if xi is None:
        return torch.stack([torch_sum(x64, x64, True), torch_sum(y64, y64, True), torch_sum(x64, y64, False)])[None]
    rows = []
    for s in range(len(xi)):
        a, b = x64[xi[s].long()], y64[yi[s].long()]
        rows.append(torch.stack([torch_sum(a, a, True), torch_sum(b, b, True), torch_sum(a, b, False)]))
    return torch.stack(rows)


def probe_roof(repeats):
    """The fp64 MFMA rate of the whole part from registers alone: -> dict(flops=, ms=, blocks=, iters=)."""
    with tempfile.TemporaryDirectory() as tmp:
        src, lib_path = os.path.join(tmp, "probe.hip"), os.path.join(tmp, "libprobe.so")
        with open(src, "w") as f:
            f.write(PROBE_SOURCE)
        # (accumulators in VGPRs, as in the kernel: otherwise hipcc copies all 64 registers to AGPRs and back around every round of the loop)
        subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-shared", "-fPIC", "-mllvm", "-amdgpu-mfma-vgpr-form", src, "-o", lib_path], check=True)
        lib = ctypes.CDLL(lib_path)
        lib.probe_launch.restype = ctypes.c_int
        lib.probe_launch.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        blocks, iters = cus * 2, 4096                     # two blocks of four waves a CU: two waves a SIMD
        out = torch.empty(blocks * 256, dtype=torch.float64, device="cuda")
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

        def run():
            code = lib.probe_launch(out.data_ptr(), blocks, iters, stream)
            if code:
                raise SystemExit(f"the probe's launch failed ({code})")

        run()
        torch.cuda.synchronize()
        ms = stats(timed(run, repeats))
        flops = blocks * 4 * iters * 8 * 2.0 * 16 * 16 * 4
        return dict(flops=flops / ms["min"] * 1e3, ms=ms, blocks=blocks, iters=iters, compute_units=cus)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_kid.py measures on the GPU: no device found")
    from gansynth_amd import _lib, kernels, kid, metrics
    torch.cuda.set_device(0)
    K = kernels.get()
    roof = probe_roof(args.repeats)
    print(f"probe: {roof['flops'] / 1e12:.2f} TFLOP/s", file=sys.stderr, flush=True)
    cases = []
    for n in SIZES:
        x, means = mixture(n, D, 0)
        y = mixture(n, D, 2, means)[0] + 0.05
        todo = [("full", None, None)]
        if n == SIZES[-1]:
            xi, yi = (torch.from_numpy(t).cuda() for t in kid.draw_subsets(n, n, SUBSETS, SUBSET_SIZE, 0))
            todo.append(("subsets", xi, yi))
        for what, xi, yi in todo:
            subsets, size = (0, 0) if xi is None else tuple(xi.shape)
            rows = size if subsets else n
            out = torch.empty(max(subsets, 1), 3, dtype=torch.float64, device="cuda")
            ws_bytes = int(K.lib.gs_kid_workspace_bytes(n, n, D, subsets, size))
            ws = torch.empty(max(ws_bytes, 256), dtype=torch.uint8, device="cuda")
            held = {}

            def device():
                _lib.check(K.lib.gs_kid_sums(x.data_ptr(), D, n, y.data_ptr(), D, n, D, xi.data_ptr() if subsets else None, yi.data_ptr() if subsets else None,
                                             subsets, size, out.data_ptr(), ws.data_ptr(), ws.numel(), kernels._stream()), "gs_kid_sums")

            def restatement():
                held["sums"] = torch_sums(x, y, xi, yi)

            fns = dict(device=device, torch=restatement)
            for fn in fns.values():
                fn()
            torch.cuda.synchronize()
            deviation = float(((out - held["sums"]).abs() / held["sums"].abs()).max())
            ms = {name: [] for name in fns}
            for block in range(5):   # alternating blocks: other work shares the machine
                for name, fn in fns.items():
                    ms[name] += timed(fn, max(args.repeats // 5, 1))
                print(f"n {n} {what}: block {block} timed", file=sys.stderr, flush=True)
            pairs = max(subsets, 1) * (rows * (rows + 1) + rows * rows)   # two triangles with their diagonals and the rectangle
            flops = 2.0 * D * pairs
            case = dict(what=what, n=n, m=n, d=D, subsets=subsets, size=size, workspace_bytes=ws_bytes, flops=flops,
                        largest_relative_deviation_from_torch_float64=deviation, device_ms=stats(ms["device"]), torch_ms=stats(ms["torch"]))
            case["torch_over_device"] = case["torch_ms"]["median"] / case["device_ms"]["median"]
            case["device_tflops"] = flops / case["device_ms"]["median"] / 1e9
            case["device_fraction_of_probed_roof"] = case["device_tflops"] * 1e12 / roof["flops"]
            case["fastest"] = "device" if case["torch_over_device"] >= 1.0 else "torch"
            if what == "full":
                real, fake = x.cpu().numpy(), y.cpu().numpy()
                wall = []
                for _ in range(2):   # (the second: nothing left to load or allocate for the first time)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    figures = metrics.kernel_inception_distance_device(real, fake)
                    torch.cuda.synchronize()
                    wall.append(time.perf_counter() - t0)
                case.update(kernel_inception_distance_wall_s=wall, figures=figures)
                del real, fake
            cases.append(case)
            del held
        del x, y
        torch.cuda.empty_cache()
    result = dict(repeats=args.repeats, datasheet_fp64_matrix_flops_unverified=DATASHEET_FP64_MATRIX_FLOPS, probed_fp64_mfma_roof=roof, cases=cases)
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
