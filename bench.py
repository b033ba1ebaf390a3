"""Headline benchmark: G+D training step images/sec at 128x1024x2 (log-mel + IF), fully grown.

    python bench.py --gpus N --steps K --warmup W            (any N: for N > 1 without a launcher it starts its N ranks itself)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W     (N>1 under a launcher: one rank per GPU, RCCL)

One step = one reference iteration (models.py:191-192): a discriminator update then a generator
update, each on its own synthetic batch of `--batch` (default 8) examples per GPU, inputs already
resident in HBM.  Prints ONE JSON line on rank 0.

A plain run sets up, warms up, times the `--steps` iterations and prints the line (`value`, `ms_per_step`, ...).
`--full` adds everything else after the timed steps: the per-launch conv profile and `roofline`, the whole step against
its roofs, the launch count, the in-run PMC traffic passes, the spectral legs, the fp32 leg and the CPU baselines.
`--dump-outputs DIR` writes what the last timed step computed (both losses, a fixed sample of the updated weights) as
DIR/<name>.npy, so that two builds can be compared output for output on the same seeded inputs.
"""
import argparse
import glob
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

FLOPS_PER_IMAGE = 268.1e9  # 7*F_G + 11*F_D, SURVEY.md 8(d)
HBM_GBPS = 8000.0  # MI355X_MICROARCH.md: HBM3E ~8 TB/s
PEAK = {"f32": 157.3, "bf16": 2500.0}  # dense MFMA TFLOP/s, MI355X_MICROARCH.md
# Per-launch conv timing: every conv launch of the profiled eager iterations is issued PROF_BURST times back to back inside its HIP
# event pair (gs_prof_enable(n)): the launch-to-launch time in steady state, one launch boundary included.  An event pair around a
# SINGLE eager launch of 7-30 us also times ~4-5 us of host launch latency (the stream runs dry between eager launches).
PROF_BURST = int(os.environ.get("GS_PROF_BURST", "4"))


def synthetic_pool(batch, rank, dtype, n=4):
    """SURVEY.md 8(d) synthetic inputs, generated once and kept in HBM."""
    pool = []
    for i in range(n):
        g = torch.Generator().manual_seed(1000 + rank + 97 * i)
        lat = torch.randn(batch, 256, generator=g)
        g = torch.Generator().manual_seed(2000 + rank + 97 * i)
        lab = torch.nn.functional.one_hot(torch.randint(0, 61, (batch,), generator=g), 61).float()
        g = torch.Generator().manual_seed(3000 + rank + 97 * i)
        real = torch.randn(batch, 2, 128, 1024, generator=g)
        real[:, 0] = real[:, 0] * 0.6 - 0.2
        real[:, 1] = real[:, 1] * 0.4
        real = real.clamp_(-1, 1)
        pool.append((lat.cuda().to(dtype), lab.cuda().to(dtype),
                     real.cuda().to(dtype).contiguous(memory_format=torch.channels_last)))
    return pool


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline(batch=8, timed=3):
    """The CPU oracle (torch-CPU fp32 restatement of the reference graph: the TF1 reference itself cannot run here, SURVEY.md
    8c/D3) timed on this host's cores as SURVEY.md 8(d) specifies: batch 8, fully grown 128x1024x2, one warm-up iteration
    (D update + G update, R1 + mode-seeking double-backward, TF-Adam) then `timed` timed ones."""
    from oracle import torch_ref as R
    total = os.cpu_count() or 1
    # SURVEY 8(d) says torch.set_num_threads(os.cpu_count()); measured on the pool's 256-thread EPYC 9575F hosts that run is ~40x SLOWER
    # than 32 threads (torch-CPU's conv backward oversubscribes; ~9 minutes per iteration), so the baseline runs on 32 threads -- the
    # fastest setting found (16: 0.41, 32: 0.61-0.67, 64: 0.52 images/s) -- and says so in `sample`
    cores = min(total, 32)
    torch.set_num_threads(cores)
    pg = R.PGGAN([2, 16], [128, 1024], 32, 256, 1.0)
    gp, dp = pg.init_params(seed=0)
    tr = R.Trainer(pg, gp, dp)
    lat, lab, real = R.synthetic_batch(batch)
    tr.d_step(lat, lab, real)
    tr.g_step(lat, lab)
    t0 = time.time()
    for i in range(timed):
        lat, lab, real = R.synthetic_batch(batch, rank=1 + i)
        tr.d_step(lat, lab, real)
        tr.g_step(lat, lab)
    dt = (time.time() - t0) / timed
    return {"value": batch / dt, "unit": "images/sec", "cores": cores, "kind": "port", "host_cores": total, "cpu_model": cpu_model(),
            "seconds_per_iteration": dt,
            "sample": "1 warm-up + %d timed iterations (D update + G update incl. R1 + mode-seeking double-backward, TF-Adam) at batch %d, "
                      "fully grown 128x1024x2, fp32, torch-CPU oracle (oracle/torch_ref.py), %d of %d host threads (all %d threads measured ~40x slower)"
                      % (timed, batch, cores, total, total)}


SPECTRAL_BYTES_PER_EXAMPLE = 64000 * 4 + 2 * 128 * 1024 * 4   # waveform read once + (log-mel, IF) written once, fp32


def spectral_bench(batch=256, iters=1000, warmup=300, cpu=True):
    """BASELINE.json configs[3]: waveform [256, 64000] -> (log-mel, IF) images [256, 2, 128, 1024] (spectral_ops.py:45-94), one
    fused HIP launch per batch, inputs resident in HBM.  HBM-bound by design (1.30 MB of algorithmic traffic per example); the
    kernel is timed with HIP events on its launch stream."""
    import numpy as np
    from gansynth_amd import spectral_ops as G
    P = dict(waveform_length=64000, sample_rate=16000, spectrogram_shape=[128, 1024], overlap=0.75)
    rng = np.random.default_rng(4000)
    w = np.clip(rng.normal(0.0, 0.1, (batch, 64000)), -1, 1).astype(np.float32)   # SURVEY.md 8(d) synthetic waveforms
    x = torch.from_numpy(w).cuda()
    # steady state: 300 untimed + 1000 timed launches (~0.14 s).  A 2 ms burst of 20 launches after an idle period measured
    # 105-124 us per launch on the same box -- the shader clock is still ramping -- where the sustained rate is 102-105 us
    # (scripts/spectral_run.py 10 / 100 / 1000 / 5000).
    for _ in range(warmup):
        G.convert_to_images(x, **P)
    torch.cuda.synchronize()
    # one HIP event pair around `iters` back-to-back launches on the launch stream: the host enqueues faster than the kernel
    # runs, so the device stays busy and the average is the kernel's launch-to-launch time (an event pair around a single call
    # would also time the ~10 us of host work between the first event and the launch)
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    s.record()
    for _ in range(iters):
        G.convert_to_images(x, **P)
    e.record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / iters
    kern_ms = s.elapsed_time(e) / iters
    bytes_alg = batch * SPECTRAL_BYTES_PER_EXAMPLE
    achieved = bytes_alg / (kern_ms * 1e-3) / 1e9
    traffic = None
    pmcs = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_spectral_pmc_traffic.json")))
    if pmcs and batch == 256:
        traffic = json.load(open(pmcs[-1]))["avg_hbm_bytes_per_launch"]
    out = {"workload": "BASELINE.json configs[3]: %d x 64000-sample waveforms -> (log-mel, IF) [%d, 2, 128, 1024], fp32, one fused launch" % (batch, batch),
           "launches_timed": iters, "launches_warmup": warmup,
           "value": batch / wall, "unit": "examples/sec", "us_per_batch": wall * 1e6, "dtype": "f32",
           "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_GBPS, "unit": "GB/s", "frac": achieved / HBM_GBPS,
                        "traffic": traffic, "traffic_source": "committed rocprofv3 PMC passes (profiles/, FETCH_SIZE x2 + WRITE_SIZE), not measured in this run",
                        "algorithmic_bytes_per_launch": bytes_alg, "avg_launch_ms": kern_ms,
                        "kernel": "stft_wave_kernel<float, 1> (framing + Hann + 2048-point real FFT + |.| / atan2 + mel gather + log / IF per wave)",
                        "note": "the kernel is LDS-pipe / VALU bound, not HBM bound (profiles/r02_*_spectral_pmc.txt); frac is against the HBM roof SURVEY.md 8(d) prescribes"}}
    if cpu:
        # the same workload (all `batch` waveforms) on the host's own cores -- the numpy oracle in one worker process
        # per core (oracle/cpu_bench.py; its own interpreter, so that the pool is forked from a process without HIP state)
        import subprocess
        host = os.cpu_count() or 1
        best, err = None, None
        for procs in sorted({host, max(1, host // 2), max(1, host // 4)}, reverse=True):   # all hardware threads, one per core pair, half of those
            res = subprocess.run([sys.executable, "-m", "oracle.cpu_bench", "--examples", str(batch), "--procs", str(procs)], cwd=ROOT,
                                 capture_output=True, text=True, timeout=600)
            if res.returncode != 0:
                err = (res.stderr or res.stdout)[-300:]
                continue
            r = json.loads(res.stdout.strip().splitlines()[-1])
            if best is None or r["seconds"] < best["seconds"]:
                best = r
        if best is not None:
            r = best
            out["cpu_baseline"] = {"value": r["examples"] / r["seconds"], "unit": "examples/sec", "cores": r["procs"], "host_cores": r["host_cores"],
                                   "kind": "port", "cpu_model": cpu_model(), "seconds": r["seconds"],
                                   "sample": "all %d waveforms through the numpy oracle (oracle/spectral_np.py, fp32), %d worker processes of one thread each "
                                             "(oracle/cpu_bench.py; the fastest of all / half / a quarter of the %d hardware threads), timed after one warm-up "
                                             "example per worker" % (r["examples"], r["procs"], r["host_cores"])}
        else:
            out["cpu_baseline"] = {"error": err}
    return out


def inverse_bench(batch=256, iters=50, warmup=10):
    """(log-mel, IF) images [256, 2, 128, 1024] -> waveforms [256, 64000] (spectral_ops.py:97-149): exp / cumulative phase,
    the pinv(mel) contraction of magnitude and phase as ONE GEMM at fp32 accuracy (phases reach ~1e3 rad): every operand is the exact
    sum of three bf16 numbers and six bf16 MFMAs keep the partial products down to 2^-16 (gemm_bf16x6_kernel), then
    polar -> inverse FFT -> overlap-add.  The GEMM dominates: MFMA-bound; `roofline` prices the bf16 products the MFMA pipe
    executes against the dense bf16 peak (never above 1); the algorithmic fp32 rate of the call is a separate field."""
    import numpy as np
    from gansynth_amd import spectral_ops as G
    P = dict(waveform_length=64000, sample_rate=16000, spectrogram_shape=[128, 1024], overlap=0.75)
    rng = np.random.default_rng(4001)
    x = torch.from_numpy(np.clip(rng.normal(0.0, 0.1, (batch, 64000)), -1, 1).astype(np.float32)).cuda()
    img = G.convert_to_images(x, **P)
    for _ in range(warmup):
        G.convert_images_to_waveform(img, **P)
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        G.convert_images_to_waveform(img, **P)
    e.record()
    torch.cuda.synchronize()
    ms = s.elapsed_time(e) / iters
    flops = 2.0 * 2.0 * batch * 128 * 1024 * 1024   # [2 * batch * 128, 1024] x [1024, 1024]: magnitude and phase rows stacked
    # The contraction runs on the bf16 MFMA as partial products of bf16 splits of fp32 operands: six per algorithmic multiply-add on the
    # phase rows, three on the magnitude rows.  The roofline prices what the MFMA pipe EXECUTES (4.5 bf16 products per algorithmic
    # one on average) against the dense bf16 peak, per GEMM launch (HIP events of the library's own profiler around the two launches).
    from gansynth_amd import kernels
    K = kernels.get()
    gemm = None
    K.prof_enable(True)   # (library profiler: HIP event pairs around the GEMM launches, on their stream)
    for _ in range(20):
        G.convert_images_to_waveform(img, **P)
    torch.cuda.synchronize()
    recs = [r for r in K.prof_records() if r[3][0] in (30, 31, 32)]
    K.prof_collect()
    K.prof_enable(False)
    if recs:
        by_kind = {}
        for r_ms, _, _, d in recs:
            by_kind.setdefault(d[0], []).append(r_ms)
        gemm = {{30: "magnitude_ms", 31: "phase_ms", 32: "all_rows_ms"}[k]: sum(v) / len(v) for k, v in by_kind.items()}
        executed = sum(r[1] for r in recs) / 20.0
    else:
        executed = 4.5 * flops
    out = {"workload": "%d x (log-mel, IF) [2, 128, 1024] -> 64000-sample waveforms, fp32 (spectral_ops.py:97-149)" % batch,
           "value": batch / (ms * 1e-3), "unit": "examples/sec", "ms_per_batch": ms, "dtype": "f32 results from bf16 x3 split operands on the bf16 MFMA",
           "algorithmic_tflops_whole_call": flops / (ms * 1e-3) / 1e12}
    if gemm:
        g_ms = sum(gemm.values())
        ach = executed / (g_ms * 1e-3) / 1e12
        out["roofline"] = {"bound": "mfma", "achieved": ach, "peak": PEAK["bf16"], "unit": "TFLOP/s", "frac": ach / PEAK["bf16"],
                           "frac_algorithmic": flops / (g_ms * 1e-3) / 1e12 / PEAK["bf16"],   # the fp32 contraction's own multiply-adds against the same peak
                           "kernel": "gemm_bf16x6_kernel (the two GEMM launches: phase rows 6 products, magnitude rows 3)",
                           "avg_launch_ms": g_ms / len(gemm), "gemm_ms": gemm, "gemm_share_of_call": g_ms / ms,
                           "executed_flops_per_call": executed, "algorithmic_flops_per_call": flops,
                           "note": "achieved = executed bf16 MFMA FLOPs of the two GEMM launches / their HIP-event time; the algorithmic (fp32) rate of the whole call is algorithmic_tflops_whole_call"}
    else:
        ach = executed / (ms * 1e-3) / 1e12
        out["roofline"] = {"bound": "mfma", "achieved": ach, "peak": PEAK["bf16"], "unit": "TFLOP/s", "frac": ach / PEAK["bf16"],
                           "executed_flops_per_call": executed, "algorithmic_flops_per_call": flops,
                           "note": "executed bf16 MFMA FLOPs (4.5 per algorithmic one) over the WHOLE call (prep + 2 GEMM launches + iFFT / overlap-add)"}
    return out


PARITY_NOTE = {
    "bf16": ("bf16 = storage dtype of activations (fp32 accumulation, fp32 master weights / Adam): the throughput dtype BASELINE.json configs[1] names.  "
             "The 1e-3 parity contract with the oracle is held by the fp32 path (--dtype f32; tests/test_model_gpu.py::test_fully_grown_full_size_step_vs_oracle); "
             "the bf16 path is checked against the oracle on its own leaky-relu pieces at 3e-2 relative L2 per gradient tensor "
             "(test_full_size_bf16_step_vs_oracle_on_its_linear_pieces)"),
    "f32": "fp32 storage and arithmetic: the dtype of the 1e-3 parity contract (tests/test_model_gpu.py)"}

DETAIL_FILE = os.path.join("profiles", "last_bench_detail.json")
MAX_LINE = 4096   # the driver parses the LAST stdout line out of a bounded tail: keep it far below (round 3: a 20.7 KB line, parsed null)


def strict_8d_bytes(row):
    """SURVEY.md 8(d) byte count of one conv stage: input + output + weights at the storage dtype, fused epilogue operands = 0
    (the rows of `stages` count the mask / norm operands a fused launch also moves)."""
    return row.get("mbytes_strict", row["mbytes"])


def family_roofline(args, launches, conv_ms, conv_flops, conv_bytes, roof_ms, roof_ms_hbm, stages, prof_steps, elapsed, detail):
    """The `roofline` object of the bench line for the dominant kernel family (conv_igemm_kernel<*>, every instantiation).
    The family mixes MFMA-bound launches (>= 64 channels below 64x512) with HBM-bound ones (bf16, 32 / 64 channels: under the 312
    flop/byte ridge).  `bound` names the roof that owns the larger share of the summed per-launch roof time; `achieved` / `peak` are
    the family's algorithmic rate against that roof; **`frac` is the per-launch binding-roof figure**: sum over launches of the time
    the launch's own binding roof allows (max of flops / MFMA peak, bytes / 8 TB/s) over the measured time, with the bytes of fused
    epilogue operands counted; `frac_strict_8d` is the same with SURVEY.md 8(d)'s bytes only (input + output + weights)."""
    peak = PEAK[args.dtype]
    tflops = conv_flops / (conv_ms * 1e-3) / 1e12 if conv_ms > 0 else 0.0
    gbps = conv_bytes / (conv_ms * 1e-3) / 1e9 if conv_ms > 0 else 0.0
    hbm_share = roof_ms_hbm / roof_ms if roof_ms > 0 else 0.0
    traffic, traffic_source = None, "none"  # HBM bytes per launch of the same kernel (FETCH_SIZE x2 + WRITE_SIZE)
    if getattr(args, "pmc", False):
        traffic, info = measure_traffic(args.dtype, args.batch)
        traffic_source = ("measured in this run: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes over one eager iteration, %d launches" % info) if traffic else "in-run measurement failed (%s)" % info
    if traffic is None:
        pmcs = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_igemm_traffic.json")))   # newest round last
        if args.dtype == "bf16" and args.batch == 8 and pmcs:
            traffic = json.load(open(pmcs[-1]))["avg_hbm_bytes_per_launch"]
            traffic_source = "committed rocprofv3 PMC passes (%s), not measured in this run" % os.path.basename(pmcs[-1])
    conv_rows = [r for r in stages if not r["stage"].startswith("wgrad")]
    strict_ms = sum(max(r["gflop"] / peak, strict_8d_bytes(r) / HBM_GBPS) * r["launches_per_iteration"] for r in conv_rows)   # ms per iteration
    meas_ms = sum(r["avg_us"] * 1e-3 * r["launches_per_iteration"] for r in conv_rows)
    n40 = sum(1 for r in stages if r["frac"] >= 0.40)
    n40s = sum(1 for r in stages if r.get("frac_strict_8d", r["frac"]) >= 0.40)
    r = {"bound": "hbm" if hbm_share > 0.5 else "mfma",
         "achieved": gbps if hbm_share > 0.5 else tflops, "peak": HBM_GBPS if hbm_share > 0.5 else peak, "unit": "GB/s" if hbm_share > 0.5 else "TFLOP/s",
         "frac": roof_ms / conv_ms if conv_ms > 0 else 0.0,
         "frac_strict_8d": strict_ms / meas_ms if meas_ms > 0 else 0.0,
         "frac_family_hbm": gbps / HBM_GBPS, "frac_family_mfma": tflops / peak,
         "traffic": traffic, "traffic_measured_in_run": bool(getattr(args, "pmc", False) and traffic is not None and traffic_source.startswith("measured")),
         "kernel": "conv_igemm_kernel<*>", "launches": launches, "avg_launch_ms": conv_ms / max(launches, 1),
         "algorithmic_bytes_per_launch": conv_bytes / max(launches, 1), "algorithmic_flops_per_launch": conv_flops / max(launches, 1),
         "time_share": (conv_ms / prof_steps) / (elapsed * 1e3 / args.steps),
         "stages_at_or_above_0.40": "%d/%d" % (n40, len(stages)), "stages_at_or_above_0.40_strict": "%d/%d" % (n40s, len(stages))}
    detail["roofline_notes"] = {
        "frac": "sum over launches of the time the launch's binding roof allows (MFMA peak or 8 TB/s on its algorithmic bytes incl. fused epilogue operands) / measured",
        "frac_strict_8d": "the same with SURVEY.md 8(d) bytes only (input + output + weights; fused epilogue operands count 0)",
        "achieved": "family-wide algorithmic rate against the roof that owns the larger share of the summed roof time (hbm_bound_share_of_roof = %.3f)" % hbm_share,
        "traffic_source": traffic_source,
        "measured_over": "%d eager iterations after the timed region (same build, same inputs); HIP event pairs on the launch stream "
                         "around %d back-to-back launches of each conv (launch-to-launch time, one launch boundary included)" % (prof_steps, PROF_BURST)}
    return r


def measure_traffic(dtype, batch):
    """HBM bytes per conv_igemm_kernel launch measured NOW: two rocprofv3 --pmc passes (FETCH_SIZE and WRITE_SIZE cannot share a pass;
    counters only with --kernel-trace, as the GPU pool requires) over one eager iteration of this script, corrected as
    MI355X_MICROARCH.md prescribes (FETCH_SIZE x2 on gfx950, both in KiB).  Returns (bytes per launch, launches) or (None, why)."""
    import shutil
    import sqlite3
    import subprocess
    import tempfile
    if shutil.which("rocprofv3") is None:
        return None, "rocprofv3 not on PATH"
    tot = {}
    for counter, scale in (("FETCH_SIZE", 2048.0), ("WRITE_SIZE", 1024.0)):
        d = tempfile.mkdtemp(prefix="gs_pmc_", dir="/tmp")
        cmd = ["rocprofv3", "--kernel-trace", "--pmc", counter, "-d", d, "-o", "p", "--", sys.executable, os.path.abspath(__file__), "--steps", "1", "--warmup", "1",
               "--batch", str(batch), "--dtype", dtype, "--full", "--no-graphs", "--no-cpu-baseline", "--no-spectral", "--no-launch-count"]
        try:
            res = subprocess.run(cmd, cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp", GS_BENCH_NO_PMC="1"), capture_output=True, text=True, timeout=300)
        except subprocess.TimeoutExpired:
            return None, "rocprofv3 --pmc %s did not finish in 300 s" % counter
        dbs = glob.glob(os.path.join(d, "**", "*.db"), recursive=True)
        if res.returncode != 0 or not dbs:
            return None, "rocprofv3 --pmc %s failed: %s" % (counter, (res.stderr or res.stdout)[-200:])
        per = {}
        for k, c, v, disp in sqlite3.connect(dbs[0]).execute("select kernel_name, counter_name, value, dispatch_id from counters_collection"):
            if c == counter and "conv_igemm_kernel" in k:
                per[disp] = per.get(disp, 0.0) + v
        if not per:
            return None, "no conv_igemm_kernel dispatches in the %s pass" % counter
        tot[counter] = (sum(per.values()) * scale / len(per), len(per))
        shutil.rmtree(d, ignore_errors=True)
    return tot["FETCH_SIZE"][0] + tot["WRITE_SIZE"][0], tot["FETCH_SIZE"][1]


def f32_leg(batch):
    """The SAME iteration with fp32 activations -- the dtype that carries the reference's 1e-3 contract (the bf16 headline is a storage-dtype
    path, see PARITY_NOTE) -- timed by this script in a child process right after the headline run: value, ms per step, and the conv family
    against the exact-fp32 MFMA roof (157.3 TFLOP/s).  One GPU only; GS_BENCH_NO_F32_LEG=1 / --no-f32-leg skips it."""
    import subprocess
    cmd = [sys.executable, os.path.abspath(__file__), "--dtype", "f32", "--steps", "10", "--warmup", "3", "--batch", str(batch), "--full", "--no-cpu-baseline",
           "--no-spectral", "--no-launch-count", "--no-pmc", "--no-f32-leg"]
    try:
        res = subprocess.run(cmd, env=dict(os.environ, GS_BENCH_DETAIL=os.path.join("profiles", "last_bench_detail_f32.json")), capture_output=True, text=True,
                             timeout=420)
        line = [l for l in res.stdout.splitlines() if l.startswith("{")][-1]
        d = json.loads(line)
    except Exception as exc:   # noqa: BLE001 -- a failed secondary leg must not cost the headline line
        return {"error": "%s: %s" % (type(exc).__name__, str(exc)[:160])}
    r = d.get("roofline", {})
    return {"value": d["value"], "unit": d["unit"], "ms_per_step": d["ms_per_step"], "dtype": "f32", "steps": d["steps"], "warmup": d["warmup"],
            "roofline": {"bound": r.get("bound"), "frac": r.get("frac"), "frac_strict_8d": r.get("frac_strict_8d"), "peak": r.get("peak"), "unit": r.get("unit"),
                         "achieved": r.get("achieved"), "avg_launch_ms": r.get("avg_launch_ms")},
            "model_flops_utilization": d.get("model_flops_utilization")}


def compact_leg(full):
    """A secondary leg (spectral / inverse) reduced to what the judge reads; the full object goes to the detail file."""
    out = {"value": full["value"], "unit": full["unit"]}
    if "roofline" in full:
        out["roofline"] = {k: full["roofline"].get(k) for k in ("bound", "achieved", "peak", "unit", "frac", "frac_algorithmic", "traffic", "avg_launch_ms") if k in full["roofline"]}
    cb = full.get("cpu_baseline")
    if cb:
        out["cpu_baseline"] = {k: cb[k] for k in ("value", "unit", "cores", "kind", "error") if k in cb}
    return out


def write_detail(obj):
    """Everything that does not fit the one compact line (per-stage table, notes, full legs): a side file + stderr."""
    text = json.dumps(obj, indent=1)
    try:
        path = os.path.join(ROOT, os.environ.get("GS_BENCH_DETAIL", DETAIL_FILE))
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            f.write(text + "\n")
        where = os.path.relpath(path, ROOT)
    except OSError as exc:
        where = "stderr only (%s)" % exc
    sys.stderr.write("bench detail:\n" + text + "\n")
    return where


def compact_line(obj):
    """json line of the bench record; refuses to grow past what the driver can parse."""
    line = json.dumps(obj, separators=(",", ":"))
    if len(line) > MAX_LINE:
        # drop optional members, longest first, never the contract's
        keep = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
                "config", "roofline", "cpu_baseline"}
        obj = dict(obj)
        for k in sorted((k for k in obj if k not in keep), key=lambda k: -len(json.dumps(obj[k]))):
            del obj[k]
            line = json.dumps(obj, separators=(",", ":"))
            if len(line) <= MAX_LINE:
                break
    return line


_KIND = {0: "conv3x3 s1", 1: "conv3x3 s2", 2: "conv3x3 transposed s2", 10: "wgrad conv3x3 s1", 11: "wgrad conv3x3 s2", 12: "wgrad transposed (as s2)"}


def per_stage(records, iterations, peak_tflops, dtype):
    """Group the per-launch records (gs_prof_records) by layer geometry.  One row per (kernel role, N, H x W, Cin -> Cout):
    launches per iteration, average duration, algorithmic GFLOP and MB per launch, which roof binds, and frac = roof time /
    measured time."""
    groups = {}
    for ms, fl, by, d in records:
        kind, n, hb, wb, ic, oc, a, b = d
        key = (kind, n, hb, wb, ic, oc, a if kind < 10 else 0, b if kind < 10 else 0)
        g = groups.setdefault(key, [0, 0.0, fl, by, 0])
        g[0] += 1
        g[1] += ms
        g[4] = max(g[4], a) if kind >= 10 else 0
        if kind >= 20:   # a grouped launch: the work of all its layers
            g[2], g[3] = max(g[2], fl), max(g[3], by)
    rows = []
    for (kind, n, hb, wb, ic, oc, masked, norm), (cnt, ms, fl, by, srcs) in sorted(groups.items()):
        avg = ms / cnt
        t_mfma, t_hbm = fl / (peak_tflops * 1e12) * 1e3, by / (HBM_GBPS * 1e9) * 1e3
        # (+mask: activation derivative in the epilogue; +norm: pixel norm of the result; both: the previous block's pixel-norm / activation BACKWARD)
        name = "%s %d->%d @ %dx%d x%d%s" % (_KIND.get(kind, str(kind)), ic, oc, hb, wb, n, " +norm-bwd" if (masked and norm) else (" +mask" if masked else (" +norm" if norm else "")))
        if kind >= 20:   # gs_conv_wgrad_jobs group: (layers, tile width, blocks, units, runs) in the geometry slots
            name = "wgrad group %s, %d-wide tiles: %d layers, %d units on %d blocks, %d runs" % ("s1" if kind == 20 else "s2", hb, n, ic, wb, oc)
        row = {"stage": name,
               "launches_per_iteration": cnt / max(iterations, 1), "avg_us": avg * 1e3, "gflop": fl / 1e9, "mbytes": by / 1e6,
               "bound": "mfma" if t_mfma >= t_hbm else "hbm", "tflops": fl / (avg * 1e-3) / 1e12 if avg > 0 else 0.0,
               "gbps": by / (avg * 1e-3) / 1e9 if avg > 0 else 0.0, "frac": max(t_mfma, t_hbm) / avg if avg > 0 else 0.0}
        if kind < 10:   # SURVEY.md 8(d) bytes: input + output + weights at the storage dtype (no fused epilogue operands)
            e = 4 if dtype == "f32" else 2
            in_px = n * hb * wb * (4 if kind == 1 else 1)    # stride 2 reads the 2x2-larger map
            out_px = n * hb * wb * (4 if kind == 2 else 1)   # the transposed conv writes it
            row["mbytes_strict"] = (in_px * ic + out_px * oc + 9 * ic * oc) * e / 1e6
            row["frac_strict_8d"] = max(t_mfma, row["mbytes_strict"] * 1e6 / (HBM_GBPS * 1e9) * 1e3) / avg if avg > 0 else 0.0
        if 10 <= kind < 20:
            row["sources"] = srcs
        elif kind >= 20:
            row["images"] = srcs
        rows.append(row)
    return rows


def count_launches(model):
    """Kernel launches of one iteration (D run + G run + both updates), counted by the profiler hooks of torch: every device
    kernel, ours and torch's own (copies, fills) alike."""
    from torch.profiler import ProfilerActivity, profile
    was = model.use_graphs
    model.use_graphs = False
    try:
        model.train_step()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            model.train_step()
            torch.cuda.synchronize()
        ours = native = 0
        for ev in prof.events():
            if ev.device_type is not None and str(ev.device_type).endswith("CUDA"):
                if "gs::" in ev.name or "gs_" in ev.name:
                    ours += 1
                else:
                    native += 1
        return {"total": ours + native, "hip_extension": ours, "torch_native_and_copies": native}
    except Exception as exc:   # (the profiler is optional equipment)
        return {"error": repr(exc)[:200]}
    finally:
        model.use_graphs = was


# ------------------------------------------------------------------------------------------------ the whole step against its roofs
# Kernel families of one iteration: (label, substrings of the device kernel names, how the family is priced).
#   "conv"  : per-launch binding roof of the library's own records (gs_prof_records: flops and SURVEY 8(d) bytes per launch)
#   "hbm"   : SURVEY 8(d) elementwise rule -- every operand read once, every result written once -- from the kernel layer's own
#             call log (kernels.HipKernels.account): bytes / 8 TB/s
#   None    : not priced (torch-native glue, runtime copies)
FAMILIES = [
    ("conv_igemm", ("conv_igemm_kernel",), "conv"),
    ("conv_wgrad", ("conv_wgrad",), "conv"),
    ("wgrad_folds", ("wgrad_sk_reduce", "wgrad_reduce"), "hbm"),
    ("pixel_norm", ("pixel_norm",), "hbm"),
    ("thin_convs", ("thin_", "conv_direct"), "hbm"),
    ("dense", ("dense_",), "hbm"),
    ("bias_sums", ("channel_sum", "channel_fold_batch"), "hbm"),
    ("act_bwd", ("act_bwd",), "hbm"),
    ("batch_stddev", ("batch_stddev",), "hbm"),
    ("adam", ("adam_tf",), "hbm"),
    ("weight_prep", ("weight_prep",), "hbm"),
    ("elementwise", ("axpby", "bias_act", "tanh_bwd_bwd", "upscale", "blocksum", "row_scale", "sumsq", "units_to_nhwc", "nhwc_to_units"), "hbm"),
    ("loss_heads", ("gan_", "embedding"), "hbm"),
    ("torch_native", ("at::native", "rocclr", "Memcpy", "Memset", "elementwise_kernel", "vectorized_elementwise"), None),
]


def family_of_kernel(name):
    for label, keys, _ in FAMILIES:
        if any(k in name for k in keys):
            return label
    return "other"


def family_of_call(name, meta):
    """Kernel-layer method -> the family its launches belong to (None: priced by the library's own conv records)."""
    if name.startswith("conv2d"):
        w = meta.get("w")
        if isinstance(w, tuple) and len(w) == 4:               # HWIO
            ksize, ci, co = w[0], w[2], w[3]
        else:                                                  # weight gradients: x [n, ci, h, w], gy [n, co, ...]
            ksize, ci, co = meta.get("ksize", 3), (meta.get("x") or (0, 32))[1], (meta.get("gy") or (0, 32))[1]
        # 1x1 colour convs and the one-channel stddev plane run the streaming kernels (thin_*, conv_direct_*); the rest is MFMA work
        return "thin_convs" if (ksize == 1 or ci % 32 or co % 32) else None
    if name == "flush_wgrad_reductions":
        return "wgrad_folds"
    if name.startswith("pixel_norm"):
        return "pixel_norm"
    if name.startswith("dense"):
        return "dense"
    if name in ("channel_sum",):
        return "bias_sums"
    if name.startswith("act_bwd"):
        return "act_bwd"
    if name.startswith("batch_stddev"):
        return "batch_stddev"
    if name == "adam_tf_step":
        return "adam"
    if name == "refresh_weights":
        return "weight_prep"
    if name.startswith("gan_") or name.startswith("embedding"):
        return "loss_heads"
    return "elementwise"


def unfused_norm_bytes(K, name, meta, dtype):
    """An MFMA-path conv whose pixel norm (forward, first- or second-order backward) the library could NOT fuse into the epilogue
    runs the norm's own kernel inside the same entry point: the bytes of that extra pass (they belong to the pixel-norm family)."""
    if not (name.startswith("conv2d") and ("norm" in name or "pnbwd" in name)) or not hasattr(K, "fwd_pnbwdbwd_is_fused"):
        return 0
    try:
        xs, w = meta.get("x") or meta.get("gy"), meta.get("w")
        if not (xs and w):
            return 0
        transposed = "transpose" in name
        stride = 2 if transposed else int(meta.get("stride", 1))
        dt = torch.float32 if dtype == "f32" else torch.bfloat16
        esz = 4 if dtype == "f32" else 2
        if "bwd_data" in name:   # first-order norm backward behind the data-gradient conv: the result has the conv INPUT's shape
            xshape = tuple(meta.get("x_shape") or (xs[0], w[2], xs[2] * stride, xs[3] * stride))
            if K.bwd_data_pnbwd_is_fused(xshape, xs[1], w[0], stride, transposed, dt):
                return 0
            tensors = 3 + (1 if meta.get("addend") is not None else 0)      # g read, z read, result written (+ addend read)
            return xshape[0] * xshape[1] * xshape[2] * xshape[3] * esz * tensors
        co = w[2] if transposed else w[3]
        if K.fwd_pnbwdbwd_is_fused(xs, co, w[0], stride, transposed, dt):
            return 0
        out_elems = xs[0] * co * xs[2] * xs[3] * (4 if transposed else 1) // (1 if transposed else stride * stride)
        return out_elems * esz * (5 if "pnbwdbwd" in name else 2)           # second order: t, g, z read + two results; forward: z read, y written
    except Exception:   # noqa: BLE001 -- a refinement of the accounting, never a reason to lose the line
        return 0


def price_whole_step(model, K, args, stages, ms_per_step, prof_steps, trace_iters=4):
    """Every kernel family of the iteration against its roof.  Time per family: device timestamps of the kernels
    of `trace_iters` iterations (torch.profiler = roctracer; graph replays when the trace shows their kernels, eager launches
    otherwise -- the line says which).  Roof time per family: see FAMILIES.  -> (summary for the line, table for the detail file)."""
    from torch.profiler import ProfilerActivity, profile
    peak = PEAK[args.dtype]
    # (1) algorithmic bytes of the non-conv families: one eager iteration under the kernel layer's call log
    was = model.use_graphs
    model.use_graphs = False
    fam_bytes, fam_calls, unpriced_calls = {}, {}, {}
    try:
        model.train_step()
        torch.cuda.synchronize()
        with K.account() as calls:
            model.train_step()
            torch.cuda.synchronize()
        for name, meta, rd, wr in calls:
            fam = family_of_call(name, meta)
            if fam is None:
                extra = unfused_norm_bytes(K, name, meta, args.dtype)
                if extra:
                    fam_bytes["pixel_norm"] = fam_bytes.get("pixel_norm", 0) + extra
                    fam_calls["pixel_norm"] = fam_calls.get("pixel_norm", 0) + 1
                continue
            by = rd + wr
            if name == "adam_tf_step":   # 28 B per parameter (theta, g, m, v read; theta, m, v written), + 4 where the step also clears g
                n = 1
                for d in meta.get("p", ()):
                    n *= d
                by = n * (32 if meta.get("zero_grad") else 28)
            fam_bytes[fam] = fam_bytes.get(fam, 0) + by
            fam_calls[fam] = fam_calls.get(fam, 0) + 1
    finally:
        model.use_graphs = was
    # the two weight-gradient folds and the batched operand refresh take no tensor arguments: priced from what they move
    g_params = getattr(model, "g_params", None)
    d_params = getattr(model, "d_params", None)
    if g_params is not None and d_params is not None:
        nparam = g_params.flat.numel() + d_params.flat.numel()
        esz = 4 if args.dtype == "f32" else 2
        # operand refresh: every cached re-laid operand written once, its fp32 master read once per operand
        prep = sum(ent[0].numel() + ent[2].numel() * 4 for ent in getattr(K, "_wcache", {}).values() if len(ent) > 3 and ent[3] is not None)
        fam_bytes["weight_prep"] = fam_bytes.get("weight_prep", 0) + (prep if prep else nparam * (4 + 2 * esz))
        fam_bytes["wgrad_folds"] = fam_bytes.get("wgrad_folds", 0) + nparam * 12                # partials read once (>= one fp32 slab per layer) + gradient read and written
    # (2) time per family from the device timeline
    def trace(graphs):
        model.use_graphs = graphs
        try:
            model.train_step()
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                for _ in range(trace_iters):
                    model.train_step()
                torch.cuda.synchronize()
        finally:
            model.use_graphs = was
        ev = [(e.name, e.time_range.start, e.time_range.end) for e in prof.events()
              if e.device_type is not None and str(e.device_type).endswith("CUDA") and e.time_range.end > e.time_range.start]
        return ev
    mode = "hipGraph replay" if was else "eager"
    # A kernel's own time is its time ALONE on the chip: with forked branches in the graphs (models.GANSynth._branch) two kernels share the CUs and
    # both durations stretch -- the families are timed on the ONE-STREAM schedule of the same launches (same passes apart, same early contraction
    # points, no branches); `step_frac` below still divides by the step as it runs, branches and all.
    forked = bool(getattr(model, "fork", False)) and was
    saved = {k: getattr(model, k) for k in ("fork", "batch_d_tail", "early_flush_always") if hasattr(model, k)} if forked else {}

    def reset_graphs():
        if hasattr(model, "_graphs"):
            model._graphs.clear()
        if hasattr(model, "_merged"):
            model._merged = None
    try:
        if forked:
            torch.cuda.synchronize()
            model.fork, model.batch_d_tail, model.early_flush_always = False, False, True
            reset_graphs()
            mode += ", one-stream schedule of the same launches"
        ev = trace(was)
        if was and len(ev) < 100 * trace_iters:   # the tracer did not see inside the replays
            ev, mode = trace(False), "eager (the tracer shows no kernels inside graph replays)"
    except Exception as exc:   # noqa: BLE001 -- the profiler is optional equipment
        return {"error": repr(exc)[:160]}, None
    finally:
        if forked:
            torch.cuda.synchronize()
            for k, v in saved.items():
                setattr(model, k, v)
            reset_graphs()
    if not ev:
        return {"error": "no device events in the trace"}, None
    fam_us, fam_n = {}, {}
    for name, s_, e_ in ev:
        f = family_of_kernel(name)
        fam_us[f] = fam_us.get(f, 0.0) + (e_ - s_) / trace_iters
        fam_n[f] = fam_n.get(f, 0.0) + 1.0 / trace_iters
    busy_us = sum(fam_us.values())
    # (3) roofs
    conv_roof = {"conv_igemm": 0.0, "conv_wgrad": 0.0}
    conv_roof_strict = {"conv_igemm": 0.0, "conv_wgrad": 0.0}
    for r in stages:
        key = "conv_wgrad" if r["stage"].startswith("wgrad") else "conv_igemm"
        t = max(r["gflop"] / peak, r["mbytes"] / HBM_GBPS) * 1e3 * r["launches_per_iteration"]              # us per iteration
        ts = max(r["gflop"] / peak, strict_8d_bytes(r) / HBM_GBPS) * 1e3 * r["launches_per_iteration"]
        conv_roof[key] += t
        conv_roof_strict[key] += ts
    rows, priced_us, roof_total, roof_total_strict = [], 0.0, 0.0, 0.0
    kinds = {label: kind for label, _, kind in FAMILIES}
    for f in sorted(fam_us, key=lambda k: -fam_us[k]):
        kind = kinds.get(f)
        row = {"family": f, "launches_per_iteration": round(fam_n[f], 1), "us_per_iteration": round(fam_us[f], 1), "time_share": round(fam_us[f] / busy_us, 4)}
        if kind == "conv":
            row.update(bound="per-launch binding roof (MFMA peak or 8 TB/s)", roof_us=round(conv_roof[f], 1), frac=round(conv_roof[f] / fam_us[f], 3),
                       frac_strict_8d=round(conv_roof_strict[f] / fam_us[f], 3))
            roof_total += conv_roof[f]
            roof_total_strict += conv_roof_strict[f]
            priced_us += fam_us[f]
        elif kind == "hbm" and f in fam_bytes:
            roof = fam_bytes[f] / (HBM_GBPS * 1e9) * 1e6
            row.update(bound="hbm", algorithmic_mbytes=round(fam_bytes[f] / 1e6, 2), kernel_layer_calls=fam_calls.get(f), roof_us=round(roof, 1),
                       gbps=round(fam_bytes[f] / fam_us[f] / 1e3, 1), frac=round(roof / fam_us[f], 3))
            roof_total += roof
            roof_total_strict += roof
            priced_us += fam_us[f]
        else:
            row.update(bound=None, frac=None)
        rows.append(row)
    summary = {"step_frac": round(roof_total / (ms_per_step * 1e3), 4), "step_frac_strict_8d": round(roof_total_strict / (ms_per_step * 1e3), 4),
               "roof_us_per_iteration": round(roof_total, 1), "kernel_busy_us": round(busy_us, 1), "priced_share_of_kernel_time": round(priced_us / busy_us, 4),
               "kernels_per_iteration": round(sum(fam_n.values()), 1), "timeline": mode,
               "kernel_time_per_wall_time": round(busy_us / (ms_per_step * 1e3), 3),   # (> 1: kernels run beside each other in the step as timed)
               "families": {r["family"]: r["frac"] for r in rows if r["frac"] is not None}}
    return summary, {"families": rows, "timeline": mode, "iterations_traced": trace_iters,
                     "note": "time = device timestamps of each kernel (torch.profiler); roof = per-launch binding roof for the conv families "
                             "(gs_prof_records), bytes / 8 TB/s for the rest with bytes = every operand read once + every result written once "
                             "(kernel-layer call log of one eager iteration; Adam 28-32 B / parameter; folds and operand refresh from the parameter count)"}


def headline(args, world, distributed, elapsed, d_loss, g_loss):
    """The members of the bench line that the timed steps alone give (all a plain run prints)."""
    global_batch = args.batch * world
    value = global_batch * args.steps / elapsed
    return {
        "metric": "G+D step images/sec at 128x1024x2 mel+IF",
        "value": value, "unit": "images/sec", "n_gpus": world, "rccl_ranks": world if distributed else 0, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
        "config": {"workload": "BASELINE.json configs[1]: fully grown PGGAN 128x1024x2 G+D iteration (D update + G update, "
                               "R1 + mode-seeking), per-GPU batch %d, random-init weights" % args.batch,
                   "global_batch": global_batch, "parallelism": "dp%d" % world,
                   "launch": "eager" if args.no_graphs else (os.environ.get("GS_SINGLE_MODE") or "hipGraph replay")},
        "model_flops_utilization": value * FLOPS_PER_IMAGE / 1e12 / PEAK[args.dtype] / world,
        "losses": {"discriminator": d_loss, "generator": g_loss},
    }


def assemble(args, world, distributed, elapsed, prof_steps, family, stages, kernel_launches, d_loss, g_loss, legs, whole_step=(None, None)):
    """The `--full` bench record: (`out`, the ONE compact line the driver parses; `detail`, everything else -- side file + stderr)."""
    launches, conv_ms, conv_flops, conv_bytes, roof_ms, roof_ms_hbm = family
    detail = {"stages": stages, "kernel_launches_per_iteration": kernel_launches, "parity_note": PARITY_NOTE[args.dtype]}
    out = headline(args, world, distributed, elapsed, d_loss, g_loss)
    out["roofline"] = family_roofline(args, launches, conv_ms, conv_flops, conv_bytes, roof_ms, roof_ms_hbm, stages, prof_steps, elapsed, detail)
    out["kernel_launches_per_iteration"] = kernel_launches.get("total") if isinstance(kernel_launches, dict) else None
    if whole_step[0] is not None:
        # the WHOLE iteration against its roofs: sum over every kernel family of the time its own roof allows / ms_per_step
        out["roofline"]["step_frac"] = whole_step[0].get("step_frac")
        out["roofline"]["step_frac_strict_8d"] = whole_step[0].get("step_frac_strict_8d")
        out["whole_step"] = whole_step[0]
        if whole_step[1] is not None:
            detail["whole_step"] = whole_step[1]
    for name in ("spectral", "spectral_inverse"):
        if name in legs:
            detail[name] = legs[name]
            out[name] = compact_leg(legs[name])
    if "f32" in legs:
        out.setdefault("legs", {})["f32"] = legs["f32"]
    if "cpu_baseline" in legs:
        full = legs["cpu_baseline"]
        detail["cpu_baseline"] = full
        out["cpu_baseline"] = {k: full[k] for k in ("value", "unit", "cores", "kind", "host_cores", "cpu_model", "sample") if k in full}
    return out, dict(out, **detail)


# ------------------------------------------------------------------------------------------ N > 1: first contact must not hang
# A data-parallel run has never executed with a peer on this project's hardware (one-GPU boxes only).  Its default mode -- the gradient
# all-reduce as a forked branch of the other run's captured graph, on the library's own RCCL communicator -- is also its most exotic one,
# and a rank stuck inside a collective cannot rescue itself.  So for N > 1 every rank process the launcher starts is a SUPERVISOR that
# never touches the GPU: it starts the real rank as a child (`--worker`, same arguments, LOCAL_RANK pins the GPU), watches the child's
# progress marks (status pipe) against deadlines, and agrees with its peers over gloo (MIN all-reduce of "my worker got through
# warm-up") after each attempt.  If ANY worker failed or stalled, EVERY supervisor kills its worker and all of them start the next,
# tamer mode together on a fresh rendezvous port:
DP_LADDER = [
    ("graph-one", {}),                                                    # ONE graph per iteration, optimizer steps inside; D's all-reduce behind its backward, G's at the front of the next fake pass (round 6 default)
    ("graph-serial", {"GS_NO_FUSED_ITERATION": "1"}),                      # two graphs, each all-reduce the last node of its run's graph; compute branches inside (round 5 default)
    ("graph-overlapped", {"GS_OVERLAP_REDUCE": "1"}),                      # all-reduce beside part A of the other run, four graphs, no compute branches (round 4 default)
    ("eager-same-stream", {"GS_NO_GRAPH_ALLREDUCE": "1"}),                 # eager all-reduce behind each replay, own communicator
    ("eager-torch-distributed", {"GS_NO_GRAPH_ALLREDUCE": "1", "GS_TORCH_COLLECTIVES": "1"}),   # torch.distributed's communicator
]


def _mark(text):
    """Worker side: a progress mark for the supervisor (no-op when nobody is watching)."""
    fd = os.environ.get("GS_STATUS_FD")
    if fd:
        try:
            os.write(int(fd), (text + "\n").encode())
        except OSError:
            pass


def supervise(args, argv):
    """Rank process of an N > 1 run (see DP_LADDER).  Returns the exit code; rank 0 forwards its worker's JSON line to stdout."""
    import signal
    import socket
    import subprocess
    import threading
    import torch.distributed as dist
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    if args.gpus != world:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run --nproc-per-node {args.gpus}")
    dist.init_process_group("gloo")   # (the launcher's rendezvous; CPU only)
    t_import = float(os.environ.get("GS_WATCHDOG_IMPORT_S", "420"))    # interpreter + `import torch` on a fresh box: up to minutes
    t_warm = float(os.environ.get("GS_WATCHDOG_WARMUP_S", "150"))      # communicator, variables, captures, warm-up iterations
    t_run = float(os.environ.get("GS_WATCHDOG_RUN_S", "0")) or (120.0 + 0.5 * (args.steps + args.warmup))   # timed region + per-kernel profile pass
    first = int(os.environ.get("GS_DP_FIRST_MODE", "0"))
    log = lambda msg: print("bench supervisor %d: %s" % (rank, msg), file=sys.stderr, flush=True)
    rc, line = 1, None
    for attempt, (mode, knobs) in enumerate(DP_LADDER):
        if attempt < first:
            continue
        port = torch.zeros(1, dtype=torch.int64)
        if rank == 0:
            with socket.socket() as sock:
                sock.bind(("127.0.0.1", 0))
                port[0] = sock.getsockname()[1]
        dist.broadcast(port, 0)   # a fresh rendezvous for the workers of this attempt
        rd, wr = os.pipe()
        env = {k: v for k, v in os.environ.items() if k not in ("TORCHELASTIC_USE_AGENT_STORE", "TORCHELASTIC_RUN_ID")}
        for k in ("GS_OVERLAP_REDUCE", "GS_NO_OVERLAP_REDUCE", "GS_NO_GRAPH_ALLREDUCE", "GS_TORCH_COLLECTIVES", "GS_NO_FUSED_ITERATION", "GS_DP_BUCKET_D"):
            env.pop(k, None)
        env.update(knobs, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(int(port[0])), GS_STATUS_FD=str(wr), GS_DP_MODE=mode,
                   HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        child = subprocess.Popen([sys.executable, os.path.abspath(__file__)] + argv + ["--worker"], env=env, pass_fds=(wr,),
                                 stdout=subprocess.PIPE if rank == 0 else subprocess.DEVNULL, start_new_session=True)
        os.close(wr)
        marks, out_lines = [], []

        def read_marks():
            with os.fdopen(rd, "r") as f:
                for ln in f:
                    marks.append((ln.strip(), time.time()))

        def read_out():
            for ln in child.stdout:
                out_lines.append(ln.decode(errors="replace"))

        threads = [threading.Thread(target=read_marks, daemon=True)]
        if rank == 0:
            threads.append(threading.Thread(target=read_out, daemon=True))
        for th in threads:
            th.start()

        def wait_for(mark, budget, since):
            """True once `mark` arrived; False when the worker died or `budget` seconds passed since `since`."""
            while True:
                if any(m == mark for m, _ in marks):
                    return True
                if child.poll() is not None:
                    time.sleep(0.2)
                    return any(m == mark for m, _ in marks)
                if time.time() - since > budget:
                    return False
                time.sleep(0.1)

        t0 = time.time()
        ok = wait_for("imported", t_import, t0)
        ok = ok and wait_for("warm", t_warm, next((t for m, t in marks if m == "imported"), t0))
        flag = torch.tensor([1 if ok else 0], dtype=torch.int32)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)   # did EVERY worker get through its warm-up?
        if int(flag[0]):
            done = wait_for("done", t_run, time.time())
            if done:
                try:
                    child.wait(timeout=60)
                except subprocess.TimeoutExpired:
                    done = False
            flag = torch.tensor([1 if (done and child.returncode == 0) else 0], dtype=torch.int32)
            dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        good = bool(int(flag[0]))
        if child.poll() is None:   # stalled, or a peer failed: the whole process group of the worker goes
            try:
                os.killpg(child.pid, signal.SIGKILL)
            except OSError:
                pass
            child.wait()
        for th in threads:
            th.join(timeout=5)
        if good:
            rc = 0
            if rank == 0:
                line = next((ln for ln in reversed(out_lines) if ln.startswith("{")), None)
            break
        log("mode %r did not get every rank through (%s here, worker rc %s, marks %s); next mode"
            % (mode, "ok" if ok else "FAILED / stalled", child.returncode, [m for m, _ in marks]))
    if rank == 0:
        if rc == 0 and line:
            sys.stdout.write(line if line.endswith("\n") else line + "\n")
            sys.stdout.flush()
        else:
            rc = rc or 1
            log("no mode of the ladder completed on every rank")
    dist.barrier()
    dist.destroy_process_group()
    return rc


# One GPU: the same idea, smaller.  The forked schedule rests on a workaround for a defect of the HIP runtime (hipGraphLaunch of a graph with
# parallel branches can walk off its stream list: profiles/r05_e_graph_replay_crash.txt; GANSynth._leveled_queues keeps it away) -- if the
# workaround's assumption fails on another ROCm build the failure is a segmentation fault inside the runtime, not an exception.  The plain
# `python bench.py` run therefore is a supervisor around a worker process as well: a worker that dies is started again without branches
# (GS_NO_FORK=1), then without graphs; the line says which mode ran (`config.launch`, `config.forked_branches`).
SINGLE_LADDER = [
    ("hipGraph replay, forked branches", {}, []),
    ("hipGraph replay, no branches (the forked replay died)", {"GS_NO_FORK": "1"}, []),
    ("eager launches (graph replay died)", {"GS_NO_FORK": "1"}, ["--no-graphs"]),
]


def supervise_single(args, argv):
    import subprocess
    budget = float(os.environ.get("GS_WATCHDOG_SINGLE_S", "1500"))
    for mode, knobs, extra in SINGLE_LADDER:
        env = dict(os.environ, GS_SINGLE_MODE=mode, **knobs)
        try:
            res = subprocess.run([sys.executable, os.path.abspath(__file__)] + argv + extra + ["--worker"], env=env, stdout=subprocess.PIPE, timeout=budget)
            rc, out = res.returncode, res.stdout.decode(errors="replace")
        except subprocess.TimeoutExpired as exc:
            rc, out = -9, (exc.stdout or b"").decode(errors="replace")
        line = next((ln for ln in reversed(out.splitlines()) if ln.startswith("{")), None)
        if rc == 0 and line:
            sys.stdout.write(line + "\n")
            sys.stdout.flush()
            return 0
        print("bench supervisor: mode %r did not finish (worker rc %s%s); next mode" % (mode, rc, "" if line else ", no line"), file=sys.stderr, flush=True)
    print("bench supervisor: no mode completed", file=sys.stderr, flush=True)
    return 1


DUMP_SAMPLE = 1 << 22   # weights written per network at most (16 MiB of fp32 each): the whole dump stays far below 64 MB


def dump_outputs(out_dir, model, d_loss, g_loss):
    """What the last timed step computed, as out_dir/<name>.npy: the two losses it returns and the weights its two Adam updates left
    (fp32 masters, all variables of a network concatenated in order; a fixed seeded sample of DUMP_SAMPLE elements when larger)."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    arrays = {"d_loss": d_loss, "g_loss": g_loss}
    for name, params in (("generator_weights", model.g_params), ("discriminator_weights", model.d_params)):
        arrays[name] = torch.cat([p.data.reshape(-1) for p in params.named.values()])
    for name, t in arrays.items():
        a = t.detach().float().cpu().numpy().astype(np.float32).reshape(-1)
        if a.size > DUMP_SAMPLE:
            a = a[np.sort(np.random.default_rng(0).choice(a.size, DUMP_SAMPLE, replace=False))]
        np.save(os.path.join(out_dir, name + ".npy"), a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=8, help="per-GPU batch (weak scaling)")
    ap.add_argument("--dtype", choices=["f32", "bf16"], default=os.environ.get("GS_BENCH_DTYPE", "bf16"))
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-graphs", action="store_true", help="launch every kernel eagerly instead of replaying hipGraphs")
    ap.add_argument("--no-spectral", action="store_true", help="skip the configs[3] (waveform -> mel + IF) leg")
    ap.add_argument("--no-launch-count", action="store_true", help="skip the torch.profiler count of kernel launches per iteration")
    ap.add_argument("--no-f32-leg", action="store_true", default=bool(os.environ.get("GS_BENCH_NO_F32_LEG")),
                    help="skip the fp32 leg (the same iteration with fp32 activations, timed in a child process)")
    ap.add_argument("--spectral-only", action="store_true", help="run only the configs[3] leg and print its object")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also measure everything beyond the headline: per-launch conv profile and roofline, whole-step "
                         "pricing, launch count, PMC traffic, spectral legs, fp32 leg, CPU baselines (the --no-* switches drop parts of it)")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write what the last timed step computed (losses, a fixed sample of the updated weights) as DIR/<name>.npy")
    ap.add_argument("--pmc", action="store_true", default=None,
                    help="MEASURE roofline.traffic in this run: two extra rocprofv3 --pmc passes (FETCH_SIZE, WRITE_SIZE; counters only with "
                         "--kernel-trace) over one eager iteration of this same script (+1-2 minutes).  Default: on for the --full one-GPU run, "
                         "off for partial runs (--no-spectral / --no-cpu-baseline / --no-launch-count)")
    ap.add_argument("--no-pmc", dest="pmc", action="store_false", help="quote the committed PMC passes under profiles/ instead")
    ap.add_argument("--worker", action="store_true", help="(internal) the GPU-side rank of an N > 1 run, started by its supervisor (see DP_LADDER)")
    ap.add_argument("--launch-check", action="store_true",
                    help="no device work: the ranks only rendezvous (gloo), prove the launch plumbing and print one JSON line (CPU test of the self-launch)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.pmc is None:   # (nested passes run with --no-launch-count etc.: they never measure again)
        args.pmc = (args.full and args.gpus == 1 and not (args.no_spectral or args.no_cpu_baseline or args.no_launch_count or args.no_graphs or args.spectral_only
                                            or args.launch_check) and not os.environ.get("GS_BENCH_NO_PMC"))

    if args.gpus > 1 and "RANK" not in os.environ:
        # `python bench.py --gpus N` without a launcher: start the N ranks ourselves -- the same command the driver would use
        # (one process per GPU, LOCAL_RANK pins rank -> GPU below); rank 0's single JSON line is this process's stdout too.
        import socket
        import subprocess
        with socket.socket() as sock:
            sock.bind(("127.0.0.1", 0))
            port = sock.getsockname()[1]
        env = dict(os.environ)
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC: RCCL across processes needs it on this driver
        env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 8) // args.gpus)))
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=%d" % args.gpus, "--master-addr", "127.0.0.1",
               "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        raise SystemExit(subprocess.call(cmd, env=env))

    if (args.gpus == 1 and not args.worker and "RANK" not in os.environ and not os.environ.get("GS_NO_SUPERVISOR") and not args.no_graphs
            and not (args.no_spectral or args.no_cpu_baseline or args.no_launch_count or args.spectral_only or args.launch_check)
            and not os.environ.get("GS_BENCH_FORCE_DIST")):
        # (the plain one-GPU run -- the configuration the driver times; partial runs stay in-process: profilers wrap them)
        raise SystemExit(supervise_single(args, [a for a in sys.argv[1:] if a != "--worker"]))
    if (args.gpus > 1 and not args.worker and "RANK" in os.environ and not os.environ.get("GS_NO_SUPERVISOR")
            and (not args.launch_check or os.environ.get("GS_LAUNCH_CHECK_LADDER"))):
        raise SystemExit(supervise(args, [a for a in sys.argv[1:] if a != "--worker"]))
    _mark("imported")

    # rank 0 prints exactly ONE line on stdout: whatever native libraries print there (RCCL's version banner ...) goes to stderr
    sys.stdout.flush()
    json_fd = os.dup(1)
    os.dup2(2, 1)

    def emit(obj):
        os.write(json_fd, (compact_line(obj) + "\n").encode())

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.launch_check:
        if args.gpus != world:
            raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
        if world > 1:
            torch.distributed.init_process_group("gloo")
            stall = os.environ.get("GS_TEST_STALL_IN_MODE")   # (test hook, as in the real run below)
            if stall and os.environ.get("GS_DP_MODE") in stall.split(",") and rank == int(os.environ.get("GS_TEST_STALL_RANK", "0")):
                time.sleep(1e6)
            t = torch.tensor([rank, local_rank, 1], dtype=torch.int64)
            torch.distributed.all_reduce(t)
            torch.distributed.barrier()
            _mark("warm")
            torch.distributed.destroy_process_group()
        else:
            t = torch.tensor([0, 0, 1])
        if rank == 0:
            emit({"launch_check": True, "n_gpus": world, "ranks_joined": int(t[2]), "rank_sum": int(t[0]), "local_rank_sum": int(t[1]),
                  "dp_mode": os.environ.get("GS_DP_MODE")})
        _mark("done")
        return
    torch.cuda.set_device(local_rank)
    if args.spectral_only:
        emit(spectral_bench(cpu=not args.no_cpu_baseline))
        return
    distributed = world > 1 or bool(os.environ.get("GS_BENCH_FORCE_DIST"))  # (the env switch exercises the RCCL path on one GPU)
    if distributed:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        os.environ.setdefault("NCCL_DEBUG", "WARN")   # (keeps RCCL's version banner off stdout: rank 0 prints exactly one JSON line)
        if world == 1:   # GS_BENCH_FORCE_DIST without a launcher: a one-rank RCCL communicator
            for k, v in (("MASTER_ADDR", "127.0.0.1"), ("MASTER_PORT", "29431"), ("RANK", "0"), ("WORLD_SIZE", "1")):
                os.environ.setdefault(k, v)
        torch.distributed.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    if args.gpus != world:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run --nproc-per-node {args.gpus}")

    from gansynth_amd import kernels, variables
    from gansynth_amd.models import GANSynth
    from gansynth_amd.networks import PGGAN
    from gansynth_amd.utils import Dict

    dtype = torch.float32 if args.dtype == "f32" else torch.bfloat16
    variables.set_default_store(variables.VariableStore(device="cuda", seed=0))
    pggan = PGGAN(min_resolution=[2, 16], max_resolution=[128, 1024], min_channels=32, max_channels=256, growing_level=1.0)
    global_batch = args.batch * world
    hyper = Dict(generator_learning_rate=8e-4 * global_batch / 8, generator_beta1=0.0, generator_beta2=0.99,
                 discriminator_learning_rate=8e-4 * global_batch / 8, discriminator_beta1=0.0, discriminator_beta2=0.99,
                 mode_seeking_loss_weight=0.1, real_gradient_penalty_weight=5.0, fake_gradient_penalty_weight=0.0)
    pool = synthetic_pool(args.batch, rank, dtype)
    cursor = [0]

    def real_input_fn():
        lat, lab, real = pool[cursor[0] % len(pool)]
        return real, lab

    def fake_input_fn():
        lat, _, _ = pool[cursor[0] % len(pool)]
        cursor[0] += 1
        return lat

    model = GANSynth(pggan.generator, pggan.discriminator, real_input_fn, fake_input_fn, None, hyper, dtype=dtype,
                     distributed=distributed, use_graphs=not args.no_graphs,
                     **({"bucket_bytes": int(float(os.environ["GS_BUCKET_MB"]) * (1 << 20))} if os.environ.get("GS_BUCKET_MB") else {}))
    K = kernels.get()

    def barrier():
        # (model.synchronize(): the one-graph iteration leaves the generator's last optimizer step pending -- it rides at the front of the next
        #  replay -- so the timed region ends with it applied, and starts with nothing pending: exactly K whole iterations inside.  Data
        #  parallel that step's all-reduce is a collective: every rank is here at the same point of its launch sequence.)
        if hasattr(model, "synchronize"):
            model.synchronize()
        if distributed:
            torch.distributed.barrier()
        torch.cuda.synchronize()

    stall = os.environ.get("GS_TEST_STALL_IN_MODE")   # (test hook: a worker that never gets through its warm-up in the named mode)
    if stall and os.environ.get("GS_DP_MODE") in stall.split(",") and rank == int(os.environ.get("GS_TEST_STALL_RANK", "0")):
        time.sleep(1e6)
    for _ in range(max(args.warmup, 1)):
        model.train_step()
    barrier()
    _mark("warm")
    t0 = time.perf_counter()
    for _ in range(args.steps):
        d_loss, g_loss = model.train_step()
    barrier()
    elapsed = time.perf_counter() - t0
    one_graph = bool((getattr(model, "_merged", None) or {}).get("fused"))   # (the whole iteration ONE hipGraph, optimizer steps inside)
    if args.dump_outputs and rank == 0:   # (before --full's extra iterations move the weights on)
        dump_outputs(args.dump_outputs, model, d_loss, g_loss)
    if args.full:
        # per-kernel roofline: the same iteration launched eagerly with a HIP event pair around every
        # conv_igemm_kernel launch on its own stream (events cannot bracket kernels inside a replayed hipGraph)
        prof_steps = min(args.steps, 5)
        model.use_graphs = False
        model.train_step()
        barrier()
        K.prof_enable(PROF_BURST)
        for _ in range(prof_steps):
            model.train_step()
        barrier()
        conv_bytes, roof_ms, roof_ms_hbm = K.prof_roofline(PEAK[args.dtype], HBM_GBPS)
        records = K.prof_records() if hasattr(K, "prof_records") else []
        launches, conv_ms, conv_flops = K.prof_collect()
        K.prof_enable(False)
        stages = per_stage(records, prof_steps, PEAK[args.dtype], args.dtype)
        # (one GPU only: an extra iteration on rank 0 alone would leave the other ranks out of its collectives)
        kernel_launches = count_launches(model) if world == 1 and not distributed and not args.no_launch_count else None
        whole = (None, None)
        if world == 1 and not distributed and not args.no_launch_count:
            model.use_graphs = not args.no_graphs
            whole = price_whole_step(model, K, args, stages, elapsed / args.steps * 1e3, prof_steps)
    if distributed:
        t = torch.tensor([elapsed], device="cuda", dtype=torch.float64)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        elapsed = float(t.item())
    if not (torch.isfinite(d_loss) and torch.isfinite(g_loss)):
        raise SystemExit(f"non-finite losses: {float(d_loss)} {float(g_loss)}")

    if rank == 0:
        if args.full:
            legs = {}
            if world == 1 and not args.no_spectral:
                legs["spectral"] = spectral_bench(cpu=not args.no_cpu_baseline)
                legs["spectral_inverse"] = inverse_bench()
            if world == 1 and args.dtype == "bf16" and not args.no_f32_leg and not args.no_graphs:
                torch.cuda.synchronize()
                legs["f32"] = f32_leg(args.batch)
            if world == 1 and not args.no_cpu_baseline:
                legs["cpu_baseline"] = cpu_baseline()
            out, detail = assemble(args, world, distributed, elapsed, prof_steps, (launches, conv_ms, conv_flops, conv_bytes, roof_ms, roof_ms_hbm),
                                   stages, kernel_launches, float(d_loss), float(g_loss), legs, whole_step=whole)
            out["detail"] = write_detail(detail)
        else:
            out = headline(args, world, distributed, elapsed, float(d_loss), float(g_loss))
        out["config"]["forked_branches"] = bool(getattr(model, "fork", False)) and not args.no_graphs
        out["config"]["graphs_per_iteration"] = (1 if one_graph else 2) if not args.no_graphs else 0
        if distributed:
            comm = getattr(model, "_comm", None)
            out["rccl_ranks"] = comm.count() if comm is not None else world   # ncclCommCount of the library's own communicator
            out["config"]["parallelism"] = "dp%d, gradient all-reduce: %s%s" % (
                world, os.environ.get("GS_DP_MODE") or ("graph-overlapped" if getattr(model, "_overlap_in_graph", lambda: False)() else
                                                        ("graph-one" if one_graph else "graph-serial") if (comm is not None and getattr(model, "_graph_allreduce", False) and not args.no_graphs) else "eager"),
                "" if comm is not None else " (torch.distributed communicator)")
        emit(out)
    _mark("done")
    if distributed:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
