#!/usr/bin/env python
"""bench.py — BASELINE.json headline metric: GCXS(CSR) x dense SpMM on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--scaling strong|weak] [--full] [--dump-outputs DIR]
    python bench.py --workload spgemm [--gpus N] [--steps K] [--warmup W]      BASELINE configs[4] (bench_spgemm.py), same schema

Workload (BASELINE.json configs[1]): A = CSR 10^6 x 10^4 at 1 % (exactly 10^8 stored elements, uniform, sorted column
indices, int32 indices, explicit compressed_axes=(0,)), B = dense 10^4 x 128 fp32, C = A @ B dense 10^6 x 128 fp32.
Inputs are generated on the device (synthetic) and are resident in HBM before the timed region.  One "step" = one
product through the product API (`sparse_amd.matmul`, the reference's NaN pass of `matmul` INCLUDED).  The product path
caches a K-tiled block stream of A on the array at its first product (inspector/executor: C ABI `spamd_spmm_tiled*`,
csrc/spmm_tiled.hip); `value` is the steady state of repeated products with the same A.  With `--full` the same line
carries what a FIRST product costs (`config.first_call_ms` = inspector + executor with a warm allocator,
`first_call_cold_ms` = the same in a fresh process, `rowgroup_ms` = the general cache-less kernel).  `--no-tiled` benches
the row-group kernel only.

A plain run sets up, warms up, times the K steps and prints the headline line (`metric`, `value`, `unit`,
`higher_is_better`, `dtype`, `ms_per_step` = wall time of the K timed steps / K, `config`); every other measurement is
behind `--full`.  `--dump-outputs DIR` writes, after the timed steps, what the last timed step returned (C = A @ B, see
`dump_outputs`) as DIR/<name>.npy; the inputs are generated from fixed seeds, so two runs with the same arguments (and
two builds of the project) can be compared output for output.

N > 1: `python bench.py --gpus N` re-launches itself under `python -m torch.distributed.run` (one rank per GPU, RCCL);
launched by torch.distributed.run directly it reads RANK / LOCAL_RANK / WORLD_SIZE.  Two modes:
  --scaling strong (default)  the ONE 10^8-nnz matrix is split into N nnz-balanced row blocks (`partition_rows_by_nnz`);
                              B arrives row-sharded and every step starts with one RCCL all-gather of B (the path's only
                              exchange step); C stays row-sharded.  value = total flops / max-over-ranks time.
  --scaling weak              every rank owns its own 10^6-row block of an (N*10^6) x 10^4 matrix; same exchange.

With `--full` the JSON line also carries `roofline` (HBM-bound: algorithmic bytes of one launch / the kernel's average
duration, measured with HIP events around K back-to-back launches of the executor on the launch stream; `traffic` is read
from the committed rocprofv3 PMC pass and labelled with its source), on rank 0 at N=1 `cpu_baseline` (the oracle's single-thread
C restatement of the reference loop, rebuilt with -march=native on this box, plus SciPy's csr @ dense as an independent
cross-check) and `paths`: the other rows of SURVEY.md section 8 at BASELINE.json's sizes (bench_paths.py).
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0      # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
HBM_MEASURED_GBS = 6290.0  # float4 copy on this part (same guide): the achievable streaming rate
LDS_READ_PEAK_BPS = 150e12 # all 256 CUs reading LDS with ds_read_b64/b128 (same guide, LDS section)
TILED_ABLATION_FILE = "profiles/r03_tiled_ablation.txt"   # round-3 ablations of the (since unchanged) executor: a pointer, not a measurement of this run


def make_csr_device(M, K, density, seed, idx_dtype=torch.int32, dtype=torch.float32, device="cuda"):
    """Uniform-without-replacement sparse matrix with exactly round(M*K*density) stored
    elements, as CSR with sorted column indices (the layout `sparse.random(...,
    format="gcxs", compressed_axes=(0,))` produces), generated on the device."""
    nnz = int(round(M * K * density))
    g = torch.Generator(device=device).manual_seed(seed)
    total = M * K
    x = torch.empty(0, dtype=torch.int64, device=device)
    while x.numel() < nnz:
        need = nnz - x.numel()
        draw = torch.randint(0, total, (int(need * 1.05) + 1024,), generator=g, device=device)
        x = torch.unique(torch.cat([x, draw]))  # sorted
    if x.numel() > nnz:
        drop = torch.randperm(x.numel(), generator=g, device=device)[: x.numel() - nnz]
        keep = torch.ones(x.numel(), dtype=torch.bool, device=device)
        keep[drop] = False
        x = x[keep]
    rows = torch.div(x, K, rounding_mode="floor")
    cols = (x - rows * K).to(idx_dtype)
    counts = torch.bincount(rows, minlength=M)
    indptr = torch.zeros(M + 1, dtype=torch.int64, device=device)
    indptr[1:] = torch.cumsum(counts, 0)
    data = torch.rand(nnz, generator=g, device=device, dtype=torch.float32).to(dtype)
    return data, cols, indptr.to(idx_dtype)


def make_powerlaw_csr_device(M, K, nnz, seed, alpha=1.0, empty_frac=0.3, idx_dtype=torch.int32, dtype=torch.float32, device="cuda"):
    """A skewed matrix (what real operands look like; `sparse.random` is uniform, _utils.py:221-346): row lengths follow a
    Zipf law (length of the r-th longest row ~ r^-alpha, capped at K: the first rows are FULL), `empty_frac` of the rows are
    empty, rows are shuffled, ~nnz stored elements in total.  Columns of a row are distinct by construction: an affine
    sequence (a_i j + b_i) mod P over a prime P >= K, entries >= K dropped (the total is therefore a little below `nnz`),
    sorted.  Returns (data, indices, indptr) like `make_csr_device`."""
    g = torch.Generator(device=device).manual_seed(seed)
    live = int(M * (1.0 - empty_frac))
    w = torch.arange(1, live + 1, device=device, dtype=torch.float64) ** (-alpha)
    # scale so that sum(min(c w, K)) = nnz (a few bisection steps on the device)
    lo, hi = 0.0, float(nnz) * 1e3
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        if float(torch.clamp(w * mid, max=K).sum()) < nnz:
            lo = mid
        else:
            hi = mid
    lens_sorted = torch.clamp(w * hi, max=K).round().to(torch.int64)
    lens = torch.zeros(M, dtype=torch.int64, device=device)
    lens[torch.randperm(M, generator=g, device=device)[:live]] = lens_sorted
    P = next(p for p in range(K, 2 * K + 100) if all(p % q for q in range(2, int(p ** 0.5) + 1)))
    a = torch.randint(1, P, (M,), generator=g, device=device)
    b = torch.randint(0, P, (M,), generator=g, device=device)
    start = torch.zeros(M + 1, dtype=torch.int64, device=device)
    start[1:] = torch.cumsum(lens, 0)
    total = int(start[-1])
    rows = torch.repeat_interleave(torch.arange(M, device=device), lens, output_size=total)
    j = torch.arange(total, device=device) - start[rows]
    cols = (a[rows] * j + b[rows]) % P
    keep = cols < K
    keys = (rows[keep] * K + cols[keep]).sort().values
    del rows, j, cols, keep
    rows = torch.div(keys, K, rounding_mode="floor")
    cols = (keys - rows * K).to(idx_dtype)
    indptr = torch.zeros(M + 1, dtype=torch.int64, device=device)
    indptr[1:] = torch.cumsum(torch.bincount(rows, minlength=M), 0)
    data = torch.rand(int(keys.numel()), generator=g, device=device, dtype=torch.float32).to(dtype)
    return data, cols, indptr.to(idx_dtype)


def algorithmic_bytes(M, K, N, nnz, val_bytes, idx_bytes):
    """nnz*(val+idx) + (M+1)*idx + K*N*val [B once] + M*N*val [C once]."""
    read = nnz * (val_bytes + idx_bytes) + (M + 1) * idx_bytes + K * N * val_bytes
    write = M * N * val_bytes
    return read, write


def dev_time(fn, reps):
    """Average milliseconds per call, HIP events on torch's current stream (the stream every C-ABI call launches on)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


DUMP_SAMPLE_BYTES = 40 << 20    # whole rows of C, sampled
DUMP_SUMS_MAX = 1 << 21         # float64 sums: 16 MB


def dump_outputs(path, c, rank, world):
    """Write what the last timed step returned, C (this rank's row block), as float32 / float64 .npy files under `path`,
    at most 64 MB in all ranks together:
      c_rows_sample      whole rows of C (float32) at a fixed, seeded sample of row numbers (<= 40 MB)
      c_sample_rows      those row numbers (float64)
      c_row_sums         the float64 sum of every row of C - of every run of ceil(rows / 2^21) consecutive rows beyond 2^21 rows
      c_col_sums         the float64 sum of every column of C
    With more than one rank every name carries `_rank<r>`."""
    os.makedirs(path, exist_ok=True)
    sfx = f"_rank{rank}" if world > 1 else ""
    c = torch.as_tensor(c)
    rows, cols = int(c.shape[0]), int(c.shape[1])
    take = min(rows, max(1, DUMP_SAMPLE_BYTES // world // (cols * 4 + 8)))    # a float32 row and its float64 number
    pick = np.sort(np.random.default_rng(20240501 + rank).choice(rows, take, replace=False)) if rows else np.zeros(0, np.int64)
    sample = c[torch.from_numpy(pick).to(c.device)].float()
    sums = c.sum(1, dtype=torch.float64)
    cap = max(1, DUMP_SUMS_MAX // world)
    if rows > cap:
        grp = -(-rows // cap)
        sums = torch.nn.functional.pad(sums, (0, -(-rows // grp) * grp - rows)).view(-1, grp).sum(1)
    out = {"c_rows_sample": sample.cpu().numpy(), "c_sample_rows": pick.astype(np.float64),
           "c_row_sums": sums.cpu().numpy(), "c_col_sums": c.sum(0, dtype=torch.float64).cpu().numpy()}
    for name, arr in out.items():
        np.save(os.path.join(path, f"{name}{sfx}.npy"), arr)


def cpu_baseline(data, idx, ptr, b, M, N, gpu_out):
    """The reference loop on the host CPU, same inputs, ONE thread (the reference's kernels are
    `@numba.jit(nopython=True, nogil=True)` without prange): (1) the oracle's C restatement rebuilt on THIS box with
    -march=native, whole workload once; (2) SciPy's `csr_array @ ndarray` on the same inputs as an
    independent single-thread implementation.  Both are compared with each other and with the GPU."""
    from oracle import build as obuild, oracle

    native = True
    try:
        oracle.use_library(obuild.build(native=True))
    except Exception:
        native = False
        obuild.build()
    h = [t.cpu().numpy() for t in (data, idx, ptr, b)]
    t0 = time.perf_counter()
    out = oracle.dot_csr_ndarray((M, N), *h)
    dt = time.perf_counter() - t0
    oracle.use_library(None)
    flops = 2.0 * h[0].shape[0] * N
    got = gpu_out.cpu().numpy()
    denom = np.maximum(np.abs(out), 1e-30)
    rel = float(np.max(np.abs(got - out) / denom))
    res = {
        "value": flops / dt / 1e9, "unit": "GFLOP/s", "cores": 1, "kind": "port",
        "sample": f"full workload once: M={M} nnz={h[0].shape[0]} N={N} fp32, {dt:.2f} s on 1 of "
                  f"{os.cpu_count()} host cores (oracle/oracle.c, gcc -O3 "
                  f"{'-march=native ' if native else ''}-ffp-contract=off)",
        "seconds": dt, "gpu_vs_cpu_max_rel_err": rel, "march_native": native,
    }
    try:
        import scipy.sparse as ss

        threads = None
        try:
            from threadpoolctl import threadpool_limits

            threads = threadpool_limits(limits=1)
        except Exception:
            pass
        a = ss.csr_array((h[0], h[1], h[2]), shape=(M, h[3].shape[0]))
        t0 = time.perf_counter()
        ref = a @ h[3]
        dts = time.perf_counter() - t0
        if threads is not None:
            threads.restore_original_limits()
        res["scipy"] = {"value": flops / dts / 1e9, "unit": "GFLOP/s", "seconds": dts, "cores": 1,
                        "what": "scipy.sparse.csr_array @ ndarray (csr_matvecs, single thread), whole workload once",
                        "oracle_vs_scipy_max_rel_err": float(np.max(np.abs(ref - out) / denom)),
                        "gpu_vs_scipy_max_rel_err": float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-30)))}
    except Exception as e:
        res["scipy"] = {"error": repr(e)}
    return res


def load_traffic(kernel_substr):
    """(HBM-side bytes per launch of the named kernel, where the number comes from).  The bytes are NOT measured in this
    run: they come from the committed rocprofv3 PMC passes (profiles/traffic.json, collected with tools/tools_pmc.sh in
    separate --pmc runs of this very script and corrected as MI355X_MICROARCH.md prescribes)."""
    path = os.path.join(ROOT, "profiles", "traffic.json")
    try:
        with open(path) as f:
            t = json.load(f)
        k = t["kernels"][kernel_substr]
        return k["traffic_bytes_per_launch"], f"profiles/traffic.json (round {k.get('round', t.get('round'))} PMC pass)"
    except Exception:
        return None, None


RCCL_PROBE = r"""
import json, os, sys, time, datetime
import torch, torch.distributed as dist
torch.cuda.set_device(0)
dist.init_process_group(backend="nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0),
                        timeout=datetime.timedelta(seconds=60))
K, N = int(sys.argv[1]), int(sys.argv[2])
b = torch.rand((K, N), device="cuda")
out = torch.empty_like(b)
for _ in range(5):
    dist.all_gather_into_tensor(out, b)
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
t0 = time.perf_counter(); e0.record()
for _ in range(50):
    dist.all_gather_into_tensor(out, b)
e1.record(); torch.cuda.synchronize()
print(json.dumps({"device_ms": e0.elapsed_time(e1) / 50, "host_wall_ms": (time.perf_counter() - t0) * 1e3 / 50,
                  "same": bool(torch.equal(out, b))}))
dist.destroy_process_group()
"""


def rccl_world1_gather_ms(K, N):
    """The FIXED part of the per-step exchange: `all_gather_into_tensor` of a K x N fp32 operand on an RCCL communicator of
    world size 1 (launch + the collective's own kernel; no xGMI traffic - that part needs the 8-GPU node), in a child
    process under a timeout so that a communicator that does not come up cannot take the bench line with it."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    try:
        r = subprocess.run([sys.executable, "-c", RCCL_PROBE, str(K), str(N)], env=env, capture_output=True, text=True, timeout=120)
        lines = [ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")]
        if not lines:
            return {"error": f"rc {r.returncode}: " + (r.stderr.strip().splitlines() or ["no output"])[-1][:300]}
        return json.loads(lines[-1])
    except Exception as e:  # noqa: BLE001
        return {"error": repr(e)[:200]}


def scaling_proxy(sp, _dist, data, idx, ptr, b_full, K, whole_ms, steps):
    """{world: {max_ms, mean_ms, nnz_imbalance, speedup}} for world in 2, 4, 8: EVERY block of the nnz-balanced partition
    multiplied alone on this GPU (B resident, `matmul` incl. its NaN pass, block streams cached as in the steady state)."""
    res = {}
    for w in (2, 4, 8):
        bounds = _dist.partition_rows_by_nnz(ptr, w)
        ms, nn = [], []
        for r in range(w):
            d, i, p, r0, r1 = _dist.shard_csr(data, idx, ptr, r, w, bounds)
            a = sp.GCXS((d.contiguous(), i.contiguous(), p.contiguous()), shape=(r1 - r0, K), compressed_axes=(0,))
            for _ in range(5):
                o = sp.matmul(a, b_full)
            ms.append(dev_time(lambda: sp.matmul(a, b_full), steps))
            nn.append(int(d.numel()))
            del a, o, d, i, p
        sp.flush_warnings()
        mean = sum(ms) / w
        res[str(w)] = {"max_ms": round(max(ms), 4), "mean_ms": round(mean, 4), "min_ms": round(min(ms), 4),
                       "time_imbalance": round(max(ms) / mean, 4), "nnz_imbalance": round(max(nn) / (sum(nn) / w), 5),
                       "speedup_vs_whole": round(whole_ms / max(ms), 3)}
    res["rccl_world1_all_gather_B"] = rccl_world1_gather_ms(K, int(b_full.shape[1]))
    g = res["rccl_world1_all_gather_B"].get("device_ms")
    if g is not None:
        for w in ("2", "4", "8"):
            res[w]["speedup_with_fixed_gather"] = round(whole_ms / (res[w]["max_ms"] + g), 3)
    res["what"] = ("every nnz-balanced row block timed ALONE on one GPU, B resident: step time at world w = max over blocks "
                   "(+ the exchange; only its fixed part, an RCCL world-size-1 all-gather, is measurable here)")
    return res


def relaunch_distributed(n):
    """`python bench.py --gpus N` without a launcher: re-exec under torch.distributed.run, one rank per GPU."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__), *sys.argv[1:]]
    return subprocess.call(cmd, env=env)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scaling", choices=["strong", "weak"], default="strong")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--cols", type=int, default=10_000)
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--density", type=float, default=0.01)
    ap.add_argument("--idx", choices=["int32", "int64"], default="int32")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline does not need: first-product costs, the default-settings loop, the "
                         "executor alone (roofline), the scaling proxy, cpu_baseline and the other section-8 rows (`paths`)")
    ap.add_argument("--dump-outputs", metavar="DIR", help="after the timed steps, write what the last one returned as DIR/<name>.npy")
    ap.add_argument("--no-cpu", action="store_true", help="with --full: skip the cpu_baseline leg")
    ap.add_argument("--no-paths", action="store_true", help="with --full: skip the other section-8 rows (`paths`)")
    ap.add_argument("--no-nan-check", action="store_true", help="switch matmul's NaN pass off in the timed region")
    ap.add_argument("--exact", action="store_true", help="bit-exact mul+add instead of FMA")
    ap.add_argument("--no-tiled", action="store_true", help="row-group kernel only (no cached block stream)")
    ap.add_argument("--workload", choices=["spmm", "spgemm"], default="spmm",
                    help="spmm = the headline (BASELINE configs[1]); spgemm = configs[4], G @ G row-block sharded (bench_spgemm.py)")
    ap.add_argument("--spgemm-n", type=int, default=1_000_000)
    ap.add_argument("--spgemm-density", type=float, default=1e-4)
    ap.add_argument("--spgemm-dtype", choices=["f32", "f64"], default="f32")
    ap.add_argument("--chunk-rows", type=int, default=125_000, help="spgemm: rows per local product (bounds the result buffers)")
    args = ap.parse_args()

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        if torch.cuda.device_count() < args.gpus:
            raise SystemExit(f"bench.py --gpus {args.gpus}: only {torch.cuda.device_count()} HIP device(s) visible")
        raise SystemExit(relaunch_distributed(args.gpus))

    if args.workload == "spgemm":
        import bench_spgemm

        if args.dump_outputs:
            raise SystemExit("bench.py --dump-outputs: the spmm workload only")
        if "--steps" not in sys.argv:
            args.steps = 3          # a step is ~90 ms of products at N = 1
        if "--warmup" not in sys.argv:
            args.warmup = 1
        return bench_spgemm.main(args)

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    dist = None
    if world > 1 or "WORLD_SIZE" in os.environ:
        import torch.distributed as dist

        dist.init_process_group(backend="nccl", device_id=device)
        world = dist.get_world_size()   # what RCCL actually formed, not what the flag asked for
        rank = dist.get_rank()

    import sparse_amd
    from sparse_amd import _dist, _dot, _kernels, _settings

    _settings.NAN_CHECK = not args.no_nan_check  # package default: on (the reference's `matmul` scans both operands)
    # the scans run in every product of the timed region; their verdicts are polled without blocking the host and drained
    # before the closing synchronize (package default "sync" makes the host wait for the scan kernels of every product,
    # which bounds the launch rate once a product takes 0.1 ms: a rank's share at 8 GPUs)
    _settings.NAN_WARNING = "deferred"
    _settings.EXACT_MULADD = bool(args.exact)
    if args.no_tiled:
        _settings.TILED_SPMM = "never"

    M, K, N = args.rows, args.cols, args.n
    idt = torch.int32 if args.idx == "int32" else torch.int64
    strong = args.scaling == "strong"
    if strong:
        # every rank generates the SAME matrix (same seed) and keeps its nnz-balanced row block
        data_g, idx_g, ptr_g = make_csr_device(M, K, args.density, seed=1234, idx_dtype=idt, device=device)
        bounds = _dist.partition_rows_by_nnz(ptr_g, world)
        data, idx, ptr, r0, r1 = _dist.shard_csr(data_g, idx_g, ptr_g, rank, world, bounds)
        data, idx, ptr = data.contiguous(), idx.contiguous(), ptr.contiguous()
        global_nnz = int(data_g.numel())
        del data_g, idx_g, ptr_g
        Mloc = r1 - r0
    else:
        data, idx, ptr = make_csr_device(M, K, args.density, seed=1234 + rank, idx_dtype=idt, device=device)
        Mloc = M
        global_nnz = None
    nnz = int(data.numel())
    a = sparse_amd.GCXS((data, idx, ptr), shape=(Mloc, K), compressed_axes=(0,))
    g = torch.Generator(device=device).manual_seed(99)
    b_full = torch.rand((K, N), generator=g, device=device, dtype=torch.float32)
    sharded_b = dist is not None and world > 1
    if sharded_b:
        b_shard = _dist.row_shard(b_full, rank, world).contiguous()

    def step(memo=False, prefetch=False):
        # B is gathered at EVERY step (memo=False), although it does not change here: the conservative figure.  The gather
        # is launched asynchronously and the local block's NaN scan is queued while it is in flight (`sharded_spmm`).
        # prefetch=True: the NEXT step's gather is launched before this step's product (still one gather per step).
        if sharded_b:
            return _dist.sharded_spmm(a, b_shard, K, memo=memo, prefetch=b_shard if prefetch else None)
        return sparse_amd.matmul(a, b_full)

    # ---- what a FIRST product with this A costs (--full; rank-local; all of it outside the timed region) ----------------
    rowgroup_ms = first_call_cold_ms = first_call_ms = inspector_ms = None
    tiled = False
    if _dot._tiled_eligible(a.data, b_full, (Mloc, N), K):
        rowgroup = lambda: _kernels.dot_csr_ndarray((Mloc, N), data, idx, ptr, b_full, exact=False)
        # (timed AFTER the timed region, warm: round 4 timed it here, inside the first-call window, and reported 9.7 ms
        # for a kernel rocprofv3 sees at 2.8 ms)

        def first_product():
            _dot.drop_derived(a)               # forget the cached block stream: inspector + executor, as at a first product
            return _dot._gcxs_times_dense(a, b_full, (Mloc, N))

        if args.full:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            first_product()
            torch.cuda.synchronize()
            first_call_cold_ms = (time.perf_counter() - t0) * 1e3   # fresh process: includes ~1 GB of first-time allocations
            first_call_ms = dev_time(first_product, 3)             # warm allocator (a program that has multiplied before)
            inspector_ms = dev_time(lambda: _kernels.csr_tiled_layout(data, idx, ptr, Mloc, K), 3)
        # the block stream every step reads, cached on `a` here as the first product would (the first product's own path)
        tiled = _dot.prepare_spmm(a)

    # the value is a STEADY-STATE rate: the first ~30 products after the set-up above (host-timed first products, the
    # inspector timing, idle gaps between them) run 5-8 % slower than the ones after them (steps 20: warm-up 3 -> 0.918 ms,
    # 10 -> 0.887, 30 -> 0.849; the kernel alone 0.83-0.85 throughout), so the device is brought to its sustained state
    # before the W warm-up steps the command line asks for (reported as `prewarm_products`)
    PREWARM = 40
    for _ in range(PREWARM):
        out = step()
    for _ in range(args.warmup):
        out = step()
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = step()
    sparse_amd.flush_warnings()      # every NaN verdict of the timed products is read inside the timed region
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
        torch.cuda.synchronize()
    wall = time.perf_counter() - t0

    tmax = torch.tensor([wall], device=device, dtype=torch.float64)
    nnz_all = torch.tensor([float(nnz)], device=device, dtype=torch.float64)
    if dist is not None:
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        gathered = [torch.zeros_like(nnz_all) for _ in range(world)]
        dist.all_gather(gathered, nnz_all)
        nnz_ranks = [int(t.item()) for t in gathered]
    else:
        nnz_ranks = [nnz]
    wall = float(tmax.item())
    ms_per_step = wall / args.steps * 1e3
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, out, rank, world)

    # ---- everything below the headline: --full only --------------------------------------------------------------------
    ms_static_b = ms_prefetch = None
    secondary_error = None
    if sharded_b and args.full:
        def timed_loop(**kw):
            step(**kw)
            torch.cuda.synchronize()
            dist.barrier()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step(**kw)
            sparse_amd.flush_warnings()
            torch.cuda.synchronize()
            dist.barrier()
            tm = torch.tensor([time.perf_counter() - t0], device=device, dtype=torch.float64)
            dist.all_reduce(tm, op=dist.ReduceOp.MAX)
            return float(tm.item()) / args.steps * 1e3

        # (the two loops below are reported BESIDE the headline, never instead of it: a failure in them - they have only
        # ever run under gloo and with one RCCL rank - must not cost the headline its line; every rank takes the same path)
        try:
            # the same loop with the gathered B memoised on (shard buffer, version): what a program that multiplies by an
            # unchanged B pays (one all-gather in total)
            ms_static_b = timed_loop(memo=True)
            # ... and with B gathered at every step, but one step AHEAD (`sharded_spmm(prefetch=...)`): the collective runs
            # on RCCL's stream beside the executor of the step before it
            ms_prefetch = timed_loop(prefetch=True)
            _dist.drop_prefetched()
        except Exception as e:      # noqa: BLE001
            secondary_error = f"{type(e).__name__}: {e}"[:300]

    # ---- the same loop under the package's DEFAULT settings (NAN_WARNING = "sync": the host waits for every product's NaN
    # verdict before it returns, as the reference's `matmul` has its warning raised inside the call) - printed beside the
    # headline, which runs with the verdicts deferred to `flush_warnings()` (round-5 verdict, item 9)
    ms_default = None
    if world == 1 and args.full:
        _settings.NAN_WARNING = "sync"
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            out = step()
        torch.cuda.synchronize()
        ms_default = (time.perf_counter() - t0) / args.steps * 1e3
        _settings.NAN_WARNING = "deferred"

    # ---- the dominant kernel alone: K back-to-back launches of the executor between two HIP events --------------------
    kernel_ms = None
    if args.full:
        if tiled:
            layout = a._tiled_layouts[torch.float32]
            kern = lambda: _kernels.dot_csr_ndarray_tiled(layout, (Mloc, N), K, b_full, out=out, exact=bool(args.exact))
        else:
            kern = lambda: _kernels.dot_csr_ndarray((Mloc, N), data, idx, ptr, b_full, exact=bool(args.exact), out=out)
        kern()
        kernel_ms = dev_time(kern, args.steps)
        if tiled:
            for _ in range(3):
                rowgroup()
            rowgroup_ms = dev_time(rowgroup, 5)   # the general cache-less kernel (every dtype / shape the executor does not take)
    # ---- what one GPU can say about scaling (no 8-GPU node is available to this run): for world sizes 2, 4, 8
    # EVERY block of the nnz-balanced partition of THIS matrix is timed alone (B resident, through `matmul`): the step time
    # of the sharded product is the MAX over the blocks + the exchange; its fixed part (an RCCL all-gather of B launched at
    # world size 1) is measured in a child process
    proxy = None
    if args.full and world == 1 and tiled and not args.no_paths:   # (not in the profiled headline run: its kernel average must be the headline's alone)
        try:
            proxy = scaling_proxy(sparse_amd, _dist, data, idx, ptr, b_full, K, ms_per_step, args.steps)
        except Exception as e:   # noqa: BLE001 - the headline line must still be printed
            proxy = {"error": repr(e)}
    nan_check_ms = None
    if args.full and _settings.NAN_CHECK:
        # what `matmul` adds to a product: the scans of both operands (A's verdict is memoised per buffer version, so in the
        # steady state this is the scan of B and the bookkeeping), HIP events around the scans alone
        def scans():
            for x in (a, b_full):
                v = _dot.check_class_nan(x, deferred=True)
                if not isinstance(v, bool):
                    v()
        scans()
        nan_check_ms = dev_time(scans, args.steps)

    if rank == 0:
        total_nnz = sum(nnz_ranks)
        flops_total = 2.0 * total_nnz * N
        flops_local = 2.0 * nnz * N
        r4 = lambda x: None if x is None else round(x, 4)
        line = {
            "metric": "GCXS x dense SpMM throughput (GFLOP/s)",
            "value": round(flops_total / (ms_per_step * 1e-3) / 1e9, 2),
            "unit": "GFLOP/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 5), "higher_is_better": True, "scaling": args.scaling,
            "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {
                "workload": (f"GCXS(CSR) {M}x{K} @ {args.density:g} ({global_nnz} nnz, {args.idx} idx) in {world} nnz-balanced row block(s)"
                             if strong else f"GCXS(CSR) {world}x({M}x{K}) @ {args.density:g} ({nnz} nnz/GPU, {args.idx} idx)")
                            + f" x dense {K}x{N} fp32",
                "world_size": world, "nnz_per_rank": nnz_ranks,
                "nnz_imbalance": round(max(nnz_ranks) / (total_nnz / world), 5) if total_nnz else 1.0,
                "rows_rank0": Mloc, "idx_dtype": args.idx,
                "parallelism": f"row-block x{world}" + (" + RCCL all-gather(B) per step" if sharded_b else ""),
                "ms_per_step_with_B_gathered_once": r4(ms_static_b),
                "ms_per_step_with_next_gather_prefetched": r4(ms_prefetch),
                "secondary_loops_error": secondary_error,
                "mul_add": "separate (bit-exact)" if args.exact else "fma",
                "nan_check_in_timed_region": bool(_settings.NAN_CHECK), "nan_check_ms_per_product": r4(nan_check_ms),
                "nan_warning": _settings.NAN_WARNING, "prewarm_products": PREWARM,
                "ms_per_step_default_settings": r4(ms_default), "default_settings": 'NAN_WARNING="sync" (verdict read inside every product)',

                "kernel": "spmm_tiled (cached block stream)" if tiled else "spmm_csr_rowgroup",
                "first_call_ms": r4(first_call_ms), "first_call_cold_ms": r4(first_call_cold_ms),
                "inspector_ms": r4(inspector_ms), "rowgroup_ms": r4(rowgroup_ms),
            },
        }
        if args.full:
            ib = 4 if idt == torch.int32 else 8
            rd, wr = algorithmic_bytes(Mloc, K, N, nnz, 4, ib)
            ach = (rd + wr) / (kernel_ms * 1e-3) / 1e9
            traffic, traffic_src = load_traffic("spmm_tiled" if tiled else "spmm_csr")
            lds_floor = nnz * N * 4 / LDS_READ_PEAK_BPS * 1e3
            line["roofline"] = {
                "bound": "hbm", "achieved": round(ach, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": round(ach / HBM_PEAK_GBS, 5), "frac_of_measured_copy_rate": round(ach / HBM_MEASURED_GBS, 5),
                "traffic": traffic, "traffic_source": traffic_src,
                "algorithmic_bytes": rd + wr, "algorithmic_read_bytes": rd,
                "kernel_ms": round(kernel_ms, 5), "gflops_per_gpu": round(flops_local / (kernel_ms * 1e-3) / 1e9, 1),
                # the ceiling of ANY design that reads one 512-byte row of B from LDS per stored element (no two rows of a
                # row group share a column at 1 % density, so there is no register-level reuse): nnz x N x 4 bytes at the
                # ~150 TB/s all CUs' ds_read_b64 deliver (MI355X_MICROARCH.md, LDS section)
                "lds_floor_ms": r4(lds_floor), "frac_of_lds_floor": r4(lds_floor / kernel_ms),
                "scaling_proxy": proxy,
                "ablation": TILED_ABLATION_FILE if tiled else None,
                "what": "rank 0: algorithmic bytes of its row block / mean of `steps` back-to-back executor launches (HIP events)",
            }
        if args.full and world == 1 and not args.no_cpu:
            try:
                line["cpu_baseline"] = cpu_baseline(data, idx, ptr, b_full, Mloc, N, out)
            except Exception as e:  # the bench line must still be printed
                line["cpu_baseline"] = {"error": repr(e)}
        if args.full and world == 1 and not args.no_paths:
            del out
            # the other section-8 rows: the FULL dict goes to an earlier stdout line and to gpurun_out/paths.json; the LAST
            # line (the one the driver parses; round 4's 23 KB line did not parse) carries compact maps only
            try:
                import bench_paths

                paths = bench_paths.run(int64_of=(data, idx, ptr, b_full, M, K, N), verbose=False)
                print(json.dumps({"paths": paths}), flush=True)
                try:
                    os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
                    with open(os.path.join(ROOT, "gpurun_out", "paths.json"), "w") as f:
                        json.dump(paths, f, indent=1)
                except OSError:
                    pass
                rows = {k: v for k, v in paths.items() if isinstance(v, dict)}
                rl = line["roofline"]
                rl["paths_frac"] = {k: round(v["frac"], 4) for k, v in rows.items() if "frac" in v}
                rl["paths_ms"] = {k: round(v["ms"], 4) for k, v in rows.items() if "ms" in v}
                rl["paths_pmc_over_algorithmic"] = {k: round(v["pmc_over_algorithmic"], 3) for k, v in rows.items()
                                                    if v.get("pmc_over_algorithmic") is not None}
                rl["paths_pmc_source"] = paths.get("_pmc_source")
                rl["paths_accounting_errors"] = paths.get("_accounting_errors", [])
                rl["paths_full"] = "previous stdout line + gpurun_out/paths.json"
            except Exception as e:
                line["roofline"]["paths_error"] = repr(e)
            # the reference's own benchmark sizes (bench_small.py; the full table: profiles/rNN_small_workloads.json): host-bound
            # microseconds per call, a few representative cases beside the single-core oracle leg
            try:
                import bench_small

                sw = bench_small.run(quick=True, reps=100)
                pick = {"dense_1000^3_gcxs0": sw["dense"].get("1000x1000x1000_gcxs0"), "spsp_1000^3_gcxs": sw["spsp"].get("1000x1000x1000_gcxs"),
                        "add_side1000_rank2_coo": sw["ewise"].get("add_side1000_rank2_coo"), "add_side1000_rank2_gcxs": sw["ewise"].get("add_side1000_rank2_gcxs"),
                        "broadcast_add_side1000_coo": sw.get("ewise_broadcast", {}).get("add_side1000_coo")}
                line["roofline"]["small_workloads_us"] = {k: {a: v[a] for a in ("us_sync", "us_pipe", "cpu_us") if a in v}
                                                          for k, v in pick.items() if v}
            except Exception as e:
                line["roofline"]["small_workloads_error"] = repr(e)
        print(json.dumps(line, separators=(",", ":")), flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
