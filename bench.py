#!/usr/bin/env python3
"""Headline benchmark: tiles/sec of one training step (fwd + CE loss + bwd [+ RCCL grad all-reduce] +
Adam) of the ResNet-50 MIL tile classifier on a bag of 64 synthetic 299x299 IHC tiles per GPU, bf16
(BASELINE.json configs[1]; `--scratch` semantics = encoder gradients on, BN frozen via freeze_bn,
i.e. the reference loop body train/train.py:32-37).

    python bench.py --gpus 1 --steps 20 --warmup 5 [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

Prints ONE JSON line on rank 0 (contract in the task statement).  A plain run sets up, warms up, times the K steps and reports
them (`value`, `ms_per_step`); every other figure is measured only with --full:
  roofline     : the dominant conv kernel instantiation, timed per launch with HIP events on the launch stream
  cpu_baseline : the CPU oracle (numerically the reference path) timed on this box's host cores (rank 0, N=1 only)
  fp32_parity_mode, rccl_world1, secondary (N=1), rccl (N>1): side runs outside the timed region
--dump-outputs DIR writes what the last timed step computed (loss, logits, a fixed sample of the updated parameters and of the
gradients) as DIR/<name>.npy in float32, so that two builds can be compared output for output on identical inputs.
"""
import argparse
import json
import os
import sys
import time


def _self_launch():
    """`python bench.py --gpus N` (N > 1) outside a torchrun environment: start N ranks ourselves, as a FRESH child process
    (`python -m torch.distributed.run`, one rank per GPU, rendezvous on 127.0.0.1) and exit with its return code.  This runs
    before torch / the HIP library are imported, so the parent never touches the GPU (no exec after GPU init, no second HIP
    context beside the ranks).  The reference's counterpart is the DDP stub of train_tile.py:227-238."""
    # under torchrun (RANK is set for every rank) this process IS a rank; a bare WORLD_SIZE=1 some schedulers pre-export is not torchrun
    if "RANK" in os.environ or ("WORLD_SIZE" in os.environ and os.environ["WORLD_SIZE"] != "1"):
        return
    n = 1
    argv = sys.argv[1:]
    for i, a in enumerate(argv):
        if a == "--gpus" and i + 1 < len(argv):
            n = int(argv[i + 1])
        elif a.startswith("--gpus="):
            n = int(a.split("=", 1)[1])
    if n <= 1:
        return
    import subprocess
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")       # dmabuf IPC only on this host driver (RCCL needs it)
    env.setdefault("OMP_NUM_THREADS", "8")
    # --standalone: torchrun picks a free rendezvous port itself (probing one here and handing it over is a race);
    # --local-addr because the container's hostname may not resolve
    cmd = [sys.executable, "-m", "torch.distributed.run", "--standalone", "--local-addr=127.0.0.1", "--nnodes=1", f"--nproc-per-node={n}",
           os.path.abspath(__file__), *argv]
    sys.exit(subprocess.run(cmd, env=env).returncode)


if __name__ == "__main__":
    _self_launch()

import torch  # noqa: E402

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from cellsegmentation_amd import functional as HF  # noqa: E402
from cellsegmentation_amd import kernels as K  # noqa: E402
from cellsegmentation_amd import synth  # noqa: E402
from cellsegmentation_amd.model import resnet as R  # noqa: E402
from cellsegmentation_amd.optim import Adam  # noqa: E402
from cellsegmentation_amd.parallel import GradReducer  # noqa: E402

PEAK_BF16_TFLOPS = 2500.0       # dense MFMA bf16, MI355X_MICROARCH.md "Chip-level parameters"
PEAK_F32_TFLOPS = 157.3
BAG = 64
SIZE = 299
ARCH = "resnet50"


def build_model(dev, dtype):
    m = R.MILresnet50()
    sd = m.state_dict()
    synth.fill_state_dict(sd)
    m.load_state_dict(sd)
    m = m.to(dev).set_compute_dtype(dtype)
    m.setmode("tile")
    m.set_encoder_grads(True)          # --scratch (train_tile.py:272-273): full conv backward
    m.train()
    return m


PEAK_HBM_GBS = 8000.0           # HBM3E, MI355X_MICROARCH.md "Chip-level parameters" (spec; ~6300 measured achievable)
MACHINE_BALANCE = PEAK_BF16_TFLOPS * 1e12 / (PEAK_HBM_GBS * 1e9)     # FLOP per byte where the two roofs meet (~312)


def conv_flops(g):
    """Algorithmic FLOPs of one conv-family launch: 2*N*P*Q*K*C*R*S with the TRUE channel counts (stem C=3, not the padded 8);
    a batched weight-gradient launch covers g["batch"] layers of that geometry."""
    c_true = 3 if (g["R"] == 7 and g["C"] == 8) else g["C"]
    return 2.0 * g["N"] * g["P"] * g["Q"] * g["K"] * c_true * g["R"] * g["S"] * g.get("batch", 1)


def conv_bytes(kind, g, es):
    """Algorithmic HBM bytes of one launch: every operand tensor once (activations in the storage dtype, weights once,
    wgrad output in fp32), plus the destination-shaped tensors the fused epilogue reads (residual / add / mask)."""
    x = g["N"] * g["H"] * g["W"] * g["C"] * es
    y = g["N"] * g["P"] * g["Q"] * g["K"] * es
    w = g["K"] * g["R"] * g["S"] * g["C"]
    if g["R"] == 1 and g["S"] == 1 and g["stride"] > 1:
        # a strided 1x1 convolution touches one pixel in stride^2 (forward and weight gradient read x at the sampled pixels only;
        # the compact data gradient's destination is already counted by `extra` = -0.75): VERDICT r4 item 8
        xs = g["N"] * g["P"] * g["Q"] * g["C"] * es
        if kind == "fwd":
            return xs + y + w * es + g["extra"] * y
        if kind == "wgrad":
            return (xs + y + w * 4) * g.get("batch", 1)
    if kind == "fwd":
        return x + y + w * es + g["extra"] * y
    if kind == "dgrad":
        return y + x + w * es + g["extra"] * x
    return (x + y + w * 4) * g.get("batch", 1)


def kernel_name(kind, g, dtype):
    """Name of the kernel instantiation that ran: reported by the library itself (cs_last_conv_variant, recorded per launch by
    kernels._timed), never re-derived here -- it is the name rocprofv3 prints for the same launch (tools/check_bench_vs_profile.py)."""
    return g.get("variant") or "unknown"


def _traffic_for(name, by_per_launch, cfg=None):
    """HBM bytes per launch from the committed PMC passes (tools/collect_traffic.py: separate FETCH_SIZE / WRITE_SIZE runs,
    gfx950-corrected), newest round first; None when the kernel was not sampled.  `cfg`: the passes of a secondary config
    (tools/bench_configs.py c4 / c5 / c5x) instead of the headline step's."""
    files = ([f"round{r}_traffic_{cfg}.json" for r in (5, 4, 3)] if cfg
             else [f"round{r}_traffic.json" for r in (5, 4, 3, 2, 1)])
    for fn in files:
        tpath = os.path.join(ROOT, "profiles", fn)
        if not os.path.exists(tpath):
            continue
        try:
            entry = json.load(open(tpath))["kernels"].get(name)
        except (ValueError, KeyError):
            entry = None
        if entry:
            return {"hbm_bytes_per_launch": entry["hbm_bytes_per_launch"], "read": entry["read_bytes_per_launch"],
                    "write": entry["write_bytes_per_launch"], "vs_algorithmic": round(entry["hbm_bytes_per_launch"] / by_per_launch, 2),
                    "source": f"profiles/{fn} (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, gfx950-corrected)"}
    return None


def roofline_from(records, steps, dtype, traffic_cfg=None):
    """Per-launch HIP-event times -> roofline of the dominant kernel instantiation (largest share of conv time) plus the dominant
    MFMA-bound and the dominant HBM-bound one.  A kernel's bound is decided by its aggregate arithmetic intensity against the
    machine balance: HBM-bound kernels are priced in algorithmic GB/s against the 8 TB/s spec, MFMA-bound ones in TFLOP/s
    against the dense bf16 peak."""
    es = 2 if dtype == torch.bfloat16 else 4
    per_kernel, per_family = {}, {}
    for kind, g, dt, ms in records:
        name = kernel_name(kind, g, dt)
        fam = f"{g['R']}x{g['S']}/{kind}"
        fl, by = conv_flops(g), conv_bytes(kind, g, es)
        for table, key in ((per_kernel, name), (per_family, fam)):
            e = table.setdefault(key, [0.0, 0.0, 0, 0.0])
            e[0] += fl; e[1] += ms; e[2] += 1; e[3] += by
    if not per_kernel:
        return None
    peak_tf = PEAK_BF16_TFLOPS if dtype == torch.bfloat16 else PEAK_F32_TFLOPS
    balance = peak_tf * 1e12 / (PEAK_HBM_GBS * 1e9)

    def row(v, per_step=False):
        out = {"tflops": round(v[0] / (v[1] * 1e-3) / 1e12, 1), "gbps": round(v[3] / (v[1] * 1e-3) / 1e9, 0),
               "flop_per_byte": round(v[0] / v[3], 1)}
        if per_step:
            out.update(ms_per_step=round(v[1] / steps, 3), launches_per_step=v[2] // steps)
        else:
            out.update(avg_ms=round(v[1] / v[2], 4), launches=v[2], launches_per_step=round(v[2] / steps, 2), ms_per_step=round(v[1] / steps, 3))
        return out

    def entry(name):
        fl, ms, n, by = per_kernel[name]
        if fl / by < balance:
            achieved, peak, unit, bound = by / (ms * 1e-3) / 1e9, PEAK_HBM_GBS, "GB/s", "hbm"
        else:
            achieved, peak, unit, bound = fl / (ms * 1e-3) / 1e12, peak_tf, "TFLOP/s", "mfma"
        tr = _traffic_for(name, by / n, traffic_cfg)
        # `traffic`: HBM bytes per launch from the PMC passes (a plain number, or null); the read / write split rides beside it
        return {"bound": bound, "achieved": round(achieved, 2), "peak": peak, "unit": unit, "frac": round(achieved / peak, 4),
                "traffic": tr["hbm_bytes_per_launch"] if tr else None, "traffic_detail": tr, "kernel": name, "avg_launch_ms": round(ms / n, 4), "launches": n,
                "share_of_conv_time": round(ms / sum(v[1] for v in per_kernel.values()), 4),
                "algorithmic_per_launch": {"gflop": round(fl / n / 1e9, 3), "mbytes": round(by / n / 1e6, 2), "flop_per_byte": round(fl / by, 1)}}

    by_time = sorted(per_kernel, key=lambda k: -per_kernel[k][1])
    out = entry(by_time[0])
    mf = [k for k in by_time if per_kernel[k][0] / per_kernel[k][3] >= balance]
    hb = [k for k in by_time if per_kernel[k][0] / per_kernel[k][3] < balance]
    out["dominant_mfma_bound"] = entry(mf[0]) if mf else None
    out["dominant_hbm_bound"] = entry(hb[0]) if hb else None
    three = [v for k, v in per_family.items() if k.startswith("3x3")]
    t3 = sum(v[0] for v in three) / (sum(v[1] for v in three) * 1e-3) / 1e12 if three else None
    out.update({"conv3x3_family_tflops": round(t3, 2) if t3 else None, "conv3x3_family_frac_of_mfma_peak": round(t3 / peak_tf, 4) if t3 else None,
                "by_kernel": {k: row(v) for k, v in sorted(per_kernel.items())},
                "by_family": {k: row(v, True) for k, v in sorted(per_family.items())}})
    return out


def per_layer_table(records, steps, dtype):
    """One line per (kind, geometry): launches/step, average time, algorithmic GB/s and TFLOP/s (stderr, --per-layer)."""
    es = 2 if dtype == torch.bfloat16 else 4
    rows = {}
    for kind, g, dt, ms in records:
        key = (kind, g["R"], g["stride"], g["C"], g["K"], g["H"], g["extra"], g.get("batch", 1))
        e = rows.setdefault(key, [0.0, 0, conv_flops(g), conv_bytes(kind, g, es), kernel_name(kind, g, dt)])
        e[0] += ms; e[1] += 1
    out = [f"{'kind':6s} {'RxR/s':6s} {'C':>5s} {'K':>5s} {'H':>4s} {'ex':>4s} {'b':>2s} {'n/step':>6s} {'avg us':>8s} {'ms/step':>8s} {'GB/s':>7s} {'TF/s':>7s}  kernel"]
    for key, (ms, n, fl, by, name) in sorted(rows.items(), key=lambda kv: -kv[1][0]):
        kind, R, st, C, Kc, H, ex, b = key
        avg = ms / n
        out.append(f"{kind:6s} {R}x{R}/{st:<2d} {C:5d} {Kc:5d} {H:4d} {ex:4.2f} {b:2d} {n / steps:6.1f} {avg * 1e3:8.1f} {ms / steps:8.3f} "
                   f"{by / (avg * 1e-3) / 1e9:7.0f} {fl / (avg * 1e-3) / 1e12:7.1f}  {name}")
    return "\n".join(out)


def _host_cpu():
    """(model string, physical cores usable by this process) from lscpu / the affinity mask."""
    model, cores_per_socket, sockets, threads_per_core = "unknown", None, None, 1
    try:
        import subprocess
        for line in subprocess.run(["lscpu"], capture_output=True, text=True, timeout=10).stdout.splitlines():
            k, _, v = line.partition(":")
            k, v = k.strip(), v.strip()
            if k == "Model name":
                model = v
            elif k == "Core(s) per socket":
                cores_per_socket = int(v)
            elif k == "Socket(s)":
                sockets = int(v)
            elif k == "Thread(s) per core":
                threads_per_core = max(1, int(v))
    except Exception:  # noqa: BLE001
        pass
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:
        avail = os.cpu_count() or 1
    physical = cores_per_socket * sockets if cores_per_socket and sockets else max(1, avail // threads_per_core)
    return model, max(1, min(physical, max(1, avail // threads_per_core) if avail < physical * threads_per_core else physical))


def cpu_baseline(micro=16, accum=4, steps=2):
    """The oracle (torch CPU fp32 NCHW, proven equal to the reference in tests/golden/make_golden.py) on the same step definition
    and the same bag of 64 tiles as the GPU (N = 64 as 16 x 4 -- four micro-batches accumulate into one
    optimizer step; with BatchNorm frozen the gradients are identical to one batch of 64).

    oneDNN's fp32 backward at micro-batch 16 does not scale to every core of a 128-core host (round 2: 2.8 tiles/s on 128 threads,
    10-15 on 16), so the number of record is the BEST of a thread sweep {16, 32, 64, all physical cores}: per candidate one warm-up
    and one timed micro-batch (16 tiles fwd+bwd), then `steps` full steps (4 micro-batches + Adam) at the fastest setting.  The
    sweep and the thread count used are part of the JSON."""
    from oracle import cellseg_oracle as orc
    model_name, cores = _host_cpu()
    n = micro * accum
    base = synth.normalise(synth.ihc_tiles(8, SIZE, 1234))
    x = base.repeat(n // 8, 1, 1, 1).contiguous()
    labels = torch.tensor([(i * 7 + 1) % 2 for i in range(n)])
    sd = orc.empty_state_dict(ARCH)
    synth.fill_state_dict(sd)
    params = []
    for k, v in sd.items():
        if v.is_floating_point() and "running" not in k and not k.startswith(("fc_image", "upconv", "seg_out")):
            v.requires_grad_()
            params.append(v)
    opt = torch.optim.Adam(params, lr=5e-4, weight_decay=1e-4)

    def micro_step(a, scale=1.0):
        sl = slice(a * micro, (a + 1) * micro)
        (orc.tile_step_loss(sd, x[sl], labels[sl], ARCH) * scale).backward()

    if os.environ.get("CELLSEG_CPU_THREADS"):
        cands = [max(1, int(os.environ["CELLSEG_CPU_THREADS"]))]
    else:
        cands = sorted({t for t in (16, 32, 64, cores) if t <= cores} or {cores})
    sweep = {}
    for t in cands:
        torch.set_num_threads(t)
        opt.zero_grad()
        micro_step(0)                                   # warm-up at this thread count (allocator, oneDNN primitives)
        t0 = time.perf_counter()
        micro_step(1)
        sweep[t] = round(micro / (time.perf_counter() - t0), 3)
    best = max(sweep, key=sweep.get)
    torch.set_num_threads(best)
    times = []
    for it in range(steps):
        t0 = time.perf_counter()
        opt.zero_grad()
        for a in range(accum):
            micro_step(a, micro / n)
        opt.step()
        times.append(time.perf_counter() - t0)
    t = sorted(times)[len(times) // 2] if len(times) % 2 else min(times)
    return {"value": round(n / t, 3), "unit": "tiles/s", "cores": best, "threads": best, "physical_cores": cores, "kind": "port",
            "cpu_model": model_name,
            "thread_sweep_tiles_per_s": {str(k): v for k, v in sweep.items()},
            "sample": f"thread sweep {cands} on one micro-batch of {micro} tiles (fwd+bwd) each, then {steps} full steps at the best "
                      f"({best} threads): bag of {n} tiles as {accum} x {micro} + Adam, ResNet-50 tile fp32",
            "s_per_step": round(t, 3)}


def cpu_baseline_c1(steps=5):
    """BASELINE.json configs[0] on the host cores: the ResNet-18 image counter step (batch 8, CE + MSE, BN train, Adam) through the
    oracle -- the reference's own CPU-runnable case, timed for tools/bench_configs.py's `c1cpu` line (part of the cpu_baseline leg:
    the only place outside tests/ and smoke() that may run the oracle)."""
    from oracle import cellseg_oracle as orc
    model_name, cores = _host_cpu()
    xc = synth.normalise(synth.ihc_tiles(8, 299, 1234))
    cnt = torch.tensor([0, 3, 12, 40, 1, 7, 25, 230]).float()
    cl = torch.tensor([0, 1, 3, 4, 1, 2, 4, 6])
    sd = orc.empty_state_dict("resnet18")
    synth.fill_state_dict(sd)
    params = []
    for k, v in sd.items():
        if v.is_floating_point() and "running" not in k and not k.startswith(("fc_tile", "upconv", "seg_out")):
            v.requires_grad_()
            params.append(v)
    opt = torch.optim.Adam(params, lr=8e-5, weight_decay=1e-4)

    def one():
        t0 = time.perf_counter()
        opt.zero_grad()
        orc.image_step_loss(sd, xc, cl, cnt, "resnet18")[2].backward()
        opt.step()
        return time.perf_counter() - t0

    # the same thread sweep as cpu_baseline(): batch 8 does not keep 128 cores busy either
    if os.environ.get("CELLSEG_CPU_THREADS"):
        cands = [max(1, int(os.environ["CELLSEG_CPU_THREADS"]))]
    else:
        cands = sorted({t for t in (8, 16, 32, 64, cores) if t <= cores} or {cores})
    sweep = {}
    for tcount in cands:
        torch.set_num_threads(tcount)
        one()                                           # warm-up at this thread count
        sweep[tcount] = round(8 / min(one(), one()), 2)
    best = max(sweep, key=sweep.get)
    torch.set_num_threads(best)
    ts = [one() for _ in range(steps)]
    t = sorted(ts)[len(ts) // 2]
    return {"value": round(8 / t, 2), "unit": "images/s", "cores": best, "threads": best, "physical_cores": cores, "kind": "port",
            "cpu_model": model_name, "thread_sweep_images_per_s": {str(k): v for k, v in sweep.items()},
            "sample": f"thread sweep {cands} (best of 2 steps each), then the median of {steps} steps at the best ({best} threads): "
                      f"ResNet-18 image counter B=8 fp32", "s_per_step": round(t, 4)}


def fp32_parity_mode_rate(dev, x, labels, steps=5, warmup=2):
    """The same step in fp32 PARITY mode (exact-f32 MFMA, fp32 activations: the mode in which tests/test_model_parity_gpu.py proves
    the 1e-4 agreement with the reference's vectors), outside the timed region: SURVEY section 7 hard part (ii) asks for both numbers
    side by side.  Never `value`."""
    model = build_model(dev, torch.float32)
    params = [p for p in model.parameters() if p.requires_grad]
    opt = torch.optim.Adam(params, lr=5e-4, weight_decay=1e-4, fused=True)

    def step():
        opt.zero_grad(set_to_none=True)
        loss = HF.cross_entropy(model(x, freeze_bn=True), labels, 1.0)
        loss.backward()
        opt.step()

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    return {"value": round(BAG / dt, 2), "unit": "tiles/s", "ms_per_step": round(dt * 1e3, 3), "steps": steps, "dtype": "fp32",
            "note": "fp32 activations + v_mfma_f32_32x32x2_f32 (first-generation kernels); the mode of the 1e-4 parity tests"}


def secondary_configs(timeout_s=240):
    """N = 1 only, outside the timed region: short runs of the other BASELINE.json configs (C1, C4 EfficientNet-B3, C5 segmentation at 299
    and 512; C1 / C4 / C5 both enqueued from Python and replayed as one HIP graph -- the EfficientNet step is ~1900 launches, and once its
    GPU time fell to 17 ms the eager figure became the HOST's on boxes that need longer than that to enqueue them) in a CHILD process (tools/bench_configs.py: its own models and allocator; started, never exec'd),
    so that the driver's record carries their throughput and the roofline of their dominant conv kernel next to the headline.
    Never `value`."""
    import subprocess
    env = dict(os.environ, STEPS="6", ROOFLINE="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_configs.py"), "c1", "c1api", "c4", "c4g", "c5", "c5g", "c5x"], capture_output=True, text=True,
                       timeout=timeout_s, env=env, cwd=ROOT)
    out = []
    for line in r.stdout.splitlines():
        if line.startswith("{"):
            try:
                out.append(json.loads(line))
            except ValueError:
                pass
    if r.returncode != 0 and not out:
        return {"error": (r.stderr or "")[-300:]}
    return out


def _rccl_debug_env():
    """Ask RCCL for its INIT / TUNING log lines in a per-process file (before the communicator exists), unless the caller already
    configured NCCL_DEBUG.  Returns the file of THIS process or None."""
    if os.environ.get("NCCL_DEBUG_FILE"):
        return os.environ["NCCL_DEBUG_FILE"]
    import tempfile
    path = os.path.join(tempfile.gettempdir(), f"cellseg_rccl_{os.getpid()}.log")
    os.environ["NCCL_DEBUG"] = "INFO"
    os.environ["NCCL_DEBUG_SUBSYS"] = "INIT,TUNING,GRAPH"
    os.environ["NCCL_DEBUG_FILE"] = path
    return path


def _parse_rccl_log(path, max_lines=12):
    """nranks, channel count and the (algorithm, protocol) lines RCCL printed for its collectives: whatever of it this RCCL build
    writes (the format is RCCL's, so this only pattern-matches and keeps a short excerpt)."""
    import re
    out = {"log": path}
    try:
        lines = open(path, errors="replace").read().splitlines()
    except (OSError, TypeError):
        return out
    algos, excerpt = [], []
    for ln in lines:
        m = re.search(r"nranks\s+(\d+)", ln)
        if m:
            out["nranks_in_log"] = int(m.group(1))
        m = re.search(r"(\d+)\s+coll channels", ln)
        if m:
            out["coll_channels"] = int(m.group(1))
        if re.search(r"algo", ln, re.I) and re.search(r"proto", ln, re.I):
            key = re.sub(r"^.*NCCL INFO\s*", "", ln)
            key = re.sub(r"\b(time|opCount|count|datatype|stream|comm)\b[ =:]*\S+", "", key).strip()
            if key not in algos:
                algos.append(key)
        if any(t in ln for t in ("Connected all", "Init COMPLETE", "Using network", "xgmi", "XGMI", "P2P")) and len(excerpt) < max_lines:
            excerpt.append(re.sub(r"^.*NCCL INFO\s*", "", ln)[:160])
    out["algo_proto"] = algos[:max_lines]
    out["excerpt"] = excerpt
    return out


def _rccl_graph_child(timeout_s=180):
    import subprocess
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--rccl-graph-probe"], capture_output=True, text=True, timeout=timeout_s,
                           cwd=ROOT, env=dict(os.environ))
    except subprocess.TimeoutExpired:
        return {"error": f"child timed out after {timeout_s} s"}
    for line in reversed(r.stdout.splitlines()):
        if line.startswith("{"):
            try:
                return json.loads(line)
            except ValueError:
                break
    return {"error": f"child exited with {r.returncode}: {(r.stderr or '')[-200:]}"}


def rccl_graph_probe(dev, steps=10):
    """Child-process body of `rccl_world1.as_one_hip_graph` (bench.py --rccl-graph-probe): the headline step with the gradient exchange
    on over a one-rank RCCL communicator, captured into one HIP graph -- collectives included -- and replayed."""
    import socket
    import torch.distributed as dist
    from cellsegmentation_amd.graphed import GraphedStep
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", str(port))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    model = build_model(dev, torch.bfloat16)
    params = [p for p in model.parameters() if p.requires_grad]
    opt = Adam(params, lr=5e-4, weight_decay=1e-4, capturable=True)
    x = synth.normalise(synth.ihc_tiles(BAG, SIZE, 1234)).contiguous().to(dev)
    labels = torch.tensor([(i * 7 + 1) % 2 for i in range(BAG)], device=dev)
    red = GradReducer(params, force_collectives=True).attach()
    red.broadcast_parameters(model)

    def step_fn(xb, lb):
        opt.zero_grad(set_to_none=True)
        loss = HF.cross_entropy(model(xb, freeze_bn=True), lb, 1.0)
        loss.backward()
        red.reduce()
        opt.step()
        return loss.detach()

    g = GraphedStep(step_fn, (x, labels), warmup=4, pre_replay=(opt.sync_hyper,))
    xs, ls = g.static_inputs
    g(xs, ls)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        g(xs, ls)
    t_host = (time.perf_counter() - t0) / steps
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    out = {"ms_per_step_with_collectives": round(dt * 1e3, 3), "tiles_per_s": round(BAG / dt, 1), "host_enqueue_ms_per_step": round(t_host * 1e3, 3),
           "buckets_sent_inside_backward": red.launches_in_backward, "capture_error_mode": "thread_local (a process group is alive)"}
    red.detach()
    dist.destroy_process_group()
    return out


def rccl_world1_side(dev, model, params, opt, x, labels, steps=10, warmup=3, use_graph=False):
    """N = 1 only, outside the timed region: the same step with the gradient exchange switched ON over a one-rank RCCL
    communicator (`GradReducer(force_collectives=True)`: 32 MB flat buckets all-reduced from inside the HIP backward on a side
    stream).  A world of one moves no bytes over xGMI, so what this prices is everything else the N > 1 path adds to a step: the
    RCCL kernel launches (ReduceOp.AVG: the 1/world scale happens inside the collective) and the side-stream hand-offs.  With `use_graph` the step -- collectives
    included -- is additionally captured into one HIP graph and replayed (what `bench.py --gpus N --graph` runs).  Never `value`."""
    import socket
    import torch.distributed as dist
    own_pg = not dist.is_initialized()
    if own_pg:
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", str(port))
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        rccl_log = _rccl_debug_env()
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    else:
        rccl_log = os.environ.get("NCCL_DEBUG_FILE")
    red = GradReducer(params, force_collectives=True).attach()
    red.broadcast_parameters(model)

    def step_fn(xb, lb):
        opt.zero_grad(set_to_none=True)
        loss = HF.cross_entropy(model(xb, freeze_bn=True), lb, 1.0)
        loss.backward()
        red.reduce()
        opt.step()
        return loss.detach()

    def run(one, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            one()
        t_host = (time.perf_counter() - t0) / n              # host time to ENQUEUE a step (the GPU may still be running)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n, t_host

    graph_out = None
    try:
        for _ in range(warmup):
            step_fn(x, labels)
        dt, t_host = run(lambda: step_fn(x, labels), steps)
        early = red.launches_in_backward
        aliased = sum(1 for p in params if p.grad is not None and red._slot[id(p)][2] == p.grad.data_ptr())
        red.time_collectives = True
        step_fn(x, labels)
        times = red.collective_times()
        exposed = red.exposed_ms()
        red.time_collectives = False
    finally:
        red.detach()
        if own_pg:
            dist.destroy_process_group()
    if use_graph:
        # the same step captured WITH its collectives, in a CHILD process: a capture with a process group alive can take the process down
        # (the watchdog thread's event queries are illegal inside a global-mode capture: seen once in three runs before GraphedStep
        # switched to thread_local mode there) -- a side number must never be able to do that to the headline line
        graph_out = _rccl_graph_child()
    return {"ms_per_step_with_collectives": round(dt * 1e3, 3), "tiles_per_s": round(BAG / dt, 1), "steps": steps,
            "host_enqueue_ms_per_step": round(t_host * 1e3, 3), "gradients_aliasing_their_bucket": f"{aliased}/{sum(1 for p in params if p.grad is not None)}",
            "buckets": len(red.buckets), "buckets_sent_inside_backward": early,
            "allreduce_ms_per_step": round(sum(t for _, t in times), 4), "exposed_ms": round(exposed, 4),
            "per_bucket": [{"mbytes": round(n / 1e6, 2), "ms": round(t, 4)} for n, t in times],
            "rccl_log": _parse_rccl_log(rccl_log),
            "as_one_hip_graph": graph_out,
            "note": "one-rank RCCL communicator (backend nccl): all-reduce (ReduceOp.AVG) per bucket, event-timed on the side stream; "
                    "top-level figures = eager step, as_one_hip_graph = the same step with its collectives captured and replayed"}


DUMP_SAMPLE = 1 << 21           # elements of the parameter / gradient samples (8 MB each in float32)
DUMP_SEED = 20240229


def dump_outputs(path, loss, logits, params):
    """--dump-outputs: what the last timed step handed its caller -- the loss, the logits of the bag and the model it left behind
    (the updated parameters and their gradients) -- as float32 .npy files.  The trainable tensors hold tens of millions of elements,
    so they are written as one fixed, seeded sample of positions in their concatenation (in `model.parameters()` order); a
    gradient the step did not produce counts as zeros."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    flat_p = torch.cat([p.detach().reshape(-1).float() for p in params])
    flat_g = torch.cat([(p.grad.detach() if p.grad is not None else torch.zeros_like(p)).reshape(-1).float() for p in params])
    total = flat_p.numel()
    idx = np.sort(np.random.default_rng(DUMP_SEED).choice(total, min(DUMP_SAMPLE, total), replace=False))
    idx_dev = torch.from_numpy(idx).to(flat_p.device)
    arrays = {"loss": loss.detach().float().reshape(()).cpu().numpy(),
              "logits": logits.detach().float().cpu().numpy(),
              "params_sample": flat_p[idx_dev].cpu().numpy(),
              "grads_sample": flat_g[idx_dev].cpu().numpy()}
    for name, a in arrays.items():
        np.save(os.path.join(path, name + ".npy"), np.ascontiguousarray(a, dtype=np.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20, help="timed steps (at least 1)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--full", action="store_true",
                    help="also measure everything beside the headline: roofline (per-launch HIP events), CPU baseline, fp32 parity mode, "
                         "one-rank RCCL side run and the other BASELINE configs (N=1), per-bucket all-reduce times (N>1)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's outputs (loss, logits, parameter / gradient samples) as DIR/<name>.npy")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--torch-adam", action="store_true", help="torch.optim.Adam(fused=True) instead of the one-launch HIP Adam (A/B)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-fp32-side", action="store_true", help="skip the fp32 parity-mode side number (N=1, bf16 runs)")
    ap.add_argument("--no-launch-timing", action="store_true", help="skip per-launch HIP events (roofline becomes null)")
    ap.add_argument("--event-every", type=int, default=5, help="HIP-event-bracket the conv launches of every Nth timed step (1 = all)")
    ap.add_argument("--no-rccl-side", action="store_true", help="skip the one-rank RCCL side run (N=1)")
    ap.add_argument("--no-secondary", action="store_true", help="skip the short runs of the other BASELINE configs (N=1)")
    ap.add_argument("--per-layer", action="store_true", help="also print a per-geometry launch table to stderr (with --full)")
    ap.add_argument("--eager", action="store_true", help="enqueue every step from Python (no HIP graph); the default at N > 1")
    ap.add_argument("--graph", action="store_true", help="replay the step as one HIP graph at N > 1 too (RCCL collectives captured)")
    ap.add_argument("--rccl-graph-probe", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"],
                    help="nccl = RCCL over xGMI (default); gloo only to rehearse the N>1 path on a box with fewer GPUs than ranks")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    # stdout carries ONE JSON line and nothing else: RCCL prints a version banner to stdout when a communicator is created, child
    # processes and libraries may print too -- file descriptor 1 points at stderr until the line itself is written
    sys.stdout.flush()
    saved_stdout = os.dup(1)
    os.dup2(2, 1)

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: launch as `python bench.py --gpus N` (it starts "
                         f"the N ranks itself) or under torchrun with --nproc-per-node equal to --gpus")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the HIP hot path has no CPU fallback")
    n_dev = torch.cuda.device_count()
    if world > 1 and args.backend == "nccl" and local_rank >= n_dev:
        raise SystemExit(f"rank {rank}: LOCAL_RANK {local_rank} but only {n_dev} GPU(s) visible")
    dev_index = local_rank % max(1, n_dev)
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    rccl_log = None
    if world > 1:
        import torch.distributed as dist
        if args.backend == "nccl":
            rccl_log = _rccl_debug_env() if args.full else None
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group("gloo")
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    if args.rccl_graph_probe:
        res = rccl_graph_probe(dev)
        sys.stdout.flush()
        os.dup2(saved_stdout, 1)
        print(json.dumps(res), flush=True)
        return

    model = build_model(dev, dtype)
    params = [p for p in model.parameters() if p.requires_grad]
    # the Adam update the reference constructs (train_tile.py:282) as ONE HIP launch (cellsegmentation_amd.optim.Adam, csrc/optim.hip;
    # tests/test_optim_gpu.py holds it to torch.optim.Adam step by step); --torch-adam: torch's own fused implementation (5 launches)
    # The step is replayed as ONE HIP graph (graphed.GraphedStep; tests/test_graphed_gpu.py: bit-for-bit the eager step) at N = 1:
    # ~220 launches cost 6 ms of Python + ctypes per step against ~7 ms of GPU work, so the eager step is within a few percent of
    # host-bound.  At N > 1 the eager path is the default (the captured-RCCL path has never run on more than one rank; --graph).
    use_graph = not args.eager and not args.torch_adam and (world == 1 or args.graph)
    opt = (torch.optim.Adam(params, lr=5e-4, weight_decay=1e-4, fused=True) if args.torch_adam
           else Adam(params, lr=5e-4, weight_decay=1e-4, capturable=use_graph))
    reducer = GradReducer(params).attach() if world > 1 else None       # buckets leave from inside the HIP backward
    if reducer is not None:
        reducer.broadcast_parameters(model)

    # synthetic IHC tiles: 64 distinct ones per rank (inputs resident in HBM)
    x = synth.normalise(synth.ihc_tiles(BAG, SIZE, 1234 + rank)).contiguous().to(dev)
    labels = torch.tensor([(i * 7 + 1) % 2 for i in range(BAG)], device=dev)
    loss_acc = torch.zeros((), device=dev)

    def step_fn(xb, lb):
        opt.zero_grad(set_to_none=True)
        out = model(xb, freeze_bn=True)
        loss = HF.cross_entropy(out, lb, 1.0)
        loss.backward()
        if reducer is not None:
            reducer.reduce()
        opt.step()
        loss_acc.add_(loss.detach())
        return loss.detach(), out.detach()

    last = [None]                                   # (loss, logits) of the latest step: what --dump-outputs writes

    def step():
        last[0] = step_fn(x, labels)

    gstep = None
    if use_graph:
        from cellsegmentation_amd.graphed import GraphedStep
        # W warm-up steps in all: W - 1 eager ones inside GraphedStep (the capture itself executes nothing), then one replay
        gstep = GraphedStep(step_fn, (x, labels), warmup=max(1, args.warmup - 1), pre_replay=(opt.sync_hyper,))
        if args.warmup >= 2:
            gstep(x, labels)
    else:
        for _ in range(args.warmup):
            step()

    def barrier():
        if world > 1:
            import torch.distributed as dist
            dist.barrier()

    # the per-launch events only serve the roofline, a --full figure: a plain run times the bare steps
    timer = K.LaunchTimer() if args.full and not args.no_launch_timing else None
    barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    # Eager mode: per-launch HIP events (two per conv-family launch, ~380 per step) cost ~1 ms of host time per step; they bracket the
    # launches of every `--event-every`-th timed step only, so the roofline is measured inside the timed region while `value` is
    # not taxed by its own instrumentation.
    # Graph mode: the K timed steps are K replays; a replay has no host-visible launches to bracket, and an eager step enqueued behind replays measured host-bound
    # (9 ms: the GPU drained before its first launch arrived), so the event-bracketed steps -- bit-identical eager steps of the same
    # trajectory (tests/test_graphed_gpu.py) -- run IMMEDIATELY AFTER the timed region (`roofline.event_steps_in_timed_region`);
    # rocprofv3 sees the kernels inside the replays, and its per-kernel averages are what tools/check_bench_vs_profile.py compares.
    timed_steps = 0
    host_by_kind = {"graph": [0.0, 0], "eager": [0.0, 0]}
    n_event_steps = 0 if timer is None else max(1, args.steps // max(1, args.event_every))
    if gstep is not None:
        # (inputs resident in HBM, as the contract asks: the captured input buffers ARE the batch -- GraphedStep skips the copy; a
        # training loop that brings a new batch per step adds a 68 MB device copy, 0.04 ms)
        xs, ls = gstep.static_inputs
        for _ in range(args.steps):
            h0 = time.perf_counter()
            last[0] = gstep(xs, ls)
            host_by_kind["graph"][0] += time.perf_counter() - h0
            host_by_kind["graph"][1] += 1
    elif timer is not None:
        with timer:
            for i in range(args.steps):
                timer.enabled = (i % args.event_every) == 0
                timed_steps += int(timer.enabled)
                h0 = time.perf_counter()
                step()
                host_by_kind["eager"][0] += time.perf_counter() - h0
                host_by_kind["eager"][1] += 1
    else:
        for _ in range(args.steps):
            h0 = time.perf_counter()
            step()
            host_by_kind["eager"][0] += time.perf_counter() - h0
            host_by_kind["eager"][1] += 1
    host_enqueue = time.perf_counter() - t0          # host time to enqueue the K steps (diagnostic: host- or GPU-bound)
    torch.cuda.synchronize()
    barrier()
    elapsed = time.perf_counter() - t0
    if world > 1:
        import torch.distributed as dist
        tt = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt.item())
    if args.dump_outputs and rank == 0:
        # before any step outside the timed region (roofline, RCCL side runs) moves the model on
        dump_outputs(args.dump_outputs, last[0][0], last[0][1], params)

    events_in_region = gstep is None
    if gstep is not None and timer is not None:
        step()                                           # (one unbracketed eager step: the queue is full again when the events start)
        with timer:
            for _ in range(n_event_steps):
                step()
                timed_steps += 1
        torch.cuda.synchronize()

    # N > 1: one more step (outside the timed region, on every rank -- it is a collective) with each bucket's all-reduce and the
    # compute stream's final wait bracketed by events, so that the first multi-GPU line explains itself
    rccl_info = None
    if reducer is not None and args.full:
        reducer.time_collectives = True
        step()
        times = reducer.collective_times()
        exposed = reducer.exposed_ms()
        reducer.time_collectives = False
        rccl_info = {"nranks": world, "backend": args.backend, "buckets": len(reducer.buckets),
                     "buckets_sent_inside_backward": reducer.launches_in_backward,
                     "allreduce_ms_per_step": round(sum(t for _, t in times), 4), "exposed_ms": round(exposed, 4),
                     "per_bucket": [{"mbytes": round(n / 1e6, 2), "ms": round(t, 4)} for n, t in times],
                     "log": _parse_rccl_log(rccl_log) if rccl_log else None}

    if rank == 0:
        final_loss = float(loss_acc.item()) / max(1, args.steps + args.warmup + (1 if rccl_info is not None else 0) + ((1 + n_event_steps) if (gstep is not None and timer is not None) else 0))
        roof = roofline_from(timer.results(), timed_steps, dtype) if timer is not None else None
        if roof is not None:
            roof["event_timed_steps"] = timed_steps
            roof["event_steps_in_timed_region"] = events_in_region
        if timer is not None and args.per_layer:
            print(per_layer_table(timer.results(), timed_steps, dtype), file=sys.stderr)
        rccl_side = None
        if world == 1 and args.full and not args.no_rccl_side:
            try:
                rccl_side = rccl_world1_side(dev, model, params, opt, x, labels, use_graph=use_graph)
            except Exception as e:  # noqa: BLE001 -- a side number must never take the headline line down
                rccl_side = {"error": f"{type(e).__name__}: {e}"[:300]}
        secondary = None
        if world == 1 and args.full and not args.no_secondary:
            try:
                secondary = secondary_configs()
            except Exception as e:  # noqa: BLE001
                secondary = {"error": f"{type(e).__name__}: {e}"[:300]}
        cpu = None
        if world == 1 and args.full and not args.no_cpu_baseline:
            cpu = cpu_baseline()
        fp32_side = None
        if world == 1 and args.full and args.dtype == "bf16" and not args.no_fp32_side:
            fp32_side = fp32_parity_mode_rate(dev, x, labels)
        out = {
            "metric": "tiles/sec fwd+bwd (ResNet-50 MIL, 299x299)",
            "value": round(world * BAG * args.steps / elapsed, 2),
            "unit": "tiles/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 3),
            "host_enqueue_ms_per_step": round(host_enqueue / args.steps * 1e3, 3),
            "host_enqueue_detail": {k: {"steps": v[1], "ms_per_step": round(v[0] / v[1] * 1e3, 3)} for k, v in host_by_kind.items() if v[1]},
            "step_mode": (("one HIP graph per step (graphed.GraphedStep replay; the batch sits in the captured input buffers) for all K timed steps"
                           + (f"; `roofline` from {n_event_steps} HIP-event-bracketed eager steps of the same trajectory right after the timed region"
                              if timer is not None else ""))
                          if gstep is not None else
                          "eager (every launch enqueued from Python" + (f"; every {args.event_every}th timed step event-bracketed)" if timer is not None else ")")),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": args.dtype,
            "data": "synthetic",
            "config": {"workload": "ResNet-50 tile classifier (train_tile.py --scratch semantics: fwd + CE + full bwd + Adam), "
                                   "bag=64 tiles of 299x299x3 per GPU, freeze_bn=True", "tiles_per_gpu": BAG,
                       "parallelism": f"dp{world}", "mean_loss": round(final_loss, 5)},
            "roofline": roof,
            "cpu_baseline": cpu,
            "fp32_parity_mode": fp32_side,
            "rccl": rccl_info,
            "rccl_world1": rccl_side,
            "secondary": secondary,
        }
        sys.stdout.flush()
        os.dup2(saved_stdout, 1)
        print(json.dumps(out), flush=True)
        os.dup2(2, 1)
    if world > 1:
        import torch.distributed as dist
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
