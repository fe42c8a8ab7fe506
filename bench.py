"""bench.py -- images/sec of one `train_hallucidet` step (Faster R-CNN, LLVIP geometry 512x640, batch 8 / GPU, fp16) on
N MI355X of one node, one process per GPU (RCCL all-reduce of the hallucination-net gradients), synthetic inputs already
resident in HBM.  Prints ONE JSON line (rank 0).

    python bench.py --gpus 1 --steps 20 --warmup 5
    python bench.py --gpus 1 --steps 20 --warmup 5 --full
    python bench.py --gpus 1 --steps 20 --warmup 5 --dump-outputs DIR
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

A plain run sets up, warms up, times `--steps` steps and prints the line (`value`, `ms_per_step`, ...): nothing else.  `--full` adds
the measurements that take runs of their own, after the timed steps (rank 0, N=1 where noted): the PCIe-inclusive rate, the
`roofline` object and the `cpu_baseline` object below (`--no-roofline` / `--no-cpu-baseline` leave one of them out).
`--dump-outputs DIR`: after the timed steps, what the last of them computed -> DIR/<name>.npy (float32 / float64, a fixed seeded
sample of the parameter and gradient arenas; the inputs are the same seeded synthetic batch in every run), so that two builds can be
compared output for output.

`roofline`: the dominant kernel is the convolution behind hd_conv2d (the conv_igemm / conv3x3_w8 / conv3x3_small kernels: every
conv / data-gradient / FC of the U-Net and the detector).  `achieved` = algorithmic FLOPs of the launches of ONE real
training step / the duration of those launches replayed once each, in step order, between HIP events on the launch stream -- the
number a rocprofv3 kernel summary of the step reproduces; `achieved_isolated` re-issues every launch 5x back to back (warm caches:
the upper bound the first round quoted).  `mfma_util` / `traffic` come from the rocprofv3 PMC passes committed under profiles/.
`cpu_baseline`: the CPU oracle (oracle/step.py, "port") on this host's cores (rank 0, N=1 only): batch 8, all cores, one warm-up
(batch 2) + one timed step, plus the U-Net alone at the reference's 8 threads -- bounded so that a `--full` run stays within
minutes; `--cpu-protocol full` runs SURVEY 8d's protocol (2 warm-ups + 3 timed steps at batch 8, 8 threads and all cores).
Other BASELINE configs: `--config retinanet16` (configs[3]) and `--config detector16` (configs[4]) print their own lines.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

MFMA_F16_PEAK_TFLOPS = 2500.0     # dense fp16 MFMA peak, /opt/skills/guides/MI355X_MICROARCH.md
MFMA_F32_PEAK_TFLOPS = 157.3      # f32-input MFMA (v_mfma_f32_32x32x2_f32) = the f32 vector rate, same guide ("Peak FP32 (matrix)")
BATCH_PER_GPU = 8
H, W = 512, 640


def _profile_json(names):
    for n in names:
        try:
            return json.load(open(os.path.join(ROOT, "profiles", n)))
        except Exception:
            continue
    return None


def _stale(j):
    """True when the PMC summary was collected on another build of the HIP sources (hallucidet_amd.build.source_digest)."""
    from hallucidet_amd.build import source_digest
    return j.get("csrc_digest") != source_digest()


def _pmc_traffic():
    """HBM bytes per launch of the dominant kernel from the rocprofv3 PMC passes (FETCH_SIZE / WRITE_SIZE in two separate
    runs, corrected as MI355X_MICROARCH.md prescribes; tools/pmc_traffic.py) committed under profiles/ for this round.
    bench.py itself cannot collect PMCs (they need rocprofv3 around the process): null if the file is absent."""
    for name in ("r06_conv_traffic.json", "r05_conv_traffic.json", "r04_conv_traffic.json", "r03_conv_traffic.json", "r02_conv_traffic.json", "r01_conv_traffic.json"):
        j = _profile_json([name])
        try:
            return round(j["traffic_bytes_per_launch"]), {"static": True, "stale": _stale(j), "source": "profiles/" + name, "commit": j.get("commit"),
                                                          "note": "PMC counters need rocprofv3 around the process: collected by tools/collect_profiles.sh, NOT measured in this run"}
        except Exception:
            continue
    return None, None


def _pmc_mfma_util():
    """MFMA-pipe utilisation of the conv kernels in a training step (SQ_VALU_MFMA_BUSY_CYCLES / (4 SIMDs x 256 CUs x busy
    clocks), tools/pmc_mfma.py on a `rocprofv3 --pmc` run of tools/bench_step.py), committed under profiles/."""
    for name in ("r06_conv_mfma_util.json", "r05_conv_mfma_util.json", "r04_conv_mfma_util.json", "r03_conv_mfma_util.json", "r02_conv_mfma_util.json"):
        j = _profile_json([name])
        try:
            return {"value": j["mfma_util"], "by_kernel": j.get("by_kernel"), "static": True, "stale": _stale(j), "source": "profiles/" + name, "commit": j.get("commit"),
                    "note": "NOT measured in this run (PMC pass of tools/collect_profiles.sh)"}
        except Exception:
            continue
    return None


def _cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except Exception:
        pass
    return "unknown CPU"


def _flush_c_stdio():
    """fflush(NULL): text that native libraries (RCCL's banner) wrote through C stdio leaves the process now, not after our JSON line."""
    try:
        import ctypes
        ctypes.CDLL(None).fflush(None)
    except Exception:
        pass


DUMP_SAMPLE = 1 << 22            # elements kept of an arena larger than this (4 Mi fp32 = 16 MiB per array)
DUMP_LIMIT_BYTES = 64 << 20


def _sample(flat, idx):
    """A fixed sample of a flat tensor (`idx`: _sample_index of its size, None = all of it) -> float32 numpy."""
    flat = flat.detach().reshape(-1)
    if idx is not None:
        flat = flat[idx.to(flat.device)]
    return flat.float().cpu().numpy()


def _sample_index(n, seed=0):
    """DUMP_SAMPLE seeded positions out of n, ascending (the same in every run on an arena of n elements); None when n fits."""
    if n <= DUMP_SAMPLE:
        return None
    return torch.randperm(n, generator=torch.Generator().manual_seed(seed))[:DUMP_SAMPLE].sort().values


def dump_outputs(dirname, loss, arena, buffers=()):
    """--dump-outputs: what the last timed step computed -> DIR/<name>.npy.  `loss`: the value fit_step returned (float64);
    `params` / `grads`: the same seeded sample of the parameter arena after the update and of the (loss-scaled) gradient arena the
    update consumed; `buffers`: the floating-point buffers (BatchNorm running statistics) after the step, concatenated."""
    import numpy as np
    idx = _sample_index(arena.flat_params.numel())
    arrays = {"loss": np.array([float(loss)], dtype=np.float64),
              "params": _sample(arena.flat_params, idx), "grads": _sample(arena.flat_grads, idx)}
    bufs = [b.detach().reshape(-1).float() for b in buffers if b.is_floating_point()]
    if bufs:
        arrays["buffers"] = torch.cat(bufs).cpu().numpy()
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_LIMIT_BYTES:
        raise SystemExit("--dump-outputs: %d bytes exceed the %d-byte limit" % (total, DUMP_LIMIT_BYTES))
    os.makedirs(dirname, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(dirname, name + ".npy"), a)


def conv_roofline(lit, batch, reps=5, peak=None):
    """Record every hd_conv2d launch of one (eager) training step, then time the recorded launches back to back."""
    import ctypes as C
    from hallucidet_amd import _abi, ops
    lib = _abi.load()
    PEAK = peak or MFMA_F16_PEAK_TFLOPS
    f32_mode = PEAK != MFMA_F16_PEAK_TFLOPS
    rec = []
    orig = ops.conv2d

    def spy(x, w, KH, KW, **kw):
        out = orig(x, w, KH, KW, **kw)
        y = out[0] if isinstance(out, tuple) else out
        C1 = x.shape[3]
        C2 = 0 if kw.get("x2") is None else kw["x2"].shape[3]
        if kw.get("out_nchw_f32"):
            n, co, ho, wo = y.shape
        else:
            n, ho, wo, co = y.shape
        pooled = kw.get("pool2") is not None and kw["pool2"].get("done")
        if pooled:      # out_pool2: y is the 2x2 sum-pooled upsampled half; the convolution still computes every output of the full map
            ho, wo, co = 2 * ho, 2 * wo, (kw.get("cout") or w.shape[0])
        dil = kw.get("in_dil", 1)
        # algorithmic FLOPs: a data-gradient over a zero-dilated input only multiplies the non-zero taps
        flops = 2.0 * n * ho * wo * co * KH * KW * (C1 + C2) / (dil * dil)
        # algorithmic bytes: every operand once (x, x2, w, y, residual, mask)
        es = x.element_size()          # 2 (fp16 storage) or 4 (--precision 32)
        by = x.numel() * es + (0 if kw.get("x2") is None else kw["x2"].numel() * es) + w.numel() * es + y.numel() * y.element_size()
        if pooled and kw["pool2"].get("skip") is not None:
            by += kw["pool2"]["skip"].numel() * es
        by += sum(t.numel() * es for t in (kw.get("res"), kw.get("mask")) if t is not None)
        rec.append(({k_: v_ for k_, v_ in kw.items() if k_ != "_defer"}, (x, w, KH, KW), flops, by, where[0]))
        return out

    # weight-gradient launches of the hallucination network (hd_wgrad): part of its "conv blocks" (BASELINE north_star)
    wrec = []
    orig_wg = ops.wgrad

    wg_flops = lambda x, dy, KH, KW, kw: 2.0 * dy.shape[0] * dy.shape[1] * dy.shape[2] * dy.shape[3] * KH * KW * (x.shape[3] + (0 if kw.get("x2") is None else kw["x2"].shape[3]))
    in_multi = [False]

    def spy_wg(x, dy, KH, KW, **kw):
        out = orig_wg(x, dy, KH, KW, **kw)
        if not in_multi[0]:          # (the entries of a multi-layer grid are recorded as ONE launch below)
            wrec.append(("one", (x, dy, KH, KW), {k_: v_ for k_, v_ in kw.items() if k_ != "_defer"}, wg_flops(x, dy, KH, KW, kw)))
        return out

    # several layers' weight gradients as one grid (hd_wgrad_multi: the U-Net backward's deferred 3x3 layers) -- replayed as that one grid
    orig_wgm = ops.wgrad_multi

    def spy_wgm(calls):
        in_multi[0] = True
        try:
            out = orig_wgm(calls)
        finally:
            in_multi[0] = False
        wrec.append(("multi", calls, None, sum(wg_flops(x, dy, KH, KW, kw) for x, dy, KH, KW, kw in calls)))
        return out

    where = ["detector"]
    rr = lit.encoder_decoder.runner
    o_fwd, o_bwd = rr.forward, rr.backward

    def tag(fn):
        def g(*a, **k):
            where[0] = "unet"
            try:
                return fn(*a, **k)
            finally:
                where[0] = "detector"
        return g
    rr.forward, rr.backward = tag(o_fwd), tag(o_bwd)
    ops.conv2d = spy
    ops.wgrad = spy_wg
    ops.wgrad_multi = spy_wgm
    import hallucidet_amd.models.detection as det_mod
    import hallucidet_amd.segmentation_models.unet as unet_mod
    r = lit.encoder_decoder.runner
    was, was_det = r.use_graphs, lit.use_detector_graph
    r.enable_graphs(False)
    lit.use_detector_graph = False          # the recording step is issued eagerly (a graph replay calls no Python wrapper)
    try:
        lit.fit_step(batch)
        torch.cuda.synchronize()
    finally:
        ops.conv2d = orig
        ops.wgrad = orig_wg
        ops.wgrad_multi = orig_wgm
        rr.forward, rr.backward = o_fwd, o_bwd
        r.enable_graphs(was)
        lit.use_detector_graph = was_det
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    tot_ms, tot_fl, tot_by = 0.0, 0.0, 0.0
    roof_ms, hbm_bound = 0.0, 0                      # every launch at ITS binding roof (MFMA peak or 8 TB/s)

    # STEP-ORDER replay: every recorded launch ONCE, in the order of the step, on its own operands (each launch finds its inputs as
    # cold in L2 as in the step: 257 different tensors, ~9 GB per pass), one event pair around each group's sequence.  This is
    # what a rocprofv3 kernel summary of the training step reproduces (profiles/README.md); re-issuing one launch 5x back to back
    # (`*_isolated`) reads 10-15 % faster.
    def replay(items, call, passes=3):
        # captured in a hipGraph: issued from Python the 257 launches are host-bound (~35 us per ctypes call), which is not what
        # the step (itself replayed from graphs) or a rocprofv3 kernel summary sees
        for it in items:
            call(it)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for it in items:
                call(it)
        g.replay()
        torch.cuda.synchronize()
        e0.record()
        for _ in range(passes):
            g.replay()
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1) / passes
        del g
        return ms
    def iso_time(call):
        """One launch `reps` times back to back, captured in a hipGraph (issued from Python a 5-us kernel is host-bound)."""
        call()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(reps):
                call()
        g.replay()
        e0.record()
        g.replay()
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1) / reps
        del g
        return ms
    conv_call = lambda it: orig(it[1][0], it[1][1], it[1][2], it[1][3], **it[0])
    grp_step = {k: replay([r_ for r_ in rec if r_[4] == k], conv_call) for k in ("unet", "detector")}
    step_conv_ms = replay(rec, conv_call)
    wg_call = lambda it: orig_wgm(it[1]) if it[0] == "multi" else orig_wg(*it[1], **it[2])
    wg_seq_ms = replay(wrec, wg_call) if wrec else 0.0
    dump = os.environ.get("HD_BENCH_DUMP")
    rows = []
    grp = {"unet": [0.0, 0.0], "detector": [0.0, 0.0]}
    for kw, (x, w, KH, KW), fl, by, origin in rec:
        tot_by += by
        roof_ms += max(fl / (PEAK * 1e12), by / 8e12) * 1e3
        hbm_bound += int(by / 8e12 > fl / (PEAK * 1e12))
        kw = {k_: v_ for k_, v_ in kw.items() if k_ != "_defer"}                                 # same epilogue (bias / res / mask / BN statistics) as in the step
        ms = iso_time(lambda: orig(x, w, KH, KW, **kw))
        tot_ms += ms
        tot_fl += fl
        grp[origin][0] += ms
        grp[origin][1] += fl
        if dump:
            rows.append((ms * 1e3, fl / 1e9, tuple(x.shape), 0 if kw.get("x2") is None else kw["x2"].shape[3], tuple(w.shape), KH,
                         kw.get("stride", 1), kw.get("in_dil", 1), bool(kw.get("up1")), bool(kw.get("want_stats")),
                         kw.get("mask") is not None, kw.get("res") is not None))
    if dump:
        with open(dump, "w") as f:
            for r_ in rows:
                f.write("%8.1f us %8.2f GF %7.1f TF  x=%s c2=%d w=%s k=%d s=%d dil=%d up=%d stats=%d mask=%d res=%d\n"
                        % (r_[0], r_[1], r_[1] / r_[0] * 1e-3 * 1e3, *r_[2:]))
    n = len(rec)
    iso = tot_fl / (tot_ms * 1e-3) / 1e12
    achieved = tot_fl / (step_conv_ms * 1e-3) / 1e12
    wg_ms = wg_fl = 0.0
    for it in wrec:
        wg_ms += iso_time(lambda: wg_call(it))
        wg_fl += it[3]
    tf = lambda fl, ms: round(fl / (ms * 1e-3) / 1e12, 1) if ms > 0 else None
    # groups are IN-STEP times (isolated re-timing in *_isolated_ms)
    wg_s = wg_seq_ms
    u_ms, u_fl = grp_step["unet"] + wg_s, grp["unet"][1] + wg_fl
    groups = {
        "unet_conv_fwd_dgrad": {"ms": round(grp_step["unet"], 3), "tflops": tf(grp["unet"][1], grp_step["unet"]), "isolated_ms": round(grp["unet"][0], 3)},
        "unet_wgrad": {"ms": round(wg_s, 3), "tflops": tf(wg_fl, wg_s), "isolated_ms": round(wg_ms, 3), "kernel": "wgrad3x3_w8_multi_kernel (two multi-layer grids per backward pass) + wgrad_kernel / wgrad3x3_small_kernel",
                       "launches": len(wrec)},
        "unet_conv_blocks_total": {"ms": round(u_ms, 3), "tflops": tf(u_fl, u_ms), "frac": round(u_fl / (u_ms * 1e-3) / 1e12 / PEAK, 4) if u_ms else None,
                                   "gflop_per_image": round(u_fl / 1e9 / BATCH_PER_GPU, 1)},
        "detector_conv": {"ms": round(grp_step["detector"], 3), "tflops": tf(grp["detector"][1], grp_step["detector"]), "isolated_ms": round(grp["detector"][0], 3)},
    }
    return {"bound": "mfma", "groups": groups, "achieved": round(achieved, 2), "achieved_isolated": round(iso, 2), "peak": PEAK,
            "unit": "TFLOP/s", "frac": round(achieved / PEAK, 4), "frac_isolated": round(iso / PEAK, 4),
            "timing": "step-order replay: the 257 hd_conv2d launches of one training step, each once, in step order, captured in one hipGraph and "
                      "replayed between HIP events on the launch stream (3 passes); `*_isolated`: each launch 5x back to back",
            "mfma_util": None if f32_mode else _pmc_mfma_util(), "traffic": None if f32_mode else _pmc_traffic()[0],
            "traffic_provenance": "not collected for the fp32 mode" if f32_mode else _pmc_traffic()[1], "traffic_unit": "HBM bytes per launch (PMC)",
            "alg_bytes_per_launch": round(tot_by / max(n, 1)),
            "kernel": "hd_conv2d_f32: conv_f32_kernel (64 x 64 tiles, v_mfma_f32_32x32x2_f32: exact f32 products and sums; peak = the f32 matrix rate)" if f32_mode else
                      "hd_conv2d: conv_igemm_kernel (4-wave implicit GEMM: conv / dgrad / FC) + gemm_w8_kernel (8-wave 256-row GEMM tiles: box head) + conv3x3_w8_kernel (8-wave patch-staged 3x3) + conv3x3_m160_kernel (160- / 320- / 96-pixel tiles, producer / consumer waves) + "
                      "conv3x3_c64_kernel / conv7x7s2_stem_kernel / conv3x3_cat128to32_kernel / conv3x3_c32to128_kernel (persistent, register-resident weights: "
                      "the 64 -> 64 channel 3x3 layers, the 7x7 stems, decoder block 3) + "
                      "conv3x3_small_kernel (16/32-channel 3x3 layers)", "launches_per_step": n,
            "avg_launch_us": round(step_conv_ms * 1e3 / max(n, 1), 2), "avg_launch_us_isolated": round(tot_ms * 1e3 / max(n, 1), 2),
            "avg_launch_gflop": round(tot_fl / max(n, 1) / 1e9, 3),
            "two_roof_floor_ms": round(roof_ms, 3), "launches_hbm_bound_at_floor": hbm_bound,
            "frac_of_two_roof_floor": round(roof_ms / step_conv_ms, 4) if step_conv_ms else None}


def _usable_cpus():
    """CPUs this process may really use: the affinity mask capped by the cgroup CPU quota (os.cpu_count() reports the host's 256
    hardware threads on the GPU boxes while the container is throttled to a fraction of them: 256 OpenMP threads then spin against
    each other and a step takes ten minutes)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            n = min(n, max(1, int(float(q) / float(per) + 0.5)))
    except (OSError, ValueError):
        try:
            q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                n = min(n, max(1, int(q / per + 0.5)))
        except (OSError, ValueError):
            pass
    return n


def cpu_baseline(protocol):
    """The CPU oracle (oracle/step.py: fp32 torch restatement of the training step, `kind` "port") on this host's cores.
    SURVEY 8d asks for batch 8, 2 warm-ups + >= 3 timed steps, at the reference's 8 threads (src/config/config.py:10-11) and
    at all cores, plus the U-Net alone -- more than ten minutes of CPU time, which the default run cannot afford.  `bounded`
    (default, ~30 s): the thread count is picked by a short sweep of the oracle U-Net on one image (the boxes report more hardware
    threads than the container may use), then one warm-up step (batch 2) and ONE timed full training step on batch 8; the U-Net
    alone (forward + backward, batch 2) is timed at the reference's 8 threads."""
    from hallucidet_amd import synthetic
    from oracle.step import OracleTrainer
    from oracle import unet as ou
    host = _cpu_model()
    usable = _usable_cpus()
    res = {"unit": "images/s", "kind": "port", "protocol": protocol}

    def timed_steps(batch_n, threads, warm, steps, warm_n=None):
        torch.set_num_threads(threads)
        tr = OracleTrainer()
        for _ in range(warm):
            tr.train_step(synthetic.make_batch(warm_n or batch_n, H, W, seed=123, device="cpu"))
        b = synthetic.make_batch(batch_n, H, W, seed=123, device="cpu")
        t0 = time.time()
        for _ in range(steps):
            tr.train_step(b)
        return batch_n * steps / (time.time() - t0)

    def unet_only(batch_n, threads, reps, net=None):
        torch.set_num_threads(threads)
        net = net or ou.Unet(classes=3).train()
        x = torch.rand(batch_n, 3, H, W)
        net(x).mean().backward()                 # warm-up
        t0 = time.time()
        for _ in range(reps):
            net(x).mean().backward()
        return batch_n * reps / (time.time() - t0)

    # thread sweep (a few seconds): powers of two up to the usable count, never beyond 128
    net = ou.Unet(classes=3).train()
    cand = sorted({min(usable, t) for t in (8, 16, 32, 64, 128)})
    sweep = {t: unet_only(1, t, 1, net) for t in cand}
    best = max(sweep, key=sweep.get)
    res["thread_sweep_unet_images_per_s"] = {str(t): round(v, 3) for t, v in sweep.items()}
    if protocol == "full":
        v_all = timed_steps(8, best, 2, 3)
        v_8 = timed_steps(8, 8, 2, 3)
        res.update(value=round(v_all, 4), cores=best, value_8_threads=round(v_8, 4), unet_only_best_threads=round(unet_only(8, best, 3), 4),
                   unet_only_8_threads=round(unet_only(8, 8, 3), 4),
                   sample="SURVEY 8d protocol: batch 8 x 512x640, 2 warm-up + 3 timed full training steps of the CPU oracle at %d threads "
                          "(`value`; best of the sweep, %d CPUs usable) and at the reference's 8 threads; U-Net forward+backward alone "
                          "likewise; host: %s" % (best, usable, host))
    else:
        v = timed_steps(8, best, 1, 3, warm_n=2)
        # the reference's own setting (Config.set_environment: 8 threads, src/config/config.py:10-11): ONE timed full step
        v8 = timed_steps(8, 8, 0, 1) if best != 8 else v
        res.update(value=round(v, 4), cores=best, value_8_threads=round(v8, 4), unet_only_8_threads=round(unet_only(2, 8, 1, net), 4),
                   sample="bounded: THREE timed full training steps of the CPU oracle (oracle/step.py, fp32 torch) on batch 8 x 512x640 at %d "
                          "threads (best of a sweep over %s; %d CPUs usable) after one warm-up step on batch 2; `value_8_threads`: one timed full step at "
                          "the reference's 8 threads (src/config/config.py:10-11); U-Net forward+backward alone on batch 2 at 8 threads; the "
                          "full SURVEY 8d protocol is `--cpu-protocol full`; host: %s" % (best, cand, usable, host))
    torch.set_num_threads(8)          # back to Config.set_environment()'s setting
    return res


def bench_detector_training(args, dev, rank, world):
    """BASELINE configs[4]: train_detector.py (Faster R-CNN, RGB, batch 16/GPU): detector forward + backward with parameter
    gradients for torchvision's trainable set, Adam, all-reduce of those gradients."""
    from hallucidet_amd import synthetic
    from hallucidet_amd.models.detector import Detector
    from hallucidet_amd.train_detector import DetectorLit
    torch.manual_seed(1)
    det = Detector(name="fasterrcnn", pretrained=False, n_classes=2, size=300).detector.to(dev)
    rgb, trgb, _, _ = synthetic.make_batch(BATCH_PER_GPU, H, W, seed=123 + rank, device=dev)
    il, _ = det.transform(rgb[:2], None)
    det.backbone.calibrate_(il.tensors)
    lit = DetectorLit(batch_size=BATCH_PER_GPU, detector=det, pretrained=False, device=dev).prepare()
    for _ in range(args.warmup):
        lit.fit_step((rgb, trgb))
    torch.cuda.synchronize()
    if dist.is_initialized():
        dist.barrier()
        _flush_c_stdio()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = lit.fit_step((rgb, trgb))
    torch.cuda.synchronize()
    if dist.is_initialized():
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    per_rank_ms = None
    if dist.is_initialized():
        mine = torch.tensor([elapsed / args.steps * 1e3], device=dev, dtype=torch.float64)
        allr = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(allr, mine)
        per_rank_ms = [round(float(v), 3) for v in allr]
        t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t)
        # the exchange is ONE plain all-reduce of the trainable arena after the backward pass (no overlap to verify); what a first N > 1
        # run must show is that the ranks hold identical parameters after the timed steps
        p = lit.arena.flat_params
        ref = p.clone()
        dist.broadcast(ref, src=0)
        drift = torch.tensor([float((p - ref).abs().max())], device=dev)
        dist.all_reduce(drift, op=dist.ReduceOp.MAX)
        param_drift = float(drift)
    if not torch.isfinite(loss):
        raise SystemExit("non-finite loss in the timed region")
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, loss, lit.arena)
    if rank == 0:
        print(json.dumps({
            "ms_per_step_by_rank": per_rank_ms, "max_parameter_difference_between_ranks": (param_drift if dist.is_initialized() else None),
            "metric": "images/sec train_detector (640x512 RGB, batch %d/GPU)" % BATCH_PER_GPU, "value": round(BATCH_PER_GPU * world * args.steps / elapsed, 2),
            "unit": "images/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 3),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f16", "data": "synthetic",
            "config": {"workload": "train_detector.py fasterrcnn RGB batch=%d/GPU (BASELINE configs[4], NOT the headline config): Faster R-CNN "
                                   "R50-FPN @300x300 forward + backward with weight gradients (layer2-4, FPN, RPN, RoI heads), Adam" % BATCH_PER_GPU,
                       "global_batch": BATCH_PER_GPU * world, "parallelism": "dp%d" % world},
            "final_loss": round(float(loss), 5), "skipped_steps": lit.optimizer.skipped_steps}), flush=True)
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also measure the PCIe-inclusive rate, the conv roofline and the CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed to DIR/<name>.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU baseline")
    ap.add_argument("--no-roofline", action="store_true", help="--full without the roofline")
    ap.add_argument("--detector", default="fasterrcnn", choices=["fasterrcnn", "retinanet"],
                    help="fasterrcnn = the configuration BASELINE.json's metric is quoted on (default); retinanet = configs[3]")
    ap.add_argument("--batch", type=int, default=0, help="images per GPU (default 8: BASELINE configs[1])")
    ap.add_argument("--config", default="", choices=["", "retinanet16", "detector16"],
                    help="retinanet16 = BASELINE configs[3] (train_hallucidet, RetinaNet, batch 16/GPU); detector16 = configs[4] "
                         "(train_detector.py, Faster R-CNN, RGB, batch 16/GPU).  Not the headline metric: their own JSON lines")
    ap.add_argument("--cpu-protocol", default="bounded", choices=["bounded", "full"])
    ap.add_argument("--precision", type=int, default=16, choices=[16, 32],
                    help="16 = BASELINE configs[1] (the headline); 32 = the reference's default --precision 32: fp32 storage and VALU "
                         "arithmetic end to end (the parity mode, untuned).  Its own JSON line, without the fp16 roofline")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    global BATCH_PER_GPU
    if args.config == "retinanet16":
        args.detector, args.batch = "retinanet", args.batch or 16
    if args.config == "detector16":
        args.batch = args.batch or 16
    if args.batch:
        BATCH_PER_GPU = args.batch

    # `python bench.py --gpus N` started plainly: become the launcher -- N children (one per GPU, the torch.distributed.run
    # environment), rank 0's JSON line relayed.  Nothing in this process has touched the GPU yet, and nothing will.
    from hallucidet_amd import launch
    if launch.need_self_launch(args.gpus):
        # the launcher never asks the runtime about devices (a fallback inside torch.cuda.device_count() can initialise HIP, after
        # which this process may not fork + exec ranks on this pool): a rank whose LOCAL_RANK has no GPU fails at set_device below
        raise SystemExit(launch.launch_ranks(args.gpus))

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    # the reference's scripts start with Config.set_environment() (train_hallucidet.py:7): 8 host threads.  torch's default is one
    # thread per hardware thread of the HOST (256), which a throttled container turns into spinning
    from hallucidet_amd.config import Config
    Config.set_environment()
    if world != args.gpus:           # pure environment validation: before anything touches a device
        raise SystemExit("bench.py --gpus %d was started with WORLD_SIZE=%d: launch it plainly (it starts its own ranks) or with "
                         "torch.distributed.run --nproc-per-node %d" % (args.gpus, world, args.gpus))
    if not (0 <= rank < world and 0 <= local < world):
        raise SystemExit("bench.py: RANK=%d / LOCAL_RANK=%d outside WORLD_SIZE=%d (one node, one rank per GPU)" % (rank, local, world))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (no GPU visible); there is no CPU path")
    if local >= torch.cuda.device_count():
        raise SystemExit("bench.py --gpus %d: rank %d has no GPU (only %d visible)" % (args.gpus, rank, torch.cuda.device_count()))
    torch.cuda.set_device(local)
    force_dist = os.environ.get("HD_FORCE_DIST") == "1"      # exercise the RCCL path on one GPU (world size 1)
    if world > 1 or force_dist:
        # (RCCL writes its NCCL_DEBUG=VERSION banner -- five lines per rank, the pool's images export that variable -- to STDOUT through C
        #  stdio, i.e. at process exit, behind the JSON line: every rank flushes C stdio after the warm-up steps, see _flush_c_stdio)
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        # the gradient arena outlives every collective on it: the allocator need not record the RCCL stream on it (0.1 ms of a 10 ms step at
        # world size 1, tools/probe_dist_host.py)
        os.environ.setdefault("TORCH_NCCL_AVOID_RECORD_STREAMS", "1")
        dist.init_process_group(backend="nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local))

    from hallucidet_amd import synthetic
    dev = "cuda:%d" % local
    if args.config == "detector16":
        return bench_detector_training(args, dev, rank, world)
    lit = synthetic.make_module(seed=123, device=dev, precision=args.precision, detector_name=args.detector)
    batch = synthetic.make_batch(BATCH_PER_GPU, H, W, seed=123 + rank, device=dev)   # per-rank shard, resident in HBM

    overlap_note = None
    if dist.is_initialized() and os.environ.get("HD_OVERLAP_ALLREDUCE", "") != "":
        lit.overlap_allreduce = os.environ["HD_OVERLAP_ALLREDUCE"] != "0"
    elif dist.is_initialized() and (world > 1 or force_dist):
        # (HD_FORCE_DIST=1 runs this branch at world size 1 too -- tests/test_scripts_gpu.py -- so that a multi-GPU run is never its
        #  first execution.)
        # Safety net for the overlapped exchange (bucketed all-reduces issued between the segmented backward graphs): before
        # anything is timed, one step is taken from the same parameters with and without the overlap; the averaged gradients
        # must agree (the reduction order inside RCCL may differ between bucketings: 1e-5 relative), on every rank.  If they
        # do not, the run falls back to the un-overlapped exchange and says so in its line.
        r = lit.encoder_decoder.runner
        p0, m0, v0 = r.flat_params.clone(), lit.optimizer.exp_avg.clone(), lit.optimizer.exp_avg_sq.clone()
        bufs0 = [b.clone() for b in lit.encoder_decoder.buffers()]
        sc0, st0, good0 = lit.optimizer.step_count, lit.scaler.scale_value, lit.scaler._good

        def one_step(ov):
            """One step from the snapshot with the seed reset; -> its averaged gradient.  State (parameters, moments, BN buffers,
            Adam's step count, the scaler's scale / clean-step count / pending update) is put back afterwards."""
            lit.overlap_allreduce = ov
            torch.manual_seed(1000 + rank)
            lit.fit_step(batch)
            torch.cuda.synchronize()
            g = r.flat_grads.clone()
            lit.scaler.resolve()                       # consume this step's overflow flag through the scaler (not behind its back)
            r.flat_params.copy_(p0); lit.optimizer.exp_avg.copy_(m0); lit.optimizer.exp_avg_sq.copy_(v0)
            for b, b0 in zip(lit.encoder_decoder.buffers(), bufs0):
                b.copy_(b0)
            lit.optimizer.step_count, lit.scaler.scale_value, lit.scaler._good, lit.scaler._update_due = sc0, st0, good0, False
            return g
        # The first step of each kind CAPTURES (U-Net graphs per exchange mode, the detector half once): a capture runs eager
        # warm-up bodies that advance the sampler's generator, so it does not draw what a replay from the same seed draws.
        # Both kinds are therefore run once unchecked; the compared pair below is two pure replays from one seed.
        one_step(False)
        one_step(True)
        grads = [one_step(False), one_step(True)]
        err = (grads[0] - grads[1]).norm() / grads[0].norm().clamp(min=1e-30)
        bad = torch.tensor([float(not (err <= 1e-4))], device=dev)
        dist.all_reduce(bad, op=dist.ReduceOp.MAX)
        lit.overlap_allreduce = not bool(bad.item())
        overlap_note = "self-check (two graph replays from one seed): overlapped vs un-overlapped averaged gradient rel-L2 %.2e -> overlap %s" % (float(err), "on" if lit.overlap_allreduce else "OFF (fallback)")
        del grads, p0, m0, v0, bufs0

    for _ in range(args.warmup):
        lit.fit_step(batch)
    torch.cuda.synchronize()
    if dist.is_initialized():
        dist.barrier()
        _flush_c_stdio()               # every rank: RCCL's start-up text (NCCL_DEBUG=VERSION is set on this pool) leaves now, not behind rank 0's line
    torch.cuda.synchronize()
    lit.averager.timing = dist.is_initialized()
    # per-step spread: one HIP event behind every step on the stream the step is issued on (an event record is a marker packet, no
    # synchronisation); the contract's number stays the wall clock around the whole region
    step_ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
    t0 = time.perf_counter()
    step_ev[0].record()
    for k in range(args.steps):
        loss = lit.fit_step(batch)
        step_ev[k + 1].record()
    torch.cuda.synchronize()
    if dist.is_initialized():
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    lit.averager.timing = False
    step_ms = sorted(step_ev[k].elapsed_time(step_ev[k + 1]) for k in range(args.steps))
    pct = lambda q: round(step_ms[min(len(step_ms) - 1, int(q * len(step_ms)))], 3)
    rccl_ranks = dist.get_world_size() if dist.is_initialized() else 1
    per_rank_ms = None
    if dist.is_initialized():
        # every rank's own clock over the timed region (rank 0 prints them: a straggler, a rank that fell back, a slow link show here)
        mine = torch.tensor([elapsed / args.steps * 1e3], device=dev, dtype=torch.float64)
        allr = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(allr, mine)
        per_rank_ms = [round(float(v), 3) for v in allr]
        t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t)
    if not torch.isfinite(loss):
        raise SystemExit("non-finite loss in the timed region")
    lit.optimizer.resolve_found_inf()          # the last timed step's overflow flag (skipped_steps below must include it)
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, loss, lit.encoder_decoder.runner, lit.encoder_decoder.buffers())

    if rank == 0:
        # everything below is rank-0-only measurement: no collective may be issued from here on (the other ranks are
        # already waiting at the final barrier), so the gradient averager is detached for the extra steps
        overlap_used = bool(lit.overlap_allreduce)      # what the TIMED steps ran with (reported below; the extra steps run detached)
        lit.averager.start = lambda g: None
        lit.averager.finish = lambda g, defer_mean=False: 1.0
        lit.averager.bucket_ready = lambda lo, hi: None
        lit.overlap_allreduce = False
        value = BATCH_PER_GPU * world * args.steps / elapsed
        out = {
            "metric": "images/sec train_hallucidet (640x512, batch 8/GPU)",
            "value": round(value, 2), "unit": "images/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 3), "ms_per_step_p50": pct(0.5), "ms_per_step_p90": pct(0.9),
            "ms_per_step_min_max": [round(step_ms[0], 3), round(step_ms[-1], 3)], "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "f16" if args.precision == 16 else "f32", "data": "synthetic",
            "config": {"workload": ("" if args.precision == 16 else "--precision 32 (fp32 storage, NOT the headline configuration) of: ") +
                                   ("train_hallucidet.py fasterrcnn LLVIP batch=8 fp16 on 1xMI355X (BASELINE configs[1]); "
                                    "U-Net resnet34 fwd+bwd, 3 frozen Faster R-CNN R50-FPN passes @300x300 (one batched evaluation of 24 images: trunk, "
                                    "RPN, RoI heads, NMS for all three; the RGB / IR passes' LOSS VALUES, which the reference computes and "
                                    "discards, are not evaluated), loss scaling, value clip 0.5, Adam") if args.detector == "fasterrcnn" else
                                   ("train_hallucidet.py retinanet batch=%d/GPU fp16 (BASELINE configs[3], NOT the headline config); " % BATCH_PER_GPU +
                                    "U-Net resnet34 fwd+bwd, 3 frozen RetinaNet R50-FPN passes @300x300, loss scaling, clip, Adam"),
                       "global_batch": BATCH_PER_GPU * world, "image": "1x512x640 IR + 3x512x640 RGB",
                       "batch_per_gpu": BATCH_PER_GPU,
                       "parallelism": "dp%d" % world, "alg_gflop_per_image": 428.5 if args.detector == "fasterrcnn" else None,
                       "step_alg_tflops": round(428.5e9 * value / 1e12, 1) if args.detector == "fasterrcnn" else None},
            "final_loss": round(float(loss), 5),
            "skipped_steps": lit.optimizer.skipped_steps,       # overflow-skipped optimizer steps in the whole run (must be 0)
            "rccl_ranks": rccl_ranks,                           # dist.get_world_size() of the process group the exchange ran on
        }
        dg = lit.__dict__.get("_det_graph")
        # how the step was issued: the U-Net's forward / segmented backward graphs and the detector half (three passes, losses,
        # backward to the image, post-processing) as hipGraph replays; `detector_replays` counts the timed + warm-up steps
        out["graphs"] = {"unet": bool(lit.encoder_decoder.runner.use_graphs), "detector": bool(dg is not None and dg.usable and dg.replays > 0),
                         "detector_captures": 0 if dg is None else dg.captures, "detector_replays": 0 if dg is None else dg.replays}
        if dist.is_initialized():
            try:
                rccl_version = ".".join(str(v) for v in torch.cuda.nccl.version())
            except Exception as exc:                     # never let a diagnostic cost the line
                rccl_version = "unavailable (%s)" % exc
            out["allreduce"] = {"payload_bytes": int(lit.encoder_decoder.runner.flat_grads.numel()) * 4, "overlap": overlap_used,
                                "note": overlap_note, "rccl_version": rccl_version, "ms_per_step_by_rank": per_rank_ms,
                                "env": {k: os.environ.get(k) for k in ("NCCL_DEBUG", "HSA_ENABLE_IPC_MODE_LEGACY", "NCCL_P2P_DISABLE", "RCCL_MSCCL_ENABLE") if os.environ.get(k) is not None},
                                # per bucket, issue order: the part of its all-reduce the backward pass did not hide (HIP events on
                                # the compute stream around the wait), mean over the timed steps of rank 0
                                "exposed_wait_per_bucket": lit.averager.exposed_wait_ms()}
        if args.full and world == 1:
            # PCIe-inclusive rate (never `value`): every step's batch comes from host memory through the product's input path
            # (hallucidet_amd.dataloader.DevicePrefetcher: uint8 images stacked into pinned memory, copied on a side HIP stream
            # while the previous step computes, divided by 255 on the GPU) -- reference: the DataLoader -> .to(device) of pl.Trainer
            from hallucidet_amd.dataloader.dataloader import DevicePrefetcher
            host = lambda t: [{k: v.cpu() for k, v in d.items()} for d in t]
            u8 = lambda t: list((t * 255.0).round().clamp_(0, 255).to(torch.uint8).cpu())
            hb = (u8(batch[0]), host(batch[1]), u8(batch[2]), host(batch[3]))

            class _HostBatches:
                def __len__(self):
                    return 13

                def __iter__(self):
                    return iter([hb] * 13)
            t1 = None
            for i, db in enumerate(DevicePrefetcher(_HostBatches(), dev)):
                if i == 3:                         # first copies out of freshly pinned pages are not representative
                    torch.cuda.synchronize()
                    t1 = time.perf_counter()
                lit.fit_step(db)
            torch.cuda.synchronize()
            out["pcie_inclusive_images_per_s"] = round(BATCH_PER_GPU * 10 / (time.perf_counter() - t1), 2)
            out["pcie_inclusive_note"] = "uint8 host batch -> pinned -> side-stream H2D overlapped with the previous step (DevicePrefetcher), 10 steps"
            # which protocol `value` follows: the bench contract asks for inputs resident in HBM when the timed region starts; SURVEY 8d
            # words the metric H2D-inclusive -- that rate is the key above, never `value`
            out["value_protocol"] = "inputs resident in HBM (bench contract); H2D-inclusive rate of SURVEY 8d: pcie_inclusive_images_per_s"
        if args.full and not args.no_roofline and args.detector == "fasterrcnn" and BATCH_PER_GPU == 8:
            out["roofline"] = conv_roofline(lit, batch, peak=MFMA_F32_PEAK_TFLOPS if args.precision == 32 else None)
        if args.full and world == 1 and not args.no_cpu_baseline and not args.config:
            out["cpu_baseline"] = cpu_baseline(args.cpu_protocol)
        _flush_c_stdio()               # RCCL's version banner sits in C stdio's buffer when stdout is a pipe: out with it BEFORE the line
        print(json.dumps(out), flush=True)
    if dist.is_initialized():
        dist.barrier()                 # ranks > 0 wait here while rank 0 finishes its roofline / baseline legs
        dist.destroy_process_group()
    _flush_c_stdio()


if __name__ == "__main__":
    main()
