"""CPU side of the device COCO mAP evaluator (hallucidet_amd/metrics/device.py): the rank gather (pack / all_gather / merge) on a
world-2 gloo group, the trainer's pass-through of global results, and the `--map-device` option."""
import os
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _scene(seed, n_img):
    """Per-image lists of different lengths (so the two ranks' padded widths differ)."""
    g = torch.Generator().manual_seed(seed)
    preds, targets = [], []
    for i in range(n_img):
        nd, ng = int(torch.randint(0, 7 + 5 * seed, (1,), generator=g)), int(torch.randint(0, 4 + seed, (1,), generator=g))
        p0, q0 = torch.rand(nd, 2, generator=g) * 100, torch.rand(ng, 2, generator=g) * 100
        preds.append({"boxes": torch.cat([p0, p0 + 1 + torch.rand(nd, 2, generator=g) * 50], 1), "scores": torch.rand(nd, generator=g),
                      "labels": torch.randint(1, 3, (nd,), generator=g)})
        targets.append({"boxes": torch.cat([q0, q0 + 1 + torch.rand(ng, 2, generator=g) * 50], 1), "labels": torch.randint(1, 3, (ng,), generator=g)})
    return preds, targets


def _gather_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from hallucidet_amd.metrics import device as md
    st = md.state_from_lists(*_scene(rank, 3 + 2 * rank), "cpu")
    merged = md.merge_states(md.gather_states(st))
    q.put((rank, {k: v.numpy().copy() for k, v in merged.items()}))
    dist.barrier()
    dist.destroy_process_group()


def test_gather_and_merge_world2_hold_the_union_in_rank_order():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gather_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = {}
    for _ in range(world):
        r, st = q.get(timeout=120)
        res[r] = {k: torch.from_numpy(v) for k, v in st.items()}
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    from hallucidet_amd.metrics import device as md
    want = md.merge_states([md.state_from_lists(*_scene(r, 3 + 2 * r), "cpu") for r in range(world)])
    assert md.state_sizes(want)[0] == 8
    for r in range(world):
        assert set(res[r]) == set(want)
        for k in want:
            assert res[r][k].dtype == want[k].dtype and torch.equal(res[r][k], want[k]), (r, k)


def test_state_packing_round_trip_and_padding():
    from hallucidet_amd.metrics import device as md
    preds, targets = _scene(1, 4)
    st = md.state_from_lists(preds, targets, "cpu")
    N, P, Q = md.state_sizes(st)
    assert N == 4 and P == max(len(p["scores"]) for p in preds) and Q == max(len(t["labels"]) for t in targets)
    for i, (p, t) in enumerate(zip(preds, targets)):
        c, gc = int(st["dc"][i]), int(st["gc"][i])
        assert c == len(p["scores"]) and gc == len(t["labels"])
        assert torch.equal(st["db"][i, :c], p["boxes"].double()) and torch.equal(st["ds"][i, :c], p["scores"].double())
        assert torch.equal(st["dl"][i, :c], p["labels"]) and torch.equal(st["gb"][i, :gc], t["boxes"].double())
        assert not st["db"][i, c:].any() and not st["gb"][i, gc:].any()
    sizes, payload = md.pack_state(st)
    assert sizes.tolist() == [N, P, Q] and payload.numel() == md.payload_bytes(N, P, Q)
    back = md.unpack_state(sizes.tolist(), payload)
    assert all(torch.equal(back[k], st[k]) for k in st)
    empty = md.empty_state("cpu")
    assert md.merge_states([empty, st]) is st


def test_global_results_pass_through_the_rank_mean():
    from hallucidet_amd.metrics.device import GlobalResult
    from hallucidet_amd.trainer import Trainer
    out = {"map_hall": GlobalResult(map=torch.tensor(0.25), map_50=torch.tensor(-1.0)), "map_rgb": {"map": torch.tensor(0.5)}}
    glob = Trainer._global_keys(out)
    assert glob == {"map_hall/map", "map_hall/map_50"}
    assert Trainer._global_keys(GlobalResult(map=torch.tensor(0.1), map_per_class=torch.tensor([0.1, 0.2]))) == {"map"}
    flat = Trainer._flat(out)
    m = Trainer._nanmean_over_ranks(dict(flat, val_loss=(3.0, 2)), passthrough=glob)
    assert m == {"map_hall/map": 0.25, "map_hall/map_50": -1.0, "map_rgb/map": 0.5, "val_loss": 1.5}


def test_map_device_option_parses_and_defaults_to_the_host_evaluator():
    from hallucidet_amd.config import Config
    from hallucidet_amd.metrics import Detection, MeanAveragePrecision
    assert Config.argument_parser([]).map_device == "cpu"
    assert Config.argument_parser(["--map-device", "cuda"]).map_device == "cuda"
    with pytest.raises(SystemExit):
        Config.argument_parser(["--map-device", "tpu"])
    m = MeanAveragePrecision()
    assert m.to("cpu") is m and m.to(torch.device("cpu")) is m
    assert type(Detection().map) is MeanAveragePrecision and type(Detection(device="cpu", class_metrics=True).map) is MeanAveragePrecision
