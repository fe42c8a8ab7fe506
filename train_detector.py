"""train_detector.py of the reference (:22-60 setup, :347-420 driver): fine-tune the detector on one modality.

    python train_detector.py --dataset llvip --train <root>/LLVIP --test <root>/LLVIP --detector fasterrcnn --modality rgb --batch 16 --epochs 200 --ext .jpg
"""
import os

import torch

from hallucidet_amd.config import Config
from hallucidet_amd.dataloader import SingleModalDataModule
from hallucidet_amd.train_detector import DetectorLit
from hallucidet_amd.trainer import Trainer


def main(argv=None):
    Config.set_environment()
    args = Config.argument_parser(argv)
    if args.ir_preprocess != "none" and args.modality != "ir":
        raise SystemExit("train_detector.py: --ir-preprocess %s pre-processes infrared images; it needs --modality ir (got --modality %s)"
                         % (args.ir_preprocess, args.modality))
    torch.manual_seed(args.seed)
    dataset = args.dataset or "llvip"
    Config.set_detector(args.detector, train_det=False, pretrained=False, dataset=dataset)
    Config.set_loss_weights(args)
    world, rank, local = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0")), int(os.environ.get("LOCAL_RANK", "0"))
    dev = "cuda:%d" % local
    torch.cuda.set_device(local)
    if world > 1:
        # the gradient arena outlives every collective on it: the allocator need not record the RCCL stream on it (0.1 ms of a 10 ms step at
        # world size 1, tools/probe_dist_host.py)
        os.environ.setdefault("TORCH_NCCL_AVOID_RECORD_STREAMS", "1")
        torch.distributed.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device(dev))
    dm = SingleModalDataModule(dataset, args.train, args.test, batch_size=args.batch, num_workers=args.num_workers, ext=args.ext or ".jpg",
                               seed=args.seed, rank=rank, world_size=world, modality=args.modality, **Config.cache_kwargs(args, dev))
    kw = dict(batch_size=args.batch, lr=1e-4 if args.lr is None else args.lr, detector_name=Config.Detector.name, pretrained=args.pretrained,
              modality=args.modality, directly_coco=args.directly_coco, device=dev, precision=args.precision,
              map_device=args.map_device, ir_preprocess=args.ir_preprocess, **Config.transform_kwargs(args), **Config.miss_rate_kwargs(args))
    if args.save_media:
        from hallucidet_amd.utils.media import MediaWriter
        kw["media"] = MediaWriter(args.save_media, every=args.media_every, offset=1, threshold=args.threshold, max_batches=args.media_max,
                                  rank=rank)
    model = DetectorLit.load_from_checkpoint(args.pre_train_path, **kw) if args.pre_train_path else DetectorLit(**kw)
    model.prepare()
    out_dir = os.path.join("lightning_logs", args.wandb_project, args.wandb_name, "_".join([dataset, args.modality, Config.Detector.name]))
    augment = None
    if args.augment == "reference":
        from hallucidet_amd.dataloader.augment import ReferenceAugmentation
        augment = ReferenceAugmentation(seed=args.seed, rank=rank)
    tr = Trainer(max_epochs=args.epochs, limit_train_batches=args.limit_train_batches, dirpath=out_dir if rank == 0 else None, monitor="val_map",
                 mode="max", early_stopping=("val_map", "max", 5), device=dev, log=print if rank == 0 else (lambda *a: None),
                 train_augment=augment, train_geometry=Config.train_geometry(args, rank))
    tr.fit(model, dm)
    if rank == 0:
        res = tr.test(model, dm)
        print("test:", {k: (v.tolist() if torch.is_tensor(v) else v) for k, v in res.items()})
        if "lamr" in res:
            print("mAP: %.2f  AP@50: %.2f  LAMR: %.2f" % tuple(round(float(res[k]) * 100, 2) for k in ("map", "map_50", "lamr")))
    if model.media is not None:
        model.media.close()
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
