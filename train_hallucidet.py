"""train_hallucidet.py of the reference (:1-60 setup, :447-548 driver) on the MI355X modules: same flags
(Config.argument_parser), LLVIP / FLIR data modules, fit -> save -> test, the three AP@50 lines of eval_hallucidet.py:180-182.

    python train_hallucidet.py --dataset llvip --train <root>/LLVIP --test <root>/LLVIP --detector fasterrcnn \
        --detector-path detector.bin --batch 8 --precision 16 --epochs 10 --ext .jpg
Multi-GPU: python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 train_hallucidet.py ...
"""
import os

import torch

from hallucidet_amd.config import Config
from hallucidet_amd.dataloader import MultiModalDataModule
from hallucidet_amd.train_hallucidet import EncoderDecoderLit
from hallucidet_amd.trainer import Trainer


def print_ap50(maps, ir_preprocess=None):
    """`ir_preprocess`: the --ir-preprocess name the IR pass ran with; named on its line (None / 'none': the reference's three lines)."""
    g = lambda k, key="map_50": round(float(maps[k][key]) * 100, 2)
    ir = "RGB Detector on IR " if ir_preprocess in (None, "none") else "RGB Detector on IR (%s)" % ir_preprocess
    # --miss-rate: under each AP@50 line the log-average miss rate of the same stream, in percent
    for name, k in ((ir, "map_ir"), ("RGB Detector on RGB", "map_rgb"), ("HalluciDet   on IR ", "map_hall")):
        print(name + " AP@50: ", g(k))
        if "lamr" in maps[k]:
            print(name + " LAMR: ", g(k, "lamr"))


def media_writer(args, rank=0):
    """--save-media DIR -> the MediaWriter of the three scripts (None when the flag is absent): the reference's cadence (every
    --media-every batches at phase 1), --threshold for the detections, at most --media-max batches per split and epoch."""
    if not args.save_media:
        return None
    from hallucidet_amd.utils.media import MediaWriter
    return MediaWriter(args.save_media, every=args.media_every, offset=1, threshold=args.threshold, max_batches=args.media_max, rank=rank)


def main(argv=None):
    Config.set_environment()
    args = Config.argument_parser(argv)
    if args.augment != "none":
        raise SystemExit("train_hallucidet.py: --augment %s is an option of train_detector.py (the reference's HalluciDet training has no "
                         "augmentation); use --augment none" % args.augment)
    torch.manual_seed(args.seed)
    dataset = args.dataset or "llvip"
    Config.set_detector(args.detector, train_det=False, pretrained=args.directly_coco, dataset=dataset)
    Config.set_loss_weights(args)
    world, rank, local = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0")), int(os.environ.get("LOCAL_RANK", "0"))
    dev = "cuda:%d" % local
    torch.cuda.set_device(local)
    if world > 1:
        # the gradient arena outlives every collective on it: the allocator need not record the RCCL stream on it (0.1 ms of a 10 ms step at
        # world size 1, tools/probe_dist_host.py)
        os.environ.setdefault("TORCH_NCCL_AVOID_RECORD_STREAMS", "1")
        torch.distributed.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device(dev))
    ext = args.ext or ".jpg"
    dm = MultiModalDataModule(dataset, args.train, args.train, args.test, args.test, batch_size=args.batch, num_workers=args.num_workers,
                              ext=ext, seed=args.seed, rank=rank, world_size=world, ablation_flag=args.ablation_flag,
                              **Config.cache_kwargs(args, dev))
    kw = dict(batch_size=args.batch, model_name=args.decoder_backbone, in_channels=Config.EncoderDecoder.in_channels_encoder,
              output_channels=Config.EncoderDecoder.out_channels_decoder, lr=1e-4 if args.lr is None else args.lr,
              detector_name=Config.Detector.name, train_det=Config.Detector.train_det, fuse_data=args.fuse_data, precision=args.precision, device=dev,
              loss_pixel=Config.Losses.pixel, loss_perceptual=Config.Losses.perceptual, loss_structural=Config.Losses.structural,
              map_device=args.map_device, **Config.miss_rate_kwargs(args),
              ir_preprocess=args.ir_preprocess, media=media_writer(args, rank), **Config.transform_kwargs(args))
    model = EncoderDecoderLit.load_from_checkpoint(args.pre_train_path, strict=False, **kw) if args.pre_train_path else EncoderDecoderLit(**kw)
    if args.detector_path:
        from hallucidet_amd.checkpoint import load_detector
        load_detector(model.detector, args.detector_path)
    model.prepare()
    out_dir = os.path.join("lightning_logs", args.wandb_project, args.wandb_name)
    tr = Trainer(max_epochs=args.epochs, limit_train_batches=args.limit_train_batches, dirpath=out_dir if rank == 0 else None,
                 monitor="map_hall/map_50", mode="max", device=dev, log=print if rank == 0 else (lambda *a: None),
                 train_geometry=Config.train_geometry(args, rank))
    tr.fit(model, dm)
    if rank == 0:
        tr.save_checkpoint(model, os.path.join(out_dir, "encoder_decoder_pl.ckpt"))
        print_ap50(tr.test(model, dm), ir_preprocess=args.ir_preprocess)
    if model.media is not None:
        model.media.close()
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
