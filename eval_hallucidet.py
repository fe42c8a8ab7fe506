"""eval_hallucidet.py of the reference (:190-230): load a HalluciDet checkpoint, run the test split, print the three AP@50
lines (:180-182).

    python eval_hallucidet.py --dataset llvip --test <root>/LLVIP --hallucidet-path best.ckpt --detector fasterrcnn --batch 8 --ext .jpg
"""
import torch

from hallucidet_amd.config import Config
from hallucidet_amd.dataloader import MultiModalDataModule
from hallucidet_amd.train_hallucidet import EncoderDecoderLit
from hallucidet_amd.trainer import Trainer
from train_hallucidet import media_writer, print_ap50


def main(argv=None):
    Config.set_environment()
    args = Config.argument_parser(argv)
    if args.augment != "none":
        raise SystemExit("eval_hallucidet.py: --augment %s is an option of train_detector.py (evaluation reads the raw images); use "
                         "--augment none" % args.augment)
    if args.augment_geometry != "none":
        raise SystemExit("eval_hallucidet.py: --augment-geometry %s is an option of the training scripts (evaluation reads the raw images); "
                         "use --augment-geometry none" % args.augment_geometry)
    torch.manual_seed(args.seed)
    dataset = args.dataset or "llvip"
    Config.set_detector(args.detector, train_det=False, pretrained=args.directly_coco, dataset=dataset)
    Config.set_loss_weights(args)        # eval_hallucidet.py:39: the test loss (and val_loss) carry the same weighted terms as training
    dev = args.device if args.device not in (None, "gpu") else "cuda"
    dm = MultiModalDataModule(dataset, args.test, args.test, args.test, args.test, batch_size=args.batch, num_workers=args.num_workers,
                              ext=args.ext or ".jpg", seed=args.seed, cache_units=("test",),
                              **Config.cache_kwargs(args, dev))          # only the test split is read: only its unit is cached
    kw = dict(batch_size=args.batch, model_name=args.decoder_backbone, detector_name=Config.Detector.name, precision=args.precision, device=dev,
              loss_pixel=Config.Losses.pixel, loss_perceptual=Config.Losses.perceptual, loss_structural=Config.Losses.structural,
              map_device=args.map_device, **Config.miss_rate_kwargs(args),
              ir_preprocess=args.ir_preprocess, media=media_writer(args), **Config.transform_kwargs(args))
    model = EncoderDecoderLit.load_from_checkpoint(args.hallucidet_path, strict=False, **kw) if args.hallucidet_path else EncoderDecoderLit(**kw)
    if args.detector_path:
        from hallucidet_amd.checkpoint import load_detector
        load_detector(model.detector, args.detector_path)
    model.encoder_decoder.to(dev)
    model.detector.to(dev)
    model.eval()            # Lightning's test loop: BatchNorm on the checkpoint's running statistics, detector in eval mode
    maps = Trainer(device=dev).test(model, dm)
    if model.media is not None:
        model.media.close()
    print_ap50(maps, ir_preprocess=args.ir_preprocess)
    return maps


if __name__ == "__main__":
    main()
