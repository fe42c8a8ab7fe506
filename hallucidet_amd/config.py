"""Subset of the reference's global `Config` that the hot path reads (src/config/config.py:6-93,204-245,310-357):
same attribute names and default values (pinned by tests/golden/config_defaults.json)."""
import os

import torch


class Config:

    class Environment:
        N_CORE = "8"
        N_THREADS_TORCH = 8
        N_GPUS = 1
        CUDNN_BENCHMARK = True
        DEBUG = False

    class Optimizer:
        name = 'adam'
        scheduler_step_size = 10
        scheduler_gamma = 0.1
        scheduler_on = True
        gradient_clip_val = 0.5

    class Losses:
        hparams_losses_weights = {
            'pixel_rgb': 0.0,
            'pixel_ir': 0.0,
            'perceptual_rgb': 0.0,
            'perceptual_ir': 0.0,
            'det_regression': 0.1,
            'det_classification': 0.1,
            'det_objectness': 0.1,
            'det_rpn_box_reg': 0.1,
            'det_bbox_ctrness': 0.1,
            'det_masked': 0.0,
        }
        pixel = None
        perceptual = None
        structural = None     # --structural: 'ssim' fills the two perceptual slots (weights perceptual_rgb / perceptual_ir)

    class EncoderDecoder:
        in_channels_encoder = 3
        out_channels_decoder = 3
        decoder_head = 'sigmoid'
        load_encoder_decoder = False

    class Detector:
        train_det = False
        name = 'fasterrcnn'
        pretrained = True
        input_size = 300   # 640 for flir (config.py:317)
        batch_norm_eps = 0.001
        batch_norm_momentum = 0.03
        eval_path = None
        modality = None
        score_threshold = 0.5

    @staticmethod
    def set_detector(detector_name='fasterrcnn', train_det=False, pretrained=True, dataset='llvip'):
        Config.Detector.name = detector_name
        Config.Detector.train_det = train_det
        Config.Detector.pretrained = pretrained
        Config.Detector.input_size = 640 if dataset == 'flir' else 300

    @staticmethod
    def set_environment():
        """config.py:262-271: eight host threads for OpenMP / BLAS / torch's intra-op pool (cudnn.benchmark has no counterpart
        here).  Matters on the GPU path too: torch's default is one thread per HARDWARE thread of the host (256 on the MI355X
        boxes) while a container is throttled to a fraction of them -- the step's small host-side tensor ops then spin against
        each other (measured: mean step 14.5-16.7 ms instead of 14.0-14.2 ms)."""
        for k in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS", "VECLIB_MAXIMUM_THREADS", "NUMEXPR_NUM_THREADS"):
            os.environ[k] = Config.Environment.N_CORE
        torch.set_num_threads(Config.Environment.N_THREADS_TORCH)

    @staticmethod
    def config_optimizer(unet, learning_rate=1e-4, name='adam'):
        """config.py:204-245 builds torch.optim.Adam(params, lr); here the same update runs as one fused kernel over the
        flat parameter arena, with Lightning's value clipping (Config.Optimizer.gradient_clip_val) folded in."""
        from .optim import FusedAdam
        if name != 'adam':
            raise NotImplementedError("the reference always uses Config.Optimizer.name == 'adam' (SURVEY 5.6)")
        return FusedAdam(unet, lr=learning_rate, clip_value=Config.Optimizer.gradient_clip_val)

    @staticmethod
    def argument_parser(argv=None):
        """config.py:96-197 -- the reference's flags and defaults (one parser for the three scripts)."""
        import argparse
        p = argparse.ArgumentParser(description='HalluciDet')
        p.add_argument('--dataset', type=str, default=None, help='llvip/flir')
        p.add_argument('--train', type=str, default=None, help='Train Dataset Path')
        p.add_argument('--valid', type=str, default=None, help='Valid Dataset Path')
        p.add_argument('--test', type=str, default=None, help='Test Dataset Path')
        p.add_argument('--n-classes', '--n_classes', '--num-classes', '--nclasses', type=int, default=2)
        p.add_argument('--detector', type=str, default='fasterrcnn', help="choices=['fasterrcnn', 'fcos', 'retinanet']")
        p.add_argument('--pretrained', action='store_true')
        p.add_argument('--fine-tuning', action='store_true')
        p.add_argument('--fine-tuning-lp', action='store_true')
        p.add_argument('--modality', type=str, default='rgb')
        p.add_argument('--threshold', type=float, default=0.5)
        p.add_argument('--epochs', type=int, default=10)
        p.add_argument('--lr', type=float, default=None)
        p.add_argument('--seed', type=int, default=123)
        p.add_argument('--wandb-project', type=str, default="hallucidet")
        p.add_argument('--wandb-name', type=str, default="detector")
        p.add_argument("--batch", type=int, default=16)
        p.add_argument("--num-workers", type=int, default=4)
        p.add_argument("--ext", "--input-ext", type=str, default=None)
        p.add_argument("--output-model", type=str, default="example.ckpt")
        p.add_argument("--detector-path", type=str, default=None)
        p.add_argument("--device", type=str, default=None)
        p.add_argument("--fuse-data", type=str, default='none')
        p.add_argument("--decoder-backbone", type=str, default='resnet34')
        p.add_argument("--precision", type=int, default=32)
        p.add_argument("--optimizer", type=str, default='adamw')
        p.add_argument("--path", type=str, default=None)
        p.add_argument("--segmentation-head", type=str, default='sigmoid')
        p.add_argument("--pixel", type=str, default=None)
        p.add_argument("--weight-pixel-rgb", type=float, default=0.0)
        p.add_argument("--weight-pixel-ir", type=float, default=0.0)
        # where validation / test compute COCO mAP: 'cpu' = the host evaluator, 'cuda' = the HIP evaluator (same numbers; with several
        # ranks it reports the mAP of the whole split instead of the mean of the per-rank values)
        p.add_argument("--map-device", type=str, default="cpu", choices=["cpu", "cuda"])
        # the log-average miss rate (Dollar et al. 2012; metrics/metrics.py) next to the mAP, from the same matches: validation / test
        # report lamr, lamr_75, lamr_small / _medium / _large and mr_fppi01.  --miss-rate-curves DIR (implies --miss-rate): after the test
        # split rank 0 writes the MR-FPPI curves as DIR/test_{stream}_class{label}.csv.  Default: off
        p.add_argument("--miss-rate", action="store_true")
        p.add_argument("--miss-rate-curves", type=str, default=None, metavar="DIR")
        # train_detector.py: 'reference' = the reference's photometric augmentation of the training split (train_detector.py:401-410),
        # applied to the uint8 batch on the GPU (dataloader/augment.py)
        p.add_argument("--augment", type=str, default="none", choices=["none", "reference"])
        # geometric augmentation of the training split on the GPU (dataloader/geometry.py, hd_geometry_u8): 'hflip' = horizontal flip
        # with probability 0.5; 'hflip_crop' = also, with probability 0.5, a random crop that contains every box, no smaller than
        # --geometry-min-scale of each side, resized back to the input's size.  Paired batches get one transform for both modalities
        # and the boxes follow.  Validation and test are never augmented.  Default: off
        p.add_argument("--augment-geometry", type=str, default="none", choices=["none", "hflip", "hflip_crop"])
        p.add_argument("--geometry-min-scale", type=float, default=0.5, metavar="S")
        # the image-space IR pre-processing baselines of the reference (models/cnnBasedThermalInfraredDA.py), on the GPU: in
        # eval_hallucidet.py / train_hallucidet.py what the "RGB Detector on IR" pass reads in validation and test; in
        # train_detector.py --modality ir what the detector is fine-tuned and evaluated on
        from .models.cnnBasedThermalInfraredDA import IR_PREPROCESS_NAMES
        p.add_argument("--ir-preprocess", type=str, default="none", choices=list(IR_PREPROCESS_NAMES))
        # detection media (utils/media.py): validation / test write the reference's panels (inputs, hallucinated output, the three "det"
        # panels with ground truths in yellow and detections above --threshold in red) as PNG grids under DIR, every N-th batch at the
        # reference's phase (batch_idx % N == 1 % N), at most K batches per split and epoch.  Default: off
        p.add_argument("--save-media", type=str, default=None, metavar="DIR")
        p.add_argument("--media-every", type=int, default=100, metavar="N")
        p.add_argument("--media-max", type=int, default=None, metavar="K")
        # 'hbm': decode the train and test datasets once into GPU memory and build every batch there with one gather launch
        # (dataloader/cache.py); a dataset that does not fit in --cache-budget-gb (10^9 bytes; default: half of the free memory of the
        # device) or whose images differ in shape stays on the DataLoader.  Default: off
        p.add_argument("--cache-dataset", type=str, default="none", choices=["none", "hbm"])
        p.add_argument("--cache-budget-gb", type=float, default=None, metavar="G")
        # the detector's input transform (models/custom_generalized_transform.py): how the image is resized to the detector's fixed size
        # -- 'nearest' is the reference's F.interpolate default and what parity is judged against; 'bilinear' is torchvision's own;
        # 'bilinear_aa' adds its antialias filter -- and whether it is normalised first ('imagenet': torchvision's mean / std, for
        # detectors whose weights expect it).  Neither is stored in a checkpoint: evaluate a detector with the flags it was trained with
        p.add_argument("--detector-resize", type=str, default="nearest", choices=["nearest", "bilinear", "bilinear_aa"])
        p.add_argument("--detector-norm", type=str, default="none", choices=["none", "imagenet"])
        p.add_argument("--perceptual", type=str, default=None)
        # the structural reconstruction loss (losses/losses.py: 1 - SSIM in hd_ssim_loss), weighted by --weight-perceptual-rgb / -ir into
        # the reference's two perceptual slots; --perceptual ssim itself selects nothing, as in the reference.  Default: off
        p.add_argument("--structural", type=str, default=None, choices=["ssim"])
        p.add_argument("--weight-perceptual-rgb", type=float, default=0.0)
        p.add_argument("--weight-perceptual-ir", type=float, default=0.0)
        p.add_argument("--weight-det-regression", type=float, default=0.1)
        p.add_argument("--weight-det-classification", type=float, default=0.1)
        p.add_argument("--weight-det-masked", type=float, default=0.0)
        p.add_argument("--weight-det-objectness", type=float, default=0.1)
        p.add_argument("--weight-det-rpn-box-reg", type=float, default=0.1)
        p.add_argument("--weight-det-bbox-ctrness", type=float, default=0.1)
        p.add_argument("--image2image-model", type=str, default=None)
        p.add_argument('--directly-coco', action='store_true')
        p.add_argument('--limit-train-batches', type=float, default=1.0)
        p.add_argument('--ablation-flag', action='store_true')
        p.add_argument("--pre-train-path", type=str, default=None)
        p.add_argument("--encoder-depth", type=int, default=5)
        p.add_argument('--hallucidet-path', type=str)
        return p.parse_args(argv)

    @staticmethod
    def detector_norm_stats(name):
        """--detector-norm -> (image_mean, image_std) for Detector / the Lit modules; 'none' -> (None, None): the reference's 0 / 1."""
        if name in (None, "none"):
            return None, None
        if name == "imagenet":
            from .resample import IMAGENET_MEAN, IMAGENET_STD
            return list(IMAGENET_MEAN), list(IMAGENET_STD)
        raise ValueError("unknown detector norm %r (none / imagenet)" % (name,))

    @staticmethod
    def transform_kwargs(args):
        """The Lit modules' transform keywords from --detector-resize / --detector-norm."""
        mean, std = Config.detector_norm_stats(args.detector_norm)
        return dict(resize_mode=args.detector_resize, image_mean=mean, image_std=std)

    @staticmethod
    def miss_rate_kwargs(args):
        """The Lit modules' miss-rate keywords from --miss-rate / --miss-rate-curves (a curve directory turns the metric on)."""
        return dict(miss_rate=bool(args.miss_rate or args.miss_rate_curves), miss_rate_curves=args.miss_rate_curves)

    @staticmethod
    def cache_kwargs(args, device):
        """The data modules' cache keywords from --cache-dataset / --cache-budget-gb."""
        budget = None if args.cache_budget_gb is None else int(args.cache_budget_gb * 1e9)
        return dict(cache=args.cache_dataset, cache_budget_bytes=budget, device=device)

    @staticmethod
    def train_geometry(args, rank=0):
        """--augment-geometry / --geometry-min-scale -> the `PairedGeometry` of the training split, or None when off."""
        if args.augment_geometry == "none":
            return None
        from .dataloader.geometry import PairedGeometry
        return PairedGeometry(p_flip=0.5, p_crop=0.5 if args.augment_geometry == "hflip_crop" else 0.0, min_scale=args.geometry_min_scale,
                              seed=args.seed, rank=rank)

    @staticmethod
    def set_loss_weights(args):
        """config.py: `set_loss_weights(args)` copies the --weight-* flags into Losses.hparams_losses_weights."""
        if args.pixel is not None:
            Config.Losses.pixel = args.pixel
        if args.perceptual is not None:
            Config.Losses.perceptual = args.perceptual
        if args.structural is not None:
            Config.Losses.structural = args.structural
        w = Config.Losses.hparams_losses_weights
        w.update(pixel_rgb=args.weight_pixel_rgb, pixel_ir=args.weight_pixel_ir, perceptual_rgb=args.weight_perceptual_rgb,
                 perceptual_ir=args.weight_perceptual_ir, det_regression=args.weight_det_regression,
                 det_classification=args.weight_det_classification, det_objectness=args.weight_det_objectness,
                 det_rpn_box_reg=args.weight_det_rpn_box_reg, det_bbox_ctrness=args.weight_det_bbox_ctrness, det_masked=args.weight_det_masked)

    @staticmethod
    def cuda_or_cpu():
        return 'cuda' if torch.cuda.is_available() else 'cpu'
