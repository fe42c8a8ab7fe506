"""Image-space IR pre-processing baselines of the reference (src/models/cnnBasedThermalInfraredDA.py, after Herrmann et al., "CNN-based
thermal infrared person detection by domain adaptation"): the static methods of its `CnnBasedThermalInfraredDA`, same names and keyword
signatures, on the GPU through `ops.ir_preprocess` (hd_ir_preprocess, csrc/ir_preprocess.hip).  The LightningModule around them is a
torchvision detector wrapper this package already has as `Detector`; `basic_preprocessing_histogram_stretching_default` (raises on its
own argument shape) and `basic_preprocessing_collor_jitter` (random) are not carried over.

Every method takes [C, H, W] or [N, C, H, W] float32 on the GPU, C in (1, 3), and returns a NEW tensor (the reference clones).  What the
reference executes is kept, quirks included:
  * stretching clamps to the two QUANTILES, not to [0, 1]; a constant channel becomes NaN;
  * equalization quantises with trunc(x * 255), so after an invert 159 of the 256 levels land one below 255 - k;
  * `channels=` is ignored by invert, blur and equalization (they act on all channels) and honoured by stretching;
  * `paralel_combination` therefore runs every listed operation on ALL channels in list order: its default is
    invert(equalization(x)).
The stretching family of the reference indexes `input[c]`, i.e. it is written for one image; here every method works per image and per
channel on a batch.  `parallel_per_channel` (channel 0 equalized, channel 1 inverted, channel 2 untouched) is what the paper describes
and the reference's code does not do: it exists only as a preset here.
"""
import torch

from .. import ops

_ALL = (0, 1, 2)
_S = ops.irp_stage
_INV, _STR, _EQ, _BLUR = (_S(ops.IRP_INVERT), _S(ops.IRP_STRETCH), _S(ops.IRP_EQUALIZE), _S(ops.IRP_BLUR))

# preset name (the value of --ir-preprocess) -> stage list of ops.ir_preprocess
IR_PREPROCESS = {
    "invert": [_INV],
    "blur": [_BLUR],
    "stretching": [_STR],
    "equalization": [_EQ],
    "invert_stretching": [_INV, _STR],
    "invert_stretching_blur": [_INV, _STR, _BLUR],
    "invert_equalization": [_INV, _EQ],
    "invert_equalization_blur": [_INV, _EQ, _BLUR],
    "parallel": [_EQ, _INV],                                                    # the reference's paralel_combination default, as executed
    "parallel_per_channel": [_S(ops.IRP_EQUALIZE, (0,)), _S(ops.IRP_INVERT, (1,))],  # the paper's description; not in the reference
}
IR_PREPROCESS_NAMES = ("none",) + tuple(IR_PREPROCESS)
_BETA = 0.003       # the one quantile level hd_ir_preprocess computes (the reference's default, "cnn-based paper")


def _run(input, stages, per_channel=False):
    """`stages` on [C, H, W] or [N, C, H, W].  A stride-0 three-channel view of a one-plane batch (Utils.expand_one_channel_to_output_channels)
    is processed as ONE plane and re-expanded, unless the stages treat the channels differently (`per_channel`)."""
    if not torch.is_tensor(input) or input.dim() not in (3, 4):
        raise ValueError("CnnBasedThermalInfraredDA: input must be a [C, H, W] or [N, C, H, W] tensor")
    x = input if input.dim() == 4 else input.unsqueeze(0)
    one_plane_view = x.shape[1] == 3 and x.stride(1) == 0
    if one_plane_view and not per_channel:
        x = x[:, :1]
    if per_channel and x.shape[1] != 3:
        raise ValueError("CnnBasedThermalInfraredDA: a per-channel combination needs three channels (got %d)" % x.shape[1])
    x = x.contiguous()
    out = None
    for i in range(0, len(stages), ops.IRP_MAX_STAGES):
        out = x = ops.ir_preprocess(x, stages[i:i + ops.IRP_MAX_STAGES])
    if out is None:
        out = x.clone()
    if one_plane_view and not per_channel:
        out = out.expand(-1, 3, -1, -1)
    return out if input.dim() == 4 else out[0]


def _stretch_stage(channels, beta):
    if float(beta) != _BETA:
        raise NotImplementedError("histogram stretching is built for beta = %r (the reference's default); got %r" % (_BETA, beta))
    return _S(ops.IRP_STRETCH, tuple(sorted(set(int(c) for c in channels))))


def _check_blur(kernel_size, sigma):
    ks = (kernel_size, kernel_size) if isinstance(kernel_size, int) else tuple(kernel_size)
    sg = None if sigma is None else ((sigma, sigma) if isinstance(sigma, (int, float)) else tuple(sigma))
    if ks != (3, 3) or (sg is not None and any(float(s) != 0.8 for s in sg)):
        raise NotImplementedError("the blur is built for kernel_size (3, 3) and its default sigma 0.8 (got %r, %r)" % (kernel_size, sigma))


class CnnBasedThermalInfraredDA:

    @staticmethod
    def basic_preprocessing_invert(input, channels=[0, 1, 2]):
        return _run(input, [_INV])

    @staticmethod
    def basic_preprocessing_blur(input, channels=[0, 1, 2], kernel_size=(3, 3), sigma=None):
        _check_blur(kernel_size, sigma)
        return _run(input, [_BLUR])

    @staticmethod
    def basic_preprocessing_histogram_stretching(input, channels=[0, 1, 2], beta=0.003):
        return _run(input, [_stretch_stage(channels, beta)])

    @staticmethod
    def basic_preprocessing_histogram_equalization(input, channels=[0, 1, 2]):
        return _run(input, [_EQ])

    @staticmethod
    def basic_preprocessing_invert_stretching(input, channels=[0, 1, 2]):
        return _run(input, [_INV, _stretch_stage(channels, _BETA)])

    @staticmethod
    def basic_preprocessing_invert_stretching_blur(input, channels=[0, 1, 2]):
        return _run(input, [_INV, _stretch_stage(channels, _BETA), _BLUR])

    @staticmethod
    def basic_preprocessing_invert_equalization(input, channels=[0, 1, 2]):
        return _run(input, [_INV, _EQ])

    @staticmethod
    def basic_preprocessing_invert_equalization_blur(input, channels=[0, 1, 2]):
        return _run(input, [_INV, _EQ, _BLUR])

    @staticmethod
    def paralel_combination(input, channel_op=['equalization', 'invert', 'none']):
        """The reference passes `channels=[idx]` to callees that ignore it: every listed operation runs on all channels, in list order;
        'none' and unknown names are skipped."""
        stages = [{"invert": _INV, "equalization": _EQ}[op] for op in channel_op if op in ("invert", "equalization")]
        return _run(input, stages)

    @staticmethod
    def apply_preset(input, name):
        """The pre-processing `--ir-preprocess NAME` selects ('none': the input itself)."""
        if name in (None, "none"):
            return input
        if name not in IR_PREPROCESS:
            raise ValueError("unknown IR pre-processing %r (one of %s)" % (name, ", ".join(IR_PREPROCESS_NAMES)))
        return _run(input, IR_PREPROCESS[name], per_channel=name == "parallel_per_channel")
