"""Timer of the multi-level RoIAlign forward (hd_roi_align_ml) and gather backward (hd_roi_align_ml_bwd_gather) on the RoI population
of one training step: 24 images at 300x300, four pyramid levels of 256 channels, 512 RoIs per image; the two forward launches of a step
(16 images without gradient, 8 with) and the backward of the 8.  Prints the three times and saves the three outputs; the kernels are
deterministic, so the files of two builds (HD_HIP_LIB selects the library) must compare bit-identical.
    python tools/bench_roi.py OUT.pt
    python tools/bench_roi.py --compare A.pt B.pt"""
import math, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

NAMES = ("16 images (8192 RoIs)", "8 images (4096 RoIs)", "backward, 8 images")


def compare(pa, pb):
    same = True
    for name, a, b in zip(NAMES, torch.load(pa), torch.load(pb)):
        eq = a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int16), b.view(torch.int16))
        same = same and eq
        print("   %-24s bit-identical: %s  elements that differ %d  non-zero share %.3f" %
              (name, eq, -1 if a.shape != b.shape else int((a != b).sum()), float((a != 0).float().mean())))
    return same


def timed(fn):
    for _ in range(3):
        out = fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        out = fn()
    e1.record(); torch.cuda.synchronize()
    return out, e0.elapsed_time(e1) / 20 * 1e3


def run(path):
    from hallucidet_amd import ops
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(5)
    n_img = 24
    sizes = [75, 38, 19, 10]
    feats = [(torch.randn(n_img, s, s, 256, generator=g) * 0.5).half().to(dev) for s in sizes]
    scales = [2.0 ** -round(math.log2(300.0 / s)) for s in sizes]
    per = 512
    # boxes: log-uniform sizes 8..300 px, some partly outside, a few degenerate
    wh = torch.exp(torch.rand(n_img * per, 2, generator=g) * math.log(300.0 / 8.0)) * 8.0
    c = torch.rand(n_img * per, 2, generator=g) * 300.0
    b = torch.cat([c - wh / 2, c + wh / 2], 1).clamp(0, 300)
    b[::97, 2:] = b[::97, :2]
    img = torch.arange(n_img).repeat_interleave(per).float()[:, None]
    rois = torch.cat([img, b], 1).to(dev)
    area = ((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])).clamp(min=1e-6)
    lvl = torch.floor(4 + torch.log2(torch.sqrt(area) / 224.0) + 1e-6).clamp(2, 5).to(torch.int32) - 2
    lvl = lvl.to(dev)
    outs = []
    for (lo, hi, name) in ((0, 16 * per, NAMES[0]), (16 * per, 24 * per, NAMES[1])):
        r, l = rois[lo:hi].contiguous(), lvl[lo:hi].contiguous()
        o, us = timed(lambda: ops.roi_align_ml(feats, scales, r, l, 7, 7, 2))
        print("   %-24s %7.1f us" % (name, us), flush=True)
        outs.append(o.cpu())
    # backward (gather form) of the 8 images with gradient
    r, l = rois[:8 * per].contiguous(), lvl[:8 * per].contiguous()
    dout = (torch.randn(8 * per, 7, 7, 256, generator=g) * 0.1).half().to(dev)
    shapes = [(8, s_, s_, 256) for s_ in sizes]
    dfs, us = timed(lambda: ops.roi_align_ml_bwd_gather(dout, r, l, shapes, scales, 2))
    print("   %-24s %7.1f us" % (NAMES[2], us), flush=True)
    outs.append(torch.cat([d.flatten() for d in dfs]).cpu())
    torch.save(outs, path)


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        raise SystemExit(0 if compare(sys.argv[2], sys.argv[3]) else 1)
    if len(sys.argv) != 2 or sys.argv[1].startswith("-"):
        raise SystemExit(__doc__)
    run(sys.argv[1])
