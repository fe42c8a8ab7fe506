"""The convolution dispatcher's route table: one line per problem of a fixed corpus with the kernel family, tile, parity flag, `stats` rows
and grid size hd_conv2d_route reports for it.  Needs no GPU (the query launches nothing; the pointers in the argument blocks are
placeholders that are never followed).

    python tools/conv_routes.py                      # print the table
    python tools/conv_routes.py --out FILE           # write it
    python tools/conv_routes.py --check tests/golden/conv_routes.txt     # exit 1 and list the lines that differ

tests/golden/conv_routes.txt is the committed record (tests/test_conv_routing_cpu.py compares against it): a change of a routing rule
shows up as a diff of that file.

A line is  `<hook> | N Hsrc Wsrc C1 C2 Cout K stride pad Ho Wo <options> -> <family> a b deep par M rows blocks`  with the options
u up1, d in_dil 2, s stats, r res, b bias, m mask, a<act>, o<out_mode>, i in_scale, p<out_pool2>, y y2, B bs_*, Z bs_z;  (a, b) are the
tile parameters of the family (include/hallucidet_hip.h, hd_conv2d_route); `-> E` marks a block hd_conv2d refuses."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FAMILIES = ["small", "c64", "stem", "c32", "cat", "gemm8", "p8", "m160", "igemm32", "igemm64"]
KSP = [(3, 1, 1), (3, 2, 1), (1, 1, 0), (1, 2, 0), (7, 2, 3), (7, 1, 0), (3, 1, 0), (5, 1, 2)]      # every (K, stride, pad) of fuzz_conv.draw_case
CH_IN = [8, 16, 24, 32, 40, 64, 72, 96, 128, 192, 256, 320, 512]                                  # fuzz_conv.CH_IN / CH_OUT
CH_OUT = [3, 8, 16, 24, 32, 40, 64, 72, 128, 136, 192, 256, 512]
# hook settings the tests use: (name, value); "" = the shipped rules
HOOKS = [("w8", v) for v in (-2, -3, 10, 11, 12, 13, 15, 16, 17, 18, 19, 20)] + [("gemm8", v) for v in (0, 128, 1128)] + \
        [("override", (128, 64, 64, 0)), ("nominal", 8)]
P = 0x1000      # placeholder for every tensor pointer


def out_size(h, k, stride, pad):
    return (h + 2 * pad - k) // stride + 1


def case(N, H, W, C1, Cout, K=3, stride=1, pad=1, C2=0, up1=False, dil=1, out_hw=None, opts=""):
    """H, W: the stored extent of x.  opts: the option letters of the module docstring, space separated."""
    Hin, Win = (2 * H, 2 * W) if up1 else (H, W)
    if dil > 1:
        Hin = Win = 0
        Ho, Wo = out_hw
    else:
        Ho, Wo = out_hw or (out_size(Hin, K, stride, pad), out_size(Win, K, stride, pad))
    return dict(N=N, H=H, W=W, Hin=Hin, Win=Win, C1=C1, C2=C2, Cout=Cout, K=K, stride=stride, pad=pad, up1=up1, dil=dil, Ho=Ho, Wo=Wo,
                opts=tuple(opts.split()))


def dgrad_of(c, opts=""):
    """the data gradient of a single-source forward problem: channels swapped, stride s as in_dil (s <= 2)"""
    H, W = c["Ho"], c["Wo"]
    return case(c["N"], H, W, c["Cout"] if c["Cout"] % 8 == 0 else 8, c["C1"] + c["C2"], c["K"], 1, c["K"] - 1 - c["pad"], dil=c["stride"],
                out_hw=(c["Hin"], c["Win"]), opts=opts)


def make_args(c, ConvArgs):
    o = c["opts"]
    act = next((int(t[1:]) for t in o if t[0] == "a"), 0)
    om = next((int(t[1:]) for t in o if t[0] == "o"), 0)
    pool2 = next((int(t[1:]) for t in o if t[0] == "p"), 0)
    a = ConvArgs()
    a.x, a.w, a.y = P, P, P
    a.x2 = P if c["C2"] else None
    a.bias, a.res, a.mask, a.stats = (P if "b" in o else None), (P if "r" in o else None), (P if "m" in o else None), (P if "s" in o else None)
    a.N, a.Hsrc, a.Wsrc, a.Hin, a.Win, a.C1, a.C2 = c["N"], c["H"], c["W"], c["Hin"], c["Win"], c["C1"], c["C2"]
    a.Ho, a.Wo, a.Cout, a.KH, a.KW, a.stride, a.pad = c["Ho"], c["Wo"], c["Cout"], c["K"], c["K"], c["stride"], c["pad"]
    a.up1, a.in_dil, a.act, a.out_mode = int(c["up1"]), c["dil"], act, om
    if "i" in o:
        a.in_scale, a.in_shift, a.in_relu = P, P, 1
    a.out_pool2, a.y2 = pool2, (P if "y" in o else None)
    if "B" in o:
        a.bs_y, a.bs_mean, a.bs_invstd, a.bs_gamma, a.bs_beta, a.bs_relu = P, P, P, P, P, 1
        a.bs_z = P if "Z" in o else None
    return a


OPTION_SETS = ["", "s", "r", "b", "a1", "a2", "m", "s r", "s b a1", "b a1 r", "o1 b a2", "o1", "o2 b", "o2", "i", "i s", "s B", "s B Z r", "s B r"]


def with_pool2(c):
    """the out_pool2 forms: everything pooled, half / 64 / 128 pooled channels + y2, and a split without y2 (refused)"""
    Cout = c["Cout"]
    forms = ["p%d" % Cout] + ["p%d y" % k for k in sorted({Cout // 2, 64, 128}) if 0 < k < Cout and k % 8 == 0] + ["p%d" % max(8, Cout // 2)]
    return [dict(c, opts=tuple(f.split())) for f in forms]


def unet_layers(N):
    """the hallucination U-Net (ResNet-34 encoder, five decoder blocks) on 512 x 640 images: forward problems"""
    L = [case(N, 512, 640, 8, 64, 7, 2, 3, opts="s")]
    h, w, cin = 128, 160, 64
    for i, ch in enumerate((64, 128, 256, 512)):
        if i:
            L += [case(N, h, w, cin, ch, 3, 2, 1, opts="s"), case(N, h, w, cin, ch, 1, 2, 0, opts="s")]
            h, w = h // 2, w // 2
        L += [case(N, h, w, ch, ch, 3, 1, 1, opts="s"), case(N, h, w, ch, ch, 3, 1, 1, opts="s r")]
        cin = ch
    for cup, skip, ch in ((512, 256, 256), (256, 128, 128), (128, 64, 64), (64, 64, 32)):
        L += [case(N, h, w, cup, ch, C2=skip, up1=True, opts="s"), case(N, 2 * h, 2 * w, ch, ch, opts="s")]
        h, w = 2 * h, 2 * w
    L += [case(N, h, w, 32, 16, up1=True, opts="s"), case(N, 2 * h, 2 * w, 16, 16, opts="s"), case(N, 2 * h, 2 * w, 16, 8, opts="o1 b a2")]
    return L


def detector_layers(N):
    """the detector's pyramid maps (75 / 38 / 19 / 10 / 5 squares): backbone bottlenecks, lateral and output convs, heads"""
    L = []
    for s, ch in ((75, 256), (38, 512), (19, 1024), (10, 2048), (5, 256)):
        mid = ch // 4
        L += [case(N, s, s, 256, 256, opts="b"), case(N, s, s, 256, 256, opts="b a1"), case(N, s, s, 256, 16, 1, 1, 0, opts="b"),
              case(N, s, s, 256, 48, 1, 1, 0, opts="b"), case(N, s, s, ch, 256, 1, 1, 0, opts="b"), case(N, s, s, ch, mid, 1, 1, 0, opts="b a1"),
              case(N, s, s, mid, mid, opts="b a1"), case(N, s, s, mid, ch, 1, 1, 0, opts="b r a1"), case(N, s, s, 256, 256, 3, 2, 1, opts="b")]
    return L


def box_head(R):
    """fc6 (a 7 x 7 'convolution' over the whole RoI) and fc7 on R boxes, and their data gradients"""
    return [case(R, 7, 7, 256, 1024, 7, 1, 0, opts="b a1"), case(R, 1, 1, 1024, 1024, 1, 1, 0, opts="b a1"),
            case(R, 1, 1, 1024, 1024, 1, 1, 0, opts="m"), case(R, 1, 1, 1024, 12544, 1, 1, 0), case(R, 1, 1, 1024, 1024, 1, 1, 0)]


def base_problems():
    """one or two problems in every family's domain (the option and hook sweeps run over these)"""
    return [case(1, 8, 8, 16, 16), case(2, 40, 64, 32, 32), case(2, 20, 32, 8, 16), case(1, 8, 16, 64, 64), case(8, 40, 60, 64, 64),
            case(1, 32, 32, 8, 64, 7, 2, 3), case(2, 24, 32, 32, 128), case(1, 3, 8, 64, 32, C2=64, up1=True),
            case(1, 1, 16, 64, 32, C2=64, up1=True), case(8, 20, 30, 64, 32, C2=64, up1=True), case(1, 10, 44, 64, 128),
            case(8, 40, 60, 128, 128), case(8, 19, 19, 256, 256), case(24, 10, 10, 256, 256), case(8, 16, 20, 512, 512),
            case(8, 16, 20, 128, 64, C2=64, up1=True), case(2, 8, 10, 512, 256, C2=256, up1=True), case(1, 9, 9, 24, 40),
            case(1, 9, 9, 64, 72, 1, 1, 0), case(8, 38, 38, 256, 512, 1, 1, 0), case(4, 33, 47, 96, 136, 3, 2, 1),
            case(4096, 1, 1, 1024, 1024, 1, 1, 0), case(2, 20, 20, 128, 128, 5, 1, 2)]


def corpus():
    """[(hook, case)], deterministic, about 2 500 entries"""
    shapes = [(1, 9, 9), (2, 20, 32), (8, 40, 60), (4, 70, 90), (1, 7, 7), (3, 33, 47)]
    plain = []
    n = 0
    for K, stride, pad in KSP:
        for i, C1 in enumerate(CH_IN):
            for j in (0, 5):
                N, H, W = shapes[n % len(shapes)] if K < 7 or stride == 2 else (shapes[n % len(shapes)][0], 7, 7)
                H, W = max(H, K), max(W, K)
                c = case(N, H, W, C1, CH_OUT[(i + j + n // 7) % len(CH_OUT)], K, stride, pad)
                plain += [c, dict(c, opts=("s",))]
                if stride == 2 and n % 3 == 0:
                    plain += [dgrad_of(c), dgrad_of(c, "s")]
                n += 1
    for C1 in (32, 64, 128):
        for C2 in (32, 64, 128):
            for k, Cout in enumerate((16, 32, 64, 128, 256)):
                N, H, W = shapes[(k + C1 // 32 + C2 // 32) % 4]
                plain += [case(N, H, W, C1, Cout, C2=C2, up1=True, opts=o) for o in ("", "s", "s B")]
                plain.append(case(N, 2 * H, 2 * W, C1, Cout, C2=C2))
    for N in (1, 8):
        fwd = unet_layers(N)
        plain += fwd
        for c in fwd:
            if c["C2"] or c["up1"]:      # decoder conv1: its data gradient is a single-source 3x3 problem with the pooled / split output
                g = case(N, c["Ho"], c["Wo"], c["Cout"], c["C1"] + c["C2"])
                plain += [g, dict(g, opts=("p%d" % c["C1"],) + (("y",) if c["C2"] else ()))]
            elif c["Cout"] >= 16:
                plain += [dgrad_of(c), dgrad_of(c, "m")] + ([dgrad_of(c, "s B"), dgrad_of(c, "s B Z r")] if c["stride"] == 1 else [])
    for N in (8, 24):
        det = detector_layers(N)
        plain += det + [dgrad_of(c) for c in det] + [dgrad_of(c, "m") for c in det[::3]]
    for R in (512, 4096, 8192, 12288):
        plain += box_head(R)
    base = base_problems()
    for c in base:
        plain += [dict(c, opts=tuple(o.split())) for o in OPTION_SETS]
        if c["K"] == 3 and c["stride"] == 1:
            plain += with_pool2(c)
    out = [("", c) for c in plain]
    swept = [dict(c, opts=tuple(o.split())) for c in base for o in ("", "s", "s B")] + [p for c in base[10:17] for p in with_pool2(c)[:2]] + \
            [dgrad_of(c) for c in base if c["stride"] == 2] + box_head(4096)
    for h in HOOKS:
        out += [("%s=%s" % (h[0], ",".join(map(str, h[1])) if isinstance(h[1], tuple) else h[1]), c) for c in swept]
    return out


def load(path=None):
    from hallucidet_amd import _abi
    lib = C.CDLL(path or _abi.LIB_PATH)
    for name in ("hd_conv2d_route", "hd_conv2d_stats_rows", "hd_conv2d_bstat_ok", "hd_conv2d_pool2_ok", "hd_conv_tune_w8", "hd_gemm_w8_mode",
                 "hd_conv_tune_override", "hd_conv_nominal_batch"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = _abi.PROTOTYPES.get(name, (C.c_int, [C.POINTER(_abi.ConvArgs), C.POINTER(C.c_int32)]))
    return lib, _abi.ConvArgs


def set_hook(lib, hook):
    """hook: "" or "name=value"; everything else goes back to the shipped rules"""
    name, _, val = hook.partition("=")
    lib.hd_conv_tune_w8(int(val) if name == "w8" else -1, 1)
    lib.hd_gemm_w8_mode(int(val) if name == "gemm8" else -1)
    lib.hd_conv_tune_override(*(map(int, val.split(",")) if name == "override" else (-1, -1, -1, -1)))
    lib.hd_conv_nominal_batch(int(val) if name == "nominal" else 0)


def key_of(hook, c):
    letters = ("u " if c["up1"] else "") + ("d " if c["dil"] == 2 else "") + " ".join(c["opts"])
    return "%s | %d %d %d %d %d %d %d %d %d %d %d %s" % (hook or "-", c["N"], c["H"], c["W"], c["C1"], c["C2"], c["Cout"], c["K"], c["stride"], c["pad"],
                                                        c["Ho"], c["Wo"], letters.strip())


def route_of(lib, a):
    """the eight numbers of hd_conv2d_route, or None where the block is refused"""
    out = (C.c_int32 * 8)()
    return list(out) if lib.hd_conv2d_route(C.byref(a), out) == 0 else None


def table(lib, ConvArgs):
    lines = []
    try:
        for hook, c in corpus():
            set_hook(lib, hook)
            r = route_of(lib, make_args(c, ConvArgs))
            lines.append(key_of(hook, c) + (" -> E" if r is None else " -> %s %s" % (FAMILIES[r[0]], " ".join(map(str, r[1:])))))
    finally:
        set_hook(lib, "")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", help="another build of the library (default: this tree's)")
    ap.add_argument("--out")
    ap.add_argument("--check")
    args = ap.parse_args()
    lines = table(*load(args.lib))
    if args.out:
        open(args.out, "w").write("\n".join(lines) + "\n")
    if args.check:
        want = open(args.check).read().splitlines()
        diff = [(a, b) for a, b in zip(want, lines) if a != b]
        for a, b in diff:
            print("- %s\n+ %s" % (a, b))
        print("conv_routes: %d cases, %d differ%s" % (len(lines), len(diff), "" if len(want) == len(lines) else ", %d recorded" % len(want)))
        return 1 if diff or len(want) != len(lines) else 0
    if not args.out:
        print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
