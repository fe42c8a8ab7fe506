"""The weight-gradient dispatcher's route table: one line per problem of a fixed corpus with what hd_wgrad_route reports for it (kernel
family, tile, tile counts, direct output, shared grid, grid size) and the default pixel split ops.wgrad_plan chooses.  Needs no GPU (the
query launches nothing; the pointers in the argument blocks are placeholders that are never followed).  The sibling of
tools/conv_routes.py, whose problem builder and layer lists it reuses.

    python tools/wgrad_routes.py                      # print the table
    python tools/wgrad_routes.py --out FILE           # write it
    python tools/wgrad_routes.py --check tests/golden/wgrad_routes.txt     # exit 1 and list the lines that differ

tests/golden/wgrad_routes.txt is the committed record (tests/test_wgrad_routing_cpu.py compares against it): a change of a routing rule
or of the split rule shows up as a diff of that file.  HD_HIP_LIB selects another build of the library.

A line is  `<hook> | N Hsrc Wsrc C1 C2 Cout K stride pad Ho Wo <options> -> <family> tm wtiles ptiles direct shared blocks nsplit`  with the
options u up1, c concat (x2), i in_scale, d dw_oihw, n<nsplit of the block>; the last number is the DEFAULT split of the problem
(ops.wgrad without nsplit), the others are hd_wgrad_route's out[1..6] (include/hallucidet_hip.h); `-> E` marks a block hd_wgrad refuses.
Hooks: `-` the shipped rules, tm=32|64|128 hd_wgrad_tune_override, HD_WGRAD_W8=0 / HD_WGRAD_SMALL=0 the environment knobs -- read once
per process, so those sections come from a fresh child process of this tool."""
import argparse
import ctypes as C
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
import conv_routes as cr      # noqa: E402

HOOKS = ["", "tm=32", "tm=64", "tm=128", "HD_WGRAD_W8=0", "HD_WGRAD_SMALL=0"]
EXTENTS = [(1, 1), (3, 8), (16, 8), (17, 9), (32, 32), (128, 160)]      # stored extent of x (up1 doubles it)
# (Cin | C1 = C2 of a concat, Cout) of the 3x3 / stride 1 / pad 1 product: every family's domain and its neighbours
PAIRS = [(16, 16), (32, 24), (64, 64), (64, 32), (128, 192), (24, 40), (72, 64), (256, 128)]
P = cr.P
SCRIPT = os.path.abspath(__file__)      # what a child process runs


def wcase(N, H, W, C1, Cout, K=3, stride=1, pad=1, C2=0, up1=False, opts="n1"):
    """a forward problem of conv_routes.case (grown to the kernel's extent where nothing would come out) with the weight gradient's options"""
    H, W = max(H, K - 2 * pad), max(W, K - 2 * pad)
    return cr.case(N, H, W, C1, Cout, K, stride, pad, C2=C2, up1=up1, opts=opts)


def product():
    """KSP x extents x {single, single up1, concat up1} x channels x {plain, in_scale} x nsplit {1, 7} x {slab, dw_oihw}: all of PAIRS for
    3x3 / 1 / 1, one rotating pair of CH_IN elsewhere"""
    out, n = [], 0
    for K, stride, pad in cr.KSP:
        for H, W in EXTENTS:
            for form in range(3):
                n += 1
                chans = PAIRS if (K, stride, pad) == (3, 1, 1) else [(cr.CH_IN[n % 13], cr.CH_IN[(5 * n + 3) % 13])]
                for cin, cout in chans:
                    out += [wcase((1, 2, 5)[n % 3], H, W, cin, cout, K, stride, pad, C2=cin if form == 2 else 0, up1=form > 0, opts=i + ns + d)
                            for i in ("", "i ") for ns in ("n1", "n7") for d in ("", " d")]
    return out


def at_the_bounds():
    """operands at hd_wgrad_w8_eligible's 2 GiB bound (x, dy, x2: on it -> general kernel, one column less -> 8-wave) and at the general
    kernel's 4 GiB bound (refused)"""
    L = [wcase(16, 1024, 1024, 64, 64), wcase(16, 1024, 1023, 64, 64), wcase(8, 1024, 1024, 64, 128), wcase(8, 1024, 1023, 64, 128),
         wcase(8, 512, 512, 64, 64, C2=128, up1=True), wcase(8, 512, 511, 64, 64, C2=128, up1=True),
         wcase(32, 1024, 1024, 64, 64), wcase(16, 1024, 1024, 128, 64)]
    return L + [dict(c, opts=("n1", "d")) for c in L]


def corpus():
    """[(hook, case)], deterministic, about 3 400 entries"""
    plain = []
    for N in (1, 2, 8):
        for c in cr.unet_layers(N):
            plain += [dict(c, opts=tuple(o.split())) for o in ("n1", "n1 d", "n7")]
            if c["C1"] in (16, 32) and not c["C2"]:
                plain.append(dict(c, opts=("i", "n1")))
    plain += [dict(c, opts=(o,)) for c in cr.detector_layers(8) for o in ("n1", "n7")]
    prod = product()
    plain += prod + at_the_bounds()
    swept = [dict(c, opts=tuple(o.split())) for c in cr.unet_layers(2) for o in ("n1", "i n1")] + at_the_bounds()[:8]
    swept += [c for o, k in ((("n1",), 3), (("i", "n1"), 9), (("n1", "d"), 9)) for c in [c for c in prod if c["opts"] == o][::k]]
    seen = set()      # (the layer lists repeat shapes)
    return [e for e in [("", c) for c in plain] + [(h, c) for h in HOOKS[1:] for c in swept] if not (key_of(*e) in seen or seen.add(key_of(*e)))]


def make_args(c, WgradArgs):
    o = c["opts"]
    a = WgradArgs()
    a.x, a.dy, a.x2 = P, P, (P if c["C2"] else None)
    a.slab, a.dw_oihw, a.dw_scale = (None, P, 1.0) if "d" in o else (P, None, 1.0)
    a.N, a.Hsrc, a.Wsrc, a.Hin, a.Win, a.C1, a.C2 = c["N"], c["H"], c["W"], c["Hin"], c["Win"], c["C1"], c["C2"]
    a.Ho, a.Wo, a.Cout, a.KH, a.KW, a.stride, a.pad, a.up1 = c["Ho"], c["Wo"], c["Cout"], c["K"], c["K"], c["stride"], c["pad"], int(c["up1"])
    a.nsplit = next(int(t[1:]) for t in o if t[0] == "n")
    if "i" in o:
        a.in_scale, a.in_shift, a.in_relu = P, P, 1
    return a


def load():
    from hallucidet_amd import _abi
    return _abi.load(), _abi.WgradArgs


def set_hook(lib, hook):
    """the in-process hooks; the environment knobs are the child process's business"""
    lib.hd_wgrad_tune_override(int(hook[3:]) if hook.startswith("tm=") else -1)


def key_of(hook, c):
    letters = ("u " if c["up1"] else "") + ("c " if c["C2"] else "") + " ".join(c["opts"])
    return "%s | %d %d %d %d %d %d %d %d %d %d %d %s" % (hook or "-", c["N"], c["H"], c["W"], c["C1"], c["C2"], c["Cout"], c["K"], c["stride"], c["pad"],
                                                        c["Ho"], c["Wo"], letters)


def route_of(lib, a):
    """the eight numbers of hd_wgrad_route, or None where the block is refused"""
    out = (C.c_int32 * 8)()
    return list(out) if lib.hd_wgrad_route(C.byref(a), out) == 0 else None


def answer(lib, WgradArgs, c):
    """the right-hand side of a line: the route of the block and the default split of the problem"""
    from hallucidet_amd import ops
    r = route_of(lib, make_args(c, WgradArgs))
    if r is None:
        return "E"
    plan = ops.wgrad_plan(c["N"], c["H"], c["W"], c["C1"], c["Ho"], c["Wo"], c["Cout"], c["K"], c["K"], C2=c["C2"], stride=c["stride"], pad=c["pad"],
                          up1=c["up1"], in_scale="i" in c["opts"])
    return "%s %s %d" % (ops.WGRAD_FAMILIES[r[0]], " ".join(map(str, r[1:7])), plan.nsplit)


def section(lib, WgradArgs, hook):
    """the lines of one hook, in this process"""
    try:
        set_hook(lib, hook)
        return [key_of(h, c) + " -> " + answer(lib, WgradArgs, c) for h, c in corpus() if h == hook]
    finally:
        set_hook(lib, "")


def table(lib, WgradArgs):
    lines = []
    for hook in HOOKS:
        if hook.startswith("HD_"):
            name, _, val = hook.partition("=")
            r = subprocess.run([sys.executable, SCRIPT, "--section", hook], env=dict(os.environ, **{name: val}), check=True, capture_output=True, text=True)
            lines += r.stdout.splitlines()
        else:
            lines += section(lib, WgradArgs, hook)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--check")
    ap.add_argument("--section", help="print the lines of one hook only (the environment is the caller's)")
    args = ap.parse_args()
    lines = section(*load(), args.section) if args.section else table(*load())
    if args.out:
        open(args.out, "w").write("\n".join(lines) + "\n")
    if args.check:
        want = open(args.check).read().splitlines()
        diff = [(a, b) for a, b in zip(want, lines) if a != b]
        for a, b in diff:
            print("- %s\n+ %s" % (a, b))
        print("wgrad_routes: %d cases, %d differ%s" % (len(lines), len(diff), "" if len(want) == len(lines) else ", %d recorded" % len(want)))
        return 1 if diff or len(want) != len(lines) else 0
    if not args.out:
        print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
