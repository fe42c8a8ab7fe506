"""The weight-gradient dispatcher's single routing decision, without a GPU: hd_wgrad_route and ops.wgrad_plan over the corpus of
tools/wgrad_routes.py against the committed table (tests/golden/wgrad_routes.txt, whose shipped section was recorded from the if-chains
the route replaced), the two older queries (hd_wgrad_w8_blocks, hd_wgrad_direct_ok) against the route they are views of, and the
geometry the U-Net's deferred-gradient planner takes from it.  Nothing here launches."""
import ctypes as C
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "wgrad_routes.txt")
FAMILIES = ("general", "small", "small-cat", "w8")


@pytest.fixture(scope="module")
def wr():
    spec = importlib.util.spec_from_file_location("wgrad_routes", os.path.join(ROOT, "tools", "wgrad_routes.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def lib(wr):
    import __graft_entry__ as ge
    ge.build()
    lib, _ = wr.load()
    yield lib
    wr.set_hook(lib, "")


@pytest.fixture(scope="module")
def table(wr, lib):
    """[(hook, case, right-hand side as a list of words)] of the corpus, computed once (two child processes for the environment knobs)"""
    from hallucidet_amd._abi import WgradArgs
    lines = wr.table(lib, WgradArgs)
    corpus = wr.corpus()
    assert len(lines) == len(corpus) and all(l.startswith(wr.key_of(h, c) + " -> ") for l, (h, c) in zip(lines, corpus))
    return [(h, c, l.split(" -> ")[1].split()) for l, (h, c) in zip(lines, corpus)]


def args_of(wr, c, **changes):
    from hallucidet_amd._abi import WgradArgs
    a = wr.make_args(c, WgradArgs)
    for k, v in changes.items():
        setattr(a, k, v)
    return a


def nsplit_of(c):
    return next(int(t[1:]) for t in c["opts"] if t[0] == "n")


def test_routes_equal_the_committed_table(wr, table):
    want = open(GOLDEN).read().splitlines()
    got = [wr.key_of(h, c) + " -> " + " ".join(rhs) for h, c, rhs in table]
    assert 2000 <= len(table) <= 3500 and len(table) == len(want)
    diff = [(w, g) for w, g in zip(want, got) if w != g]
    assert not diff, "%d routes changed (python tools/wgrad_routes.py --check tests/golden/wgrad_routes.txt), first: %s" % (len(diff), diff[:3])
    for hook in ("", "HD_WGRAD_W8=0", "HD_WGRAD_SMALL=0"):
        fams = {rhs[0] for h, _, rhs in table if h == hook}
        missing = set(FAMILIES) - fams - ({"w8"} if "W8" in hook else set()) - ({"small-cat"} if "SMALL" in hook else set())
        assert not missing and "E" in fams, "the %r section no longer reaches %s" % (hook, missing or "a refusal")


def test_w8_blocks_and_direct_ok_are_views_of_the_route(wr, lib, table):
    """on every block hd_wgrad accepts: hd_wgrad_w8_blocks > 0 <=> family w8 (then the route's weight tiles), hd_wgrad_direct_ok == 1 <=>
    family w8, nsplit == 1, no in_scale (the route's out[4]).  A refused block has no family of its own: the two queries then answer for
    the problem behind it (the same shape asked plainly), and 0 for every in_scale block outside the small kernel's domain."""
    n = n8 = 0
    for hook, c, rhs in table:
        if hook.startswith("HD_"):
            continue                             # (the knobs are read once per process: those sections are the child's)
        wr.set_hook(lib, hook)
        a = args_of(wr, c)
        blocks, direct = lib.hd_wgrad_w8_blocks(C.byref(a)), lib.hd_wgrad_direct_ok(C.byref(a))
        if rhs[0] == "E":
            r = wr.route_of(lib, args_of(wr, dict(c, opts=("n1",))))
            w8 = r is not None and FAMILIES[r[0]] == "w8" and "i" not in c["opts"]
            assert (blocks > 0) == w8 and (not w8 or blocks == r[2]), (hook, c, blocks, r)
            assert direct == (1 if w8 and nsplit_of(c) == 1 else 0), (hook, c, direct, r)
            continue
        r = wr.route_of(lib, a)
        assert FAMILIES[r[0]] == rhs[0] and [str(v) for v in r[1:7]] == rhs[1:7] and r[7] == 0, (hook, c, r, rhs)
        w8 = rhs[0] == "w8"
        assert (blocks > 0) == w8 and blocks == (r[2] if w8 else 0), (hook, c, blocks, r)
        assert direct == r[4] == (1 if w8 and nsplit_of(c) == 1 and "i" not in c["opts"] else 0), (hook, c, direct, r)
        assert r[5] == (1 if w8 else 0) and r[6] == r[2] * nsplit_of(c) and (r[1] > 0) == (rhs[0] == "general"), (hook, c, r)
        n += 1
        n8 += w8
    assert n > 800 and n8 > 100
    wr.set_hook(lib, "")


def test_families_keep_to_their_domains_under_every_hook(table):
    """in_scale runs in the small kernel or is refused; small => Cout <= 32 and w8 => Cout % 64 == 0 (the disjointness that lets wg_route test
    either domain without excluding the other); a tile override reaches neither special kernel, HD_WGRAD_W8=0 no 8-wave kernel, and
    HD_WGRAD_SMALL=0 the small kernel only for a raw operand, which nothing else implements."""
    seen = set()
    for hook, c, rhs in table:
        fam = rhs[0]
        seen.add((hook.split("=")[0], fam))
        if "i" in c["opts"]:
            assert fam in ("small", "E"), (hook, c, rhs)
        if fam in ("small", "small-cat"):
            assert c["Cout"] <= 32 and (c["C2"] == 0) == (fam == "small"), (hook, c, rhs)
        if fam == "w8":
            assert c["Cout"] % 64 == 0 and (c["C1"] + c["C2"]) % 64 == 0, (hook, c, rhs)
        if hook.startswith("tm="):
            assert fam in ("E", "general") and (fam == "E" or rhs[1] == hook[3:]), (hook, c, rhs)
        if hook == "HD_WGRAD_W8=0":
            assert fam != "w8", (hook, c, rhs)
        if hook == "HD_WGRAD_SMALL=0":
            assert fam != "small-cat" and (fam != "small" or "i" in c["opts"]), (hook, c, rhs)
    assert {("HD_WGRAD_SMALL", "small"), ("HD_WGRAD_SMALL", "w8"), ("HD_WGRAD_W8", "small-cat"), ("tm", "general"), ("tm", "E")} <= seen


def test_default_split_is_at_least_one_and_keeps_the_slab_within_64_mib(table):
    n = 0
    for hook, c, rhs in table:
        if rhs[0] == "E":
            continue
        ns, slab_bytes = int(rhs[7]), int(rhs[7]) * c["Cout"] * c["K"] * c["K"] * (c["C1"] + c["C2"]) * 4
        assert ns >= 1 and (ns == 1 or slab_bytes <= (64 << 20)), (hook, c, rhs)
        n += ns > 1
    assert n > 500


def test_wgrad_plan_reports_the_route_and_refuses_what_hd_wgrad_refuses(wr, lib):
    from hallucidet_amd import _abi, ops
    wr.set_hook(lib, "")
    p = ops.wgrad_plan(8, 128, 160, 64, 128, 160, 64, 3, 3, pad=1)
    assert p[:7] == ("w8", 0, 1, 8 * 8 * 20, False, True, 256) and p.nsplit == 256
    assert ops.wgrad_plan(8, 128, 160, 64, 128, 160, 64, 3, 3, pad=1, nsplit=1, dw=True).direct
    p = ops.wgrad_plan(2, 128, 160, 64, 256, 320, 32, 3, 3, C2=64, pad=1, up1=True)
    assert (p.family, p.weight_tiles, p.pixel_tiles, p.nsplit, p.blocks) == ("small-cat", 1, 2 * 32 * 10, 256, 256)
    p = ops.wgrad_plan(2, 9, 7, 24, 9, 7, 40, 1, 1, nsplit=3)
    assert p == ("general", 64, 1, 4, False, False, 3, 3)
    with pytest.raises(_abi.HipCallError, match="consumer-side BatchNorm"):
        ops.wgrad_plan(1, 8, 8, 64, 8, 8, 64, 3, 3, pad=1, in_scale=True)
    with pytest.raises(_abi.HipCallError, match="dw_oihw"):
        ops.wgrad_plan(1, 8, 8, 64, 8, 8, 64, 3, 3, pad=1, nsplit=2, dw=True)


@pytest.mark.parametrize("N", [1, 2, 8])
def test_unet_planner_takes_its_geometry_from_the_route(wr, lib, monkeypatch, N):
    """UnetRunner._plan_wgrads over the forward record of a 512 x 640 batch (shapes only: meta tensors) hands _plan_wgrad_splits, per launch
    group, exactly (weight tiles, pixel tiles) of the layers hd_wgrad_route sends to the 8-wave kernel -- the numbers it used to work out
    itself as (Cin / 64) * (Cout / 64) and N * ceil(Ho / 16) * ceil(Wo / 8)."""
    import torch
    from hallucidet_amd.segmentation_models import unet
    wr.set_hook(lib, "")
    runner = unet.UnetRunner(unet.Unet("resnet34", classes=3))
    meta = lambda *s: torch.empty(s, dtype=torch.float16, device="meta")
    rec = {}

    def put(u, x, x2=None, up1=False):
        h, w = (2 * x.shape[1], 2 * x.shape[2]) if up1 else x.shape[1:3]
        y = meta(N, (h + 2 * u.pad - u.k) // u.stride + 1, (w + 2 * u.pad - u.k) // u.stride + 1, u.cout_p)
        rec[u.name] = dict(x=x, x2=x2, up1=up1, y=y)
        return y

    feats = [put(runner.stem, meta(N, 512, 640, 8))]
    t = meta(N, 128, 160, 64)                    # after the max-pool
    for blocks in runner.stages:
        for us, ud in blocks:
            t0 = t
            for u in us:
                t = put(u, t)
            if ud is not None:
                put(ud, t0)
        feats.append(t)
    for (c1, c2, _, _), skip in zip(runner.dec, feats[-2::-1] + [None]):
        t = put(c2, put(c1, t, x2=skip, up1=True))
    runner.saved = dict(rec=rec)
    fed = []
    monkeypatch.setattr(unet, "_plan_wgrad_splits", lambda geo: fed.append(list(geo)) or [1] * len(geo))
    plan = runner._plan_wgrads()
    want, names = [[], []], [[], []]
    for g, segs in enumerate(([u for d in runner.dec for u in d[:2]] + [u for si in (3, 2) for us, ud in runner.stages[si] for u in us + ([ud] if ud else [])],
                              [u for si in (1, 0) for us, ud in runner.stages[si] for u in us + ([ud] if ud else [])])):
        for u in segs:
            r = rec[u.name]
            c = wr.cr.case(N, r["x"].shape[1], r["x"].shape[2], r["x"].shape[3], u.cout_p, u.k, u.stride, u.pad, C2=0 if r["x2"] is None else r["x2"].shape[3],
                           up1=r["up1"], opts="n1")
            assert (c["Ho"], c["Wo"]) == tuple(r["y"].shape[1:3])
            route = wr.route_of(lib, args_of(wr, c))
            if FAMILIES[route[0]] == "w8":
                assert route[2:4] == [(c["C1"] + c["C2"]) // 64 * (c["Cout"] // 64), N * -(-c["Ho"] // 16) * -(-c["Wo"] // 8)]
                want[g].append(tuple(route[2:4]))
                names[g].append(u.name)
    assert fed == want and len(want[0]) >= 20 and len(want[1]) >= 10
    assert plan == {n: (1, t) for g in (0, 1) for n, (_, t) in zip(names[g], want[g])}
