"""The convolution dispatcher's single routing decision, without a GPU: hd_conv2d_route over the corpus of tools/conv_routes.py against
the committed table (tests/golden/conv_routes.txt, recorded from the if-chains the route replaced), and the three queries
(hd_conv2d_stats_rows, hd_conv2d_bstat_ok, hd_conv2d_pool2_ok) against the route they must agree with.  None of them launches."""
import ctypes as C
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "conv_routes.txt")
SMALL, C64, STEM, C32, CAT, GEMM8, P8, M160, IGEMM32, IGEMM64 = range(10)
P = 0x1000


@pytest.fixture(scope="module")
def cr():
    spec = importlib.util.spec_from_file_location("conv_routes", os.path.join(ROOT, "tools", "conv_routes.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def lib(cr):
    import __graft_entry__ as ge
    ge.build()
    lib, _ = cr.load()
    yield lib
    cr.set_hook(lib, "")


@pytest.fixture(scope="module")
def blocks(cr, lib):
    """[(hook, case, route or None)] of the corpus, computed once"""
    from hallucidet_amd._abi import ConvArgs
    out = []
    for hook, c in cr.corpus():
        cr.set_hook(lib, hook)
        out.append((hook, c, cr.route_of(lib, cr.make_args(c, ConvArgs))))
    cr.set_hook(lib, "")
    return out


def args_of(cr, c, **changes):
    from hallucidet_amd._abi import ConvArgs
    a = cr.make_args(c, ConvArgs)
    for k, v in changes.items():
        setattr(a, k, v)
    return a


def with_bs(a):
    a.stats, a.bs_y, a.bs_mean, a.bs_invstd = P, P, P, P
    return a


def test_routes_equal_the_committed_table(cr, lib):
    want = open(GOLDEN).read().splitlines()
    from hallucidet_amd._abi import ConvArgs
    got = cr.table(lib, ConvArgs)
    assert 2000 <= len(got) <= 3200 and len(got) == len(want)
    diff = [(w, g) for w, g in zip(want, got) if w != g]
    assert not diff, "%d routes changed (python tools/conv_routes.py --check tests/golden/conv_routes.txt), first: %s" % (len(diff), diff[:3])
    fams = {l.split(" -> ")[1].split()[0] for l in got}
    assert fams >= set(cr.FAMILIES), "the corpus no longer reaches %s" % (set(cr.FAMILIES) - fams)
    assert any(l.split()[-4] == "1" for l in got if not l.endswith("E")), "no parity-class launch in the corpus"


def test_stats_rows_is_the_routes_row_count_with_or_without_the_slab(cr, lib, blocks):
    n = 0
    for hook, c, r in blocks:
        cr.set_hook(lib, hook)
        with_slab, without = lib.hd_conv2d_stats_rows(C.byref(args_of(cr, c, stats=P))), lib.hd_conv2d_stats_rows(C.byref(args_of(cr, c, stats=None)))
        assert with_slab == without, (hook, c)
        if r is not None:
            assert r[6] == with_slab > 0, (hook, c, r)
            n += 1
            if "s" in c["opts"]:                 # launched with the slab: the rows are those of the family that runs
                assert r[0] not in (C32, GEMM8) and r[4] == 0, (hook, c, r)
                if r[0] in (IGEMM32, IGEMM64):
                    assert r[6] == -(-r[5] // r[1]) and r[5] == c["N"] * c["Ho"] * c["Wo"], (hook, c, r)
                elif r[0] in (C64, STEM, CAT):
                    assert r[6] == r[7], (hook, c, r)
    assert n > 2000


def test_bstat_ok_ignores_the_bs_fields_and_names_a_family_that_implements_them(cr, lib, blocks):
    ones = 0
    for hook, c, _ in blocks:
        if any(t in c["opts"] for t in ("b", "m", "o1", "o2")) or any(t[0] == "a" and t != "a0" for t in c["opts"]):
            continue                             # bs_* exclude bias / mask / act / non-f16 output: no such block can be launched
        cr.set_hook(lib, hook)
        plain = args_of(cr, c, bs_y=None, bs_z=None, bs_mean=None, bs_invstd=None, bs_gamma=None, bs_beta=None)
        ok = lib.hd_conv2d_bstat_ok(C.byref(plain))
        assert ok == lib.hd_conv2d_bstat_ok(C.byref(with_bs(args_of(cr, c)))), (hook, c)
        if any(t[0] == "p" for t in c["opts"]):
            continue                             # (no kernel combines the sums with out_pool2: nothing to route)
        r = cr.route_of(lib, with_bs(args_of(cr, c)))
        if ok == 1:
            ones += 1
            assert r is not None and r[0] in (C64, P8, M160), (hook, c, r)
            assert r[6] == lib.hd_conv2d_stats_rows(C.byref(with_bs(args_of(cr, c, stats=None)))), (hook, c, r)
        else:
            assert r is None, (hook, c, r)       # hd_conv2d refuses bs_* where the query says 0
    assert ones > 300


def pool2_request_is_implemented(c, r):
    """the rules of include/hallucidet_hip.h (hd_conv_args.out_pool2), per family"""
    o = c["opts"]
    pool2 = next((int(t[1:]) for t in o if t[0] == "p"), 0)
    even = c["Ho"] % 2 == 0 and c["Wo"] % 2 == 0
    plain = not any(t in o for t in ("s", "r", "b", "m", "B")) and not any(t[0] == "a" and t != "a0" for t in o)
    split_ok = pool2 <= c["Cout"] and (c["Cout"] - pool2) % 8 == 0 and (pool2 == c["Cout"] or "y" in o)
    if not pool2 or r is None:
        return False
    if r[0] == SMALL:
        return pool2 == c["Cout"] and "y" not in o and even and "s" not in o and "i" not in o and "o1" not in o and "o2" not in o
    if r[0] == C32:
        return pool2 == 64 and "y" in o and even
    if r[0] == P8:
        return plain and even and pool2 % 128 == 0 and split_ok
    if r[0] == M160:
        return plain and even and pool2 % 64 == 0 and split_ok
    return False


def test_pool2_ok_is_one_exactly_where_the_routes_family_implements_the_request(cr, lib, blocks):
    ones = 0
    for hook, c, _ in blocks:
        cr.set_hook(lib, hook)
        ok = lib.hd_conv2d_pool2_ok(C.byref(args_of(cr, c)))
        if not any(t[0] == "p" for t in c["opts"]):
            assert ok == 0, (hook, c)
            continue
        r = cr.route_of(lib, args_of(cr, c))
        assert (r is not None) == (ok == 1), (hook, c, r)
        # where hd_conv2d refuses the block, the family is that of the same problem without the request
        r = r or cr.route_of(lib, args_of(cr, c, out_pool2=0, y2=None))
        assert ok == (1 if pool2_request_is_implemented(c, r) else 0), (hook, c, r)
        ones += ok
    assert ones > 50


@pytest.mark.parametrize("hw", [(3, 8), (1, 16)])
def test_rows_promised_for_the_cat_shapes_with_bs_are_the_rows_of_the_launch(cr, lib, hw):
    """3x3 / up1 / 64 + 64 -> 32: the cat 128 -> 32 kernel does not implement bs_*, so with them the problem runs on an 8-wave tile with
    another row count (3 x 8: 1 row without, 2 with; 1 x 16: 2 without, 1 with).  The query answers for the block as launched."""
    cr.set_hook(lib, "")
    c = cr.case(1, hw[0], hw[1], 64, 32, C2=64, up1=True)
    assert cr.route_of(lib, args_of(cr, c, stats=P))[0] == CAT
    launched = cr.route_of(lib, with_bs(args_of(cr, c)))
    assert launched[0] in (P8, M160)
    assert lib.hd_conv2d_stats_rows(C.byref(with_bs(args_of(cr, c, stats=None)))) == launched[6] == lib.hd_conv2d_stats_rows(C.byref(with_bs(args_of(cr, c))))
    th, tw = (launched[1], launched[2]) if launched[0] == M160 else ((32 if (launched[1] & 3) in (0, 2) else 16), 8)
    assert launched[6] == -(-2 * hw[0] // th) * -(-2 * hw[1] // tw)
    assert lib.hd_conv2d_stats_rows(C.byref(args_of(cr, c))) == -(-2 * hw[0] // 8) * -(-2 * hw[1] // 16) != launched[6]
