"""The detector-input resize (--detector-resize) without a GPU: the host tap tables against torch on float64, the legacy nearest index,
the coverage figures of the README, argument errors on the host and at the C boundary, and the flags' way to the transform."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from hallucidet_amd import resample
from hallucidet_amd.resample import resample_taps

AXES = [(1, 3), (3, 1), (7, 5), (9, 4), (4, 9), (5, 11), (37, 30), (53, 30), (512, 300), (640, 300), (1024, 300), (1280, 300), (512, 640),
        (640, 640)]
IDS = ["%dto%d" % a for a in AXES]


def _torch_axis(x, n_out, mode):
    """F.interpolate along the first axis of a float64 [in, K] matrix -> [out, K]."""
    t = torch.from_numpy(x)[None, None]
    kw = dict(mode="bilinear", align_corners=False, antialias=(mode == "bilinear_aa"))
    return F.interpolate(t, size=(n_out, x.shape[1]), **kw)[0, 0].numpy()


@pytest.mark.parametrize("n_in,n_out", AXES, ids=IDS)
@pytest.mark.parametrize("mode", ["bilinear", "bilinear_aa"])
def test_table_reproduces_torch_on_float64(n_in, n_out, mode):
    t = resample_taps(n_in, n_out, mode)
    rng = np.random.default_rng(n_in * 1000 + n_out)
    x = rng.standard_normal((n_in, 5))
    x[:, 0] = np.arange(n_in)                       # a ramp: a shifted tap shows as a whole unit
    got = np.zeros((n_out, 5))
    for o in range(n_out):                          # the tables as the kernel applies them, in float64
        for i in range(t.count[o]):
            got[o] += t.weight64[o, i] * x[t.start[o] + i]
    ref = _torch_axis(x, n_out, mode)
    rel = np.abs(got - ref).max() / max(np.abs(ref).max(), 1.0)
    assert rel <= 1e-12, rel
    # the forward form: non-negative, a partition of unity before the fp32 rounding, zero past the count
    assert (t.weight64 >= 0).all() and (t.weight >= 0).all()
    assert np.abs(t.weight64.sum(1) - 1.0).max() <= 1e-12
    assert t.T == t.count.max() <= resample.MAX_TAPS and t.count.min() >= 1
    assert t.start.min() >= 0 and (t.start + t.count).max() <= n_in
    for o in range(n_out):
        assert (t.weight[o, t.count[o]:] == 0).all()
    assert t.weight.dtype == np.float32 and t.start.dtype == np.int32 and t.count.dtype == np.int32
    assert (t.weight == t.weight64.astype(np.float32)).all()
    # the low part: what fp32 drops of the float64 weight, itself an fp32 number; weight + weight_lo is the weight to about 2^-48
    assert t.weight_lo.dtype == np.float32 and t.weight_lo.shape == t.weight.shape
    assert (t.weight_lo == (t.weight64 - t.weight.astype(np.float64)).astype(np.float32)).all()
    assert (np.abs(t.weight_lo) <= 2.0 ** -24 * t.weight).all()
    assert np.abs(t.weight.astype(np.float64) + t.weight_lo.astype(np.float64) - t.weight64).max() <= 2.0 ** -48


@pytest.mark.parametrize("n_in,n_out", AXES, ids=IDS)
@pytest.mark.parametrize("mode", resample.MODES)
def test_transposed_form_holds_exactly_the_forward_entries(n_in, n_out, mode):
    t = resample_taps(n_in, n_out, mode)
    fwd = sorted((int(t.start[o]) + i, o, float(t.weight[o, i])) for o in range(n_out) for i in range(t.count[o]))
    assert t.rstart.shape == (n_in + 1,) and t.rstart[0] == 0 and t.rstart[-1] == t.nnz == len(fwd)
    assert t.rstart.dtype == np.int32 and t.rout.dtype == np.int32 and t.rweight.dtype == np.float32
    bwd = []
    for r in range(n_in):
        row = t.rout[t.rstart[r]:t.rstart[r + 1]]
        assert (np.diff(row) > 0).all()                                   # ascending output index within a row
        bwd += [(r, int(o), float(w)) for o, w in zip(row, t.rweight[t.rstart[r]:t.rstart[r + 1]])]
    assert bwd == fwd                                                     # the same weights bit for bit, not recomputed
    assert (t.dense(np.float32) != 0).sum() == t.nnz                       # and every listed entry moves data


@pytest.mark.parametrize("n_in,n_out", AXES, ids=IDS)
def test_nearest_indices_equal_torch(n_in, n_out):
    t = resample_taps(n_in, n_out, "nearest")
    assert t.T == 1 and (t.count == 1).all() and (t.weight == 1.0).all()
    ramp = torch.arange(n_in, dtype=torch.float32).view(1, 1, n_in, 1)
    ref = F.interpolate(ramp, size=(n_out, 1), mode="nearest").view(-1).to(torch.int64).numpy()
    assert (t.start == ref).all(), np.nonzero(t.start != ref)[0]
    # the existing kernel's formula (nn_src of csrc/elementwise.hip), spelled out
    scale = np.float32(n_in) / np.float32(n_out)
    want = np.minimum(np.floor(np.arange(n_out, dtype=np.float32) * scale).astype(np.int64), n_in - 1)
    assert (t.start == want).all()


def test_coverage_figures_come_from_the_transposed_tables():
    """Share of the pixels of one image with a non-zero resize gradient (README 'Detector input resize'): product of the two axes'
    shares of non-empty transposed rows."""
    def cov(h, w, ho, wo, mode):
        return 100.0 * resample_taps(h, ho, mode).coverage() * resample_taps(w, wo, mode).coverage()
    table = {(512, 640, 300, 300): (27.47, 93.75, 100.0), (1024, 1280, 300, 300): (6.87, 27.47, 100.0), (512, 640, 640, 640): (100.0, 100.0, 100.0)}
    for shape, want in table.items():
        got = tuple(cov(*shape, m) for m in resample.MODES)
        assert all(abs(g - w) < 0.005 for g, w in zip(got, want)), (shape, got)


def test_coverage_equals_autograd_on_float64():
    """The tables' coverage is what torch autograd reports (small shapes; the README's figures were computed this way)."""
    for (h, w, ho, wo) in [(9, 7, 4, 5), (37, 53, 30, 30), (4, 5, 9, 11)]:
        for mode in resample.MODES:
            x = torch.rand(1, 1, h, w, dtype=torch.float64, requires_grad=True)
            if mode == "nearest":
                y = F.interpolate(x, size=(ho, wo))
            else:
                y = F.interpolate(x, size=(ho, wo), mode="bilinear", align_corners=False, antialias=(mode == "bilinear_aa"))
            y.sum().backward()
            want = float((x.grad != 0).double().mean())
            got = resample_taps(h, ho, mode).coverage() * resample_taps(w, wo, mode).coverage()
            assert abs(got - want) < 1e-12, (h, w, ho, wo, mode)


def test_host_argument_errors():
    with pytest.raises(ValueError, match="mode"):
        resample_taps(8, 4, "bicubic")
    with pytest.raises(ValueError, match="taps"):
        resample_taps(1000, 10, "bilinear_aa")           # a support of 100 input pixels either side
    with pytest.raises(ValueError, match="taps"):
        resample_taps(330, 20, "bilinear_aa")            # 2 * 16.5 taps
    assert resample_taps(1000, 10, "bilinear").T == 2    # the two-tap mode has no such limit
    for bad in [(0, 4), (4, 0), (-1, 3)]:
        with pytest.raises(ValueError, match=">= 1"):
            resample_taps(bad[0], bad[1], "bilinear")
    with pytest.raises(ValueError, match="image_mean"):
        resample.normalize_stats([0.1, 0.2], [1.0])
    with pytest.raises(ValueError, match="image_std"):
        resample.normalize_stats([0.0], [1.0, 1.0, 1.0, 1.0])
    with pytest.raises(ValueError, match="> 0"):
        resample.normalize_stats([0.0], [1.0, 0.0, 1.0])
    assert resample.normalize_stats([0.5], None) == ((0.5, 0.5, 0.5), (1.0, 1.0, 1.0))
    assert resample.normalize_stats(None, None) == ((0.0,) * 3, (1.0,) * 3)


def test_transform_takes_the_mode_and_the_statistics():
    from hallucidet_amd.models.custom_generalized_transform import CustomGeneralizedRCNNTransform as T
    t = T(300, 300, [0.0] * 3, [1.0] * 3, fixed_size=(300, 300))
    assert t.interpolation == "nearest" and t._legacy and "nearest" in repr(t)
    t = T(300, 300, [0.485, 0.456, 0.406], [0.229], fixed_size=(300, 300), interpolation="bilinear_aa")
    assert not t._legacy and t.std == (0.229,) * 3
    assert "bilinear_aa" in repr(t) and "0.485" in repr(t) and "0.229" in repr(t)
    assert not T(300, 300, [0.0], [1.0], fixed_size=(300, 300), interpolation="bilinear")._legacy
    assert not T(300, 300, [0.5], [1.0], fixed_size=(300, 300))._legacy
    with pytest.raises(ValueError, match="interpolation"):
        T(300, 300, [0.0], [1.0], fixed_size=(300, 300), interpolation="bicubic")
    with pytest.raises(ValueError, match="image_mean"):
        T(300, 300, [0.0, 0.0], [1.0], fixed_size=(300, 300))
    with pytest.raises(ValueError, match="> 0"):
        T(300, 300, [0.0], [0.0], fixed_size=(300, 300))
    with pytest.raises(NotImplementedError):
        T(300, 300, [0.0], [1.0], interpolation="bilinear")              # fixed_size stays mandatory


def test_flags_reach_config():
    from hallucidet_amd.config import Config
    args = Config.argument_parser([])
    assert args.detector_resize == "nearest" and args.detector_norm == "none"
    args = Config.argument_parser(["--detector-resize", "bilinear_aa", "--detector-norm", "imagenet"])
    assert args.detector_resize == "bilinear_aa" and args.detector_norm == "imagenet"
    assert Config.detector_norm_stats("none") == (None, None)
    assert Config.detector_norm_stats("imagenet") == (list(resample.IMAGENET_MEAN), list(resample.IMAGENET_STD))
    with pytest.raises(SystemExit):
        Config.argument_parser(["--detector-resize", "bicubic"])


def test_ops_wrapper_refuses_mismatches(monkeypatch):
    from hallucidet_amd import ops
    monkeypatch.setattr(ops, "_need_cuda", lambda *ts: None)
    x = torch.empty(2, 3, 8, 12, device="meta")
    with pytest.raises(ValueError, match="mode"):
        ops.image_resample(x, 4, 4, "bicubic")
    with pytest.raises(TypeError, match="float32"):
        ops.image_resample(x.half(), 4, 4, "bilinear")
    with pytest.raises(ValueError, match="dense"):
        ops.image_resample(x[:, :, :, ::2], 4, 4, "bilinear")
    with pytest.raises(ValueError, match="mean"):
        ops.image_resample(x, 4, 4, "bilinear", mean=[0.1, 0.2])
    with pytest.raises(ValueError, match="std"):
        ops.image_resample(x, 4, 4, "bilinear", std=[1.0, 0.0, 1.0])
    with pytest.raises(ValueError, match="channels"):
        ops.image_resample(torch.empty(2, 9, 8, 12, device="meta"), 4, 4, "bilinear")
    with pytest.raises(ValueError, match="out must be"):
        ops.image_resample(x, 4, 4, "bilinear", out=torch.empty(2, 4, 5, 8, device="meta", dtype=torch.float16))
    with pytest.raises(ValueError, match="dy must be"):
        ops.image_resample_bwd(torch.empty(2, 4, 4, 16, device="meta", dtype=torch.float16), 2, 3, 8, 12, "bilinear")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from hallucidet_amd import _abi
    return _abi.load()


def test_c_entry_points_reject_bad_arguments(lib):
    """Null pointers and shapes are refused with a status code and a text before anything is launched (host buffers pose as device
    pointers: no call here reaches a launch)."""
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    std0 = (ctypes.c_float * 3)(1.0, 0.0, 1.0)
    for name in ("hd_image_resample", "hd_image_resample_f32"):
        f = getattr(lib, name)
        assert f(None, 0, 0, None, 1, 3, 4, 4, 2, 2, 8, p, p, p, 1, p, p, p, 1, None, None, None, None, None) == -1
        assert name.encode()[:17] in lib.hd_last_error() and b"null" in lib.hd_last_error()
        assert f(p, 48, 16, p, 1, 3, 4, 4, 2, 2, 8, None, p, p, 1, p, p, p, 1, None, None, None, None, None) == -1
        assert b"tap table" in lib.hd_last_error()
        assert f(p, 48, 16, p, 1, 3, 4, 0, 2, 2, 8, p, p, p, 1, p, p, p, 1, None, None, None, None, None) == -1
        assert b"bad shape" in lib.hd_last_error()
        assert f(p, 48, 16, p, 1, 9, 4, 4, 2, 2, 8, p, p, p, 1, p, p, p, 1, None, None, None, None, None) == -1
        assert b"Cr" in lib.hd_last_error()
        assert f(p, 48, 16, p, 1, 3, 4, 4, 2, 2, 16, p, p, p, 1, p, p, p, 1, None, None, None, None, None) == -1
        assert b"Cp" in lib.hd_last_error()
        assert f(p, 48, 16, p, 1, 3, 4, 4, 2, 2, 8, p, p, p, 33, p, p, p, 1, None, None, None, None, None) == -1
        assert b"taps" in lib.hd_last_error()
        assert f(p, 48, 8, p, 1, 3, 4, 4, 2, 2, 8, p, p, p, 1, p, p, p, 1, None, None, None, None, None) == -1
        assert b"cstride" in lib.hd_last_error()
        assert f(p, 8, 0, p, 2, 3, 4, 4, 2, 2, 8, p, p, p, 1, p, p, p, 1, None, None, None, None, None) == -1
        assert b"nstride" in lib.hd_last_error()
        assert f(p, 48, 16, p, 1, 3, 4, 4, 2, 2, 8, p, p, p, 1, p, p, p, 1, None, std0, None, None, None) == -1
        assert b"std" in lib.hd_last_error()
        assert f(p, 48, 16, p, 1, 3, 4, 4, 2, 2, 8, p, p, p, 1, p, p, p, 1, None, None, p, None, None) == -1          # one low-part table alone
        assert b"weight_lo" in lib.hd_last_error()
    for name in ("hd_image_resample_bwd", "hd_image_resample_bwd_f32"):
        f = getattr(lib, name)
        assert f(None, None, 1, 3, 4, 4, 2, 2, 8, p, p, p, 2, p, p, p, 2, None, 1.0, None) == -1
        assert b"hd_image_resample_bwd" in lib.hd_last_error() and b"null" in lib.hd_last_error()
        assert f(p, p, 1, 3, 4, 4, 2, 2, 8, p, p, None, 2, p, p, p, 2, None, 1.0, None) == -1
        assert b"tap table" in lib.hd_last_error()
        assert f(p, p, 0, 3, 4, 4, 2, 2, 8, p, p, p, 2, p, p, p, 2, None, 1.0, None) == -1
        assert b"bad shape" in lib.hd_last_error()
        assert f(p, p, 1, 9, 4, 4, 2, 2, 8, p, p, p, 2, p, p, p, 2, None, 1.0, None) == -1
        assert b"Cr" in lib.hd_last_error()
        assert f(p, p, 1, 3, 4, 4, 2, 2, 8, p, p, p, 0, p, p, p, 2, None, 1.0, None) == -1
        assert b"entries" in lib.hd_last_error()
        assert f(p, p, 1, 3, 4, 4, 2, 2, 8, p, p, p, 65, p, p, p, 2, None, 1.0, None) == -1
        assert b"entries" in lib.hd_last_error()
        assert f(p, p, 1, 3, 4, 4, 2, 2, 8, p, p, p, 2, p, p, p, 2, std0, 1.0, None) == -1
        assert b"std" in lib.hd_last_error()


def _check(lib, t, **over):
    a = {k: np.array(getattr(t, k)) for k in ("start", "count", "weight", "rstart", "rout", "rweight", "weight_lo")}
    a.update({k: v for k, v in over.items() if k in a})
    q = lambda v: v.ctypes.data_as(ctypes.c_void_p)
    return lib.hd_resample_taps_check(q(a["start"]), q(a["count"]), q(a["weight"]), over.get("in_size", t.in_size), t.out_size, over.get("T", t.T),
                                      q(a["rstart"]), q(a["rout"]), q(a["rweight"]), over.get("nnz", t.nnz), q(a["weight_lo"]))


def test_c_table_check_accepts_every_table_and_names_a_bad_index(lib):
    for n_in, n_out in AXES:
        for mode in resample.MODES:
            t = resample_taps(n_in, n_out, mode)
            assert _check(lib, t) == 0, (n_in, n_out, mode, lib.hd_last_error())
            resample.check_taps(t)
    t = resample_taps(9, 4, "bilinear_aa")
    assert lib.hd_resample_taps_check(None, None, None, 9, 4, 1, None, None, None, 1, None) == -1 and b"null" in lib.hd_last_error()
    assert _check(lib, t, T=33) == -1 and b"taps" in lib.hd_last_error()
    assert _check(lib, t, in_size=8) == -1 and b"leave the input" in lib.hd_last_error()          # the last taps now end past the input
    s = np.array(t.start); s[0] = -1
    assert _check(lib, t, start=s) == -1 and b"leave the input" in lib.hd_last_error()
    c = np.array(t.count); c[1] = t.T + 1
    assert _check(lib, t, count=c) == -1 and b"count[1]" in lib.hd_last_error()
    w = np.array(t.weight); w[2, 0] = np.nan
    assert _check(lib, t, weight=w) == -1 and b"finite" in lib.hd_last_error()
    r = np.array(t.rout); r[3] = 4
    assert _check(lib, t, rout=r) == -1 and b"outside the output" in lib.hd_last_error()
    r = np.array(t.rout); r[0] = -2
    assert _check(lib, t, rout=r) == -1 and b"outside the output" in lib.hd_last_error()
    rs = np.array(t.rstart); rs[4] = t.nnz + 5
    assert _check(lib, t, rstart=rs) == -1 and b"rstart" in lib.hd_last_error()
    rw = np.array(t.rweight); rw[5] *= 0.5
    assert _check(lib, t, rweight=rw) == -1 and b"forward weight" in lib.hd_last_error()
    assert _check(lib, t, nnz=t.nnz - 1) == -1 and b"entries" in lib.hd_last_error()
    wl = np.array(t.weight_lo); wl[1, 0] = t.weight[1, 0] * 2.0 ** -20
    assert _check(lib, t, weight_lo=wl) == -1 and b"weight_lo[1][0]" in lib.hd_last_error()
