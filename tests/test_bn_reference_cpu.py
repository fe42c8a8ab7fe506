"""The float64 BatchNorm definitions of tests/_bn_reference.py checked without a GPU: against torch's own batch_norm and its
autograd, and the input builders / tolerances against the properties the GPU tests rely on."""
import pytest
import torch
import torch.nn.functional as F

import _bn_reference as R


def _double_case(npix, C, seed):
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    return {"y": rnd(npix, C) * 1.5 + rnd(C), "res": rnd(npix, C), "dz": rnd(npix, C), "gamma": rnd(C), "beta": rnd(C),
            "rm": rnd(C), "rv": torch.rand(C, generator=g, dtype=torch.float64) + 0.5}


def _stat_row(y):
    return torch.cat([y.sum(0), (y * y).sum(0)]).reshape(1, -1)


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("momentum", [0.25, 1.0])      # exact in fp32: the kernels take momentum as a float
def test_forward_matches_torch_batch_norm(with_res, relu, momentum):
    npix, C, eps = 37, 5, 0.0078125
    d = _double_case(npix, C, 1)
    rm, rv = d["rm"].clone(), d["rv"].clone()
    want = F.batch_norm(d["y"], rm, rv, d["gamma"], d["beta"], training=True, momentum=momentum, eps=eps)
    if with_res:
        want = want + d["res"]
    if relu:
        want = torch.relu(want)
    f = R.ref_finalize(_stat_row(d["y"]), npix, d["gamma"], d["beta"], d["rm"], d["rv"], momentum, eps)
    got, mag = R.ref_apply(d["y"], f["scale"], f["shift"], d["res"] if with_res else None, relu)
    assert torch.allclose(got, want, rtol=0, atol=1e-10)
    assert torch.allclose(f["running_mean"], rm, rtol=0, atol=1e-10) and torch.allclose(f["running_var"], rv, rtol=0, atol=1e-10)
    assert torch.allclose(f["mean"], d["y"].mean(0), rtol=0, atol=1e-10)
    assert torch.allclose(f["invstd"], 1 / torch.sqrt(d["y"].var(0, unbiased=False) + eps), rtol=0, atol=1e-10)
    assert bool((mag >= got.abs() - 1e-12).all())


def test_finalize_count_one_keeps_the_biased_variance_and_clamps():
    part = torch.tensor([[1.0, 3.0, 1.5, 1.0]], dtype=torch.float64)       # C = 2: var 0.5, and 1 - 9 < 0 -> 0
    f = R.ref_finalize(part, 1, None, None, torch.zeros(2), torch.zeros(2), 1.0, 0.25)
    assert torch.equal(f["var"], torch.tensor([0.5, 0.0], dtype=torch.float64))
    assert torch.equal(f["running_var"], f["var"]) and torch.equal(f["invstd"][1:], torch.tensor([2.0], dtype=torch.float64))


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("gscale,accumulate", [(1.0, False), (0.5, True), (2.0 ** -7, False)])
def test_backward_matches_autograd(with_res, relu, gscale, accumulate):
    npix, C, eps = 41, 6, 0.0078125
    d = _double_case(npix, C, 2)
    y, res = d["y"].clone().requires_grad_(True), d["res"].clone().requires_grad_(True)
    gamma, beta = d["gamma"].clone().requires_grad_(True), d["beta"].clone().requires_grad_(True)
    z = F.batch_norm(y, None, None, gamma, beta, training=True, eps=eps)
    if with_res:
        z = z + res
    if relu:
        z = torch.relu(z)
    (z * d["dz"]).sum().backward()
    f = R.ref_finalize(_stat_row(d["y"]), npix, d["gamma"], d["beta"], None, None, 0.1, eps)
    zsaved = z.detach() if (with_res and relu) else None          # a residual unit's mask comes from its saved output
    s = R.ref_bwd_sums(d["dz"], zsaved, d["y"], f["mean"], f["invstd"], d["gamma"], d["beta"], relu)
    part = torch.cat([s["sg"], s["sgx"]]).reshape(1, -1)
    old_g, old_b = (d["rm"], d["rv"]) if accumulate else (None, None)
    b = R.ref_bwd_apply(d["dz"], zsaved, d["y"], f["mean"], f["invstd"], d["gamma"], d["beta"], part, relu, gscale, old_g, old_b)
    assert torch.allclose(b["dy"], y.grad, rtol=0, atol=1e-10)
    if with_res:
        assert torch.allclose(b["dres"], res.grad, rtol=0, atol=1e-10)
    want_g, want_b = gscale * gamma.grad, gscale * beta.grad
    if accumulate:
        want_g, want_b = want_g + old_g, want_b + old_b
    assert torch.allclose(b["dgamma"], want_g, rtol=0, atol=1e-10) and torch.allclose(b["dbeta"], want_b, rtol=0, atol=1e-10)
    assert bool((b["dy_mag"] >= b["dy"].abs() - 1e-12).all())
    assert bool((s["abs_sg"] >= s["sg"].abs()).all()) and bool((s["abs_sgx"] >= s["sgx"].abs()).all())


@pytest.mark.parametrize("npix,C,dtype", [(20000, 8, torch.float16), (3001, 64, torch.float32), (257, 2048, torch.float16)])
def test_integer_inputs_sum_exactly_in_fp32_in_any_order(npix, C, dtype):
    d = R.integer_inputs(npix, C, dtype, 3, with_z=True)
    pre = R.preactivation(d["y"], d["mean"], d["invstd"], d["gamma"], d["beta"])
    assert bool((pre.abs() >= 0.125).all()) and torch.equal(pre.to(dtype).double(), pre)
    for z in (None, d["z"]):
        s = R.ref_bwd_sums(d["dz"], z, d["y"], d["mean"], d["invstd"], d["gamma"], d["beta"], True)
        gk = s["gk"].float()
        t = gk * ((d["y"].float() - d["mean"]) * d["invstd"])
        perm = torch.randperm(npix, generator=torch.Generator().manual_seed(4))
        for terms, want in ((gk, s["sg"]), (t, s["sgx"])):
            fwd = torch.zeros(C)
            for chunk in terms.split(97):                            # a serial fp32 chain of 97-pixel pieces ...
                fwd = fwd + chunk.sum(0, dtype=torch.float32)
            other = terms[perm].flip(0).reshape(-1, C).cumsum(0, dtype=torch.float32)[-1]     # ... and a shuffled running sum
            assert torch.equal(fwd, other) and torch.equal(fwd.double(), want)
        assert float(s["abs_sgx"].max()) < 2 ** 23


@pytest.mark.parametrize("npix,C,dtype", [(1, 8, torch.float16), (2000, 8, torch.float16), (300, 2048, torch.float32)])
def test_random_inputs_keep_the_mask_away_from_zero(npix, C, dtype):
    d = R.random_inputs(npix, C, dtype, 5, with_z=True)
    assert R.mask_margin_violations(d) == 0
    assert d["y"].dtype == dtype and d["dz"].dtype == dtype and d["mean"].dtype == torch.float32
    # the kernel's own test, emulated: one fused multiply-add in fp32, rounded to the storage type
    sc = d["gamma"] * d["invstd"]
    sh = d["beta"] - d["mean"] * d["gamma"] * d["invstd"]
    fma = (d["y"].double() * sc.double() + sh.double()).float().to(dtype)
    assert torch.equal(fma > 0, R.ref_mask(None, d["y"], d["mean"], d["invstd"], d["gamma"], d["beta"], True))


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("with_res,relu", [(False, False), (True, True)])
def test_fp32_emulation_of_bn_apply_is_inside_the_element_tolerance(dtype, with_res, relu):
    npix, C = 4099, 64
    d = R.random_inputs(npix, C, dtype, 6, with_res=True)
    g = torch.Generator().manual_seed(7)
    scale = (torch.randn(C, generator=g) * 2).float()
    shift = torch.randn(C, generator=g).float()
    res = d["res"] if with_res else None
    f = (d["y"].double() * scale.double() + shift.double()).float()          # fmaf: one rounding
    if with_res:
        f = f + res.float()
    if relu:
        f = torch.relu(f)
    want, mag = R.ref_apply(d["y"], scale, shift, res, relu)
    ratio = R.worst_ratio(f.to(dtype), want, R.elem_tol(want, mag, dtype))
    assert ratio <= 1.0, ratio


def test_sliced_stat_rows_add_up():
    y = torch.randn(103, 6, generator=torch.Generator().manual_seed(8)).half()
    for rows in (1, 7, 103):
        p = R.sliced_stat_rows(y, rows)
        assert p.shape == (rows, 12) and p.dtype == torch.float32
        assert torch.allclose(p.double().sum(0), _stat_row(y.double())[0], rtol=1e-6, atol=0)
    assert torch.equal(R.sliced_stat_rows(y, 103)[:, :6], y.float())
