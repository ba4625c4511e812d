"""`nvalchemiops.math` on the device: real spherical harmonics up to L = 2, their gradients, Gaussian-type multipole densities and their
Fourier-side factors (kernels in csrc/multipole.hip) against closed forms written out here in numpy / torch, at rtol = atol = 1e-10 -- the
reference's own bar (test/math/test_gto.py:214)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = dict(rtol=1e-10, atol=1e-10)
NCOMP = {0: 1, 1: 4, 2: 9}
PARITY = np.array([1, -1, -1, -1, 1, 1, 1, 1, 1])


def _ylm(xyz, lib=np):
    """The nine real orthonormal harmonics of the direction of xyz[..., 3] (numpy arrays or torch tensors)."""
    x, y, z = xyz[..., 0], xyz[..., 1], xyz[..., 2]
    r2 = x * x + y * y + z * z
    r = lib.sqrt(r2)
    pi = np.pi
    c1, c2, c20, c22 = np.sqrt(3 / (4 * pi)), 0.5 * np.sqrt(15 / pi), 0.25 * np.sqrt(5 / pi), 0.25 * np.sqrt(15 / pi)
    one = x * 0 + 1
    return lib.stack([one / np.sqrt(4 * pi), c1 * y / r, c1 * z / r, c1 * x / r, c2 * x * y / r2, c2 * y * z / r2, c20 * (3 * z * z - r2) / r2,
                      c2 * x * z / r2, c22 * (x * x - y * y) / r2], -1)


def _points(n=500, seed=0, scale=3.0):
    return np.random.default_rng(seed).normal(size=(n, 3)) * scale


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=DEV)


@pytest.mark.parametrize("l_max", [0, 1, 2])
def test_spherical_harmonics_against_closed_forms(l_max):
    from nvalchemiops.math import eval_spherical_harmonics_pytorch

    pts = _points()
    got = eval_spherical_harmonics_pytorch(_dev(pts), L_max=l_max)
    assert got.shape == (500, NCOMP[l_max]) and got.dtype == torch.float64 and got.device.type == "cuda"
    np.testing.assert_allclose(got.cpu().numpy(), _ylm(pts)[:, :NCOMP[l_max]], **TOL)
    # float32 input, a CPU tensor moved by `device`, a non-contiguous view
    np.testing.assert_allclose(eval_spherical_harmonics_pytorch(torch.as_tensor(pts), L_max=l_max, device=DEV).cpu().numpy(),
                               _ylm(pts)[:, :NCOMP[l_max]], **TOL)
    wide = _dev(np.concatenate([pts, pts], 1))
    np.testing.assert_allclose(eval_spherical_harmonics_pytorch(wide[:, 3:], L_max=l_max).cpu().numpy(), _ylm(pts)[:, :NCOMP[l_max]], **TOL)
    assert eval_spherical_harmonics_pytorch(_dev(pts[:0]), L_max=l_max).shape == (0, NCOMP[l_max])


def test_harmonics_are_orthonormal_on_the_sphere():
    """Product-Gauss quadrature: Gauss-Legendre in cos(theta) (exact for the degree-4 products with 16 nodes) times a uniform grid in phi."""
    from nvalchemiops.math import eval_spherical_harmonics_pytorch

    ct, wt = np.polynomial.legendre.leggauss(16)
    phi = 2 * np.pi * (np.arange(32) + 0.5) / 32
    st = np.sqrt(1 - ct * ct)
    pts = np.stack([np.outer(st, np.cos(phi)), np.outer(st, np.sin(phi)), np.outer(ct, np.ones_like(phi))], -1).reshape(-1, 3)
    w = np.outer(wt, np.full(32, 2 * np.pi / 32)).reshape(-1)
    for radius in (1.0, 0.01, 250.0):  # functions of the direction only
        y = eval_spherical_harmonics_pytorch(_dev(pts * radius), L_max=2).cpu().numpy()
        np.testing.assert_allclose((y * w[:, None]).T @ y, np.eye(9), rtol=0, atol=1e-10)


def test_harmonic_gradients():
    from nvalchemiops.math import eval_spherical_harmonics_gradient_pytorch, eval_spherical_harmonics_pytorch

    pts = _points(300, seed=1)
    pts = pts[np.linalg.norm(pts, axis=1) > 0.5]
    for l_max in (0, 1, 2):
        got = eval_spherical_harmonics_gradient_pytorch(_dev(pts), L_max=l_max)
        assert got.shape == (len(pts), NCOMP[l_max], 3) and got.dtype == torch.float64
    got = got.cpu().numpy()
    # torch.autograd of the same closed forms
    tp = torch.tensor(pts, dtype=torch.float64, requires_grad=True)
    y = _ylm(tp, lib=torch)
    ref = torch.stack([torch.autograd.grad(y[:, c].sum(), tp, retain_graph=True)[0] for c in range(9)], 1).numpy()
    np.testing.assert_allclose(got, ref, **TOL)
    # central differences of the device harmonics: h = 1e-5 on |r| > 0.5 leaves h^2 |Y'''| / 6 ~ 1e-9 of truncation and 1e-16 / h = 1e-11 of rounding
    h = 1e-5
    for a in range(3):
        d = np.zeros(3)
        d[a] = h
        fd = (eval_spherical_harmonics_pytorch(_dev(pts + d)) - eval_spherical_harmonics_pytorch(_dev(pts - d))).cpu().numpy() / (2 * h)
        np.testing.assert_allclose(got[:, :, a], fd, rtol=0, atol=1e-7)
    # the harmonics do not depend on |r|: no radial component
    assert np.abs(np.einsum("nca,na->nc", got, pts)).max() < 1e-12


@pytest.mark.parametrize("sigma", [0.7, 1.3])
def test_gto_density_against_closed_forms_and_integrals(sigma):
    from nvalchemiops.math import eval_gto_density_pytorch

    pts = _points(400, seed=2, scale=1.5)
    norm = np.sqrt(4 * np.pi) / (2 * np.pi * sigma ** 2) ** 1.5
    ref = norm * _ylm(pts) * np.exp(-(pts ** 2).sum(1) / (2 * sigma ** 2))[:, None]
    for l_max in (0, 1, 2):
        got = eval_gto_density_pytorch(_dev(pts), sigma, L_max=l_max)
        assert got.shape == (400, NCOMP[l_max]) and got.dtype == torch.float64
        np.testing.assert_allclose(got.cpu().numpy(), ref[:, :NCOMP[l_max]], **TOL)
    # midpoint rule on a cube of +- 8 sigma (the Gaussian's tail beyond it is < 1e-13), cell centres so that no point is the origin: the
    # L = 0 density integrates to 1, the L > 0 ones to 0 (odd, or with a zero angular average; the grid has the cube's symmetry, under
    # which x^2 - y^2, 3 z^2 - r^2 and the mixed products sum to zero exactly)
    n = 96
    h = 16 * sigma / n
    ax = (np.arange(n) + 0.5) * h - 8 * sigma
    grid = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    integ = eval_gto_density_pytorch(_dev(grid), sigma, L_max=2).sum(0).cpu().numpy() * h ** 3
    assert abs(integ[0] - 1.0) < 1e-10, integ[0]
    assert np.abs(integ[1:]).max() < 1e-10, integ[1:]


@pytest.mark.parametrize("sigma", [0.7, 1.3])
def test_gto_fourier_against_closed_forms(sigma):
    from nvalchemiops.math import eval_gto_fourier_pytorch

    k = _points(400, seed=3, scale=1.2)
    gauss = np.exp(-0.5 * (k ** 2).sum(1) * sigma ** 2)[:, None]
    y = _ylm(k)
    ref_re = np.concatenate([gauss, np.zeros((400, 3)), -0.25 * np.sqrt(4 * np.pi) * y[:, 4:] * gauss], 1)
    ref_im = np.concatenate([np.zeros((400, 1)), 0.5 * np.sqrt(4 * np.pi) * y[:, 1:4] * gauss, np.zeros((400, 5))], 1)
    for l_max in (0, 1, 2):
        re, im = eval_gto_fourier_pytorch(_dev(k), sigma, L_max=l_max)
        assert re.shape == im.shape == (400, NCOMP[l_max]) and re.dtype == im.dtype == torch.float64
        np.testing.assert_allclose(re.cpu().numpy(), ref_re[:, :NCOMP[l_max]], **TOL)
        np.testing.assert_allclose(im.cpu().numpy(), ref_im[:, :NCOMP[l_max]], **TOL)
    re, im = (t.cpu().numpy() for t in eval_gto_fourier_pytorch(_dev(k), sigma, L_max=2))
    # which part is zero for each L: L = 0 and L = 2 are real, L = 1 is imaginary -- exactly
    assert np.all(im[:, 0] == 0) and np.all(im[:, 4:] == 0) and np.all(re[:, 1:4] == 0)
    assert np.abs(im[:, 1:4]).max() > 0.01 and np.abs(re[:, 4:]).max() > 0.01


def test_gto_fourier_l0_is_the_transform_of_the_l0_density():
    """integral rho_00(r) exp(-i k.r) d^3r by the midpoint rule on +- 8 sigma (spectrally accurate for a Gaussian: the aliasing error of
    spacing h is exp(-(2 pi / h - |k|)^2 sigma^2 / 2), below 1e-16 here) equals exp(-k^2 sigma^2 / 2); the imaginary part vanishes."""
    from nvalchemiops.math import eval_gto_density_pytorch, eval_gto_fourier_pytorch

    sigma, n = 0.9, 64
    h = 16 * sigma / n
    ax = (np.arange(n) + 0.5) * h - 8 * sigma
    grid = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    rho = eval_gto_density_pytorch(_dev(grid), sigma, L_max=0)[:, 0]
    k = np.array([[0.0, 0.0, 0.0], [0.5, 0.0, 0.0], [0.3, -0.8, 1.1], [2.0, 1.0, -1.5]])
    phase = _dev(grid) @ _dev(k).T
    num_re = (rho[:, None] * torch.cos(phase)).sum(0).cpu().numpy() * h ** 3
    num_im = -(rho[:, None] * torch.sin(phase)).sum(0).cpu().numpy() * h ** 3
    re, im = eval_gto_fourier_pytorch(_dev(k), sigma, L_max=0)
    np.testing.assert_allclose(re[:, 0].cpu().numpy(), num_re, **TOL)
    np.testing.assert_allclose(im[:, 0].cpu().numpy(), num_im, rtol=0, atol=1e-10)


def test_origin_parity_and_shapes():
    from nvalchemiops.math import (eval_gto_density_pytorch, eval_gto_fourier_pytorch, eval_spherical_harmonics_gradient_pytorch,
                                   eval_spherical_harmonics_pytorch)

    zero = torch.zeros((2, 3), dtype=torch.float64, device=DEV)
    y0 = eval_spherical_harmonics_pytorch(zero).cpu().numpy()
    np.testing.assert_allclose(y0[:, 0], 1 / np.sqrt(4 * np.pi), **TOL)
    assert np.all(y0[:, 1:] == 0)  # 1 / r is rsqrt(r^2 + 1e-30): every L > 0 harmonic vanishes at the origin
    assert np.all(eval_spherical_harmonics_gradient_pytorch(zero).cpu().numpy()[:, 0] == 0)  # Y00 is constant (no value is promised for L > 0 there)
    sigma = 0.8
    d0 = eval_gto_density_pytorch(zero, sigma).cpu().numpy()
    np.testing.assert_allclose(d0[:, 0], 1 / (2 * np.pi * sigma ** 2) ** 1.5, **TOL)
    assert np.all(d0[:, 1:] == 0)
    re, im = (t.cpu().numpy() for t in eval_gto_fourier_pytorch(zero, sigma))
    assert np.all(re[:, 0] == 1.0) and np.all(re[:, 1:] == 0) and np.all(im == 0)  # k = 0: the total charge of the L = 0 density, nothing else
    pts = _points(200, seed=4)
    for fn, args in ((eval_spherical_harmonics_pytorch, ()), (eval_gto_density_pytorch, (sigma,))):
        a, b = fn(_dev(pts), *args).cpu().numpy(), fn(_dev(-pts), *args).cpu().numpy()
        np.testing.assert_allclose(b, a * PARITY, rtol=0, atol=1e-15)  # L = 1 odd, L = 0 and L = 2 even
    (ra, ia), (rb, ib) = eval_gto_fourier_pytorch(_dev(pts), sigma), eval_gto_fourier_pytorch(_dev(-pts), sigma)
    np.testing.assert_allclose(rb.cpu().numpy(), ra.cpu().numpy() * PARITY, rtol=0, atol=1e-15)
    np.testing.assert_allclose(ib.cpu().numpy(), ia.cpu().numpy() * PARITY, rtol=0, atol=1e-15)
    ga, gb = eval_spherical_harmonics_gradient_pytorch(_dev(pts)).cpu().numpy(), eval_spherical_harmonics_gradient_pytorch(_dev(-pts)).cpu().numpy()
    np.testing.assert_allclose(gb, -ga * PARITY[:, None], rtol=0, atol=1e-14)
    for l_max in (0, 1, 2):
        assert eval_spherical_harmonics_pytorch(_dev(pts), l_max).shape == (200, NCOMP[l_max])
        assert eval_spherical_harmonics_gradient_pytorch(_dev(pts), l_max).shape == (200, NCOMP[l_max], 3)
        assert eval_gto_density_pytorch(_dev(pts), sigma, l_max).shape == (200, NCOMP[l_max])
        assert all(t.shape == (200, NCOMP[l_max]) for t in eval_gto_fourier_pytorch(_dev(pts), sigma, l_max))
    with pytest.raises(KeyError):
        eval_spherical_harmonics_pytorch(_dev(pts), L_max=3)
