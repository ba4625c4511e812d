"""Mathematical building blocks of the multipole path -- drop-in for the host-callable part of nvalchemiops/math:

    spherical_harmonics   real orthonormal Y_lm of r / |r| for L <= 2 and their gradients (math/spherical_harmonics.py:793, :847)
    gto                   Gaussian-type multipole densities and their Fourier-side factors for L <= 2 (math/gto.py:762, :811)

Elementwise float64 HIP kernels in csrc/multipole.hip behind `mi_sph_harm / mi_sph_harm_grad / mi_gto_density / mi_gto_fourier`.  The
reference's Warp device functions (`@wp.func`: `spherical_harmonic_00`, `gto_density_l1`, `wp_erfc`, ...) are callable only from other
Warp kernels and have no counterpart in a package without Warp; the four `eval_*_pytorch` wrappers are the module's host API.
"""
from nvalchemiops.math.gto import eval_gto_density_pytorch, eval_gto_fourier_pytorch
from nvalchemiops.math.spherical_harmonics import eval_spherical_harmonics_gradient_pytorch, eval_spherical_harmonics_pytorch

__all__ = ["eval_spherical_harmonics_pytorch", "eval_spherical_harmonics_gradient_pytorch", "eval_gto_density_pytorch", "eval_gto_fourier_pytorch"]
