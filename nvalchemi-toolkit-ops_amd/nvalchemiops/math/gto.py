"""Gaussian-type multipole basis functions up to L = 2 (math/gto.py: `eval_gto_density_pytorch` :762, `eval_gto_fourier_pytorch` :811).

    density   phi_lm(r) = sqrt(4 pi) / (2 pi sigma^2)^(3/2) Y_lm(r^) exp(-r^2 / (2 sigma^2))       (L = 0: the normalised Gaussian)
    Fourier   exp(-k^2 sigma^2 / 2) times 1 (L = 0, real part), (1/2) sqrt(4 pi) Y_1m(k^) (L = 1, IMAGINARY part),
              -(1/4) sqrt(4 pi) Y_2m(k^) (L = 2, real part); the other part is zero.

Component order and the 1e-30 regularisation of 1 / r are those of `nvalchemiops.math.spherical_harmonics`.  The L > 0 Fourier factors are
the reference's convention; they are not the transforms of the L > 0 densities above, which carry no r^l factor.
"""
from __future__ import annotations

import ctypes

import torch

from nvalchemiops import _capi as C
from nvalchemiops.math.spherical_harmonics import NUM_COMPONENTS, _launch, _points


def eval_gto_density_pytorch(positions: torch.Tensor, sigma: float, L_max: int = 2, device=None) -> torch.Tensor:
    """phi_lm at every row of positions[N, 3]: [N, 1 | 4 | 9] float64 (KeyError for an unsupported L_max)."""
    nc = NUM_COMPONENTS[L_max]
    return _launch("mi_gto_density", _points(positions, device), (nc,), ctypes.c_double(float(sigma)), int(L_max))


def eval_gto_fourier_pytorch(k_vectors: torch.Tensor, sigma: float, L_max: int = 2, device=None) -> tuple[torch.Tensor, torch.Tensor]:
    """(real, imag), each [K, 1 | 4 | 9] float64, of the Fourier-side factors at every row of k_vectors[K, 3]."""
    nc = NUM_COMPONENTS[L_max]
    k = _points(k_vectors, device)
    real = torch.empty((k.shape[0], nc), dtype=torch.float64, device=k.device)
    imag = torch.empty_like(real)
    with torch.cuda.device(k.device):
        rc = C.lib().mi_gto_fourier(C.ptr(k), k.shape[0], ctypes.c_double(float(sigma)), int(L_max), C.ptr(real), C.ptr(imag), C.stream_of(k))
    C.check(rc, "mi_gto_fourier")
    return real, imag


__all__ = ["eval_gto_density_pytorch", "eval_gto_fourier_pytorch"]
