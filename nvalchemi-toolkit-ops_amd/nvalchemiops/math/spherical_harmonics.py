"""Real spherical harmonics up to L = 2 (math/spherical_harmonics.py: `eval_spherical_harmonics_pytorch` :793,
`eval_spherical_harmonics_gradient_pytorch` :847).

Component order: [Y00, Y1-1 (y), Y10 (z), Y1+1 (x), Y2-2 (xy), Y2-1 (yz), Y20 (3 z^2 - r^2), Y2+1 (xz), Y2+2 (x^2 - y^2)], orthonormal on the
sphere.  1 / r is rsqrt(r^2 + 1e-30): the L > 0 values are 0 at the origin and Y00 is 1 / sqrt(4 pi) everywhere.  The gradients are the
analytic derivatives of Y_lm(r / |r|) with respect to r; they are singular at the origin and regularised by that epsilon only.
"""
from __future__ import annotations

import torch

from nvalchemiops import _capi as C

NUM_COMPONENTS = {0: 1, 1: 4, 2: 9}


def _points(points: torch.Tensor, device) -> torch.Tensor:
    """[N, 3] float64 contiguous on the computing device (the reference's wrappers take float64 and allocate the output on `device`)."""
    p = points.detach()
    if device is not None:
        p = p.to(device)
    C.require_device(p)
    if p.dim() != 2 or p.shape[1] != 3:
        raise ValueError(f"expected an [N, 3] tensor, got {tuple(p.shape)}")
    return p.to(torch.float64).contiguous()


def _launch(name: str, points: torch.Tensor, shape_tail: tuple, *scalars) -> torch.Tensor:
    out = torch.empty((points.shape[0],) + shape_tail, dtype=torch.float64, device=points.device)
    with torch.cuda.device(points.device):
        rc = getattr(C.lib(), name)(C.ptr(points), points.shape[0], *scalars, C.ptr(out), C.stream_of(points))
    C.check(rc, name)
    return out


def eval_spherical_harmonics_pytorch(positions: torch.Tensor, L_max: int = 2, device=None) -> torch.Tensor:
    """Y_lm(r / |r|) for every row of positions[N, 3]: [N, 1 | 4 | 9] float64 for L_max = 0 | 1 | 2 (KeyError otherwise)."""
    nc = NUM_COMPONENTS[L_max]
    return _launch("mi_sph_harm", _points(positions, device), (nc,), int(L_max))


def eval_spherical_harmonics_gradient_pytorch(positions: torch.Tensor, L_max: int = 2, device=None) -> torch.Tensor:
    """d Y_lm(r / |r|) / d r for every row of positions[N, 3]: [N, 1 | 4 | 9, 3] float64 (KeyError for an unsupported L_max)."""
    nc = NUM_COMPONENTS[L_max]
    return _launch("mi_sph_harm_grad", _points(positions, device), (nc, 3), int(L_max))


__all__ = ["eval_spherical_harmonics_pytorch", "eval_spherical_harmonics_gradient_pytorch"]
