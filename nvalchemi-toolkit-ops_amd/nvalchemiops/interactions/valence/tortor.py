"""Torsion-torsion (CMAP) terms: E = F_m(s phi_1, s phi_2) over the two consecutive dihedrals of five atoms, F_m a bicubic interpolant of a
tabulated map on a uniform periodic grid.  AMOEBA's protein and nucleic-acid backbone correction and CHARMM's CMAP are this operator.

The maps are prepared once (`TorsionTorsionMaps`: node derivatives by periodic cubic splines, one 32-byte record per node); the terms run on
`mi_torsion_torsion` (csrc/valence.hip), the term / gather / fold kernels of the other valence terms with a term function that reads the four
corner records of its cell straight through the cache.  Staging a block's map in LDS was measured, was slower and is gone."""
from __future__ import annotations

import ctypes
import math

import torch

from nvalchemiops import _capi as C
from nvalchemiops.interactions.electrostatics import _pairs as P
from nvalchemiops.interactions.valence.functions import VALENCE_FORCES, VALENCE_VIRIAL, _check
from nvalchemiops.interactions.valence.terms import TorsionTorsionTerms


def _periodic_spline_derivative(f: torch.Tensor, dim: int) -> torch.Tensor:
    """Node derivatives of the periodic cubic spline through `f` along `dim`, spacing 2 pi / n: the solution of the cyclic system
    d_{i-1} + 4 d_i + d_{i+1} = 3 (f_{i+1} - f_{i-1}) / h, applied as the circulant inverse whose first row is the cosine sum
    (1 / n) sum_k cos(2 pi j k / n) / (4 + 2 cos(2 pi k / n))."""
    n = f.shape[dim]
    h = 2.0 * math.pi / n
    k = torch.arange(n, dtype=torch.float64, device=f.device)
    row = (torch.cos(2.0 * math.pi * torch.outer(k, k) / n) / (4.0 + 2.0 * torch.cos(2.0 * math.pi * k / n))).sum(1) / n
    inverse = row[(k.long()[:, None] - k.long()[None, :]) % n]
    rhs = 3.0 * (torch.roll(f, -1, dim) - torch.roll(f, 1, dim)) / h
    return torch.movedim(torch.tensordot(rhs, inverse, dims=([dim], [1])), -1, dim)


class TorsionTorsionMaps:
    """The maps of `torsion_torsion`, prepared once.

    `values` [M, n1, n2] holds M maps on one uniform periodic grid over [-pi, pi)^2: node (i, j) sits at (-pi + 2 pi i / n1,
    -pi + 2 pi j / n2), the endpoint pi is not duplicated (a table that repeats it, as Tinker's 25 x 25 parameter blocks do, is passed without
    its last row and column).  n1, n2 >= 3.  Maps on another grid go to another `TorsionTorsionMaps` and another call.

    The constructor computes the node derivatives f_1 = dF/dx, f_2 = dF/dy and f_12 = d2F/dxdy in float64, whatever the dtype of `values`,
    by periodic cubic splines along the grid lines (f_12 is the spline derivative along the second axis of f_1), and stores `nodes`
    float64 [M, n1, n2, 4], one interleaved record (f, f_1, f_2, f_12) per node.  The interpolant F_m is the bicubic patch those sixteen corner
    numbers define in every cell (the Numerical Recipes `bcuint` construction in Hermite form): it reproduces f, f_1, f_2 and f_12 at the
    nodes and is C1 everywhere.  `to(device)` returns a copy."""

    def __init__(self, values: torch.Tensor):
        if not isinstance(values, torch.Tensor) or values.dim() != 3 or not values.is_floating_point():
            raise ValueError(f"values must be a floating-point tensor of shape [num_maps, n1, n2], got {tuple(getattr(values, 'shape', ()))}")
        m, n1, n2 = values.shape
        if m < 1 or n1 < 3 or n2 < 3 or m * n1 * n2 > (1 << 28):
            raise ValueError(f"values must hold at least one map of at least 3 x 3 nodes (at most 2^28 nodes in all), got {tuple(values.shape)}")
        f = values.detach().to(torch.float64)
        f1 = _periodic_spline_derivative(f, 1)
        self.nodes = torch.stack([f, f1, _periodic_spline_derivative(f, 2), _periodic_spline_derivative(f1, 2)], dim=-1).contiguous()

    def to(self, device) -> "TorsionTorsionMaps":
        other = object.__new__(TorsionTorsionMaps)
        other.nodes = self.nodes.to(device)
        return other

    @property
    def device(self) -> torch.device:
        return self.nodes.device

    @property
    def num_maps(self) -> int:
        return self.nodes.shape[0]

    def __repr__(self) -> str:
        return f"TorsionTorsionMaps(num_maps={self.num_maps}, grid={tuple(self.nodes.shape[1:3])}, device={self.device})"


def _launch(positions, cell, batch_idx, atoms, slot_ptr, slot_idx, nodes, map_index, signs, flags, weights=None, energies=True):
    """One `mi_torsion_torsion` launch: (energies | None and forces | None in the positions dtype, float64 virial [nsys, 3, 3] | None)."""
    C.require_device(positions, cell, batch_idx, atoms, slot_ptr, slot_idx, nodes, map_index, signs, weights)
    dt, dev, n, t = positions.dtype, positions.device, positions.shape[0], atoms.shape[0]
    pos = positions.detach().contiguous()
    cells = None if cell is None else cell.detach().reshape(-1, 3, 3).to(dt).contiguous()
    batched = batch_idx is not None and cells is not None
    nsys = cells.shape[0] if batched else 1
    bi = C.i32(batch_idx) if batched else None
    atoms, slot_ptr, slot_idx, map_index = C.i32(atoms), C.i32(slot_ptr), C.i32(slot_idx), C.i32(map_index)
    nodes, signs = nodes.detach().to(torch.float64).contiguous(), signs.detach().to(torch.float64).contiguous()
    L = C.lib()
    e = torch.empty(n, dtype=dt, device=dev) if energies else None
    f = torch.empty((n, 3), dtype=dt, device=dev) if flags & VALENCE_FORCES else None
    part = torch.empty((nsys, int(L.mi_valence_blocks()), 9), dtype=torch.float64, device=dev) if flags & VALENCE_VIRIAL else None
    nbytes = int(L.mi_torsion_torsion_scratch_bytes(t, int(flags)))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    rc = L.mi_torsion_torsion(C.ptr(pos), C.ptr(atoms), C.ptr(nodes), C.ptr(map_index), C.ptr(signs), nodes.shape[0], nodes.shape[1],
                              nodes.shape[2], C.ptr(cells), C.ptr(bi), C.ptr(weights), C.ptr(slot_ptr), C.ptr(slot_idx),
                              ctypes.c_longlong(slot_idx.shape[0]), n, t, nsys, C.dtype_code(dt), int(flags), C.ptr(e), C.ptr(f), C.ptr(part),
                              C.ptr(scratch), ctypes.c_size_t(nbytes), C.stream_of(pos))
    C.check(rc, "mi_torsion_torsion")
    return e, f, C.fold_virial9(part) if part is not None else None


def _forward(positions, cell, batch_idx, atoms, slot_ptr, slot_idx, nodes, map_index, signs, forces, virial):
    """(energies, forces | None, virial | None) in the positions dtype, no autograd graph: what the eager call and the op both run."""
    flags = (VALENCE_FORCES if forces else 0) | (VALENCE_VIRIAL if virial else 0)
    e, f, vir = _launch(positions, cell, batch_idx, atoms, slot_ptr, slot_idx, nodes, map_index, signs, flags)
    return e, f, vir.to(positions.dtype) if virial else None


def _adjoint(positions, cell, batch_idx, atoms, slot_ptr, slot_idx, nodes, map_index, signs, grad_energies):
    """Float64 dL/dpositions of L = sum_i g_i E_i: the forward kernels with weights."""
    g = grad_energies.detach().to(torch.float64).contiguous()
    _, f, _ = _launch(positions, cell, batch_idx, atoms, slot_ptr, slot_idx, nodes, map_index, signs, VALENCE_FORCES, weights=g, energies=False)
    return -f.to(torch.float64)


@C.traceable
def torsion_torsion(positions: torch.Tensor, terms: TorsionTorsionTerms, maps: TorsionTorsionMaps, cell: torch.Tensor | None = None, *,
                    batch_idx: torch.Tensor | None = None, compute_forces: bool = False, compute_virial: bool = False):
    """Torsion-torsion (CMAP) terms over the atoms (a, b, c, d, e) of a `TorsionTorsionTerms`:

        E_t = F_m(s phi_1, s phi_2),    phi_1 = dihedral(a, b, c, d),  phi_2 = dihedral(b, c, d, e)

    with the dihedral of `torsion` (radians, trans is pi), m = terms.map_index[t], s = terms.signs[t] = +-1 the chirality sign the caller
    chose (the energy itself carries no sign), and F_m the bicubic interpolant of map m of `maps` (`TorsionTorsionMaps`).  An angle of exactly
    pi, on a node or on a cell edge lands in a valid cell: the cell index is taken modulo the grid size and the interpolant is C1, so either
    neighbouring patch gives the same value and gradient.

    `cell`, `batch_idx`, the minimum images, the atom shares (E_t / 5 per atom), forces, virial (needs a cell), float32 or float64 positions
    with float64 arithmetic and float64 maps, bit-reproducible sums and the autograd / `torch.compile` path through `alchemiops::_torsion_torsion`
    are those of the other valence functions.  Returns ``energies`` [N], or a tuple (energies, forces [N, 3], virial [num_systems, 3, 3]) holding
    only the items asked for.  Energies are differentiable once w.r.t. positions; differentiating the explicit forces or virial raises
    NotImplementedError (second derivatives).  There is no gradient w.r.t. the map values.  A table built with `validate=False` whose term names
    an atom outside [0, N) or a map outside [0, M) contributes exact zeros.  CPU tensors raise NativeLibraryError: there is no fallback."""
    if not isinstance(terms, TorsionTorsionTerms):
        raise TypeError(f"terms must be a TorsionTorsionTerms, got {type(terms)}")
    if not isinstance(maps, TorsionTorsionMaps):
        raise TypeError(f"maps must be a TorsionTorsionMaps, got {type(maps)}")
    if terms.max_map is not None and terms.max_map >= maps.num_maps:
        raise ValueError(f"terms name map {terms.max_map} but maps holds {maps.num_maps}")
    nsys = _check(None, positions, terms, None, cell, batch_idx, compute_virial)
    n, dev, dt = positions.shape[0], positions.device, positions.dtype
    want = (True, compute_forces, compute_virial)
    if n == 0 or terms.num_terms == 0:
        z = lambda *shape: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
        return P.select((z(n), z(n, 3), z(nsys, 3, 3)), want)
    args = (positions, cell, batch_idx, terms.atoms, terms.slot_ptr, terms.slot_idx, maps.nodes, terms.map_index, terms.signs, bool(compute_forces),
            bool(compute_virial))
    return P.dispatch("torsion_torsion_op", _forward, args, (positions,), want)


__all__ = ["TorsionTorsionMaps", "torsion_torsion"]
