"""Particle-mesh Ewald for point quadrupoles: the mesh counterpart of `ewald_quadrupole_correction`, O(N + M log M) where the explicit
reciprocal sum of `quadrupole.py` is O(N K).  It completes the ladder charges / dipoles / quadrupoles x explicit Ewald / mesh.

`pme_quadrupole_correction` returns what atomic point quadrupoles add to the periodic energy of point charges and point dipoles -- the
charge-quadrupole, dipole-quadrupole and quadrupole-quadrupole energy -- with the reciprocal half on a mesh, and is ADDED to what
`particle_mesh_ewald` and `pme_dipole_correction` return (neither changes).  The real-space half is `ewald_quadrupole_real_space`, unchanged.
The reference package has no counterpart.

HIP kernels (csrc/pme.hip, last section): `mi_pme_quadrupole_spread` (one pass over the atoms writes the charge-and-dipole mesh and the
quadrupole mesh), `mi_pme_quadrupole_gather` (potential, gradient, Hessian and -- where forces are asked for -- third derivatives of two meshes
in one pass) and `mi_pme_quadrupole_virial` (the k-space virial of the cross spectrum).  Between them runs the mesh solve of the charge PME,
through `_solve` of `pme_dipole.py`.  Forward and adjoint are the same launches without and with per-atom weights.  The spread adds with
floating-point atomics, always in float64, with the consequences `pme_dipole.py` describes: float64 outputs are reproducible up to the arrival
order of these adds, float32 outputs are the same in every run.  The gather forms its stencil and spline tables in float64 whatever the
dtype and rounds them once, so that a float32 call gathers with the weights it spread with.
"""
from __future__ import annotations

import math

import torch

from nvalchemiops import _capi as C
from nvalchemiops.interactions.electrostatics import _multipoles as M
from nvalchemiops.interactions.electrostatics import pme_dipole as _pd
from nvalchemiops.interactions.electrostatics.quadrupole import FLAGS, _check_real, _dipoles_or_zeros, check_quadrupoles, ewald_quadrupole_real_space

_MODEL = """Smooth PME with analytic spline derivatives, one multipole order beyond `pme_dipole_correction`.  Atom i carries q_i, mu_i and a
    symmetric Cartesian quadrupole Q_i, `quadrupoles` [N, 3, 3] (the second Taylor coefficient 1/2 sum q d d; a traceless AMOEBA / Stone
    quadrupole Theta enters as Q = Theta / 3; tracelessness is not required, and 1/2 (Q + Q^T) of what is given is used).  With W_i(g) the
    order-p B-spline weight of atom i at mesh point g, grad the Cartesian gradient w.r.t. r_i, l_i = q_i + mu_i . grad and
    Theta_i = Q_i : grad grad:

        rho_l = sum_i l_i W_i (ONE mesh for charges and dipoles),  rho_T = sum_i Theta_i W_i,  phi_X = IFFT[G FFT(rho_X) / sf^2]
        phi_L = phi_l + phi_T
        E_i = l_i W_i . phi_T + Theta_i W_i . phi_L + (4 alpha^3 / (3 sqrt(pi))) q_i tr Q_i - (4 alpha^5 / (5 sqrt(pi))) (2 Q_i:Q_i + (tr Q_i)^2)
        G = 2 pi exp(-k^2 / 4 alpha^2) / (k^2 V) (0 at k = 0) and sf^2 = the squared sinc product to the power p, as `pme_reciprocal_space`

    the mesh form of l_i Theta_j + Theta_i L_j: the same partition over the atoms and the same self term as
    `ewald_quadrupole_reciprocal_space`, to whose per-atom energies it converges with the mesh.  Nothing is a difference of two quadratic
    forms: zero quadrupoles give exactly 0.0 in every output but quadrupole_grads.  Gaussian units, tin-foil boundary.  `spline_order` is 5 or
    6: the forces need the third derivative of the spline, which is discontinuous at order 4 (and the second, which the energy needs, is only
    continuous there): order 4 or below raises ValueError.  The quadrupole terms carry k^4 and converge more slowly with the mesh than the charge
    or dipole terms: on a 6-atom test box the relative error of the per-atom energies is 5e-4 / 7e-5 at order 5 and 5e-5 / 1.5e-5 at order 6
    on meshes of 16^3 / 24^3 points."""

_RETURNS = """Returns ``energies`` [N], or a tuple holding only what was asked for, in this order: energies, forces [N, 3], charge_grads [N],
    dipole_grads [N, 3], quadrupole_grads [N, 3, 3], virial [num_systems, 3, 3]; all in the positions dtype (per-atom sums in the positions
    dtype, epilogue and k-space virial in float64).  forces = -dE/dr, charge_grads = dE/dq, dipole_grads = dE/dmu, quadrupole_grads = dE/dQ of
    the total E = sum_i E_i.  quadrupole_grads is symmetric (the field gradient at the atom; it does not vanish for zero quadrupoles).
    dipole_grads does not depend on the dipoles: minus dipole_grads is the electric field of the quadrupoles at each atom, which is what
    `induced_dipoles(external_field=...)` takes.  virial = -dE/d(strain) under x -> (I + eps) x at fixed alpha and mesh, with the multipoles
    held fixed in the laboratory frame: nine independent components, NOT symmetric.

    Energies are differentiable once w.r.t. positions, charges, dipoles and quadrupoles, for any upstream gradient on the per-atom energies
    (the same kernels run as their own adjoint, over four meshes); the call then goes through the `alchemiops::_pme_quadrupole_reciprocal_space`
    op, as it does under `torch.compile`.  Differentiating the explicit forces, gradients or virial raises NotImplementedError.  Gradients
    w.r.t. cell and alpha are out of scope (NotImplementedError at backward): use `compute_virial`.  Also out of scope: a tile-owned spread,
    caller-supplied k arrays, `cell=None` clusters, octupoles, spherical-tensor input, Thole damping of quadrupole fields, surface
    (non-tin-foil) terms.  The spread uses float64 atomic adds: float64 outputs are reproducible only up to the arrival order of these adds
    (last bits); float32 outputs are the same in every run.  CPU tensors raise NativeLibraryError: there is no fallback."""

ORDERS = (5, 6)


def _check_order(spline_order) -> int:
    return M.check_order(spline_order, ORDERS, "quadrupole", "the forces need the third derivative of the spline, which is discontinuous at "
                         "order 4, where the second derivative the energy needs is only continuous")


def _check_recip(positions, charges, dipoles, quadrupoles, cell, alpha, batch_idx):
    _pd._check_recip(positions, charges, dipoles, cell, alpha, batch_idx)
    check_quadrupoles(positions, quadrupoles)


# ---- launches -----------------------------------------------------------------------------------------------------------------------------
def _spread_launch(p, dims, order, weights, meshes):
    pos = p["pos"]
    rc = C.lib().mi_pme_quadrupole_spread(C.ptr(pos), C.ptr(p["q"]), C.ptr(p["mu"]), C.ptr(p["qd"]), C.ptr(weights), C.ptr(p["bi"]),
                                          C.ptr(p["cit"]), pos.shape[0], int(p["nsys"]), *dims, int(order), p["code"], C.ptr(meshes),
                                          C.stream_of(pos))
    C.check(rc, "mi_pme_quadrupole_spread")


def _spread(p, dims, order, weights=None):
    """[2 | 4, nsys, nx, ny, nz]: rho_l, rho_T (and their g-weighted twins), zero-filled by the entry point.  float32 calls add in float64 and
    round once, the policy of `pme_dipole._spread` -- here without its switch (`pme_dipole._SPREAD_FLOAT32_IN_FLOAT64`): the gather forms
    its stencil in float64 whatever the dtype, and a spread from float32 stencils would not be the one it is the adjoint of."""
    return M.mesh_spread(p, dims, order, _spread_launch, True, weights)


def _gather(p, dims, order, mesh_a, mesh_b, want, weights=None, out=None):
    """One `mi_pme_quadrupole_gather` launch over (A, B): float64 (energies | None, forces in the positions dtype | None, charge sums | None,
    dipole sums | None, quadrupole sums [n, 3, 3] | None) as `want` asks for them; with `out` the launch adds to its tensors."""
    pos = p["pos"]
    e, f, cg, dg, qg = M.allocate(pos, M.QUADRUPOLE, want) if out is None else out
    rc = C.lib().mi_pme_quadrupole_gather(C.ptr(pos), C.ptr(p["q"]), C.ptr(p["mu"]), C.ptr(p["qd"]), C.ptr(weights), C.ptr(p["bi"]),
                                          C.ptr(p["cit"]), C.ptr(mesh_a), C.ptr(mesh_b), C.ptr(p["al"]), pos.shape[0], int(p["nsys"]), *dims,
                                          int(order), p["code"], int(out is not None), C.ptr(e), C.ptr(f), C.ptr(cg), C.ptr(dg), C.ptr(qg),
                                          C.stream_of(pos))
    C.check(rc, "mi_pme_quadrupole_gather")
    return e, f, cg, dg, qg


def _virial(p, spec, sums, dims, order):
    """Float64 [nsys, 3, 3]: the k-space virial of the cross spectrum plus the term of the multipoles that follow the strain."""
    L = C.lib()
    dev, dg, qg = p["pos"].device, sums[3], sums[4]
    part = torch.empty((p["nsys"], int(L.mi_pme_quadrupole_virial_blocks()), 9), dtype=torch.float64, device=dev)
    rc = L.mi_pme_quadrupole_virial(C.ptr(spec[0]), C.ptr(spec[1]), C.ptr(p["recip"]), C.ptr(p["al"]), C.ptr(p["vol"]), int(p["nsys"]), *dims,
                                    int(order), p["code"], C.ptr(part), C.stream_of(p["pos"]))
    C.check(rc, "mi_pme_quadrupole_virial")
    # the multipoles' fractional components follow the strain: + sum_i (dE/dmu_i)_a mu_i,b + 2 sum_i (G_i Q_i)_ab per system, G_i = dE/dQ_i
    # without its self terms (index order and the factor 2 matter: the virial is not symmetric)
    al = M.per_atom(p, p["al"].to(torch.float64))
    c3 = (4.0 * al**3 / (3.0 * math.sqrt(math.pi))).reshape(-1, 1, 1)
    c5 = (4.0 * al**5 / (5.0 * math.sqrt(math.pi))).reshape(-1, 1, 1)
    mu64, q64, qd64 = p["mu"].to(torch.float64), p["q"].to(torch.float64).reshape(-1, 1, 1), p["qd"].to(torch.float64)
    qd64 = 0.5 * (qd64 + qd64.transpose(1, 2))
    eye = torch.eye(3, dtype=torch.float64, device=dev)
    tr = qd64.diagonal(dim1=1, dim2=2).sum(-1).reshape(-1, 1, 1)
    bare = qg - c3 * q64 * eye + c5 * (4.0 * qd64 + 2.0 * tr * eye)
    outer = dg.unsqueeze(2) * mu64.unsqueeze(1) + 2.0 * bare @ qd64
    return M.strained_multipole_virial(p, part, outer)


def _recip_forward(positions, charges, dipoles, quadrupoles, cell, alpha, batch_idx, nx, ny, nz, order, *flags):
    """(energies, forces | None, charge_grads | None, dipole_grads | None, quadrupole_grads | None, virial | None) in the positions dtype, no
    autograd graph: what the eager call and the `alchemiops::_pme_quadrupole_reciprocal_space` op both run."""
    return M.mesh_forward(MESH, (positions, charges, dipoles, quadrupoles, cell, alpha, batch_idx), (nx, ny, nz), order, (True,) + flags)


def _recip_adjoint(positions, charges, dipoles, quadrupoles, cell, alpha, batch_idx, nx, ny, nz, order, grad_energies):
    """Float64 (dL/dpositions, dL/dcharges, dL/ddipoles, dL/dquadrupoles) of L = sum_i g_i E_i, over (phi_T, phi_L) and (phi^g_T, phi^g_l +
    phi^g_T); the self terms x g_i."""
    return M.mesh_adjoint(MESH, (positions, charges, dipoles, quadrupoles, cell, alpha, batch_idx), (nx, ny, nz), order, grad_energies)


# ---- public -------------------------------------------------------------------------------------------------------------------------------
@C.traceable
def pme_quadrupole_reciprocal_space(positions: torch.Tensor, charges: torch.Tensor, dipoles: torch.Tensor | None, quadrupoles: torch.Tensor,
                                    cell: torch.Tensor, alpha, mesh_dimensions: tuple[int, int, int] | None = None,
                                    mesh_spacing: float | None = None, spline_order: int = 5, batch_idx: torch.Tensor | None = None,
                                    compute_forces: bool = False, compute_charge_gradients: bool = False,
                                    compute_dipole_gradients: bool = False, compute_quadrupole_gradients: bool = False,
                                    compute_virial: bool = False):
    """Mesh (reciprocal-space) half of the point-quadrupole PME term, the quadrupolar self term included: what has to be ADDED to
    `pme_reciprocal_space` + `pme_dipole_reciprocal_space` when the atoms carry point quadrupoles `quadrupoles` [N, 3, 3] beside their charges
    and dipoles (`dipoles=None`: no dipoles).  MODEL

    `alpha` is a number or one value per system; with `batch_idx`, `cell` is [num_systems, 3, 3] and all systems share the mesh dimensions.
    `mesh_spacing` is turned into dimensions as `particle_mesh_ewald` does.

    RETURNS"""
    dipoles = _dipoles_or_zeros(positions, dipoles)
    _check_recip(positions, charges, dipoles, quadrupoles, cell, alpha, batch_idx)
    want = (True, compute_forces, compute_charge_gradients, compute_dipole_gradients, compute_quadrupole_gradients, compute_virial)
    return M.mesh_reciprocal_space(MESH, (positions, charges, dipoles, quadrupoles), cell, alpha, mesh_dimensions, mesh_spacing, spline_order,
                                   batch_idx, want)


@C.traceable
def pme_quadrupole_correction(positions: torch.Tensor, charges: torch.Tensor, dipoles: torch.Tensor | None, quadrupoles: torch.Tensor,
                              cell: torch.Tensor, alpha=None, mesh_spacing: float | None = None,
                              mesh_dimensions: tuple[int, int, int] | None = None, spline_order: int = 5, batch_idx: torch.Tensor | None = None,
                              neighbor_list: torch.Tensor | None = None, neighbor_ptr: torch.Tensor | None = None,
                              neighbor_shifts: torch.Tensor | None = None, neighbor_matrix: torch.Tensor | None = None,
                              neighbor_matrix_shifts: torch.Tensor | None = None, mask_value: int | None = None, compute_forces: bool = False,
                              compute_charge_gradients: bool = False, compute_dipole_gradients: bool = False,
                              compute_quadrupole_gradients: bool = False, compute_virial: bool = False, accuracy: float = 1e-6):
    """What has to be ADDED to the periodic energy of point charges and point dipoles (`particle_mesh_ewald` plus `pme_dipole_correction`, or
    their explicit counterparts) so that it becomes the energy of charges, dipoles and point quadrupoles `quadrupoles` [N, 3, 3]: the
    charge-quadrupole, dipole-quadrupole and quadrupole-quadrupole energy, `ewald_quadrupole_real_space` + `pme_quadrupole_reciprocal_space`.
    The mesh counterpart of `ewald_quadrupole_correction`, to which it converges with the mesh.  `dipoles=None` means no dipoles.  MODEL

    The real-space half is the pair sum of `ewald_quadrupole_real_space` over the list (see there for its terms).  `alpha` and the mesh are
    estimated exactly as `pme_dipole_correction` estimates them when not given (`accuracy`; the estimate is that of the charge term, and the
    quadrupole terms converge more slowly on a mesh: see above); pass the values the other routines used, or any others: the sum of both
    halves does not depend on alpha beyond the truncation error.  Under `torch.compile(fullgraph=True)` pass `alpha` and `mesh_dimensions`
    (the estimate reads device data).  THE LIST MUST BE FULL (symmetric); a half or truncated list is not detected.  A matrix entry equal to
    `mask_value` (default: N) or outside [0, N) is padding.

    RETURNS"""
    if mask_value is None:
        mask_value = positions.shape[0]
    dipoles = _dipoles_or_zeros(positions, dipoles)
    _check_real(positions, charges, dipoles, quadrupoles, cell, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix,
                neighbor_matrix_shifts, batch_idx, alpha, compute_virial)
    want = (True, compute_forces, compute_charge_gradients, compute_dipole_gradients, compute_quadrupole_gradients, compute_virial)
    return M.mesh_correction(MESH, (positions, charges, dipoles, quadrupoles), cell, alpha, mesh_spacing, mesh_dimensions, spline_order, batch_idx,
                             (neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts), mask_value, want, accuracy)


# what `_multipoles.mesh_*` run for this operator, bound here at import (see `pme_dipole.MESH`)
MESH = dict(grads=M.QUADRUPOLE, flags=FLAGS, check_order=_check_order, spread=_spread, gather=_gather, virial=_virial, forward=_recip_forward,
            op="pme_quadrupole_reciprocal_space_op", real=ewald_quadrupole_real_space, recip=pme_quadrupole_reciprocal_space)

for _fn in (pme_quadrupole_reciprocal_space, pme_quadrupole_correction):
    _fn.__doc__ = _fn.__doc__.replace("MODEL", _MODEL).replace("RETURNS", _RETURNS)
del _fn

__all__ = ["pme_quadrupole_reciprocal_space", "pme_quadrupole_correction"]
