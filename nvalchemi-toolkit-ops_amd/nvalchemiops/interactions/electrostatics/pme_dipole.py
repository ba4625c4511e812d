"""Particle-mesh Ewald for point dipoles: the mesh counterpart of `ewald_dipole_correction`, O(N + M log M) where the explicit reciprocal sum
of `dipole.py` is O(N K).

`pme_dipole_correction` returns what atomic point dipoles add to the periodic energy of point charges -- the charge-dipole and dipole-dipole
energy -- with the reciprocal half on a mesh, and is ADDED to what `particle_mesh_ewald` returns (which does not change).  The real-space
half is `ewald_dipole_real_space`, unchanged.  The reference package has no counterpart.

Three HIP kernels (csrc/pme.hip, last section): `mi_pme_dipole_spread` (one pass over the atoms writes the charge mesh and the dipole mesh),
`mi_pme_dipole_gather` (potential, gradient and Hessian of two meshes in one pass) and `mi_pme_dipole_virial` (the k-space virial of the
cross spectrum).  Between them runs the mesh solve of the charge PME, `mi_pme_solve_tabled` or hipFFT plan -> `mi_pme_convolve` -> plan: the
solve is linear, so the meshes of one call are further systems of one batched solve.  Forward and adjoint are the same launches without and
with per-atom weights.  The spread adds with floating-point atomics, always in float64: for float64 inputs the meshes, and hence ALL outputs,
are reproducible only up to the arrival order of these adds (differences in the last bits from run to run), as for the charge PME's
small-system path; for float32 inputs the float64 sums are rounded to float32 once, which makes the meshes and all outputs the same in every
run (in float32 arrival order the forces moved by up to 1e-6 of their largest component from run to run).
"""
from __future__ import annotations

import math

import torch

from nvalchemiops import _capi as C
from nvalchemiops.interactions.electrostatics import _multipoles as M
from nvalchemiops.interactions.electrostatics import _pairs as P
from nvalchemiops.interactions.electrostatics.dipole import FLAGS, ewald_dipole_real_space

_MODEL = """Smooth PME with analytic spline derivatives (Toukmaji, Sagui, Board, Darden).  With frac = cell^-T r, mesh coordinate m_d = frac_d n_d,
    W_i(g) = prod_d M_p(p/2 + m_d - g_d) the order-p B-spline weight of atom i at mesh point g and grad the Cartesian gradient w.r.t. r_i:

        rho_q = sum_i q_i W_i,  rho_mu = sum_i mu_i . grad W_i,  phi_X = IFFT[G FFT(rho_X) / sf^2],  phi_t = phi_q + phi_mu
        E_i = q_i W_i . phi_mu + mu_i . grad W_i . phi_t - (2 alpha^3 / (3 sqrt(pi))) |mu_i|^2
        G = 2 pi exp(-k^2 / 4 alpha^2) / (k^2 V) (0 at k = 0) and sf^2 = the squared sinc product to the power p, as `pme_reciprocal_space`

    i.e. the mesh energy of the charge distribution q_i + mu_i . grad_i minus its charge-charge part, which `pme_reciprocal_space` holds.
    Gaussian units, tin-foil boundary: no surface term and no background term; the last term is the dipolar self energy.  `spline_order` is 4, 5
    or 6: the forces need the second derivative of the spline, which is discontinuous at order 3 and zero below (ValueError)."""

_RETURNS = """Returns ``energies`` [N], or a tuple holding only what was asked for, in this order: energies, forces [N, 3], charge_grads [N],
    dipole_grads [N, 3], virial [num_systems, 3, 3]; all in the positions dtype (per-atom sums in the positions dtype, epilogue and k-space
    virial in float64).  forces = -dE/dr, charge_grads = dE/dq, dipole_grads = dE/dmu of the total E = sum_i E_i: dipole_grads is minus the
    electric field at the atom (it does not vanish for zero dipoles), and the torque on a dipole is mu x (-dipole_grads).  virial =
    -dE/d(strain) under x -> (I + eps) x at fixed alpha and mesh, with the dipoles held fixed in the laboratory frame: it has nine independent
    components and is NOT symmetric.  For dipoles defined in local frames (`rotate_multipoles`), `multipole_frame_forces` turns that torque into
    forces on the frame atoms and returns the term the virial lacks.

    Energies are differentiable once w.r.t. positions, charges and dipoles, for any upstream gradient on the per-atom energies (the same
    kernels run as their own adjoint); the call then goes through the `alchemiops::_pme_dipole_reciprocal_space` op, as it does under
    `torch.compile`.  Differentiating the explicit forces, gradients or virial raises NotImplementedError.  Gradients w.r.t. cell and alpha are
    out of scope (NotImplementedError at backward): use `compute_virial`.  Also out of scope: quadrupoles (`pme_quadrupole_correction` adds them
    on the mesh, `ewald_quadrupole_correction` by explicit Ewald summation), a tile-owned spread, caller-supplied
    k arrays, `cell=None` clusters, surface (non-tin-foil) terms.  The spread uses float64 atomic adds: float64 outputs are reproducible only
    up to the arrival order of these adds (last bits); float32 outputs are the same in every run.  CPU tensors raise NativeLibraryError: there is no fallback."""

ORDERS = (4, 5, 6)
_SPREAD_FLOAT32_IN_FLOAT64 = True  # float32 calls: the spread adds in float64 and rounds once (see `_spread`); the dipole term only -- `pme_quadrupole._spread` always does, its gather depends on it


def _check_order(spline_order) -> int:
    return M.check_order(spline_order, ORDERS, "dipole", "the forces need a continuous second derivative of the spline")


def _check_recip(positions, charges, dipoles, cell, alpha, batch_idx):
    if cell is None:
        raise ValueError("cell is required: the point-dipole Ewald sum is periodic (cell=None clusters are out of scope)")
    C.dtype_code(positions.dtype)
    C.check_per_atom(positions.shape[0], charges=charges, batch_idx=batch_idx)
    P.check_dipoles(positions, dipoles)
    C.check_neighbor_data(positions.shape[0], cell=cell, alpha=alpha)


# ---- launches -----------------------------------------------------------------------------------------------------------------------------
def _spread_launch(p, dims, order, weights, meshes):
    pos = p["pos"]
    rc = C.lib().mi_pme_dipole_spread(C.ptr(pos), C.ptr(p["q"]), C.ptr(p["mu"]), C.ptr(weights), C.ptr(p["bi"]), C.ptr(p["cit"]), pos.shape[0],
                                      int(p["nsys"]), *dims, int(order), p["code"], C.ptr(meshes), C.stream_of(pos))
    C.check(rc, "mi_pme_dipole_spread")


def _spread(p, dims, order, weights=None):
    """[2 | 4, nsys, nx, ny, nz]: rho_q, rho_mu (and their g-weighted twins), zero-filled by the entry point."""
    return M.mesh_spread(p, dims, order, _spread_launch, _SPREAD_FLOAT32_IN_FLOAT64, weights)


def _gather(p, dims, order, mesh_a, mesh_b, want, weights=None, out=None):
    """One `mi_pme_dipole_gather` launch over (A, B): float64 (energies | None, forces in the positions dtype | None, charge sums | None,
    dipole sums | None) as `want` asks for them; with `out` the launch adds to its tensors."""
    pos = p["pos"]
    e, f, cg, dg = M.allocate(pos, M.DIPOLE, want) if out is None else out
    rc = C.lib().mi_pme_dipole_gather(C.ptr(pos), C.ptr(p["q"]), C.ptr(p["mu"]), C.ptr(weights), C.ptr(p["bi"]), C.ptr(p["cit"]), C.ptr(mesh_a),
                                      C.ptr(mesh_b), C.ptr(p["al"]), pos.shape[0], int(p["nsys"]), *dims, int(order), p["code"],
                                      int(out is not None), C.ptr(e), C.ptr(f), C.ptr(cg), C.ptr(dg), C.stream_of(pos))
    C.check(rc, "mi_pme_dipole_gather")
    return e, f, cg, dg


def _self_coefficient(p):
    """2 alpha^3 / (3 sqrt(pi)) per atom, float64."""
    c = 2.0 * p["al"].to(torch.float64) ** 3 / (3.0 * math.sqrt(math.pi))
    return M.per_atom(p, c)


def _virial(p, spec, sums, dims, order):
    """Float64 [nsys, 3, 3]: the k-space virial of the cross spectrum plus the term of the dipoles that follow the strain."""
    L = C.lib()
    part = torch.empty((p["nsys"], int(L.mi_pme_dipole_virial_blocks()), 9), dtype=torch.float64, device=p["pos"].device)
    rc = L.mi_pme_dipole_virial(C.ptr(spec[0]), C.ptr(spec[1]), C.ptr(p["recip"]), C.ptr(p["al"]), C.ptr(p["vol"]), int(p["nsys"]), *dims,
                                int(order), p["code"], C.ptr(part), C.stream_of(p["pos"]))
    C.check(rc, "mi_pme_dipole_virial")
    # the dipoles' fractional components follow the strain: + sum_i (dE/dmu_i without its self term)_a mu_i,b per system (index order matters)
    mu64 = p["mu"].to(torch.float64)
    outer = (sums[3] + 2.0 * _self_coefficient(p).unsqueeze(1) * mu64).unsqueeze(2) * mu64.unsqueeze(1)
    return M.strained_multipole_virial(p, part, outer)


def _recip_forward(positions, charges, dipoles, cell, alpha, batch_idx, nx, ny, nz, order, *flags):
    """(energies, forces | None, charge_grads | None, dipole_grads | None, virial | None) in the positions dtype, no autograd graph: what the
    eager call and the `alchemiops::_pme_dipole_reciprocal_space` op both run."""
    return M.mesh_forward(MESH, (positions, charges, dipoles, cell, alpha, batch_idx), (nx, ny, nz), order, (True,) + flags)


def _recip_adjoint(positions, charges, dipoles, cell, alpha, batch_idx, nx, ny, nz, order, grad_energies):
    """Float64 (dL/dpositions, dL/dcharges, dL/ddipoles) of L = sum_i g_i E_i, over (phi_mu, phi_t) and (phi^g_mu, phi^g_q + phi^g_mu); the self
    term is -c g_i |mu_i|^2."""
    return M.mesh_adjoint(MESH, (positions, charges, dipoles, cell, alpha, batch_idx), (nx, ny, nz), order, grad_energies)


# ---- public -------------------------------------------------------------------------------------------------------------------------------
@C.traceable
def pme_dipole_reciprocal_space(positions: torch.Tensor, charges: torch.Tensor, dipoles: torch.Tensor, cell: torch.Tensor, alpha,
                                mesh_dimensions: tuple[int, int, int] | None = None, mesh_spacing: float | None = None, spline_order: int = 5,
                                batch_idx: torch.Tensor | None = None, compute_forces: bool = False, compute_charge_gradients: bool = False,
                                compute_dipole_gradients: bool = False, compute_virial: bool = False):
    """Mesh (reciprocal-space) half of the point-dipole PME term, the dipolar self term included: what has to be ADDED to
    `pme_reciprocal_space` when the atoms carry point dipoles `dipoles` [N, 3] beside their charges.  MODEL

    `alpha` is a number or one value per system; with `batch_idx`, `cell` is [num_systems, 3, 3] and all systems share the mesh dimensions.
    `mesh_spacing` is turned into dimensions as `particle_mesh_ewald` does.

    RETURNS"""
    _check_recip(positions, charges, dipoles, cell, alpha, batch_idx)
    return M.mesh_reciprocal_space(MESH, (positions, charges, dipoles), cell, alpha, mesh_dimensions, mesh_spacing, spline_order, batch_idx,
                                   (True, compute_forces, compute_charge_gradients, compute_dipole_gradients, compute_virial))


@C.traceable
def pme_dipole_correction(positions: torch.Tensor, charges: torch.Tensor, dipoles: torch.Tensor, cell: torch.Tensor, alpha=None,
                          mesh_spacing: float | None = None, mesh_dimensions: tuple[int, int, int] | None = None, spline_order: int = 5,
                          batch_idx: torch.Tensor | None = None, neighbor_list: torch.Tensor | None = None,
                          neighbor_ptr: torch.Tensor | None = None, neighbor_shifts: torch.Tensor | None = None,
                          neighbor_matrix: torch.Tensor | None = None, neighbor_matrix_shifts: torch.Tensor | None = None,
                          mask_value: int | None = None, compute_forces: bool = False, compute_charge_gradients: bool = False,
                          compute_dipole_gradients: bool = False, compute_virial: bool = False, accuracy: float = 1e-6):
    """What has to be ADDED to `particle_mesh_ewald` (or any point-charge periodic energy) so that it becomes the energy of point charges plus
    point dipoles `dipoles` [N, 3]: the charge-dipole and dipole-dipole energy, `ewald_dipole_real_space` + `pme_dipole_reciprocal_space`.
    The mesh counterpart of `ewald_dipole_correction`, to which it converges with the mesh.  MODEL

    The real-space half is the pair sum of `ewald_dipole_real_space` over the list (see there for its terms).  `alpha` and the mesh are
    estimated exactly as `particle_mesh_ewald` estimates them when not given (`accuracy`); pass the values the charge routine used, or any
    others: the sum of both halves does not depend on alpha beyond the truncation error.  Under `torch.compile(fullgraph=True)` pass `alpha`
    and `mesh_dimensions` (the estimate reads device data).  THE LIST MUST BE FULL (symmetric); a half or truncated list is not detected.  A
    matrix entry equal to `mask_value` (default: N) or outside [0, N) is padding.

    RETURNS"""
    if mask_value is None:
        mask_value = positions.shape[0]
    if neighbor_list is not None and neighbor_matrix is not None:
        raise ValueError("pass the list in ONE format: neighbor_list (with neighbor_ptr) or neighbor_matrix, not both")
    P.check_dipole_lists(positions, charges, dipoles, cell, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts,
                         batch_idx, alpha, compute_virial)
    return M.mesh_correction(MESH, (positions, charges, dipoles), cell, alpha, mesh_spacing, mesh_dimensions, spline_order, batch_idx,
                             (neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts), mask_value,
                             (True, compute_forces, compute_charge_gradients, compute_dipole_gradients, compute_virial), accuracy)


# what `_multipoles.mesh_*` run for this operator.  The functions are bound here, at import: rebinding `_spread`, `_gather`, `_virial` or
# `_recip_forward` on the module afterwards does not reach them (only `_SPREAD_FLOAT32_IN_FLOAT64` is read at call time).
MESH = dict(grads=M.DIPOLE, flags=FLAGS, check_order=_check_order, spread=_spread, gather=_gather, virial=_virial, forward=_recip_forward,
            op="pme_dipole_reciprocal_space_op", real=ewald_dipole_real_space, recip=pme_dipole_reciprocal_space)

for _fn in (pme_dipole_reciprocal_space, pme_dipole_correction):
    _fn.__doc__ = _fn.__doc__.replace("MODEL", _MODEL).replace("RETURNS", _RETURNS)
del _fn

__all__ = ["pme_dipole_reciprocal_space", "pme_dipole_correction"]
