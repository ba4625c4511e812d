"""Dispersion PME (LJ-PME): the r^-6 lattice sum of `ewald.py` with its reciprocal half on a mesh, O(N + M log M) where the explicit sum of
`ewald_dispersion_reciprocal_space` is O(N K).

`pme_dispersion_correction` is `ewald_dispersion_real_space` (unchanged) plus `pme_dispersion_reciprocal_space`, and is ADDED to what
`lennard_jones` returns exactly as `ewald_dispersion_correction` is.  The reference package has no counterpart.

Launch sequence of the mesh half: `mi_spline_spread` of the coefficients (tile-owned and free of atomics where the library prefers tiles,
atomic adds into a zeroed mesh otherwise; float32 calls spread in float64 and round once) -> R2C (`mi_fft_lds`, or the guarded plans / dense
DFT behind `_pme._fft_plan`) -> `mi_pme_dispersion_convolve` (the r^-6 operator, and the virial in the same pass) -> C2R ->
`mi_pme_dispersion_gather` (csrc/dispersion_pme.hip).  The adjoint is the same sequence over two meshes, the second spread from g_i c_i, in
one batched transform each way."""
from __future__ import annotations

import torch

from nvalchemiops import _capi as C
from nvalchemiops import spline as S
from nvalchemiops.interactions.electrostatics import _multipoles as M
from nvalchemiops.interactions.electrostatics import _pairs as P
from nvalchemiops.interactions.electrostatics import pme as _pme
from nvalchemiops.interactions.electrostatics.pme import _prepare_cell
from nvalchemiops.interactions.vdw import ewald as E

_MODEL = """With beta = `alpha`, b = |k| / (2 beta), f(b) = (1 - 2 b^2) exp(-b^2) + 2 sqrt(pi) b^3 erfc(b) (the f of the explicit sum), `coefficients`
    c [N] with C6_ij = c_i c_j, frac = cell^-T r, mesh coordinate m_d = frac_d n_d and W_i(g) = prod_d M_p(p/2 + m_d - g_d) the order-p B-spline
    weight of atom i at mesh point g:

        rho = sum_i c_i W_i,   phi = IFFT_unscaled[D FFT(rho)],   D(m) = -(pi^1.5 beta^3 / (6 V)) f(b_m) / sf^2(m)
        E_i = c_i sum_g W_i(g) phi(g) + (beta^6 / 12) c_i^2

    over the FULL spectrum, m = 0 included: f(0) = 1, so D(0) IS the k = 0 term of the explicit sum.  sf^2 is the squared sinc product to the
    power p (clamped at 1e-10), as `pme_reciprocal_space` forms it.  The operator is self-adjoint: forces = -2 c_i grad W_i . phi and
    dE/dc_i = 2 W_i . phi + (beta^6 / 6) c_i.  The sum converges to `ewald_dispersion_reciprocal_space` with the mesh.  `spline_order` is 4, 5
    or 6 (ValueError otherwise) and every mesh dimension is at least the order."""

_RETURNS = """Returns ``energies`` [N], or a tuple holding only what was asked for, in this order: energies, forces [N, 3], coefficient_grads [N],
    virial [num_systems, 3, 3]; all in the positions dtype (stencils, per-atom epilogue and k-space sums in float64).  forces = -dE/dr and
    coefficient_grads = dE/dc of the total E = sum_i E_i; virial = -dE/d(strain) under x -> (I + eps) x with fractional coordinates, mesh and
    alpha fixed (symmetric; the self term does not strain):
    virial_ab = sum_m h_m D_m |rho_m|^2 [delta_ab + (f'(b) / f(b)) k_a k_b / (2 beta |k|)], f'(b) = -6 b exp(-b^2) + 6 sqrt(pi) b^2 erfc(b).

    Energies are differentiable once w.r.t. positions and coefficients, for any upstream gradient on the per-atom energies (the same kernels
    run as their own adjoint); the call then goes through the `alchemiops::_pme_dispersion_reciprocal_space` op, as it does under
    `torch.compile`.  Differentiating the explicit forces, gradients or virial raises NotImplementedError.  Gradients w.r.t. cell and alpha are
    out of scope (NotImplementedError at backward): use `compute_virial`.  Also out of scope: an alpha / mesh estimator, the seven-term
    expansion of the arithmetic rule, reduced sites, `cell=None` clusters.  Where the spread runs on atomic adds (small systems, meshes
    without a tile), float64 outputs are reproducible up to the arrival order of those adds; float32 outputs and every tile-owned run are the
    same in every run.  CPU tensors raise NativeLibraryError: there is no fallback."""

ORDERS = (4, 5, 6)


def _check_order(spline_order) -> int:
    return M.check_order(spline_order, ORDERS, "dispersion", "the forces need a continuous derivative of the spline and the kernels are built for these")


def _inputs(positions, coefficients, cells, alpha, batch_idx):
    """Detached contiguous launch tensors in the positions dtype plus the cell geometry (cell^-T, 2 pi cell^-1, volume) of `mi_pme_prepare`."""
    dt, dev, n = positions.dtype, positions.device, positions.shape[0]
    C.require_device(positions, coefficients, cells, alpha, batch_idx)
    code = C.dtype_code(dt)
    batched = batch_idx is not None
    cc = cells.detach().to(dt).reshape(-1, 3, 3).contiguous()
    nsys = cc.shape[0] if batched else 1
    cc = cc[:nsys].contiguous()
    p = dict(pos=positions.detach().contiguous(), c=coefficients.detach().to(dt).contiguous(),
             al=alpha.detach().to(dt).reshape(-1)[:nsys].contiguous(), bi=C.i32(batch_idx) if batched else None, nsys=nsys, code=code)
    cit, recip = torch.empty_like(cc), torch.empty_like(cc)
    vol, ctot = torch.empty(nsys, dtype=dt, device=dev), torch.empty(nsys, dtype=dt, device=dev)
    C.check(C.lib().mi_pme_prepare(C.ptr(cc), C.ptr(p["c"]), C.ptr(p["bi"]), n, nsys, code, C.ptr(cit), C.ptr(recip), C.ptr(vol), C.ptr(ctot),
                                   C.stream_of(positions)), "mi_pme_prepare")
    p.update(cit=cit, recip=recip, vol=vol)
    return p


def _spread(p, dims, order, weights=None):
    """[1 | 2, nsys, nx, ny, nz] in the positions dtype: rho and, with `weights` g, the mesh of g_i c_i.  Plain per-atom values through
    `mi_spline_spread`; a float32 call adds in float64 and rounds once, as `_multipoles.mesh_spread(wide=True)` does, which is also what the
    float64 stencils of the gather expect."""
    pos, vals, cit = p["pos"], p["c"], p["cit"]
    narrow = pos.dtype == torch.float32
    if narrow:
        pos, vals, cit = pos.to(torch.float64), vals.to(torch.float64), cit.to(torch.float64)
    meshes = torch.empty((1 if weights is None else 2, p["nsys"]) + tuple(dims), dtype=pos.dtype, device=pos.device)
    values = (vals,) if weights is None else (vals, (weights * vals.to(torch.float64)).to(pos.dtype))
    for mesh, v in zip(meshes, values):  # true B-splines whatever `reference_spline_orders` says: `_check_order` has refused that switch
        S._launch_spread(pos, v, cit, p["bi"], p["nsys"], dims, int(order) | C.SPLINE_RESOLVED, False, out=mesh)
    return meshes.to(torch.float32) if narrow else meshes


def _solve(p, meshes, dims, order, virial):
    """(phi like `meshes`, float64 virial [nsys, 3, 3] of mesh 0 | None): R2C, the r^-6 operator in place, C2R -- every mesh of the call in one
    batched transform each way."""
    nx, ny, nz = dims
    m, nsys = meshes.shape[0], p["nsys"]
    dt, dev, code = meshes.dtype, meshes.device, p["code"]
    L = C.lib()
    spec = torch.empty((m, nsys, nx, ny, nz // 2 + 1), dtype=torch.complex64 if dt == torch.float32 else torch.complex128, device=dev)
    _pme._fft_plan(dev, dims, m * nsys, code, False)(meshes, spec)
    part = torch.empty((nsys, int(L.mi_pme_dispersion_virial_blocks()), 6), dtype=torch.float64, device=dev) if virial else None
    rc = L.mi_pme_dispersion_convolve(C.ptr(spec), C.ptr(p["recip"]), C.ptr(p["al"]), C.ptr(p["vol"]), int(nsys), int(m), nx, ny, nz, int(order), code,
                                      C.ptr(spec), C.ptr(part), C.stream_of(meshes))
    C.check(rc, "mi_pme_dispersion_convolve")
    phi = torch.empty_like(meshes)
    _pme._fft_plan(dev, dims, m * nsys, code, True)(spec, phi)
    return phi, C.fold_virial(part) if virial else None


def _gather(p, dims, order, phi, want, phi_g=None, weights=None):
    """One `mi_pme_dispersion_gather` launch: float64 (energies | None, forces in the positions dtype | None, coefficient sums | None)."""
    pos = p["pos"]
    n, dev = pos.shape[0], pos.device
    e = torch.empty(n, dtype=torch.float64, device=dev) if want[0] else None
    f = torch.empty((n, 3), dtype=pos.dtype, device=dev) if want[1] else None
    cg = torch.empty(n, dtype=torch.float64, device=dev) if want[2] else None
    rc = C.lib().mi_pme_dispersion_gather(C.ptr(pos), C.ptr(p["c"]), C.ptr(weights), C.ptr(p["bi"]), C.ptr(p["cit"]), C.ptr(phi), C.ptr(phi_g),
                                          C.ptr(p["al"]), n, int(p["nsys"]), *dims, int(order), p["code"], C.ptr(e), C.ptr(f), C.ptr(cg),
                                          C.stream_of(pos))
    C.check(rc, "mi_pme_dispersion_gather")
    return e, f, cg


def _recip_forward(positions, coefficients, cell, alpha, batch_idx, nx, ny, nz, order, forces, cgrads, virial):
    """(energies, forces | None, coefficient_grads | None, virial | None) in the positions dtype, no autograd graph: what the eager call and
    the `alchemiops::_pme_dispersion_reciprocal_space` op both run."""
    n, dev, dt = positions.shape[0], positions.device, positions.dtype
    want = (True, forces, cgrads, virial)
    if n == 0:
        return E._zeros(0, P.num_systems(cell, batch_idx), dt, dev, want)
    dims = (int(nx), int(ny), int(nz))
    p = _inputs(positions, coefficients, cell, alpha, batch_idx)
    phi, vir = _solve(p, _spread(p, dims, order), dims, order, virial)
    e, f, cg = _gather(p, dims, order, phi[0], want[:3])
    return e.to(dt), f, cg.to(dt) if cgrads else None, vir.to(dt) if virial else None


def _recip_adjoint(positions, coefficients, cell, alpha, batch_idx, nx, ny, nz, order, grad_energies):
    """Float64 (dL/dpositions, dL/dcoefficients) of L = sum_i g_i E_i: the mesh of g_i c_i rides in the same transforms, and the gather runs in
    its adjoint form over (phi, phi^g); the self term takes g_i."""
    n, dev = positions.shape[0], positions.device
    if n == 0:
        return torch.zeros((0, 3), dtype=torch.float64, device=dev), torch.zeros(0, dtype=torch.float64, device=dev)
    dims = (int(nx), int(ny), int(nz))
    p = _inputs(positions, coefficients, cell, alpha, batch_idx)
    g = M.weights_of(grad_energies)
    phi, _ = _solve(p, _spread(p, dims, order, weights=g), dims, order, False)
    _, f, cg = _gather(p, dims, order, phi[0], (False, True, True), phi_g=phi[1], weights=g)
    return -f.to(torch.float64), cg


# ---- public -------------------------------------------------------------------------------------------------------------------------------
@C.traceable
def pme_dispersion_reciprocal_space(positions: torch.Tensor, coefficients: torch.Tensor, cell: torch.Tensor, alpha, *,
                                    mesh_dimensions: tuple[int, int, int] | None = None, mesh_spacing: float | None = None,
                                    spline_order: int = 5, batch_idx: torch.Tensor | None = None, compute_forces: bool = False,
                                    compute_coefficient_gradients: bool = False, compute_virial: bool = False):
    """Mesh (reciprocal-space) half of the dispersion lattice sum, the k = 0 and self terms included: the mesh counterpart of
    `ewald_dispersion_reciprocal_space`.  MODEL

    `alpha` is a number or one value per system, and is required, as is one of `mesh_dimensions` / `mesh_spacing` (turned into dimensions as
    `particle_mesh_ewald` does): there is no estimator.  With `batch_idx`, `cell` is [num_systems, 3, 3] and all systems share the mesh
    dimensions.

    RETURNS"""
    E._check_common(positions, coefficients, cell, batch_idx, alpha)
    order = _check_order(spline_order)
    cells, n_sys = _prepare_cell(cell)
    dims = M.mesh_dims(cells, mesh_dimensions, mesh_spacing, order)
    want = (True, compute_forces, compute_coefficient_gradients, compute_virial)
    n, dt, dev = positions.shape[0], positions.dtype, positions.device
    if n == 0:
        return P.select(P.zeros(0, P.num_systems(cell, batch_idx), dt, dev, ()), want)
    alpha_t = M._mesh_alpha(alpha, n_sys, positions)
    args = (positions, coefficients.to(dt), cells, alpha_t, batch_idx, *dims, order, bool(compute_forces), bool(compute_coefficient_gradients),
            bool(compute_virial))
    return P.dispatch("pme_dispersion_reciprocal_space_op", _recip_forward, args, (positions, coefficients, cells, alpha_t), want)


@C.traceable
def pme_dispersion_correction(positions: torch.Tensor, coefficients: torch.Tensor, cell: torch.Tensor, alpha, *,
                              mesh_dimensions: tuple[int, int, int] | None = None, mesh_spacing: float | None = None, spline_order: int = 5,
                              neighbor_list: torch.Tensor | None = None, neighbor_ptr: torch.Tensor | None = None,
                              neighbor_shifts: torch.Tensor | None = None, neighbor_matrix: torch.Tensor | None = None,
                              neighbor_matrix_shifts: torch.Tensor | None = None, mask_value: int = -1, batch_idx: torch.Tensor | None = None,
                              counted_cutoff: float | None = None, counted_taper: float | None = None, compute_forces: bool = False,
                              compute_coefficient_gradients: bool = False, compute_virial: bool = False):
    """The r^-6 lattice sum of a dispersion potential with its reciprocal half on a mesh, `ewald_dispersion_real_space` +
    `pme_dispersion_reciprocal_space`: what has to be ADDED to a `lennard_jones` energy truncated at `counted_cutoff` (tapered from
    `counted_taper`) on the same list so that its attractive part becomes the sum over the lattice.  The mesh counterpart of
    `ewald_dispersion_correction`, to which it converges with the mesh.  MODEL

    The real-space half is the pair sum of `ewald_dispersion_real_space` over the list (see there for its terms and for `counted_cutoff` /
    `counted_taper`).  `alpha` is required, and so is one of `mesh_dimensions` / `mesh_spacing`: there is no estimator.  THE LIST MUST BE FULL
    (symmetric); a half or truncated list is not detected.  A matrix entry equal to `mask_value` or outside [0, N) is padding.

    RETURNS"""
    E._check_common(positions, coefficients, cell, batch_idx, alpha)
    order = _check_order(spline_order)
    dims = M.mesh_dims(_prepare_cell(cell)[0], mesh_dimensions, mesh_spacing, order)
    flags = dict(compute_forces=compute_forces, compute_coefficient_gradients=compute_coefficient_gradients, compute_virial=compute_virial)
    real = E.ewald_dispersion_real_space(positions, coefficients, cell, alpha, neighbor_list=neighbor_list, neighbor_ptr=neighbor_ptr,
                                         neighbor_shifts=neighbor_shifts, neighbor_matrix=neighbor_matrix,
                                         neighbor_matrix_shifts=neighbor_matrix_shifts, mask_value=mask_value, batch_idx=batch_idx,
                                         counted_cutoff=counted_cutoff, counted_taper=counted_taper, **flags)
    rec = pme_dispersion_reciprocal_space(positions, coefficients, cell, alpha, mesh_dimensions=dims, spline_order=order, batch_idx=batch_idx,
                                          **flags)
    return M.add_halves(real, rec)


for _fn in (pme_dispersion_reciprocal_space, pme_dispersion_correction):
    _fn.__doc__ = _fn.__doc__.replace("MODEL", _MODEL).replace("RETURNS", _RETURNS)
del _fn

__all__ = ["pme_dispersion_reciprocal_space", "pme_dispersion_correction"]
