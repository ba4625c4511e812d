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

import ctypes
import math

import torch

from nvalchemiops import _capi as C
from nvalchemiops.interactions.electrostatics import _pairs as P
from nvalchemiops.interactions.electrostatics import pme as _pme
from nvalchemiops.interactions.electrostatics.dipole import ewald_dipole_real_space
from nvalchemiops.interactions.electrostatics.pme import _prepare_alpha, _prepare_cell

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
    components and is NOT symmetric.

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
    order = C.plain_spline_order(spline_order)
    if order not in ORDERS:
        raise ValueError(f"spline_order must be 4, 5 or 6 for the dipole mesh sum (the forces need a continuous second derivative of the spline), "
                         f"got {order}")
    if int(spline_order) & C.SPLINE_REFERENCE_ORDERS or (not int(spline_order) & C.SPLINE_RESOLVED and not C.tracing()
                                                          and C.reference_spline_orders_active()):
        raise ValueError("the dipole mesh sum has no reference evaluation of the spline orders (reference_spline_orders): the reference package has "
                         "no dipole term")
    return order


def _mesh_dims(cells, mesh_dimensions, mesh_spacing, order):
    if mesh_dimensions is None:
        if mesh_spacing is None:
            raise ValueError("Either mesh_dimensions or mesh_spacing must be provided")
        mesh_dimensions = _pme.mesh_spacing_to_dimensions(cells, mesh_spacing)
    dims = tuple(int(v) for v in mesh_dimensions)
    if len(dims) != 3:
        raise ValueError(f"mesh_dimensions must hold three integers, got {mesh_dimensions}")
    if min(dims) < order:
        raise ValueError(f"every mesh dimension must be at least the spline order {order}, got {dims}")
    return dims


def _check_recip(positions, charges, dipoles, cell, alpha, batch_idx):
    if cell is None:
        raise ValueError("cell is required: the point-dipole Ewald sum is periodic (cell=None clusters are out of scope)")
    C.dtype_code(positions.dtype)
    C.check_per_atom(positions.shape[0], charges=charges, batch_idx=batch_idx)
    P.check_dipoles(positions, dipoles)
    C.check_neighbor_data(positions.shape[0], cell=cell, alpha=alpha)


# ---- launches -----------------------------------------------------------------------------------------------------------------------------
def _inputs(positions, charges, dipoles, cells, alpha, batch_idx):
    """Detached contiguous launch tensors plus the cell geometry (cell^-T, 2 pi cell^-1, volume) of `mi_pme_prepare`."""
    dt, dev, n = positions.dtype, positions.device, positions.shape[0]
    C.require_device(positions, charges, dipoles, cells, alpha, batch_idx)
    code = C.dtype_code(dt)
    batched = batch_idx is not None
    cc = cells.detach().to(dt).reshape(-1, 3, 3).contiguous()
    nsys = cc.shape[0] if batched else 1
    cc = cc[:nsys].contiguous()
    p = dict(pos=positions.detach().contiguous(), q=charges.detach().to(dt).contiguous(), mu=dipoles.detach().to(dt).contiguous(),
             al=alpha.detach().to(dt).reshape(-1)[:nsys].contiguous(), bi=C.i32(batch_idx) if batched else None, nsys=nsys, code=code, cells=cc)
    cit, recip = torch.empty_like(cc), torch.empty_like(cc)
    vol, qtot = torch.empty(nsys, dtype=dt, device=dev), torch.empty(nsys, dtype=dt, device=dev)
    C.check(C.lib().mi_pme_prepare(C.ptr(cc), C.ptr(p["q"]), C.ptr(p["bi"]), n, nsys, code, C.ptr(cit), C.ptr(recip), C.ptr(vol), C.ptr(qtot),
                                   C.stream_of(positions)), "mi_pme_prepare")
    p.update(cit=cit, recip=recip, vol=vol)
    return p


def _spread(p, dims, order, weights=None):
    """[2 | 4, nsys, nx, ny, nz]: rho_q, rho_mu (and their g-weighted twins), zero-filled by the entry point."""
    pos = p["pos"]
    if pos.dtype == torch.float32 and _SPREAD_FLOAT32_IN_FLOAT64:
        # float32 atomic adds in arrival order move the last bits of the meshes from run to run, and the Hessian sums of the gather carry
        # that into the forces at 1e-6 of their largest component.  Added in float64 and rounded once, the float32 meshes are the same
        # in every run (but for a sum that lands on a rounding boundary of float32).
        wide = {k: p[k].to(torch.float64) for k in ("pos", "q", "mu", "cit")}
        return _spread(dict(p, code=C.dtype_code(torch.float64), **wide), dims, order, weights).to(torch.float32)
    meshes = torch.empty((4 if weights is not None else 2, p["nsys"]) + dims, dtype=pos.dtype, device=pos.device)
    rc = C.lib().mi_pme_dipole_spread(C.ptr(pos), C.ptr(p["q"]), C.ptr(p["mu"]), C.ptr(weights), C.ptr(p["bi"]), C.ptr(p["cit"]), pos.shape[0],
                                      int(p["nsys"]), *dims, int(order), p["code"], C.ptr(meshes), C.stream_of(pos))
    C.check(rc, "mi_pme_dipole_spread")
    return meshes


def _solve(p, meshes, dims, order, need_spec):
    """phi_X = IFFT[G FFT(rho_X) / sf^2] of every mesh of `meshes` [M, nsys, nx, ny, nz] in ONE batched call: the M x nsys meshes are systems
    of the charge PME's solve, with the cell, alpha and volume rows repeated.  Returns (potentials, like `meshes`; spectra [M, nsys, nx, ny, nzr]
    or None).  The fused in-LDS solve where it is supported, hipFFT plan -> `mi_pme_convolve` -> plan otherwise, as `_reciprocal_front` does."""
    nx, ny, nz = dims
    m, nsys = meshes.shape[0], p["nsys"]
    b = m * nsys
    dt, dev, code = meshes.dtype, meshes.device, p["code"]
    st = C.stream_of(meshes)
    recip, al, vol = p["recip"].repeat(m, 1, 1), p["al"].repeat(m), p["vol"].repeat(m)
    cdt = torch.complex64 if dt == torch.float32 else torch.complex128
    L = C.lib()
    if _pme._MESH_SOLVE is not False and L.mi_pme_solve_supported(b, nx, ny, nz, code):
        nbytes = int(L.mi_pme_solve_scratch_bytes(b, nx, ny, nz, 1, code))
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        real = torch.empty((m, nsys, nx, ny, nz), dtype=dt, device=dev)
        spec = torch.empty((m, nsys, nx, ny, nz // 2 + 1), dtype=cdt, device=dev) if need_spec else None
        rc = L.mi_pme_solve_tabled(C.ptr(meshes), C.ptr(recip), C.ptr(al), C.ptr(vol), b, nx, ny, nz, int(order), 0, code, C.ptr(scratch),
                                   ctypes.c_size_t(nbytes), C.ptr(real), C.ptr(spec), C.ptr(_pme._solve_tables(dev, dims, code)), st)
        C.check(rc, "mi_pme_solve_tabled")
        return real, spec
    spec = torch.empty((m, nsys, nx, ny, nz // 2 + 1), dtype=cdt, device=dev)
    _pme._fft_plan(dev, dims, b, code, False)(meshes, spec)
    conv = torch.empty_like(spec)
    rc = L.mi_pme_convolve(C.ptr(spec), C.ptr(recip), C.ptr(al), C.ptr(vol), b, nx, ny, nz, int(order), 0, code, None, None, 0, C.ptr(conv), st)
    C.check(rc, "mi_pme_convolve")
    real = torch.empty((m, nsys, nx, ny, nz), dtype=dt, device=dev)
    _pme._fft_plan(dev, dims, b, code, True)(conv, real)
    return real, spec


def _gather(p, dims, order, mesh_a, mesh_b, weights=None, accumulate=False, out=None, energies=False, forces=False, cgrads=False, dgrads=False):
    """One `mi_pme_dipole_gather` launch over (A, B): float64 (energies | None, forces in the positions dtype | None, charge sums | None,
    dipole sums | None); `accumulate` adds to the tensors of `out`."""
    pos = p["pos"]
    n, dev = pos.shape[0], pos.device
    f64 = dict(dtype=torch.float64, device=dev)
    if accumulate:
        e, f, cg, dg = out
    else:
        e = torch.empty(n, **f64) if energies else None
        f = torch.empty((n, 3), dtype=pos.dtype, device=dev) if forces else None
        cg = torch.empty(n, **f64) if cgrads else None
        dg = torch.empty((n, 3), **f64) if dgrads else None
    rc = C.lib().mi_pme_dipole_gather(C.ptr(pos), C.ptr(p["q"]), C.ptr(p["mu"]), C.ptr(weights), C.ptr(p["bi"]), C.ptr(p["cit"]), C.ptr(mesh_a),
                                      C.ptr(mesh_b), C.ptr(p["al"]), n, int(p["nsys"]), *dims, int(order), p["code"], int(accumulate), C.ptr(e),
                                      C.ptr(f), C.ptr(cg), C.ptr(dg), C.stream_of(pos))
    C.check(rc, "mi_pme_dipole_gather")
    return e, f, cg, dg


def _self_coefficient(p):
    """2 alpha^3 / (3 sqrt(pi)) per atom, float64."""
    c = 2.0 * p["al"].to(torch.float64) ** 3 / (3.0 * math.sqrt(math.pi))
    return c[p["bi"].long()] if p["bi"] is not None else c.expand(p["pos"].shape[0])


def _recip_forward(positions, charges, dipoles, cell, alpha, batch_idx, dims, order, forces, cgrads, dgrads, virial):
    """(energies, forces | None, charge_grads | None, dipole_grads | None, virial | None) in the positions dtype, no autograd graph: what the
    eager call and the `alchemiops::_pme_dipole_reciprocal_space` op both run."""
    n, dev, dt = positions.shape[0], positions.device, positions.dtype
    want = (True, forces, cgrads, dgrads, virial)
    if n == 0:
        return tuple(r if w else None for r, w in zip(P.zeros(0, P.num_systems(cell, batch_idx), dt, dev), want))
    dims = tuple(int(v) for v in dims)
    p = _inputs(positions, charges, dipoles, cell, alpha, batch_idx)
    phi, spec = _solve(p, _spread(p, dims, order), dims, order, need_spec=virial)
    phi[0] += phi[1]  # phi_t = phi_q + phi_mu: the gather reads (A, B) = (phi_mu, phi_t)
    e, f, cg, dg = _gather(p, dims, order, phi[1], phi[0], energies=True, forces=forces, cgrads=cgrads, dgrads=dgrads or virial)
    vir = None
    if virial:
        L = C.lib()
        part = torch.empty((p["nsys"], int(L.mi_pme_dipole_virial_blocks()), 9), dtype=torch.float64, device=dev)
        rc = L.mi_pme_dipole_virial(C.ptr(spec[0]), C.ptr(spec[1]), C.ptr(p["recip"]), C.ptr(p["al"]), C.ptr(p["vol"]), int(p["nsys"]), *dims,
                                    int(order), p["code"], C.ptr(part), C.stream_of(positions))
        C.check(rc, "mi_pme_dipole_virial")
        # the dipoles' fractional components follow the strain: + sum_i (dE/dmu_i without its self term)_a mu_i,b per system (index order matters)
        mu64 = p["mu"].to(torch.float64)
        outer = (dg + 2.0 * _self_coefficient(p).unsqueeze(1) * mu64).unsqueeze(2) * mu64.unsqueeze(1)
        vir = C.fold_virial9(part)
        if p["bi"] is not None:
            vir = vir.index_add(0, p["bi"].long(), outer)
        else:
            vir = vir + outer.sum(0, keepdim=True)
        vir = vir.to(dt)
    return e.to(dt), f, cg.to(dt) if cgrads else None, dg.to(dt) if dgrads else None, vir


def _recip_adjoint(positions, charges, dipoles, cell, alpha, batch_idx, dims, order, grad_energies):
    """Float64 (dL/dpositions, dL/dcharges, dL/ddipoles) of L = sum_i g_i E_i.  The gather is its own adjoint: the g-weighted meshes ride in
    the same spread and the same batched solve (four meshes), and
        dL/dtheta_i = g_i x [gather over (phi_mu, phi_t)] + [gather over (phi^g_mu, phi^g_q + phi^g_mu)],   self term -c g_i |mu_i|^2."""
    n, dev = positions.shape[0], positions.device
    f64 = dict(dtype=torch.float64, device=dev)
    if n == 0:
        return torch.zeros((0, 3), **f64), torch.zeros(0, **f64), torch.zeros((0, 3), **f64)
    dims = tuple(int(v) for v in dims)
    p = _inputs(positions, charges, dipoles, cell, alpha, batch_idx)
    g = grad_energies.detach().to(torch.float64).contiguous()
    phi, _ = _solve(p, _spread(p, dims, order, weights=g), dims, order, need_spec=False)
    phi[0] += phi[1]
    phi[2] += phi[3]
    out = _gather(p, dims, order, phi[1], phi[0], weights=g, forces=True, cgrads=True, dgrads=True)
    _, f, gq, gmu = _gather(p, dims, order, phi[3], phi[2], accumulate=True, out=out)
    return -f.to(torch.float64), gq, gmu


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
    order = _check_order(spline_order)
    cells, n_sys = _prepare_cell(cell)
    dims = _mesh_dims(cells, mesh_dimensions, mesh_spacing, order)
    n, dev, dt = positions.shape[0], positions.device, positions.dtype
    want = (True, compute_forces, compute_charge_gradients, compute_dipole_gradients, compute_virial)
    if n == 0:
        return P.select(P.zeros(0, P.num_systems(cell, batch_idx), dt, dev), want)
    alpha_t = (_pme._traceable_alpha if C.tracing() else _prepare_alpha)(alpha, n_sys, dt, dev)
    flags = tuple(bool(w) for w in want[1:])
    if P.needs_op(positions, charges, dipoles, cell, alpha_t):
        from nvalchemiops import _eops

        res = _eops.pme_dipole_reciprocal_space_op(positions, charges.to(dt), dipoles.to(dt), cells, alpha_t, batch_idx, *dims, order, *flags)
    else:
        res = _recip_forward(positions, charges, dipoles, cells, alpha_t, batch_idx, dims, order, *flags)
    return P.select(res, want)


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
    order = _check_order(spline_order)
    cells, n_sys = _prepare_cell(cell)
    if mesh_dimensions is not None:
        mesh_dimensions = _mesh_dims(cells, mesh_dimensions, None, order)
    if positions.shape[0] == 0:
        want = (True, compute_forces, compute_charge_gradients, compute_dipole_gradients, compute_virial)
        return P.select(P.zeros(0, P.num_systems(cell, batch_idx), positions.dtype, positions.device), want)
    C.require_device(positions, charges, dipoles, cell, batch_idx)
    if alpha is None:
        est = _pme.estimate_pme_parameters(positions, cells, batch_idx, accuracy)
        alpha = est.alpha
        if mesh_dimensions is None and mesh_spacing is None:
            mesh_dimensions = tuple(est.mesh_dimensions)
    alpha_t = (_pme._traceable_alpha if C.tracing() else _prepare_alpha)(alpha, n_sys, positions.dtype, positions.device)
    if mesh_dimensions is None:
        mesh_dimensions = (_pme.mesh_spacing_to_dimensions(cells, mesh_spacing) if mesh_spacing is not None
                           else _pme.estimate_pme_mesh_dimensions(cells, alpha_t, accuracy))
    mesh_dimensions = _mesh_dims(cells, mesh_dimensions, None, order)
    flags = dict(compute_forces=compute_forces, compute_charge_gradients=compute_charge_gradients,
                 compute_dipole_gradients=compute_dipole_gradients, compute_virial=compute_virial)
    rs = ewald_dipole_real_space(positions, charges, dipoles, cells, alpha_t, neighbor_list=neighbor_list, neighbor_ptr=neighbor_ptr,
                                 neighbor_shifts=neighbor_shifts, neighbor_matrix=neighbor_matrix, neighbor_matrix_shifts=neighbor_matrix_shifts,
                                 mask_value=mask_value, batch_idx=batch_idx, **flags)
    rec = pme_dipole_reciprocal_space(positions, charges, dipoles, cells, alpha_t, mesh_dimensions=mesh_dimensions, spline_order=order,
                                      batch_idx=batch_idx, **flags)
    if isinstance(rs, tuple):
        return tuple(a + b for a, b in zip(rs, rec))
    return rs + rec


for _fn in (pme_dipole_reciprocal_space, pme_dipole_correction):
    _fn.__doc__ = _fn.__doc__.replace("MODEL", _MODEL).replace("RETURNS", _RETURNS)
del _fn

__all__ = ["pme_dipole_reciprocal_space", "pme_dipole_correction"]
