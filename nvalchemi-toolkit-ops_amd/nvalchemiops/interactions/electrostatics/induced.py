"""Induced point dipoles: the dipoles that minimise, per system,

    U(mu) = sum_i |mu_i|^2 / (2 a_i) + E_dip(q, mu) - sum_i mu_i . F_i

with a_i the isotropic polarisability of atom i, F an optional external field and E_dip the charge-dipole and dipole-dipole energy of this
package: `ewald_dipole_real_space` + `pme_dipole_reciprocal_space` (or `ewald_dipole_reciprocal_space`), self term and tin-foil boundary
included.  E_dip is bilinear in (q, mu) and quadratic in mu, so the solution satisfies mu_i / a_i + dE_dip/dmu_i - F_i = 0: a linear system
H mu = b with H = diag(1 / a) + T, T the dipole-dipole operator, and b = -dE_dip/dmu at mu = 0, plus F.  The reference package has no
counterpart.

The geometry does not change during a solve, so the real-space part of T is a constant operator over the caller's FULL neighbour list.
`mi_induced_pair_tensors` (csrc/induced.hip) evaluates it once -- the only erfc / exp / sqrt of a solve -- and every matrix-vector product is
`mi_induced_apply`, a sparse product of 3 x 3 blocks over 44 bytes per list slot, plus one reciprocal-space dipole-gradient call on the search
direction.  The solver is Jacobi-preconditioned conjugate gradients (preconditioner diag(a)); all per-system scalars live on the device
(`mi_induced_cg_update`, `mi_induced_cg_direction`) and every sum of these kernels is a fixed-order fold.

In `thole_induced_dipoles` the energy is E_dip + `thole_dipole_correction` (exponential Thole damping, thole.py): `mi_thole_induced_pair_tensors` stores the
damped coefficients in the same layout, and everything after the set-up is the same code.
"""
from __future__ import annotations

from collections import namedtuple

import torch

from nvalchemiops import _capi as C
from nvalchemiops.interactions.electrostatics import _multipoles as M
from nvalchemiops.interactions.electrostatics import _pairs as P
from nvalchemiops.interactions.electrostatics import dipole as D
from nvalchemiops.interactions.electrostatics import pme_dipole as PD
from nvalchemiops.interactions.electrostatics import thole as TH

F64 = torch.float64
InducedDipoleResult = namedtuple("InducedDipoleResult", ["dipoles", "polarization_energy", "iterations", "residual"])


class InducedDipoleError(RuntimeError):
    """The conjugate-gradient solve did not reach `tolerance` within `max_iterations`, or it met a search direction of non-positive
    curvature: the operator is not positive definite (the polarisation catastrophe of undamped point dipoles)."""


def _check(positions, charges, polarizability, cell, external_field, batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix,
           neighbor_matrix_shifts, reciprocal, alpha, mesh_dimensions, mesh_spacing, spline_order, k_vectors, k_cutoff, tolerance, max_iterations,
           check_interval, initial_dipoles, thole=None) -> int:
    """Every argument error, before anything is launched (`_pairs.check_dipole_lists` for the list and the required cell).  Returns the number
    of systems: the cell count."""
    if positions.dim() != 2 or positions.shape[1] != 3:
        raise ValueError(f"positions must have shape [num_atoms, 3], got {tuple(positions.shape)}")
    n = positions.shape[0]
    if neighbor_list is not None and neighbor_matrix is not None:
        raise ValueError("pass the list in ONE format: neighbor_list (with neighbor_ptr) or neighbor_matrix, not both")
    # (there are no input dipoles: `positions` stands in for the [N, 3] array whose shape the shared check looks at)
    P.check_dipole_lists(positions, charges, positions, cell, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts,
                         batch_idx, alpha, False)
    if isinstance(polarizability, torch.Tensor) and polarizability.dim() > 0:
        C.check_per_atom(n, polarizability=polarizability)
        if polarizability.dim() != 1:
            raise ValueError(f"polarizability must have one entry per atom: expected shape [{n}], got {tuple(polarizability.shape)}")
    elif not isinstance(polarizability, (int, float, torch.Tensor)):
        raise TypeError(f"polarizability must be a number or torch.Tensor, got {type(polarizability)}")
    for name, t in (("external_field", external_field), ("initial_dipoles", initial_dipoles)):
        if t is not None and tuple(t.shape) != (n, 3):
            raise ValueError(f"{name} must have one vector per atom: expected shape [{n}, 3], got {tuple(t.shape)}")
    if reciprocal not in ("pme", "ewald"):
        raise ValueError(f"reciprocal must be 'pme' or 'ewald', got {reciprocal!r}")
    if thole is not None:
        TH.check_thole(thole)
    nsys = cell.shape[0] if cell.dim() == 3 else 1
    C.check_neighbor_data(n, cell=cell, alpha=alpha)
    if reciprocal == "pme":
        if k_cutoff is not None:
            raise ValueError("k_cutoff belongs to reciprocal='ewald'")
        if k_vectors is not None:
            raise ValueError("k_vectors belong to reciprocal='ewald'")
        order = PD._check_order(spline_order)
        if mesh_dimensions is not None:
            M.mesh_dims(cell.reshape(-1, 3, 3), mesh_dimensions, None, order)
    else:
        if mesh_dimensions is not None or mesh_spacing is not None:
            raise ValueError("mesh_dimensions / mesh_spacing belong to reciprocal='pme'")
        if k_vectors is not None and (k_vectors.shape[-1] != 3 or k_vectors.dim() not in (2, 3)
                                      or (k_vectors.dim() == 3 and k_vectors.shape[0] not in (1, nsys))):
            raise ValueError(f"k_vectors must have shape [K, 3] or [{nsys}, K, 3], got {tuple(k_vectors.shape)}")
    if nsys > 1 and batch_idx is None:
        raise ValueError(f"batch_idx is required for {nsys} systems")
    if not float(tolerance) > 0.0:
        raise ValueError(f"tolerance must be positive, got {tolerance}")
    if int(max_iterations) < 1:
        raise ValueError(f"max_iterations must be at least 1, got {max_iterations}")
    if int(check_interval) < 1:
        raise ValueError(f"check_interval must be at least 1, got {check_interval}")
    return nsys


class _Operator:
    """H = diag(1 / a) + T of one geometry: the stored real-space tensors and the reciprocal-space dipole-gradient call.  `reciprocal=None`
    is the mode without a reciprocal part (`cluster_induced_dipoles`: no cell, no alpha, no shifts): the stored operator holds the bare
    1 / r^3, 3 / r^5 coefficients, H x is the stored-operator product alone, and the energy is `coulomb_dipole_correction`."""

    name = "induced_dipoles"  # the public function in error messages

    def __init__(self, positions, polar, cell, batch_idx, nsys, lists, mask_value, reciprocal, alpha, mesh_dimensions, mesh_spacing, spline_order,
                 k_vectors, k_cutoff, accuracy, thole=None):
        dt, dev, n = positions.dtype, positions.device, positions.shape[0]
        self.n, self.nsys, self.dt, self.dev = n, nsys, dt, dev
        self.pos = positions.detach().contiguous()
        self.polar = polar.detach().to(dt).contiguous()
        self.bi = C.i32(batch_idx) if nsys > 1 else None
        self.batch_idx = batch_idx if nsys > 1 else None
        self.cells = None if cell is None else cell.detach().to(dt).reshape(-1, 3, 3).contiguous()
        self.reciprocal = reciprocal
        self.thole = None if thole is None else float(thole)  # the Thole width: B_n + D_n in the stored operator, E_dip + E_thole in the energy
        self.alpha = self.kv = self.dims = self.order = None
        if reciprocal is not None:
            self._reciprocal_parameters(alpha, mesh_dimensions, mesh_spacing, spline_order, k_vectors, k_cutoff, accuracy)
        ls = P.list_inputs(*lists)
        self.idx, self.nptr, self.m, self.sh, self.slots = ls["idx"], ls["nptr"], ls["m"], ls["sh"], ls["n_entries"]
        L = C.lib()
        self.blocks, self.words = int(L.mi_induced_blocks()), int(L.mi_induced_state_words())
        self.tensors = torch.empty((int(L.mi_induced_tensor_words()), self.slots), dtype=F64, device=dev)
        self.nbr = torch.empty(self.slots, dtype=torch.int32, device=dev)
        self.diag, self.precond = torch.empty(n, dtype=F64, device=dev), torch.empty(n, dtype=F64, device=dev)
        self.mask_value = int(mask_value)
        self.pair_tensors()
        self.mask = (self.polar > 0).to(F64).unsqueeze(1)  # the projector onto the polarisable atoms
        zq, zmu = torch.zeros(n, dtype=dt, device=dev), torch.zeros((n, 3), dtype=dt, device=dev)
        if reciprocal == "pme":  # launch tensors of the reciprocal call, made once: only the dipoles change between iterations
            self.rp = M.mesh_inputs(self.pos, zq, zmu, self.cells, self.alpha, self.batch_idx)
        elif reciprocal == "ewald":
            self.rp = D._recip_inputs(self.pos, zq, zmu, self.cells, self.kv, self.alpha, self.batch_idx)

    def pair_tensors(self):
        if self.reciprocal is None:
            rc = C.lib().mi_cluster_induced_pair_tensors(C.ptr(self.pos), C.ptr(self.polar), self.n, C.dtype_code(self.dt), C.ptr(self.idx),
                                                         C.ptr(self.nptr), int(self.m), self.mask_value, self.slots, C.ptr(self.tensors),
                                                         C.ptr(self.nbr), C.ptr(self.diag), C.ptr(self.precond),
                                                         C.cdouble(0.0 if self.thole is None else self.thole), C.stream_of(self.pos))
            C.check(rc, "mi_cluster_induced_pair_tensors")
            return
        args = (C.ptr(self.pos), C.ptr(self.polar), C.ptr(self.cells), C.ptr(self.alpha), C.ptr(self.bi), self.n, self.nsys, C.dtype_code(self.dt),
                C.ptr(self.idx), C.ptr(self.sh), C.ptr(self.nptr), int(self.m), self.mask_value, self.slots, C.ptr(self.tensors), C.ptr(self.nbr),
                C.ptr(self.diag), C.ptr(self.precond))
        if self.thole is None:
            C.check(C.lib().mi_induced_pair_tensors(*args, C.stream_of(self.pos)), "mi_induced_pair_tensors")
        else:
            C.check(C.lib().mi_thole_induced_pair_tensors(*args, C.cdouble(self.thole), C.stream_of(self.pos)), "mi_thole_induced_pair_tensors")

    def _reciprocal_parameters(self, alpha, mesh_dimensions, mesh_spacing, spline_order, k_vectors, k_cutoff, accuracy):
        """alpha, and the mesh or the k-vectors, as `pme_dipole_correction` / `ewald_dipole_correction` would choose them."""
        from nvalchemiops.interactions.electrostatics import ewald as EW, pme as PME
        from nvalchemiops.interactions.electrostatics.k_vectors import generate_k_vectors_ewald_summation
        from nvalchemiops.interactions.electrostatics.parameters import estimate_ewald_parameters

        cells, dt, dev = self.cells, self.dt, self.dev
        if self.reciprocal == "pme":
            self.order = PD._check_order(spline_order)
            if alpha is None:
                est = PME.estimate_pme_parameters(self.pos, cells, self.batch_idx, accuracy)
                alpha = est.alpha
                if mesh_dimensions is None and mesh_spacing is None:
                    mesh_dimensions = tuple(est.mesh_dimensions)
            self.alpha = PME._prepare_alpha(alpha, self.nsys, dt, dev).detach().to(dt).contiguous()
            if mesh_dimensions is None:
                mesh_dimensions = (PME.mesh_spacing_to_dimensions(cells, mesh_spacing) if mesh_spacing is not None
                                   else PME.estimate_pme_mesh_dimensions(cells, self.alpha, accuracy))
            self.dims = M.mesh_dims(cells, mesh_dimensions, None, self.order)
        else:
            if alpha is None or (k_cutoff is None and k_vectors is None):
                params = estimate_ewald_parameters(self.pos, cells, self.batch_idx, accuracy)
                alpha = params.alpha if alpha is None else alpha
                k_cutoff = params.reciprocal_space_cutoff if k_cutoff is None else k_cutoff
            self.alpha = EW._prepare_alpha(alpha, self.nsys, dt, dev).detach().to(dt).contiguous()
            self.kv = (k_vectors if k_vectors is not None else generate_k_vectors_ewald_summation(cells, k_cutoff)).detach()

    def per_atom(self, v):
        return (v[self.bi.long()] if self.bi is not None else v.expand(self.n)).unsqueeze(1)

    # ---- the pieces of H x ----------------------------------------------------------------------------------------------------------------
    def reciprocal_gradient(self, x):
        """float64 [N, 3] dE_recip/dmu at zero charges and the dipoles x (linear in x), projected onto the polarisable atoms: the dipole
        gradient of the public reciprocal-space function -- same launches, the energies skipped, the same rounding to the positions dtype.
        None without a reciprocal part."""
        if self.reciprocal is None:
            return None
        with torch.no_grad():
            p = dict(self.rp, mu=x.to(self.dt).contiguous())
            if self.reciprocal == "pme":
                phi, _ = M.mesh_solve(p, PD._spread(p, self.dims, self.order), self.dims, self.order, need_spec=False)
                phi[0] += phi[1]
                dg = PD._gather(p, self.dims, self.order, phi[1], phi[0], (False, False, False, True))[3]
            else:
                dg = D._gather(p, D._table(p), (False, False, False, True))[3]
        return (dg.to(self.dt).to(F64) * self.mask).contiguous()

    def apply(self, x, y_in=None, partial=None):
        """y = y_in + x / a + T_real x (`mi_induced_apply`), and the per-system block partials of x . y when asked for."""
        y = torch.empty((self.n, 3), dtype=F64, device=self.dev)
        rc = C.lib().mi_induced_apply(C.ptr(self.tensors), C.ptr(self.nbr), C.ptr(self.diag), C.ptr(x), C.ptr(y_in), C.ptr(self.bi), self.n,
                                      self.nsys, C.ptr(self.nptr), int(self.m), self.slots, C.ptr(y), C.ptr(partial), C.stream_of(x))
        C.check(rc, "mi_induced_apply")
        return y

    def full(self, x, partial=None):
        """H x with every term of the public energies."""
        return self.apply(x, self.reciprocal_gradient(x), partial)

    def dot(self, x, y):
        """float64 [nsys] per-system sums of x . y in the fixed order of the product kernel's fold."""
        part = torch.empty((self.nsys, self.blocks), dtype=F64, device=self.dev)
        rc = C.lib().mi_induced_dot(C.ptr(x), C.ptr(y), C.ptr(self.bi), self.n, self.nsys, C.ptr(part), C.stream_of(x))
        C.check(rc, "mi_induced_dot")
        return part.sum(1)

    def right_hand_side(self, charges, field, lists, mask_value):
        """b = -dE_dip/dmu at mu = 0 (+ F) on the polarisable atoms, [N, 3] float64: one call each of the public real-space and
        reciprocal-space functions."""
        kw = dict(zip(("neighbor_list", "neighbor_ptr", "neighbor_shifts", "neighbor_matrix", "neighbor_matrix_shifts"), lists))
        q = charges.detach().to(self.dt)
        mu0 = torch.zeros((self.n, 3), dtype=self.dt, device=self.dev)
        with torch.no_grad():
            if self.reciprocal is None:
                from nvalchemiops.interactions.electrostatics.cluster import coulomb_dipole_correction

                g = coulomb_dipole_correction(self.pos, q, mu0, mask_value=mask_value, compute_dipole_gradients=True, **kw)[1].to(F64)
            else:
                g = D.ewald_dipole_real_space(self.pos, q, mu0, self.cells, self.alpha, mask_value=mask_value, batch_idx=self.batch_idx,
                                              compute_dipole_gradients=True, **kw)[1].to(F64)
            if self.reciprocal == "pme":
                g = g + PD.pme_dipole_reciprocal_space(self.pos, q, mu0, self.cells, self.alpha, mesh_dimensions=self.dims, spline_order=self.order,
                                                       batch_idx=self.batch_idx, compute_dipole_gradients=True)[1].to(F64)
            elif self.reciprocal == "ewald":
                g = g + D.ewald_dipole_reciprocal_space(self.pos, q, mu0, self.cells, self.kv, self.alpha, batch_idx=self.batch_idx,
                                                        compute_dipole_gradients=True)[1].to(F64)
            if self.thole is not None:
                g = g + TH.thole_dipole_correction(self.pos, q, mu0, self.polar, self.cells, thole=self.thole, mask_value=mask_value,
                                                   batch_idx=self.batch_idx, compute_dipole_gradients=True, **kw)[1].to(F64)
        b = -g if field is None else field.detach().to(F64) - g
        return (b * self.mask).contiguous()


def _conjugate_gradients(op: _Operator, b, initial, tolerance, max_iterations, check_interval, what):
    """Jacobi-preconditioned CG on H x = b.  `b` is [N, 3] float64 and zero on non-polarisable atoms; the iteration starts from a b (the
    preconditioner applied to b) or from `initial` [N, 3], and ||b|| is the norm the tolerance refers to in both cases.  Returns
    (x [N, 3], state [nsys, words]).  The host reads the done / breakdown flags once every `check_interval` iterations and at no other time."""
    L, n, nsys, dev = C.lib(), op.n, op.nsys, op.dev
    f64 = dict(dtype=F64, device=dev)
    state = [torch.zeros((nsys, op.words), **f64), torch.zeros((nsys, op.words), **f64)]
    part_y, part_rr = torch.empty((nsys, op.blocks), **f64), torch.empty((nsys, op.blocks, 2), **f64)
    r, p = torch.empty((n, 3), **f64), torch.empty((n, 3), **f64)
    stream = C.stream_of(r)

    def update(y, mode, x):
        C.check(L.mi_induced_cg_update(C.ptr(y), C.ptr(part_y), C.ptr(op.precond), C.ptr(op.bi), n, nsys, mode, C.ptr(x), C.ptr(r), C.ptr(p),
                                       C.ptr(state[0]), C.ptr(state[1]), C.ptr(part_rr), stream), "mi_induced_cg_update")

    def direction(mode):
        C.check(L.mi_induced_cg_direction(C.ptr(part_rr), C.ptr(op.precond), C.ptr(op.bi), n, nsys, mode, C.cdouble(tolerance), C.ptr(r),
                                          C.ptr(p), C.ptr(state[1]), C.ptr(state[0]), stream), "mi_induced_cg_direction")

    # ||b||: the residual of x = 0 is b itself; a system with b = 0 is done here and keeps x = 0
    update((-b).contiguous(), 1, None)
    direction(1)
    start = op.precond.unsqueeze(1) * b if initial is None else initial.detach().to(F64) * op.mask
    x = torch.where(op.per_atom(state[0][:, 1]) > 0, start, torch.zeros_like(start)).contiguous()
    update(op.full(x) - b, 1, None)
    direction(2)
    converged = False
    for it in range(1, int(max_iterations) + 1):
        y = op.apply(p, op.reciprocal_gradient(p), part_y)
        update(y, 0, x)
        direction(0)
        if it % int(check_interval) == 0 or it == int(max_iterations):
            flags = state[0][:, [2, 6]].cpu()  # the one host read
            broken = torch.nonzero(flags[:, 1]).flatten().tolist()
            if broken:
                raise InducedDipoleError(
                    f"{what}: the operator is not positive definite for " + ", ".join(f"system {s}" for s in broken[:16])
                    + (f" and {len(broken) - 16} more" if len(broken) > 16 else "")
                    + ": a search direction p with p.Hp <= 0 was met (the polarisation catastrophe of undamped point dipoles: a polarisability "
                    "too large for the shortest distance)")
            converged = bool((flags[:, 0] != 0).all())
            if converged:
                break
    if not converged:
        st = state[0].cpu()
        res = torch.sqrt(st[:, 7] / st[:, 1])
        bad = [(s, float(res[s])) for s in range(nsys) if st[s, 2] == 0]
        raise InducedDipoleError(
            f"{what}: no convergence to tolerance {tolerance:g} within {int(max_iterations)} iterations for "
            + ", ".join(f"system {s} (residual {v:.3e})" for s, v in bad[:16]) + (f" and {len(bad) - 16} more" if len(bad) > 16 else ""))
    return x, state[0]


def _info(state):
    """(iterations int64 [nsys], relative residual ||r|| / ||b|| float64 [nsys]) from the solver state, on the device."""
    rr, bb = state[:, 7], state[:, 1]
    return state[:, 3].to(torch.int64), torch.where(bb > 0, torch.sqrt(rr / torch.where(bb > 0, bb, torch.ones_like(bb))), torch.zeros_like(rr))


def _thole_energy(op: _Operator, positions, charges, dipoles, polar, lists, mask_value):
    """Total E_thole(charges, dipoles) of a damped solve from the differentiable public function (also w.r.t. the polarisabilities)."""
    kw = dict(zip(("neighbor_list", "neighbor_ptr", "neighbor_shifts", "neighbor_matrix", "neighbor_matrix_shifts"), lists))
    dt = positions.dtype
    return TH.thole_dipole_correction(positions, charges.to(dt), dipoles.to(dt), polar.to(dt), op.cells, thole=op.thole, batch_idx=op.batch_idx,
                                      mask_value=mask_value, **kw).sum()


def _dipole_energy(op: _Operator, positions, charges, dipoles, lists, mask_value, polar=None):
    """Total E_dip(charges, dipoles) from the differentiable public functions, alpha and the mesh / k-vectors of the solve held fixed; plus
    E_thole of a damped solve (`polar` then gives the polarisabilities to differentiate; default: the operator's own)."""
    kw = dict(zip(("neighbor_list", "neighbor_ptr", "neighbor_shifts", "neighbor_matrix", "neighbor_matrix_shifts"), lists))
    q, mu = charges.to(positions.dtype), dipoles.to(positions.dtype)
    if op.reciprocal is None:
        from nvalchemiops.interactions.electrostatics.cluster import coulomb_dipole_correction

        e = coulomb_dipole_correction(positions, q, mu, mask_value=mask_value, **kw).sum()
    elif op.reciprocal == "pme":
        e = PD.pme_dipole_correction(positions, q, mu, op.cells, alpha=op.alpha, mesh_dimensions=op.dims, spline_order=op.order,
                                     batch_idx=op.batch_idx, mask_value=mask_value, **kw).sum()
    else:
        e = D.ewald_dipole_correction(positions, q, mu, op.cells, alpha=op.alpha, k_vectors=op.kv, batch_idx=op.batch_idx, mask_value=mask_value,
                                      **kw).sum()
    if op.thole is None:
        return e
    return e + _thole_energy(op, positions, charges, dipoles, op.polar if polar is None else polar, lists, mask_value)


class _InducedDipoles(torch.autograd.Function):
    """The solve under autograd: implicit differentiation of the stationarity condition, no new kernels.  With g = dL/dmu and z = H^-1 g (one
    more solve with the stored operator):  dL/dF = z,  dL/da_i = (z_i . mu_i) / a_i^2, and for theta in {positions, charges}
    dL/dtheta = -1/2 d/dtheta [E_dip(q, mu + z) - E_dip(q, mu - z)]  with mu and z held fixed.  A damped solve has E_dip + E_thole in that
    difference, and E_thole depends on the polarisabilities: dL/da gains -1/2 d/da [E_thole(q, mu + z) - E_thole(q, mu - z)]."""

    @staticmethod
    def forward(ctx, positions, charges, polar, field, op, b, initial, lists, mask_value, solver):
        x, state = _conjugate_gradients(op, b, initial, *solver, op.name)
        mu = x
        ctx.save_for_backward(positions, charges, polar, mu)
        ctx.op, ctx.lists, ctx.mask_value, ctx.solver = op, lists, mask_value, solver
        ctx.field_dtype = None if field is None else field.dtype
        state = state.clone()
        ctx.mark_non_differentiable(state)
        return mu.to(positions.dtype), state

    @staticmethod
    def backward(ctx, g, _g_state):
        if torch.is_grad_enabled():
            raise NotImplementedError(f"{ctx.op.name}: second derivatives are not supported (the backward pass is itself a linear solve and is "
                                      "not recorded)")
        positions, charges, polar, mu = ctx.saved_tensors
        op, need = ctx.op, ctx.needs_input_grad
        if g is None:
            return (None,) * 10
        z, _ = _conjugate_gradients(op, (g.detach().to(F64) * op.mask).contiguous(), None, *ctx.solver, f"{op.name} (backward)")
        g_pos = g_q = g_polar = g_field = None
        if need[2]:
            a = polar.detach().to(F64)
            ok = a > 0
            g_polar = torch.where(ok, (z * mu).sum(1) / torch.where(ok, a * a, torch.ones_like(a)), torch.zeros_like(a)).to(polar.dtype)
        if need[3]:
            g_field = z.to(ctx.field_dtype)
        damped_polar = need[2] and op.thole is not None
        if need[0] or need[1] or damped_polar:
            with torch.enable_grad():
                leaves = [positions.detach().requires_grad_(need[0]), charges.detach().requires_grad_(need[1]),
                          polar.detach().requires_grad_(damped_polar)]
                if need[0] or need[1]:
                    energy = lambda d: _dipole_energy(op, leaves[0], leaves[1], d, ctx.lists, ctx.mask_value, leaves[2])  # noqa: E731
                else:  # the polarisabilities alone: only E_thole depends on them
                    energy = lambda d: _thole_energy(op, leaves[0], leaves[1], d, leaves[2], ctx.lists, ctx.mask_value)  # noqa: E731
                diff = energy(mu + z) - energy(mu - z)
                grads = list(torch.autograd.grad(-0.5 * diff, [t for t in leaves if t.requires_grad], allow_unused=True))
            if need[0]:
                g_pos = grads.pop(0)
            if need[1]:
                g_q = grads.pop(0)
            if damped_polar:
                g_polar = g_polar + grads.pop(0).to(polar.dtype)
        return g_pos, g_q, g_polar, g_field, None, None, None, None, None, None


def induced_dipoles(positions: torch.Tensor, charges: torch.Tensor, polarizability, cell: torch.Tensor, *,
                    external_field: torch.Tensor | None = None, batch_idx: torch.Tensor | None = None,
                    neighbor_list: torch.Tensor | None = None, neighbor_ptr: torch.Tensor | None = None,
                    neighbor_shifts: torch.Tensor | None = None, neighbor_matrix: torch.Tensor | None = None,
                    neighbor_matrix_shifts: torch.Tensor | None = None, mask_value: int | None = None, reciprocal: str = "pme", alpha=None,
                    mesh_dimensions: tuple[int, int, int] | None = None, mesh_spacing: float | None = None, spline_order: int = 5,
                    k_vectors: torch.Tensor | None = None, k_cutoff: float | None = None, accuracy: float = 1e-6, tolerance: float = 1e-8,
                    max_iterations: int = 200, check_interval: int = 4, initial_dipoles: torch.Tensor | None = None,
                    return_info: bool = False):
    """Induced point dipoles: the minimiser, per system, of

        U(mu) = sum_i |mu_i|^2 / (2 a_i) + E_dip(q, mu) - sum_i mu_i . F_i

    q = `charges` [N], a = `polarizability` ([N], or a number; isotropic), F = `external_field` [N, 3] (optional) and E_dip the charge-dipole
    and dipole-dipole energy of point dipoles as this package defines it: `ewald_dipole_real_space` + `pme_dipole_reciprocal_space`
    (reciprocal="pme") or `ewald_dipole_reciprocal_space` (reciprocal="ewald"), dipolar self term and tin-foil boundary included.  The result
    satisfies mu_i / a_i + dE_dip/dmu_i - F_i = 0: the `dipole_grads` of `pme_dipole_correction` / `ewald_dipole_correction` at the returned
    dipoles, plus mu / a - F, vanish.  The forces of a polarisable step are therefore `*_dipole_correction(compute_forces=True)` at the
    returned dipoles: stationarity means that no response term is needed.  An atom with a_i <= 0 (or NaN) is not polarisable: its dipole is
    exactly 0.  A cell is required: the dipole routines are periodic.

    THE LIST MUST BE FULL, with the conventions of `ewald_dipole_real_space`: matrix or CSR, single or batched; an entry equal to `mask_value`
    (default: N) or outside [0, N) is padding; entries with r <= 1e-8 are skipped.  The number of systems is the number of cells.
    `alpha=None` takes the estimate `pme_dipole_correction` / `ewald_dipole_correction` would take, as do the mesh (`mesh_dimensions` |
    `mesh_spacing`) and the k-vectors (`k_vectors` | `k_cutoff`).

    Solver: conjugate gradients with the Jacobi preconditioner diag(a), started from mu = a b (b = -dE_dip/dmu at mu = 0, plus F: the
    right-hand side) or from `initial_dipoles` (the warm start of an MD step).  The real-space operator is evaluated once
    (`mi_induced_pair_tensors`) and applied as a stored sparse operator of 3 x 3 blocks (`mi_induced_apply`); each iteration adds one
    reciprocal-space dipole-gradient call on the search direction.  A system is done when ||r_s|| <= tolerance ||b_s||; done systems are
    frozen; a system with b = 0 is done at iteration 0 with dipoles exactly 0.  The host looks at the done flags every `check_interval`
    iterations.  `InducedDipoleError` after `max_iterations`, and -- with another message -- when a search direction p with p.Hp <= 0 is
    met: H is then not positive definite, the polarisation catastrophe of undamped point dipoles (a polarisability of the order of the
    cube of the shortest distance).  All solver arithmetic is float64 and the solver's own kernels are free of atomics.  With
    reciprocal="ewald" nothing in the loop uses atomics (the explicit dipole sum is bit-reproducible): two identical calls, and a call on a
    side stream, give bit-identical dipoles.  With reciprocal="pme" the mesh spread adds with atomics in arrival order, so the dipoles of
    two identical calls agree to the tolerance, not to the bit.  With float32 positions the reciprocal-space calls return float32 gradients,
    which limits the attainable tolerance to about 1e-6.

    Returns `dipoles` [N, 3] in the positions dtype; with `return_info=True` a named tuple (dipoles, polarization_energy [num_systems] =
    -1/2 sum mu . b = U at the solution, iterations [num_systems], residual [num_systems] = ||r_s|| / ||b_s||).  `dipoles` is differentiable
    with respect to positions, charges, polarizability and external_field by implicit differentiation (one more solve with the same stored
    operator and two evaluations of the public energy functions; alpha, the mesh and the k-vectors are held fixed; the dipole functions
    have no cell adjoint, so `cell` is not differentiable).  Differentiating twice raises NotImplementedError, and so does tracing with
    torch.compile: the solve has a data-dependent trip count.  CPU tensors raise NativeLibraryError: there is no fallback.

    These are undamped point dipoles.  `thole_induced_dipoles` is the same solve with exponential Thole damping, which keeps H positive
    definite at the distances of bonded atoms.

    Out of scope: anisotropic polarisabilities, clusters without a cell, quadrupoles, a cell gradient, an extended-Lagrangian or predictor
    scheme.  A differently damped permanent field can be passed through `external_field` with zero charges; the field of permanent quadrupoles
    is minus the `dipole_grads` of `ewald_quadrupole_correction` (or, on the mesh, of `pme_quadrupole_correction`), passed the same way."""
    return _solve(None, positions, charges, polarizability, cell, external_field, batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts,
                  neighbor_matrix, neighbor_matrix_shifts, mask_value, reciprocal, alpha, mesh_dimensions, mesh_spacing, spline_order, k_vectors,
                  k_cutoff, accuracy, tolerance, max_iterations, check_interval, initial_dipoles, return_info)


def thole_induced_dipoles(positions: torch.Tensor, charges: torch.Tensor, polarizability, cell: torch.Tensor, *, thole: float | None = 0.39,
                          external_field: torch.Tensor | None = None, batch_idx: torch.Tensor | None = None,
                          neighbor_list: torch.Tensor | None = None, neighbor_ptr: torch.Tensor | None = None,
                          neighbor_shifts: torch.Tensor | None = None, neighbor_matrix: torch.Tensor | None = None,
                          neighbor_matrix_shifts: torch.Tensor | None = None, mask_value: int | None = None, reciprocal: str = "pme", alpha=None,
                          mesh_dimensions: tuple[int, int, int] | None = None, mesh_spacing: float | None = None, spline_order: int = 5,
                          k_vectors: torch.Tensor | None = None, k_cutoff: float | None = None, accuracy: float = 1e-6,
                          tolerance: float = 1e-8, max_iterations: int = 200, check_interval: int = 4,
                          initial_dipoles: torch.Tensor | None = None, return_info: bool = False):
    """`induced_dipoles` with exponential Thole damping of width `thole` (AMOEBA uses 0.39): every argument, convention, return value and
    error of `induced_dipoles`, with E_dip + `thole_dipole_correction` in the place of E_dip everywhere.  The stored operator holds B_n + D_n
    (`mi_thole_induced_pair_tensors`: same layout, same product and CG kernels), the right-hand side and the implicit gradients include the
    damped charge field, and dL/dpolarizability gains the derivative of E_thole.  The returned dipoles make
    `dipole_grads(*_dipole_correction) + dipole_grads(thole_dipole_correction) + mu / a - F` vanish.  With damping H stays positive definite
    at the distances of bonded atoms, where the undamped operator is not.  `thole=None` is `induced_dipoles` itself: the same launches and,
    with reciprocal="ewald", the same bits.  `thole` that is not finite or not positive raises ValueError before anything is launched.

    (`induced_dipoles` keeps its argument list as it is; the damped solve is this function of its own and not a keyword there.)

    Out of scope: per-pair Thole widths, the linear Thole form and AMOEBA's separate direct-field damping and polarisation groups, and what
    `induced_dipoles` leaves out."""
    return _solve(thole, positions, charges, polarizability, cell, external_field, batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts,
                  neighbor_matrix, neighbor_matrix_shifts, mask_value, reciprocal, alpha, mesh_dimensions, mesh_spacing, spline_order, k_vectors,
                  k_cutoff, accuracy, tolerance, max_iterations, check_interval, initial_dipoles, return_info)


def _empty_result(nsys, dt, dev, return_info):
    empty = torch.zeros((0, 3), dtype=dt, device=dev)
    zeros = torch.zeros(nsys, dtype=dt, device=dev)
    return InducedDipoleResult(empty, zeros, torch.zeros(nsys, dtype=torch.int64, device=dev), zeros.clone()) if return_info else empty


def _run(op: _Operator, positions, charges, polar, external_field, lists, mask_value, solver, initial_dipoles, return_info):
    """The solve on a built operator, with or without autograd, and its result: what every public solver function ends in."""
    dt = positions.dtype
    b = op.right_hand_side(charges, external_field, lists, mask_value)
    diff = torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in (positions, charges, polar, external_field))
    if diff:
        dipoles, state = _InducedDipoles.apply(positions, charges, polar, external_field, op, b, initial_dipoles, lists, mask_value, solver)
        mu64 = dipoles.detach().to(F64).contiguous()
    else:
        mu64, state = _conjugate_gradients(op, b, initial_dipoles, *solver, op.name)
        dipoles = mu64.to(dt)
    if not return_info:
        return dipoles
    iterations, residual = _info(state)
    return InducedDipoleResult(dipoles, (-0.5 * op.dot(mu64, b)).to(dt), iterations, residual.to(dt))


def _solve(thole, positions, charges, polarizability, cell, external_field, batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts,
           neighbor_matrix, neighbor_matrix_shifts, mask_value, reciprocal, alpha, mesh_dimensions, mesh_spacing, spline_order, k_vectors, k_cutoff,
           accuracy, tolerance, max_iterations, check_interval, initial_dipoles, return_info):
    """What `induced_dipoles` (thole None) and `thole_induced_dipoles` run."""
    if C.tracing():
        raise NotImplementedError("induced_dipoles cannot be traced by torch.compile: the solve iterates until a device-side convergence "
                                  "flag is set.  Call it outside the compiled region (torch.compiler.disable).")
    nsys = _check(positions, charges, polarizability, cell, external_field, batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix,
                  neighbor_matrix_shifts, reciprocal, alpha, mesh_dimensions, mesh_spacing, spline_order, k_vectors, k_cutoff, tolerance,
                  max_iterations, check_interval, initial_dipoles, thole)
    n, dev, dt = positions.shape[0], positions.device, positions.dtype
    if mask_value is None:
        mask_value = n
    per_atom_polar = isinstance(polarizability, torch.Tensor) and polarizability.dim() > 0
    if n == 0:
        return _empty_result(nsys, dt, dev, return_info)
    C.require_device(positions, charges, polarizability if per_atom_polar else None, cell, external_field, batch_idx, neighbor_list, neighbor_ptr,
                     neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts, k_vectors, initial_dipoles)
    with torch.cuda.device(dev):
        polar = (polarizability if per_atom_polar
                 else torch.full((n,), float(polarizability), dtype=dt, device=dev))
        lists = (neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts)
        op = _Operator(positions, polar, cell, batch_idx, nsys, lists, mask_value, reciprocal, alpha, mesh_dimensions, mesh_spacing, spline_order,
                       k_vectors, k_cutoff, accuracy, thole)
        return _run(op, positions, charges, polar, external_field, lists, int(mask_value),
                    (float(tolerance), int(max_iterations), int(check_interval)), initial_dipoles, return_info)


__all__ = ["induced_dipoles", "thole_induced_dipoles", "InducedDipoleError", "InducedDipoleResult"]
