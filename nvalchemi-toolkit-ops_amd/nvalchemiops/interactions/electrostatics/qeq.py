"""Charge equilibration: the charges that minimise, per system s,

    E(q) = sum_i chi_i q_i + 1/2 sum_i J_i q_i^2 + E_el(q)        subject to   sum_{i in s} q_i = Q_s

with E_el the Gaussian-charge electrostatic energy of this package: `ewald_real_space` + `pme_reciprocal_space` (or
`ewald_reciprocal_space`) + `gaussian_charge_correction` with a cell, erf(r / g_ij) / r pairs + Gaussian self-energies without one.
E_el = 1/2 q^T A q is a quadratic form, so the solution satisfies chi + H q = lambda_s on every atom of s, H = diag(J) + A.
The reference package has no counterpart.

The geometry does not change during a solve, so the real-space part of A is a constant sparse matrix over the caller's FULL neighbour list.
`mi_qeq_pair_coefficients` (csrc/qeq.hip) evaluates it once -- the only erfc / exp / sqrt of a solve -- and every matrix-vector product is
`mi_qeq_apply`, a sparse product over 12 bytes per list slot, plus one reciprocal-space call of the existing public functions on the
search direction.  The solver is conjugate gradients on P H P, P the projector that removes the per-system mean: directions stay in the
constraint subspace, where the rank-two neutralising-background pieces of A vanish and P H P is positive definite for J > 0.  All per-system
scalars live on the device (`mi_qeq_cg_update`, `mi_qeq_cg_direction`) and every sum of these kernels is a fixed-order fold: a solve without a
cell is bit-reproducible.  A periodic solve is not: the reciprocal-space calls it makes add with atomics in arrival order.
"""
from __future__ import annotations

import math
from collections import namedtuple

import torch

from nvalchemiops import _capi as C
from nvalchemiops.interactions.electrostatics import _pairs as P
from nvalchemiops.interactions.electrostatics import gaussian as G

F64 = torch.float64
ChargeEquilibrationResult = namedtuple("ChargeEquilibrationResult", ["charges", "chemical_potential", "iterations", "residual"])


class ChargeEquilibrationError(RuntimeError):
    """The conjugate-gradient solve did not reach `tolerance` within `max_iterations`."""


def _check(positions, electronegativity, hardness, sigma, cell, total_charge, batch_idx, num_systems, neighbor_list, neighbor_ptr, neighbor_shifts,
           neighbor_matrix, neighbor_matrix_shifts, reciprocal, alpha, mesh_dimensions, mesh_spacing, k_vectors, k_cutoff, tolerance,
           max_iterations, check_interval, initial_charges) -> int:
    """Every argument error, before anything is launched (`_pairs.check_lists` for the list, sigma and the cell-less rules).  Returns the number
    of systems: the cell count with a cell; otherwise `num_systems`, else the length of a `total_charge` tensor, else 1 -- never a host read
    of `batch_idx`."""
    n = positions.shape[0] if positions.dim() == 2 else -1
    if positions.dim() != 2 or positions.shape[1] != 3:
        raise ValueError(f"positions must have shape [num_atoms, 3], got {tuple(positions.shape)}")
    P.check_lists(positions, None, sigma, cell, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts, batch_idx, False)
    for name, t in (("electronegativity", electronegativity), ("hardness", hardness), ("initial_charges", initial_charges)):
        if t is not None:
            C.check_per_atom(n, **{name: t})
            if t.dim() != 1:
                raise ValueError(f"{name} must have one entry per atom: expected shape [{n}], got {tuple(t.shape)}")
    if reciprocal not in ("pme", "ewald"):
        raise ValueError(f"reciprocal must be 'pme' or 'ewald', got {reciprocal!r}")
    if cell is None:
        given = [k for k, v in (("alpha", alpha), ("mesh_dimensions", mesh_dimensions), ("mesh_spacing", mesh_spacing), ("k_vectors", k_vectors),
                                ("k_cutoff", k_cutoff)) if v is not None]
        if given:
            raise ValueError(f"{', '.join(given)} need a cell: without one there is no reciprocal-space part")
        if num_systems is not None:
            nsys = int(num_systems)
        elif isinstance(total_charge, torch.Tensor) and total_charge.dim() == 1:
            nsys = total_charge.shape[0]
        else:
            nsys = 1
        if nsys < 1:
            raise ValueError(f"num_systems must be at least 1, got {nsys}")
    else:
        nsys = cell.shape[0] if cell.dim() == 3 else 1
        C.check_neighbor_data(n, cell=cell, num_systems=num_systems, alpha=alpha)
        if reciprocal == "pme" and k_cutoff is not None:
            raise ValueError("k_cutoff belongs to reciprocal='ewald'")
        if reciprocal == "ewald" and (mesh_dimensions is not None or mesh_spacing is not None):
            raise ValueError("mesh_dimensions / mesh_spacing belong to reciprocal='pme'")
    if nsys > 1 and batch_idx is None:
        raise ValueError(f"batch_idx is required for {nsys} systems")
    if isinstance(total_charge, torch.Tensor):
        if total_charge.dim() > 1 or (total_charge.dim() == 1 and total_charge.shape[0] != nsys):
            raise ValueError(f"total_charge must be a number or have shape [{nsys}] (one per system), got {tuple(total_charge.shape)}")
    elif not isinstance(total_charge, (int, float)):
        raise TypeError(f"total_charge must be a number or torch.Tensor, got {type(total_charge)}")
    if not float(tolerance) > 0.0:
        raise ValueError(f"tolerance must be positive, got {tolerance}")
    if int(max_iterations) < 1:
        raise ValueError(f"max_iterations must be at least 1, got {max_iterations}")
    if int(check_interval) < 1:
        raise ValueError(f"check_interval must be at least 1, got {check_interval}")
    return nsys


class _Operator:
    """H = diag(J) + A of one geometry: the stored real-space coefficients, the reciprocal-space call and the background term."""

    def __init__(self, positions, hardness, sigma, cell, batch_idx, nsys, lists, mask_value, reciprocal, alpha, mesh_dimensions, mesh_spacing,
                 spline_order, k_vectors, k_cutoff, accuracy):
        neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts = lists
        dt, dev, n = positions.dtype, positions.device, positions.shape[0]
        self.n, self.nsys, self.dt, self.dev = n, nsys, dt, dev
        self.pos = positions.detach().contiguous()
        self.sigma = sigma.detach().to(dt).contiguous()
        self.bi = C.i32(batch_idx) if nsys > 1 else None
        self.batch_idx = batch_idx if nsys > 1 else None
        # atoms per system without a host read of batch_idx (bincount reads its maximum back); adding ones is exact in any order
        self.counts = (torch.zeros(nsys, dtype=F64, device=dev).index_add_(0, self.bi.long(), torch.ones(n, dtype=F64, device=dev))
                       if self.bi is not None else torch.full((1,), float(n), dtype=F64, device=dev))
        self.cells = None if cell is None else cell.detach().to(dt).reshape(-1, 3, 3).contiguous()
        self.reciprocal, self.spline_order = reciprocal, C.resolve_spline_order(spline_order)
        self.alpha = self.kv = self.dims = self.k_cutoff = None
        self.kv_given = False
        if self.cells is not None:
            self._reciprocal_parameters(alpha, mesh_dimensions, mesh_spacing, k_vectors, k_cutoff, accuracy)
        ls = P.list_inputs(neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts)
        self.idx, self.nptr, self.m, sh32, slots = ls["idx"], ls["nptr"], ls["m"], ls["sh"], ls["n_entries"]
        self.coef = torch.empty(slots, dtype=F64, device=dev)
        self.nbr = torch.empty(slots, dtype=torch.int32, device=dev)
        self.diag = torch.empty(n, dtype=F64, device=dev)
        self.blocks, self.words = int(C.lib().mi_qeq_blocks()), int(C.lib().mi_qeq_state_words())
        hard64 = hardness.detach().to(F64).contiguous()
        rc = C.lib().mi_qeq_pair_coefficients(C.ptr(self.pos), C.ptr(self.sigma), C.ptr(hard64), C.ptr(self.cells),
                                              C.ptr(self.alpha), C.ptr(self.bi if self.cells is not None else None), n, nsys, C.dtype_code(dt),
                                              C.ptr(self.idx), C.ptr(sh32), C.ptr(self.nptr), int(self.m),
                                              int(mask_value), C.ptr(self.coef), C.ptr(self.nbr), C.ptr(self.diag), C.stream_of(self.pos))
        C.check(rc, "mi_qeq_pair_coefficients")
        if self.cells is not None:  # background term of the correction: (2 pi / V_s) (sum_j x_j s_j + X_s s_i)
            sp = torch.clamp(self.sigma.to(F64), min=0.0)
            self.s, self.sigma64 = (sp * sp).contiguous(), self.sigma.to(F64).contiguous()
            self.pref = 2.0 * math.pi / torch.abs(torch.linalg.det(self.cells.to(F64)))

    def _reciprocal_parameters(self, alpha, mesh_dimensions, mesh_spacing, k_vectors, k_cutoff, accuracy):
        """alpha, and the mesh or the k-vectors, as `particle_mesh_ewald` / `ewald_summation` would choose them."""
        from nvalchemiops.interactions.electrostatics import ewald as EW, pme as PME
        from nvalchemiops.interactions.electrostatics.k_vectors import generate_k_vectors_ewald_summation
        from nvalchemiops.interactions.electrostatics.parameters import (estimate_ewald_parameters, estimate_pme_mesh_dimensions,
                                                                         estimate_pme_parameters, mesh_spacing_to_dimensions)

        cells, dt, dev = self.cells, self.dt, self.dev
        if self.reciprocal == "pme":
            if alpha is None:
                est = estimate_pme_parameters(self.pos, cells, self.batch_idx, accuracy)
                alpha = est.alpha
                if mesh_dimensions is None and mesh_spacing is None:
                    mesh_dimensions = tuple(est.mesh_dimensions)
            self.alpha = PME._prepare_alpha(alpha, self.nsys, dt, dev).detach().to(dt).contiguous()
            if mesh_dimensions is None:
                mesh_dimensions = (mesh_spacing_to_dimensions(cells, mesh_spacing) if mesh_spacing is not None
                                   else estimate_pme_mesh_dimensions(cells, self.alpha, accuracy))
            self.dims = tuple(int(v) for v in mesh_dimensions)
        else:
            if alpha is None or (k_cutoff is None and k_vectors is None):
                params = estimate_ewald_parameters(self.pos, cells, self.batch_idx, accuracy)
                alpha = params.alpha if alpha is None else alpha
                k_cutoff = params.reciprocal_space_cutoff if k_cutoff is None else k_cutoff
            self.alpha = EW._prepare_alpha(alpha, self.nsys, dt, dev).detach().contiguous()
            self.k_cutoff, self.kv_given = k_cutoff, k_vectors is not None
            self.kv = (k_vectors if k_vectors is not None else generate_k_vectors_ewald_summation(cells, k_cutoff)).detach()

    def reciprocal_gradient(self, x):
        """float64 dE_recip/dq at the charges x (linear in x): one call of the public reciprocal-space function."""
        from nvalchemiops.interactions.electrostatics import ewald as EW, pme as PME

        with torch.no_grad():
            xq = x.to(self.dt)
            if self.reciprocal == "pme":
                cg = PME.pme_reciprocal_space(self.pos, xq, self.cells, self.alpha, mesh_dimensions=self.dims, spline_order=self.spline_order,
                                              batch_idx=self.batch_idx, compute_charge_gradients=True)[1]
            else:
                cg = EW.ewald_reciprocal_space(self.pos, xq, self.cells, self.kv, self.alpha, batch_idx=self.batch_idx,
                                               compute_charge_gradients=True)[1]
        return cg.to(F64)

    def background_gradient(self, x):
        """float64 (2 pi / V_s)(sum_j x_j s_j + X_s s_i): dE/dq of the correction's neutralising background (fixed-order sums)."""
        xsum, xssum, _ = G._system_sums(dict(q=x, sigma=self.sigma64, bi=self.bi, nsys=self.nsys))
        at = (lambda v: v[self.bi.long()]) if self.bi is not None else (lambda v: v)
        return at(self.pref * xssum) + at(self.pref * xsum) * self.s

    def long_range(self, x, projected: bool):
        """Everything of H x that is not in the stored coefficients, or None without a cell.  For a direction of zero total charge
        (`projected`) the background term is constant per system and the projection removes it: it is not evaluated."""
        if self.cells is None:
            return None
        y = self.reciprocal_gradient(x)
        return y if projected else y + self.background_gradient(x)

    def apply(self, x, y_in=None, partial=None):
        """y = y_in + diag x + A_real x (`mi_qeq_apply`), and the per-system block partials of {sum y, x.y} when asked for."""
        y = torch.empty(self.n, dtype=F64, device=self.dev)
        rc = C.lib().mi_qeq_apply(C.ptr(self.coef), C.ptr(self.nbr), C.ptr(self.diag), C.ptr(x), C.ptr(y_in), C.ptr(self.bi), self.n, self.nsys,
                                  C.ptr(self.nptr), int(self.m), C.ptr(y), C.ptr(partial), C.stream_of(x))
        C.check(rc, "mi_qeq_apply")
        return y

    def full(self, x, add=None, partial=None):
        """H x (+ add) with every term of the public energies, for any x."""
        lr = self.long_range(x, projected=False)
        y_in = lr if add is None else (add if lr is None else lr + add)
        return self.apply(x, None if y_in is None else y_in.contiguous(), partial)

    def system_sums(self, v):
        """float64 [nsys] per-system sums of a float64 per-atom vector, in the fixed order of the product kernel's fold."""
        part = torch.empty((self.nsys, self.blocks, 2), dtype=F64, device=self.dev)
        zeros, y = torch.zeros(self.n, dtype=F64, device=self.dev), torch.empty(self.n, dtype=F64, device=self.dev)
        rc = C.lib().mi_qeq_apply(None, None, C.ptr(self.diag), C.ptr(zeros), C.ptr(v), C.ptr(self.bi), self.n, self.nsys, None, 0, C.ptr(y),
                                  C.ptr(part), C.stream_of(v))
        C.check(rc, "mi_qeq_apply")
        return part.sum(1)[:, 0]

    def per_atom(self, v):
        return v[self.bi.long()] if self.bi is not None else v.expand(self.n)


def _conjugate_gradients(op: _Operator, starts, tolerance, max_iterations, check_interval, what):
    """Projected CG on P H P.  `starts` is a list of (x, g): g = (right-hand side negated) + H x, i.e. the gradient at x; the LAST entry is
    where the iteration starts (its x is updated in place and returned), the first one defines the norm ||b|| the tolerance refers to.  A later
    entry may be a function of the per-system b.b of the first (a device tensor) that returns its (x, g).
    Returns (x, state [nsys, words]).  The host reads the `done` flags once every `check_interval` iterations and at no other time."""
    L, n, nsys, dev = C.lib(), op.n, op.nsys, op.dev
    f64 = dict(dtype=F64, device=dev)
    state = [torch.zeros((nsys, op.words), **f64), torch.zeros((nsys, op.words), **f64)]
    part_y, part_rr = torch.empty((nsys, op.blocks, 2), **f64), torch.empty((nsys, op.blocks), **f64)
    r, p = torch.empty(n, **f64), torch.empty(n, **f64)
    stream = C.stream_of(r)

    def update(y, mode, x):
        C.check(L.mi_qeq_cg_update(C.ptr(y), C.ptr(part_y), C.ptr(op.counts), C.ptr(op.bi), n, nsys, mode, C.ptr(x), C.ptr(r), C.ptr(p),
                                   C.ptr(state[0]), C.ptr(state[1]), C.ptr(part_rr), stream), "mi_qeq_cg_update")

    def direction(mode):
        C.check(L.mi_qeq_cg_direction(C.ptr(part_rr), C.ptr(op.bi), n, nsys, mode, C.cdouble(tolerance), C.ptr(r), C.ptr(p), C.ptr(state[1]),
                                      C.ptr(state[0]), stream), "mi_qeq_cg_direction")

    x, zeros = None, torch.zeros(n, **f64)
    for k, start in enumerate(starts):
        x, g = start(state[0][:, 1]) if callable(start) else start
        # the partials of g through the product kernel's fold: y = g + 0
        C.check(L.mi_qeq_apply(None, None, C.ptr(op.diag), C.ptr(zeros), C.ptr(g), C.ptr(op.bi), n, nsys, None, 0, C.ptr(g),
                               C.ptr(part_y), stream), "mi_qeq_apply")
        update(g, 1, x)
        direction(1 if k == 0 else 2)
    converged = False
    for it in range(1, int(max_iterations) + 1):
        y = op.apply(p, op.long_range(p, projected=True), part_y)
        update(y, 0, x)
        direction(0)
        if it % int(check_interval) == 0 or it == int(max_iterations):
            converged = bool((state[0][:, 2] != 0).all())  # the one host read
            if converged:
                break
    if not converged:
        st = state[0].cpu()
        res = torch.sqrt(st[:, 0] / st[:, 1])
        bad = [(s, float(res[s])) for s in range(nsys) if st[s, 2] == 0]
        raise ChargeEquilibrationError(
            f"{what}: no convergence to tolerance {tolerance:g} within {int(max_iterations)} iterations for "
            + ", ".join(f"system {s} (residual {v:.3e})" for s, v in bad[:16]) + (f" and {len(bad) - 16} more" if len(bad) > 16 else ""))
    return x, state[0]


def _info(state):
    """(iterations int64 [nsys], relative residual ||r|| / ||b|| float64 [nsys]) from the solver state, on the device."""
    rr, bb = state[:, 0], state[:, 1]
    return state[:, 3].to(torch.int64), torch.where(bb > 0, torch.sqrt(rr / torch.where(bb > 0, bb, torch.ones_like(bb))), torch.zeros_like(rr))


def _solve(op: _Operator, chi, total, initial, tolerance, max_iterations, check_interval):
    """(q float64 [N], state): q0 = Q_s / N_s, or `initial` shifted per system onto the constraint; ||b|| is that of the uniform start in
    both cases, so `tolerance` means the same for a warm start."""
    uniform = op.per_atom(total / torch.clamp(op.counts, min=1.0)).contiguous()
    starts = [(uniform, op.full(uniform, add=chi))]
    if initial is not None:
        q0 = initial.detach().to(F64).contiguous()
        q0 = q0 + op.per_atom((total - op.system_sums(q0)) / torch.clamp(op.counts, min=1.0))

        def warm(bb):
            # a system whose uniform start has b = 0 exactly is solved by that start: it keeps it (it is done at once, whatever it is handed)
            x = torch.where(op.per_atom(bb) > 0, q0, uniform).contiguous()
            return x, op.full(x, add=chi)

        starts.append(warm)
    return _conjugate_gradients(op, starts, tolerance, max_iterations, check_interval, "charge_equilibration")


def _electrostatic_energy(op: _Operator, positions, charges, sigma, cell, lists, mask_value):
    """Total E_el(charges) from the differentiable public functions (the backward's d(z^T A q)/d(positions, sigma, cell))."""
    from nvalchemiops.interactions.electrostatics import coulomb as CO, ewald as EW, pme as PME
    from nvalchemiops.interactions.electrostatics.k_vectors import generate_k_vectors_ewald_summation

    neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts = lists
    kw = dict(neighbor_list=neighbor_list, neighbor_ptr=neighbor_ptr, neighbor_shifts=neighbor_shifts, neighbor_matrix=neighbor_matrix,
              neighbor_matrix_shifts=neighbor_matrix_shifts)
    q = charges.to(positions.dtype)
    e = G.gaussian_charge_correction(positions, q, sigma, cell, mask_value=mask_value, batch_idx=op.batch_idx, **kw).sum()
    if cell is None:
        # point-charge part: `coulomb_energy` without cutoff or damping on a unit cell with zero shifts.  It counts padding as j >= fill_value,
        # so padding is rewritten to N; its matrix form carries the prefactor 1 where the list form carries 1/2.
        n, dev = op.n, op.dev
        unit = torch.eye(3, dtype=F64, device=dev).reshape(1, 3, 3)
        if neighbor_list is not None:
            zeros = torch.zeros((neighbor_list.shape[1], 3), dtype=torch.int32, device=dev)
            # entries outside [0, N) are padding for the solve; here they become the row's own index, a pair at distance 0 that is skipped
            row, col = neighbor_list[0], neighbor_list[1]
            neighbor_list = torch.stack([row, torch.where((col < 0) | (col >= n), row, col)])
            return e + CO.coulomb_energy(positions.to(F64), q.to(F64), unit, 1e300, 0.0, neighbor_list=neighbor_list, neighbor_ptr=neighbor_ptr,
                                         neighbor_shifts=zeros).sum()
        nm = neighbor_matrix.to(torch.int32)
        nm = torch.where((nm == int(mask_value)) | (nm < 0) | (nm >= n), torch.full_like(nm, n), nm)
        zeros = torch.zeros(tuple(nm.shape) + (3,), dtype=torch.int32, device=dev)
        return e + 0.5 * CO.coulomb_energy(positions.to(F64), q.to(F64), unit, 1e300, 0.0, neighbor_matrix=nm, neighbor_matrix_shifts=zeros,
                                           fill_value=n).sum()
    cells = cell.reshape(-1, 3, 3)
    if op.reciprocal == "pme":
        return e + PME.particle_mesh_ewald(positions, q, cells, alpha=op.alpha, mesh_dimensions=op.dims, spline_order=op.spline_order,
                                           batch_idx=op.batch_idx, mask_value=mask_value, **kw).sum()
    kv = op.kv if op.kv_given else generate_k_vectors_ewald_summation(cells, op.k_cutoff)
    return (e + EW.ewald_real_space(positions, q, cells, op.alpha, mask_value=mask_value, batch_idx=op.batch_idx, **kw).sum()
            + EW.ewald_reciprocal_space(positions, q, cells, kv, op.alpha, batch_idx=op.batch_idx).sum())


class _ChargeEquilibration(torch.autograd.Function):
    """The solve under autograd: implicit differentiation of the stationarity conditions, no new kernels.  With g = dL/dq and
    z = (P H P)^+ P g (one more solve with the stored operator):  dL/dchi = -z,  dL/dJ = -z q,  dL/dQ_s = mean_s(g - H z), and for
    theta in {positions, sigma, cell}  dL/dtheta = -d(z^T A q)/dtheta  with  z^T A q = 1/2 [E_el(q + z) - E_el(q - z)]."""

    @staticmethod
    def forward(ctx, positions, chi, hardness, sigma, cell, total, op, initial, lists, mask_value, solver):
        q, state = _solve(op, chi.detach().to(F64).contiguous(), total.detach().to(F64), initial, *solver)
        ctx.save_for_backward(positions, chi, hardness, sigma, total, q, *(() if cell is None else (cell,)))
        ctx.op, ctx.lists, ctx.mask_value, ctx.solver, ctx.periodic = op, lists, mask_value, solver, cell is not None
        out = q.to(positions.dtype)
        state = state.clone()
        ctx.mark_non_differentiable(state)
        return out, state

    @staticmethod
    def backward(ctx, g, _g_state):
        if torch.is_grad_enabled():
            raise NotImplementedError("charge_equilibration: second derivatives are not supported (the backward pass is itself a linear solve "
                                      "and is not recorded)")
        positions, chi, hardness, sigma, total, q = ctx.saved_tensors[:6]
        cell = ctx.saved_tensors[6] if ctx.periodic else None
        op, need = ctx.op, ctx.needs_input_grad
        if g is None:
            return (None,) * 11
        g64 = g.detach().to(F64).contiguous()
        z, _ = _conjugate_gradients(op, [(torch.zeros(op.n, dtype=F64, device=op.dev), (-g64).contiguous())], *ctx.solver,
                                    "charge_equilibration (backward)")
        g_pos = g_chi = g_j = g_sigma = g_cell = g_total = None
        if need[1]:
            g_chi = (-z).to(chi.dtype)
        if need[2]:
            g_j = (-z * q).to(hardness.dtype)
        if need[5]:
            part = torch.empty((op.nsys, op.blocks, 2), dtype=F64, device=op.dev)
            op.full(z, add=-g64, partial=part)  # y = H z - g
            per_system = -part.sum(1)[:, 0] / torch.clamp(op.counts, min=1.0)
            g_total = per_system.to(total.dtype)
        if need[0] or need[3] or (need[4] and cell is not None):
            with torch.enable_grad():
                leaves = [positions.detach().requires_grad_(need[0]), sigma.detach().requires_grad_(need[3]),
                          None if cell is None else cell.detach().requires_grad_(need[4])]
                diff = (_electrostatic_energy(op, leaves[0], q + z, leaves[1], leaves[2], ctx.lists, ctx.mask_value)
                        - _electrostatic_energy(op, leaves[0], q - z, leaves[1], leaves[2], ctx.lists, ctx.mask_value))
                wanted = [t for t in leaves if t is not None and t.requires_grad]
                grads = list(torch.autograd.grad(-0.5 * diff, wanted, allow_unused=True))
            if need[0]:
                g_pos = grads.pop(0)
            if need[3]:
                g_sigma = grads.pop(0)
            if need[4] and cell is not None:
                g_cell = grads.pop(0)
                g_cell = None if g_cell is None else g_cell.reshape(cell.shape)
        return g_pos, g_chi, g_j, g_sigma, g_cell, g_total, None, None, None, None, None


def charge_equilibration(positions: torch.Tensor, electronegativity: torch.Tensor, hardness: torch.Tensor, sigma, cell: torch.Tensor | None = None, *,
                         total_charge=0.0, batch_idx: torch.Tensor | None = None, num_systems: int | None = None,
                         neighbor_list: torch.Tensor | None = None, neighbor_ptr: torch.Tensor | None = None,
                         neighbor_shifts: torch.Tensor | None = None, neighbor_matrix: torch.Tensor | None = None,
                         neighbor_matrix_shifts: torch.Tensor | None = None, mask_value: int = -1, reciprocal: str = "pme", alpha=None,
                         mesh_dimensions: tuple[int, int, int] | None = None, mesh_spacing: float | None = None, spline_order: int = 4,
                         k_vectors: torch.Tensor | None = None, k_cutoff: float | None = None, accuracy: float = 1e-6, tolerance: float = 1e-8,
                         max_iterations: int = 200, check_interval: int = 4, initial_charges: torch.Tensor | None = None,
                         return_info: bool = False):
    """Equilibrated charges: the minimiser, per system s, of

        E(q) = sum_i chi_i q_i + 1/2 sum_i J_i q_i^2 + E_el(q)      subject to   sum_{i in s} q_i = Q_s

    chi = `electronegativity` [N], J = `hardness` [N] (> 0), Q = `total_charge` (a number, or a [num_systems] tensor), and E_el the energy of
    Gaussian charge clouds of width `sigma` ([N], or a number; sigma_i <= 0 is a point charge) as this package defines it:

      with a cell     `ewald_real_space` + `pme_reciprocal_space` (reciprocal="pme") or `ewald_reciprocal_space` (reciprocal="ewald"), self and
                      background terms included, + `gaussian_charge_correction` (pair, self and neutralising-background terms);
      cell=None       1/2 sum_entries q_i q_j erf(r / g_ij) / r + sum_i q_i^2 / (2 sqrt(pi) sigma_i); no shifts and no reciprocal arguments.

    E_el = 1/2 q^T A q, so the result satisfies chi_i + J_i q_i + (A q)_i = lambda_s on every atom of s: the dE/dq of the public energy
    functions at the returned charges, plus chi + J q, is constant per system.

    THE LIST MUST BE FULL, with the conventions of `gaussian_charge_correction`: matrix or CSR, single or batched; an entry equal to
    `mask_value` or outside [0, N) is padding; entries with r <= 1e-8 are skipped, the smearing of an entry is dropped for r / g_ij >= 6.
    The number of systems is the number of cells; without a cell it is `num_systems`, else the length of a `total_charge` tensor, else 1
    (never read from `batch_idx`).  `alpha=None` takes the estimate `particle_mesh_ewald` / `ewald_summation` would take, as do the mesh
    (`mesh_dimensions` | `mesh_spacing`) and the k-vectors (`k_vectors` | `k_cutoff`).

    Solver: conjugate gradients on the operator projected onto sum q = Q_s, started from q = Q_s / N_s or from `initial_charges` shifted
    onto the constraint (the warm start of an MD step).  The real-space operator is evaluated once (`mi_qeq_pair_coefficients`) and applied
    as a stored sparse matrix (`mi_qeq_apply`); each iteration adds one reciprocal-space call on the search direction.  A system is done
    when ||r_s|| <= tolerance ||b_s||, b the right-hand side of the uniform start; done systems are frozen.  The host looks at the done
    flags every `check_interval` iterations.  `ChargeEquilibrationError` after `max_iterations`.  All solver arithmetic is float64 and the
    solver's own kernels are free of atomics: with `cell=None` two identical calls give bit-identical charges.  With a cell the
    reciprocal-space calls add with atomics in arrival order, so charges of two identical calls agree to the tolerance, not to the bit.
    The criterion is relative: where b itself is rounding noise -- identical atoms on a perfect lattice with Q != 0, whose uniform start
    already is the solution -- it cannot be met and the call raises; perturb such an input or treat the uniform charges as the answer.
    A system with b = 0 exactly returns the uniform start, with or without `initial_charges`.  (With float32 positions the reciprocal-space calls return float32
    gradients, which limits the attainable tolerance to about 1e-6.)

    Returns `charges` [N] in the positions dtype; with `return_info=True` a named tuple (charges, chemical_potential [num_systems] = lambda_s,
    iterations [num_systems], residual [num_systems] = ||r_s|| / ||b_s||).  `charges` is differentiable with respect to electronegativity,
    hardness, total_charge, positions, sigma and cell by implicit differentiation (one more solve with the same stored operator and two
    evaluations of the public energy functions; alpha, the mesh and user-supplied k-vectors are held fixed).  Differentiating twice raises
    NotImplementedError, and so does tracing with torch.compile: the solve has a data-dependent trip count.  CPU tensors raise
    NativeLibraryError: there is no fallback."""
    if C.tracing():
        raise NotImplementedError("charge_equilibration cannot be traced by torch.compile: the solve iterates until a device-side convergence "
                                  "flag is set.  Call it outside the compiled region (torch.compiler.disable).")
    nsys = _check(positions, electronegativity, hardness, sigma, cell, total_charge, batch_idx, num_systems, neighbor_list, neighbor_ptr,
                  neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts, reciprocal, alpha, mesh_dimensions, mesh_spacing, k_vectors, k_cutoff,
                  tolerance, max_iterations, check_interval, initial_charges)
    n, dev, dt = positions.shape[0], positions.device, positions.dtype
    tensors = (positions, electronegativity, hardness, sigma if isinstance(sigma, torch.Tensor) and sigma.dim() > 0 else None, cell, batch_idx,
               neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts, k_vectors, initial_charges,
               total_charge if isinstance(total_charge, torch.Tensor) and total_charge.dim() > 0 else None)
    if n == 0:
        empty = torch.zeros(0, dtype=dt, device=dev)
        zeros = torch.zeros(nsys, dtype=dt, device=dev)
        return ChargeEquilibrationResult(empty, zeros, torch.zeros(nsys, dtype=torch.int64, device=dev), zeros.clone()) if return_info else empty
    C.require_device(*tensors)
    dev_guard = torch.cuda.device(dev)
    with dev_guard:
        sig = G._sigma_tensor(sigma, n, dt, dev)
        total = (total_charge.to(device=dev) if isinstance(total_charge, torch.Tensor) else torch.tensor(float(total_charge), device=dev, dtype=F64))
        total_n = total.detach().to(F64).expand(nsys) if total.dim() == 0 else total
        lists = (neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts)
        op = _Operator(positions, hardness, sig, cell, batch_idx, nsys, lists, mask_value, reciprocal, alpha, mesh_dimensions, mesh_spacing,
                       spline_order, k_vectors, k_cutoff, accuracy)
        solver = (float(tolerance), int(max_iterations), int(check_interval))
        diff = torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad
                                               for t in (positions, electronegativity, hardness, sig, cell, total))
        if diff:
            total_in = total if total.dim() == 1 else total.expand(nsys)
            charges, state = _ChargeEquilibration.apply(positions, electronegativity, hardness, sig, cell, total_in, op, initial_charges, lists,
                                                        int(mask_value), solver)
            q64 = charges.detach().to(F64)
        else:
            q64, state = _solve(op, electronegativity.detach().to(F64).contiguous(), total_n.detach().to(F64), initial_charges, *solver)
            charges = q64.to(dt)
        if not return_info:
            return charges
        part = torch.empty((nsys, op.blocks, 2), dtype=F64, device=dev)
        op.full(q64.contiguous(), add=electronegativity.detach().to(F64), partial=part)  # chi + H q: its per-system mean is lambda_s
        lam = part.sum(1)[:, 0] / torch.clamp(op.counts, min=1.0)
        iterations, residual = _info(state)
        return ChargeEquilibrationResult(charges, lam.to(dt), iterations, residual.to(dt))


__all__ = ["charge_equilibration", "ChargeEquilibrationError", "ChargeEquilibrationResult"]
