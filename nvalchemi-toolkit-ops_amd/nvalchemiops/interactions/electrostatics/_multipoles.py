"""The call layer the nine point-multipole operator halves (the explicit and mesh Ewald sums of point dipoles and quadrupoles, Thole damping,
the bare cluster sums) and their four composites share above `_pairs.py`, each piece once: the output tuples, the pair-sum
skeleton, the mesh skeleton, the composite bodies and the dispatch tail.  Plain functions on tuples and dicts: TorchDynamo inlines them where
a public function is traced, and the eager path pays a call, not an object, per piece.  What an operator keeps to itself -- its signature and
docstring, its device check, its ABI calls, its self-term and virial epilogues, its error messages -- stays in its module.

An operator is described by `grads`, the per-atom shapes of its gradient outputs after the forces: its outputs are (energies [n], forces
[n, 3], one gradient per shape, virial [nsys, 3, 3]), `want` is one truth value per output (the energies' is True), and the adjoint returns
the float64 gradient of the positions followed by one per shape.  Every buffer comes from `torch.empty` looked up on the module at call time.
"""
from __future__ import annotations

import ctypes

import torch

from nvalchemiops import _capi as C
from nvalchemiops.interactions.electrostatics import _pairs as P
from nvalchemiops.interactions.electrostatics import pme as _pme
from nvalchemiops.interactions.electrostatics.pme import _prepare_alpha, _prepare_cell

# per-atom shapes of the gradient outputs after the forces: always the charges' () and the dipoles' (3,), then the operator's fourth, if any
DIPOLE, QUADRUPOLE, THOLE = ((), (3,)), ((), (3,), (3, 3)), ((), (3,), ())
_ONE_FORMAT = "pass the list in ONE format: neighbor_list (with neighbor_ptr) or neighbor_matrix, not both"


# ---- outputs --------------------------------------------------------------------------------------------------------------------------------
# (the at most three gradients are indexed out, not looped over: these run on every eager call of a host-bound operator)
def allocate(pos, grads, want):
    """Float64 (energies, charge sums, dipole sums[, the fourth gradient's sums]) and the forces in the positions dtype, in output order; None
    for what `want` = (energies, forces, one per gradient) does not ask for."""
    n, dev = pos.shape[0], pos.device
    f64 = dict(dtype=torch.float64, device=dev)
    e = torch.empty(n, **f64) if want[0] else None
    f = torch.empty((n, 3), dtype=pos.dtype, device=dev) if want[1] else None
    cg = torch.empty(n, **f64) if want[2] else None
    dg = torch.empty((n, 3), **f64) if want[3] else None
    if len(grads) == 2:
        return e, f, cg, dg
    return e, f, cg, dg, torch.empty((n,) + grads[2], **f64) if want[4] else None


def pair_scratch(p, flags: int, blocks: int, nbytes: int):
    """(virial block partials [nsys, blocks, 9] | None, scratch bytes) of a pair-sum launch."""
    dev = p["pos"].device
    part = torch.empty((p["nsys"], blocks, 9), dtype=torch.float64, device=dev) if flags & P.VIRIAL else None
    return part, torch.empty(nbytes, dtype=torch.uint8, device=dev)


def if_wanted(res, want):
    return tuple(r if w else None for r, w in zip(res, want))


def finish(sums, virial, want, dt):
    """The outputs in dtype `dt`, None for what was not asked for: `sums` as `allocate` returned them (anything after them is not read),
    `virial` float64 [nsys, 3, 3] | None."""
    cg, dg, vir = sums[2].to(dt) if want[2] else None, sums[3].to(dt) if want[3] else None, virial.to(dt) if want[-1] else None
    if len(want) == 5:
        return sums[0].to(dt), sums[1], cg, dg, vir
    return sums[0].to(dt), sums[1], cg, dg, sums[4].to(dt) if want[4] else None, vir


def zero_gradients(n, dev, grads):
    """The adjoint of a call that launches nothing: float64 zeros for the positions and every gradient."""
    return tuple(torch.zeros((n,) + s, dtype=torch.float64, device=dev) for s in ((3,),) + grads)


def weights_of(grad_energies):
    return grad_energies.detach().to(torch.float64).contiguous()


def add_halves(rs, rec):
    if isinstance(rs, tuple):
        return tuple(a + b for a, b in zip(rs, rec))
    return rs + rec


# ---- pair sums over a full list: `launch(p, flags, weights=None, energies=True)` makes the operator's one ABI call ---------------------------------
def pair_forward(p, launch, grads, want):
    """The outputs of a pair sum in the positions dtype, no autograd graph: what the eager call and the `alchemiops::` op both run."""
    pos = p["pos"]
    n, dt = pos.shape[0], pos.dtype
    if n == 0 or p["n_entries"] == 0:
        return if_wanted(P.zeros(n, p["nsys"], dt, pos.device, *grads), want)
    sums = launch(p, P.flag_bits(want))  # (..., virial block partials | None)
    return finish(sums, C.fold_virial9(sums[-1]) if want[-1] else None, want, dt)


def pair_adjoint(p, launch, grads, grad_energies):
    """Float64 gradients of L = sum_i g_i E_i w.r.t. the positions and every differentiable input: the forward kernel with weights."""
    pos = p["pos"]
    n = pos.shape[0]
    if n == 0 or p["n_entries"] == 0:
        return zero_gradients(n, pos.device, grads)
    every = P.FORCES | P.CHARGE_GRAD | P.THIRD_GRAD | (P.FOURTH_GRAD if len(grads) == 3 else 0)
    sums = launch(p, every, weights=weights_of(grad_energies), energies=False)
    return (-sums[1].to(torch.float64),) + sums[2:-1]


def check_positions_and_format(positions, neighbor_list, neighbor_matrix):
    if positions.dim() != 2 or positions.shape[1] != 3:
        raise ValueError(f"positions must have shape [num_atoms, 3], got {tuple(positions.shape)}")
    if neighbor_list is not None and neighbor_matrix is not None:
        raise ValueError(_ONE_FORMAT)


def check_optional_cell_lists(positions, charges, dipoles, cell, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix,
                              neighbor_matrix_shifts, batch_idx, compute_virial):
    """`_pairs.check_dipole_lists` with a cell, the cell-less rules of `_pairs.check_lists` without one."""
    if cell is None:
        P.check_lists(positions, charges, 0.0, None, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts, batch_idx,
                      compute_virial)
        P.check_dipoles(positions, dipoles)
    else:
        P.check_dipole_lists(positions, charges, dipoles, cell, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts,
                             batch_idx, None, compute_virial)


def num_systems(cell, batch_idx) -> int:
    """`_pairs.num_systems` where the cell is optional (clusters)."""
    return cell.reshape(-1, 3, 3).shape[0] if (cell is not None and batch_idx is not None) else 1


# ---- dispatch tail ----------------------------------------------------------------------------------------------------------------------------
def dispatch(op, forward, multipoles, no_adjoint, rest, want):
    """Through the `_eops` op named `op` under torch.compile or when autograd has to record the call, else straight to `forward`; then the
    outputs that were asked for.  The arguments of both are `multipoles` (positions, charges, dipoles, ...: the differentiable inputs),
    `no_adjoint` (cell, alpha, k-vectors: tensors whose gradient the op refuses) and `rest` (index tensors and plain scalars, which cannot
    require a gradient and are not looked at), then one flag per output."""
    flags = tuple(bool(w) for w in want[1:])
    if P.needs_op(*multipoles, *no_adjoint):
        from nvalchemiops import _eops

        dt = multipoles[0].dtype
        res = getattr(_eops, op)(multipoles[0], *[t.to(dt) for t in multipoles[1:]], *no_adjoint, *rest, *flags)
    else:
        res = forward(*multipoles, *no_adjoint, *rest, *flags)
    return P.select(res, want)


def no_atoms(positions, nsys, grads, want):
    return P.select(P.zeros(0, nsys, positions.dtype, positions.device, *grads), want)


# ---- mesh -------------------------------------------------------------------------------------------------------------------------------------
# An operator on the mesh is a dict: grads, flags (the compute_* keywords of its public functions), check_order (its `_check_order`), spread /
# gather / virial (its launches and its virial epilogue), forward (its `_recip_forward`), op (the `_eops` name), real / recip (the public
# halves of its composite).  The explicit composites need grads, flags, real and recip only.
def check_order(spline_order, allowed, what, why) -> int:
    """The plain spline order, if it is one of `allowed`; `what` ("dipole") and `why` word the operator's errors."""
    order = C.plain_spline_order(spline_order)
    if order not in allowed:
        orders = ", ".join(str(o) for o in allowed[:-1]) + f" or {allowed[-1]}"
        raise ValueError(f"spline_order must be {orders} for the {what} mesh sum ({why}), got {order}")
    if int(spline_order) & C.SPLINE_REFERENCE_ORDERS or (not int(spline_order) & C.SPLINE_RESOLVED and not C.tracing()
                                                          and C.reference_spline_orders_active()):
        raise ValueError(f"the {what} mesh sum has no reference evaluation of the spline orders (reference_spline_orders): the reference package "
                         f"has no {what} term")
    return order


def mesh_dims(cells, mesh_dimensions, mesh_spacing, order):
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


def mesh_inputs(positions, charges, dipoles, cells, alpha, batch_idx, quadrupoles=None):
    """Detached contiguous launch tensors in the positions dtype plus the cell geometry (cell^-T, 2 pi cell^-1, volume) of `mi_pme_prepare`."""
    dt, dev, n = positions.dtype, positions.device, positions.shape[0]
    C.require_device(quadrupoles)
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
    if quadrupoles is not None:
        p["qd"] = quadrupoles.detach().to(dt).contiguous()
    return p


def mesh_spread(p, dims, order, launch, wide: bool, weights=None):
    """[2 | 4, nsys, nx, ny, nz]: the operator's two meshes (and their g-weighted twins), zero-filled by the entry point `launch` calls."""
    pos = p["pos"]
    if pos.dtype == torch.float32 and wide:
        # float32 atomic adds in arrival order move the last bits of the meshes from run to run, and the Hessian sums of the gather carry
        # that into the forces at 1e-6 of their largest component.  Added in float64 and rounded once, the float32 meshes are the same
        # in every run (but for a sum that lands on a rounding boundary of float32).
        up = {k: p[k].to(torch.float64) for k in ("pos", "q", "mu", "qd", "cit") if k in p}
        return mesh_spread(dict(p, code=C.dtype_code(torch.float64), **up), dims, order, launch, wide, weights).to(torch.float32)
    meshes = torch.empty((4 if weights is not None else 2, p["nsys"]) + dims, dtype=pos.dtype, device=pos.device)
    launch(p, dims, order, weights, meshes)
    return meshes


def per_atom(p, values):
    """One value per system -> one per atom."""
    return values[p["bi"].long()] if p["bi"] is not None else values.expand(p["pos"].shape[0])


def strained_multipole_virial(p, part, outer):
    """Float64 [nsys, 3, 3]: the k-space block partials folded, plus the per-atom term `outer` [n, 3, 3] of the multipoles that follow the strain."""
    vir = C.fold_virial9(part)
    if p["bi"] is not None:
        return vir.index_add(0, p["bi"].long(), outer)
    return vir + outer.sum(0, keepdim=True)


def _mesh_args(inputs):
    """(positions, ..., cell, alpha, batch_idx) -> the arguments of `mesh_inputs` (the quadrupoles, if any, last)."""
    return inputs[:3] + inputs[-3:] + inputs[3:-3]


def mesh_forward(ops, inputs, dims, order, want):
    """The outputs of a mesh half in the positions dtype, no autograd graph: what the eager call and the `alchemiops::` op both run.
    `inputs` = (positions, charges, dipoles[, quadrupoles], cell, alpha, batch_idx)."""
    positions, cell, batch_idx = inputs[0], inputs[-3], inputs[-1]
    dt, virial = positions.dtype, want[-1]
    if positions.shape[0] == 0:
        return if_wanted(P.zeros(0, P.num_systems(cell, batch_idx), dt, positions.device, *ops["grads"]), want)
    dims = tuple(int(v) for v in dims)
    p = mesh_inputs(*_mesh_args(inputs))
    phi, spec = mesh_solve(p, ops["spread"](p, dims, order), dims, order, need_spec=virial)
    phi[0] += phi[1]  # the gather reads (A, B) = (the second potential, the sum of both)
    sums = ops["gather"](p, dims, order, phi[1], phi[0], (True,) + tuple(want[1:3]) + tuple(w or virial for w in want[3:-1]))
    return finish(sums, ops["virial"](p, spec, sums, dims, order) if virial else None, want, dt)


def mesh_adjoint(ops, inputs, dims, order, grad_energies):
    """Float64 gradients of L = sum_i g_i E_i.  The gather is its own adjoint: the g-weighted meshes ride in the same spread and the same
    batched solve (four meshes), and dL/dtheta_i = g_i x [gather over (A, B)] + [gather over (A^g, B^g)], self terms x g_i."""
    positions, grads = inputs[0], ops["grads"]
    if positions.shape[0] == 0:
        return zero_gradients(0, positions.device, grads)
    dims = tuple(int(v) for v in dims)
    p = mesh_inputs(*_mesh_args(inputs))
    g = weights_of(grad_energies)
    phi, _ = mesh_solve(p, ops["spread"](p, dims, order, weights=g), dims, order, need_spec=False)
    phi[0] += phi[1]
    phi[2] += phi[3]
    every = (False,) + (True,) * (1 + len(grads))
    out = ops["gather"](p, dims, order, phi[1], phi[0], every, weights=g)
    _, f, *gs = ops["gather"](p, dims, order, phi[3], phi[2], every, out=out)
    return (-f.to(torch.float64), *gs)


def mesh_solve(p, meshes, dims, order, need_spec):
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


def _mesh_alpha(alpha, n_sys, positions):
    return (_pme._traceable_alpha if C.tracing() else _prepare_alpha)(alpha, n_sys, positions.dtype, positions.device)


def mesh_reciprocal_space(ops, multipoles, cell, alpha, mesh_dimensions, mesh_spacing, spline_order, batch_idx, want):
    """The body of a public mesh half after its argument checks."""
    order = ops["check_order"](spline_order)
    cells, n_sys = _prepare_cell(cell)
    dims = mesh_dims(cells, mesh_dimensions, mesh_spacing, order)
    positions = multipoles[0]
    if positions.shape[0] == 0:
        return no_atoms(positions, P.num_systems(cell, batch_idx), ops["grads"], want)
    return dispatch(ops["op"], ops["forward"], multipoles, (cells, _mesh_alpha(alpha, n_sys, positions)), (batch_idx, *dims, order), want)


def _real_half(ops, multipoles, cells, alpha_t, batch_idx, lists, mask_value, flags):
    return ops["real"](*multipoles, cells, alpha_t, neighbor_list=lists[0], neighbor_ptr=lists[1], neighbor_shifts=lists[2], neighbor_matrix=lists[3],
                       neighbor_matrix_shifts=lists[4], mask_value=mask_value, batch_idx=batch_idx, **flags)


def mesh_correction(ops, multipoles, cell, alpha, mesh_spacing, mesh_dimensions, spline_order, batch_idx, lists, mask_value, want, accuracy):
    """The body of `pme_*_correction` after its list checks: estimate alpha and the mesh, add the two halves."""
    order = ops["check_order"](spline_order)
    cells, n_sys = _prepare_cell(cell)
    if mesh_dimensions is not None:
        mesh_dimensions = mesh_dims(cells, mesh_dimensions, None, order)
    positions = multipoles[0]
    if positions.shape[0] == 0:
        return no_atoms(positions, P.num_systems(cell, batch_idx), ops["grads"], want)
    C.require_device(*multipoles, cell, batch_idx)
    if alpha is None:
        est = _pme.estimate_pme_parameters(positions, cells, batch_idx, accuracy)
        alpha = est.alpha
        if mesh_dimensions is None and mesh_spacing is None:
            mesh_dimensions = tuple(est.mesh_dimensions)
    alpha_t = _mesh_alpha(alpha, n_sys, positions)
    if mesh_dimensions is None:
        mesh_dimensions = (_pme.mesh_spacing_to_dimensions(cells, mesh_spacing) if mesh_spacing is not None
                           else _pme.estimate_pme_mesh_dimensions(cells, alpha_t, accuracy))
    mesh_dimensions = mesh_dims(cells, mesh_dimensions, None, order)
    flags = dict(zip(ops["flags"], want[1:]))
    rs = _real_half(ops, multipoles, cells, alpha_t, batch_idx, lists, mask_value, flags)
    rec = ops["recip"](*multipoles, cells, alpha_t, mesh_dimensions=mesh_dimensions, spline_order=order, batch_idx=batch_idx, **flags)
    return add_halves(rs, rec)


# ---- explicit Ewald composite -------------------------------------------------------------------------------------------------------------------
def ewald_correction(ops, multipoles, cell, alpha, k_vectors, k_cutoff, batch_idx, lists, mask_value, want, accuracy):
    """The body of `ewald_*_correction` after its list checks: estimate alpha and the k cutoff, generate the k-vectors, add the two halves.
    `ops`: grads and the public halves real / recip."""
    from nvalchemiops.interactions.electrostatics.k_vectors import generate_k_vectors_ewald_summation
    from nvalchemiops.interactions.electrostatics.parameters import estimate_ewald_parameters

    cells, n_sys = _prepare_cell(cell)
    positions = multipoles[0]
    if positions.shape[0] == 0:
        return no_atoms(positions, P.num_systems(cell, batch_idx), ops["grads"], want)
    C.require_device(*multipoles, cell, k_vectors, batch_idx)
    if alpha is None or (k_cutoff is None and k_vectors is None):
        params = estimate_ewald_parameters(positions, cells, batch_idx, accuracy)
        if alpha is None:
            alpha = params.alpha
        if k_cutoff is None:
            k_cutoff = params.reciprocal_space_cutoff
    alpha_t = _prepare_alpha(alpha, n_sys, positions.dtype, positions.device)
    if k_vectors is None:
        k_vectors = generate_k_vectors_ewald_summation(cells, k_cutoff)
    flags = dict(zip(ops["flags"], want[1:]))
    rs = _real_half(ops, multipoles, cells, alpha_t, batch_idx, lists, mask_value, flags)
    rec = ops["recip"](*multipoles, cells, k_vectors, alpha_t, batch_idx=batch_idx, **flags)
    return add_halves(rs, rec)
