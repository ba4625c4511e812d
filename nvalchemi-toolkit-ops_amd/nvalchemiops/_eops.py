"""`alchemiops::*` custom ops of the electrostatics path -- the torch.compile / autograd seam of the value-returning ops.

The reference registers every spline / PME / Ewald op with `warp_custom_op` = `torch.library.custom_op` + `register_fake` +
`register_autograd`, the backward being a recorded Warp tape (autograd.py:124-297; op definitions spline.py:1500-2200,
interactions/electrostatics/pme.py:273-1163, ewald.py:263-2318).  Here the same op NAMES and ARGUMENT LISTS are registered on
the HIP kernels, with
  * fake (meta) implementations that return the TRUE output dtype (the reference's return float64 whatever the input is:
    SURVEY Appendix B.11), so `torch.compile(..., fullgraph=True)` can trace through the whole PME composition;
  * hand-written adjoints instead of a tape: spread <-> gather are each other's adjoints, position / cell gradients come from the
    gather-gradient kernel, `spline_gather_vec3` (the force gather) has its adjoint too -- so forces of the reciprocal part can be
    differentiated once more (force-matching training); Green function and corrections have closed-form derivatives; the
    real-space sum uses `mi_ewald_real_bwd`, the explicit-k sum two more passes of its forward kernels.
The real-space FORCES and CHARGE GRADIENTS are differentiable too (`mi_ewald_real_forces_bwd`: second derivatives of the pair sum), so a
loss on total PME forces or charge gradients back-propagates to positions, charges, cell and alpha; so are the cut-off Coulomb forces and
`spline_gather_gradient`, and the forces / charge gradients of the explicit-k reciprocal sum (positions, charges, alpha, cell volume and --
round 3 -- the k-vectors: every array the reference lists in `grad_arrays` has its adjoint here).  Third derivatives raise
NotImplementedError (never a silent zero).

The public functions (`spline_spread`, `particle_mesh_ewald`, ...) call these ops when something requires grad or when they are
being traced; otherwise they take the direct ctypes path (no dispatcher overhead, fused kernels).
"""
from __future__ import annotations

import ctypes
import importlib
import math
from typing import Optional

import torch
from torch import Tensor

from nvalchemiops import _capi as C

_NS = "alchemiops"
_SECOND_ORDER = ("{op}: derivatives of the '{what}' output are second derivatives of the pair kernels, which this build does not "
                 "provide (the reference differentiates them through its Warp tape); differentiate the energies instead.")


def _op(name, fn, fake, backward=None, setup=None):
    op = torch.library.custom_op(f"{_NS}::{name}", fn, mutates_args=())
    op.register_fake(fake)
    if backward is not None:
        op.register_autograd(backward, setup_context=setup)
    return op


def _cit(cell: Tensor, cell_inv_t: Optional[Tensor], dtype) -> Tensor:
    """[B,3,3] transposed inverse cell in `dtype` (the reference recomputes it inside the op when not given)."""
    if cell_inv_t is not None:
        return cell_inv_t.to(dtype).reshape(-1, 3, 3)
    c = cell if cell.dim() == 3 else cell.unsqueeze(0)
    return torch.linalg.inv(c.to(dtype)).transpose(-1, -2)


# =====================================================================================================================================
# per-system sums of per-atom values (adjoints reduce per-atom terms to [B] gradients of alpha / volume / total charge)
# =====================================================================================================================================
def _segment_sum(values: Tensor, batch_idx: Optional[Tensor], num_systems: int) -> Tensor:
    v = values.detach().contiguous()
    out = torch.zeros(num_systems, dtype=v.dtype, device=v.device)
    if v.shape[0]:
        bi = None if batch_idx is None else C.i32(batch_idx)
        C.check(C.lib().mi_segment_sum(C.ptr(v), C.ptr(bi), v.shape[0], C.dtype_code(v.dtype), C.ptr(out), C.stream_of(v)), "mi_segment_sum")
    return out


segment_sum_op = torch.library.custom_op("nvalchemiops::segment_sum", _segment_sum, mutates_args=())
segment_sum_op.register_fake(lambda values, batch_idx, num_systems: values.new_empty((num_systems,)))
segment_sum_op.register_autograd(lambda ctx, g: (g[ctx.sel] if ctx.sel is not None else g.expand(ctx.n), None, None),
                                 setup_context=lambda ctx, inputs, output: (setattr(ctx, "sel", None if inputs[1] is None else inputs[1].long()),
                                                                           setattr(ctx, "n", inputs[0].shape[0])) and None)


def seg_sum(x: Tensor, batch_idx: Optional[Tensor], num_systems: int) -> Tensor:
    """sum of x over the atoms of each system, [B].  One wave-aggregated atomic per wave and system (`mi_segment_sum`) for fp32 / fp64
    instead of `index_add` with one same-address atomic per ATOM: on a single 100k-atom system the latter took 6.5 ms per call and was
    48 % of the GPU time of a PME training step (profiles/r03_kernel_stats_train_before.csv)."""
    if x.dtype in (torch.float32, torch.float64) and x.dim() == 1 and x.is_cuda:
        return segment_sum_op(x, batch_idx, num_systems)
    if batch_idx is None:
        return x.sum(0, keepdim=True)
    return torch.zeros((num_systems,) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device).index_add(0, batch_idx.long(), x)


# =====================================================================================================================================
# guarded mesh FFTs (round 5): rfftn / irfftn of the op-by-op composition through the library's self-tested plan cache
# =====================================================================================================================================
# The composition (pme._reciprocal_composed: what runs under torch.compile and for the outputs the fused autograd node does not cover)
# used to call torch.fft directly, as the reference does (pme.py:1398, :1422, :1455-1457).  rocFFT on this stack can return a wrong
# transform for some mesh shapes depending on what the process planned before -- through torch.fft too -- so these two ops
# route the same unscaled transforms through `pme._fft_plan`: a hipFFT plan that reproduced a known answer at creation, or the library's
# dense DFT when it did not.  Each is the other's adjoint up to the half-spectrum weights, so first and higher derivatives stay ops.
def _half_weights(nz: int, like: Tensor, interior: float) -> Tensor:
    """[nz/2+1] real weights: `interior` for the bins that stand for two conjugate frequencies, 1 for the self-conjugate ones (DC, Nyquist)."""
    w = torch.full((nz // 2 + 1,), interior, dtype=like.real.dtype if like.is_complex() else like.dtype, device=like.device)
    w[0] = 1.0
    if nz % 2 == 0:
        w[-1] = 1.0
    return w


def _mesh_rfftn(mesh: Tensor) -> Tensor:
    from nvalchemiops.interactions.electrostatics import pme as P

    m = mesh.detach().contiguous()
    b, nx, ny, nz = m.shape
    out = torch.empty((b, nx, ny, nz // 2 + 1), dtype=torch.complex64 if m.dtype == torch.float32 else torch.complex128, device=m.device)
    P._fft_plan(m.device, (nx, ny, nz), b, C.dtype_code(m.dtype), False)(m.clone(), out)  # (an R2C transform may use its input as scratch)
    return out


def _mesh_irfftn(spec: Tensor, nz: int) -> Tensor:
    from nvalchemiops.interactions.electrostatics import pme as P

    sp = spec.detach().contiguous().clone()  # the multi-dimensional C2R consumes its input
    b, nx, ny, _ = sp.shape
    rdt = torch.float32 if sp.dtype == torch.complex64 else torch.float64
    out = torch.empty((b, nx, ny, int(nz)), dtype=rdt, device=sp.device)
    P._fft_plan(sp.device, (nx, ny, int(nz)), b, C.dtype_code(rdt), True)(sp, out)
    return out


mesh_rfftn_op = torch.library.custom_op("nvalchemiops::mesh_rfftn", _mesh_rfftn, mutates_args=())
mesh_rfftn_op.register_fake(lambda mesh: mesh.new_empty(tuple(mesh.shape[:3]) + (mesh.shape[3] // 2 + 1,),
                                                         dtype=torch.complex64 if mesh.dtype == torch.float32 else torch.complex128))
mesh_irfftn_op = torch.library.custom_op("nvalchemiops::mesh_irfftn", _mesh_irfftn, mutates_args=())
mesh_irfftn_op.register_fake(lambda spec, nz: spec.new_empty(tuple(spec.shape[:3]) + (int(nz),),
                                                             dtype=torch.float32 if spec.dtype == torch.complex64 else torch.float64))


def _mesh_rfftn_bwd(ctx, g):
    # y_k = sum_n x_n e^{-ikn} over the half spectrum: dL/dx_n = Re sum_k g_k e^{+ikn} with every stored bin counted ONCE -- the C2R
    # transform counts the interior bins twice, hence the 1/2
    return mesh_irfftn_op(g * _half_weights(ctx.nz, g, 0.5), ctx.nz)


def _mesh_irfftn_bwd(ctx, g):
    # x_n = sum_k c_k Re(y_k e^{+ikn}), c = 2 for the interior bins: dL/dy_k = c_k (R2C g)_k
    spec = mesh_rfftn_op(g)
    return spec * _half_weights(ctx.nz, spec, 2.0), None


mesh_rfftn_op.register_autograd(_mesh_rfftn_bwd, setup_context=lambda ctx, inputs, output: setattr(ctx, "nz", int(inputs[0].shape[3])))
mesh_irfftn_op.register_autograd(_mesh_irfftn_bwd, setup_context=lambda ctx, inputs, output: setattr(ctx, "nz", int(inputs[1])))


def mesh_rfftn(mesh: Tensor) -> Tensor:
    """Unscaled rfftn over the last three dimensions of a [nx, ny, nz] or [B, nx, ny, nz] mesh (torch.fft.rfftn(norm="backward"))."""
    return mesh_rfftn_op(mesh.unsqueeze(0)).squeeze(0) if mesh.dim() == 3 else mesh_rfftn_op(mesh)


def mesh_irfftn(spec: Tensor, nz: int) -> Tensor:
    """Unscaled irfftn over the last three dimensions (torch.fft.irfftn(norm="forward", s=(nx, ny, nz)))."""
    return mesh_irfftn_op(spec.unsqueeze(0), nz).squeeze(0) if spec.dim() == 3 else mesh_irfftn_op(spec, nz)


# =====================================================================================================================================
# B-spline spread / gather
# =====================================================================================================================================
def _spread_impl(positions, values, batch_idx, cit, nsys, dims, order):
    from nvalchemiops.spline import _launch_spread

    pos = positions.detach().contiguous()
    bi = None if batch_idx is None else C.i32(batch_idx)
    return _launch_spread(pos, values.detach().to(pos.dtype).contiguous(), cit.detach().to(pos.dtype).contiguous(), bi, nsys, dims, int(order),
                          bi is not None)


def _gather_impl(positions, mesh, batch_idx, cit, order, grad=False):
    from nvalchemiops.spline import _launch_gather

    pos = positions.detach().contiguous()
    bi = None if batch_idx is None else C.i32(batch_idx)
    return _launch_gather(pos, mesh.detach().to(pos.dtype).contiguous(), cit.detach().to(pos.dtype).contiguous(), bi, int(order), grad=grad)


def _gather_vec3_impl(positions, charges, mesh, batch_idx, cit, order):
    pos = positions.detach().contiguous()
    m = mesh.detach().to(pos.dtype).contiguous()
    q = charges.detach().to(pos.dtype).contiguous()
    c = cit.detach().to(pos.dtype).contiguous()
    bi = None if batch_idx is None else C.i32(batch_idx)
    nx, ny, nz = m.shape[-4:-1]
    out = torch.empty((pos.shape[0], 3), dtype=pos.dtype, device=pos.device)
    rc = C.lib().mi_spline_gather_vec3(C.ptr(pos), C.ptr(q), C.ptr(m), C.ptr(bi), C.ptr(c), pos.shape[0], c.shape[0], nx, ny, nz, C.spline_order_arg(order),
                                       C.dtype_code(pos.dtype), C.ptr(out), C.stream_of(pos))
    C.check(rc, "mi_spline_gather_vec3")
    return out


# Backward formulas are traced by AOT autograd under torch.compile, so every kernel launch inside them is an op as well.  These
# two are not in the reference's op set (its backward is a Warp tape): they live in this build's own namespace.
def _frac_grad(positions: Tensor, mesh: Tensor, batch_idx: Optional[Tensor], cell_inv_t: Tensor, spline_order: int) -> Tensor:
    return _gather_impl(positions, mesh, batch_idx, cell_inv_t, spline_order, grad=True)


def _frac_grad_fake(positions, mesh, batch_idx, cell_inv_t, spline_order):
    return positions.new_empty((positions.shape[0], 3))


frac_grad_op = torch.library.custom_op("nvalchemiops::spline_gather_frac_grad", _frac_grad, mutates_args=())
frac_grad_op.register_fake(_frac_grad_fake)
frac_grad_op.register_autograd(lambda ctx, g: (_ for _ in ()).throw(NotImplementedError(_SECOND_ORDER.format(
    op="nvalchemiops::spline_gather_frac_grad", what="position / cell gradient"))), setup_context=lambda ctx, inputs, output: None)


def _coordinate_grads(weight, gfrac, pos, cit, bi):
    """frac = cell_inv_t . r  =>  dL/dr_b = w sum_a gfrac_a cit[a][b] ;  dL/dcit[s][a][b] = sum_{i in s} w_i gfrac_i[a] r_i[b].
    Elementwise contractions + reductions: a per-atom batched 3x3 GEMM (einsum) was 11 % of the GPU time of a PME training step, and the
    [3,N] x [N,3] GEMM formulation of the cell term is worse still (rocBLAS runs a K = N fp64 product with a 3x3 result in one workgroup:
    5 ms at 100k atoms).  Batch: nine per-system segment sums (`seg_sum`), not one same-address atomic per atom."""
    wg = gfrac if weight is None else gfrac * weight.unsqueeze(-1)  # (None: the weights are inside gfrac already, channel ops below)
    if bi is None:  # single system: cit is [1,3,3]
        return (wg.unsqueeze(-1) * cit[0]).sum(1), (wg.unsqueeze(-1) * pos.unsqueeze(-2)).sum(0, keepdim=True)
    gpos = (wg.unsqueeze(-1) * cit[bi.long()]).sum(1)
    outer = (wg.unsqueeze(-1) * pos.unsqueeze(-2)).reshape(-1, 9)
    gcit = torch.stack([seg_sum(outer[:, k].contiguous(), bi, cit.shape[0]) for k in range(9)], dim=-1).reshape(-1, 3, 3)
    return gpos, gcit


def _like_cell_inv_t(gcit, cell_inv_t):
    return None if cell_inv_t is None else gcit.reshape(cell_inv_t.shape).to(cell_inv_t.dtype)


def _n(need, k):
    """needs_input_grad[k]; False for a trailing optional argument the caller left out (the tuple then ends before it)."""
    return k < len(need) and need[k]


def _fit(need, grads):
    """One gradient per argument the op was CALLED with (a direct call may omit the trailing optional `cell_inv_t`)."""
    return tuple(grads[: len(need)])


def _cell_grad_without_cit(gc, cit, cell, cell_inv_t, needed):
    """The op was called WITHOUT `cell_inv_t` (reference signature: it is optional), so cell^-T was formed from `cell` inside the op
    and the gradient has to reach `cell` itself: cit = cell^-T  =>  dL/dcell = -cit (dL/dcit)^T cit.  None when `cell_inv_t` was given
    (the gradient then flows through that argument) or `cell` needs no gradient -- never a silently missing cell gradient."""
    if cell_inv_t is not None or not needed or gc is None:
        return None
    c = cit.detach().to(gc.dtype)
    g = -(c @ gc.transpose(-1, -2) @ c)
    if cell.reshape(-1, 3, 3).shape[0] != g.shape[0]:
        g = g.sum(0, keepdim=True)
    return g.reshape(cell.shape).to(cell.dtype)


# ---- spread -------------------------------------------------------------------------------------------------------------------------
def _spline_spread(positions: Tensor, values: Tensor, cell: Tensor, mesh_nx: int, mesh_ny: int, mesh_nz: int, spline_order: int,
                   cell_inv_t: Optional[Tensor] = None) -> Tensor:
    return _spread_impl(positions, values, None, _cit(cell, cell_inv_t, positions.dtype), 1, (mesh_nx, mesh_ny, mesh_nz), spline_order)[0]


def _spline_spread_fake(positions, values, cell, mesh_nx, mesh_ny, mesh_nz, spline_order, cell_inv_t=None):
    return positions.new_empty((mesh_nx, mesh_ny, mesh_nz))


def _batch_spline_spread(positions: Tensor, values: Tensor, batch_idx: Tensor, cell: Tensor, num_systems: int, mesh_nx: int, mesh_ny: int,
                         mesh_nz: int, spline_order: int, cell_inv_t: Optional[Tensor] = None) -> Tensor:
    cit = _cit(cell, cell_inv_t, positions.dtype)
    if cit.shape[0] == 1 and num_systems > 1:
        cit = cit.expand(num_systems, 3, 3)
    return _spread_impl(positions, values, batch_idx, cit, num_systems, (mesh_nx, mesh_ny, mesh_nz), spline_order)


def _batch_spline_spread_fake(positions, values, batch_idx, cell, num_systems, mesh_nx, mesh_ny, mesh_nz, spline_order, cell_inv_t=None):
    return positions.new_empty((num_systems, mesh_nx, mesh_ny, mesh_nz))


def _spread_setup(batched):
    def setup(ctx, inputs, output):
        if batched:
            positions, values, batch_idx, cell, num_systems, _, _, _, order, cell_inv_t = inputs
        else:
            positions, values, cell, _, _, _, order, cell_inv_t = inputs
            batch_idx, num_systems = None, 1
        ctx.save_for_backward(positions, values, cell, cell_inv_t, batch_idx)
        ctx.order, ctx.nsys = order, num_systems
    return setup


def _spread_backward(batched):
    gather = lambda *a: (torch.ops.alchemiops._batch_spline_gather if batched else torch.ops.alchemiops._spline_gather)(*a)  # noqa: E731

    def backward(ctx, gmesh):
        positions, values, cell, cell_inv_t, batch_idx = ctx.saved_tensors
        need = ctx.needs_input_grad
        cit = _cit(cell, cell_inv_t, positions.dtype)
        if batched and cit.shape[0] == 1 and ctx.nsys > 1:
            cit = cit.expand(ctx.nsys, 3, 3)
        g = gmesh.contiguous()
        gvals = gpos = gcit = None
        vi, ci = (1, 9) if batched else (1, 7)
        if need[vi]:  # d/dvalues = gather(grad_mesh): the gather op, so this branch can be differentiated again
            gvals = gather(positions, g, batch_idx, cell, ctx.order, cell_inv_t) if batched else gather(positions, g, cell, ctx.order, cell_inv_t)
        cell_i = 3 if batched else 2
        gcell = None
        if need[0] or _n(need, ci) or (cell_inv_t is None and need[cell_i]):
            gfrac = frac_grad_op(positions, g if batched else g.unsqueeze(0), batch_idx, cit, ctx.order)
            gpos, gc = _coordinate_grads(values.detach().to(positions.dtype), gfrac, positions.detach(), cit.detach(), None if batch_idx is None else batch_idx)
            gcit = _like_cell_inv_t(gc if (cell_inv_t is None or cell_inv_t.reshape(-1, 3, 3).shape[0] == gc.shape[0]) else gc.sum(0, keepdim=True), cell_inv_t)
            gcell = _cell_grad_without_cit(gc, cit, cell, cell_inv_t, need[cell_i])
        if batched:
            return _fit(need, (gpos if need[0] else None, gvals, None, gcell, None, None, None, None, None, gcit if _n(need, 9) else None))
        return _fit(need, (gpos if need[0] else None, gvals, gcell, None, None, None, None, gcit if _n(need, 7) else None))
    return backward


spline_spread_op = _op("_spline_spread", _spline_spread, _spline_spread_fake, _spread_backward(False), _spread_setup(False))
batch_spline_spread_op = _op("_batch_spline_spread", _batch_spline_spread, _batch_spline_spread_fake, _spread_backward(True), _spread_setup(True))


# ---- gather -------------------------------------------------------------------------------------------------------------------------
def _spline_gather(positions: Tensor, mesh: Tensor, cell: Tensor, spline_order: int, cell_inv_t: Optional[Tensor] = None) -> Tensor:
    return _gather_impl(positions, mesh.unsqueeze(0), None, _cit(cell, cell_inv_t, positions.dtype), spline_order)


def _spline_gather_fake(positions, mesh, cell, spline_order, cell_inv_t=None):
    return positions.new_empty((positions.shape[0],))


def _batch_spline_gather(positions: Tensor, mesh: Tensor, batch_idx: Tensor, cell: Tensor, spline_order: int,
                         cell_inv_t: Optional[Tensor] = None) -> Tensor:
    cit = _cit(cell, cell_inv_t, positions.dtype)
    if cit.shape[0] == 1 and mesh.shape[0] > 1:
        cit = cit.expand(mesh.shape[0], 3, 3)
    return _gather_impl(positions, mesh, batch_idx, cit, spline_order)


def _batch_spline_gather_fake(positions, mesh, batch_idx, cell, spline_order, cell_inv_t=None):
    return positions.new_empty((positions.shape[0],))


def _gather_setup(batched):
    def setup(ctx, inputs, output):
        if batched:
            positions, mesh, batch_idx, cell, order, cell_inv_t = inputs
        else:
            positions, mesh, cell, order, cell_inv_t = inputs
            batch_idx = None
        ctx.save_for_backward(positions, mesh, cell, cell_inv_t, batch_idx)
        ctx.order = order
    return setup


def _gather_backward(batched):
    def backward(ctx, gout):
        positions, mesh, cell, cell_inv_t, batch_idx = ctx.saved_tensors
        need = ctx.needs_input_grad
        cit = _cit(cell, cell_inv_t, positions.dtype)
        nsys = mesh.shape[0] if batched else 1
        if batched and cit.shape[0] == 1 and nsys > 1:
            cit = cit.expand(nsys, 3, 3)
        g = gout.contiguous()
        nx, ny, nz = mesh.shape[-3:]
        gmesh = gpos = gcit = None
        ci = 5 if batched else 4
        if need[1]:  # d/dmesh = spread(grad_out): the spread op, differentiable again
            if batched:
                gmesh = torch.ops.alchemiops._batch_spline_spread(positions, g, batch_idx, cell, nsys, nx, ny, nz, ctx.order, cell_inv_t)
            else:
                gmesh = torch.ops.alchemiops._spline_spread(positions, g, cell, nx, ny, nz, ctx.order, cell_inv_t)
        cell_i = 3 if batched else 2
        gcell = None
        if need[0] or _n(need, ci) or (cell_inv_t is None and need[cell_i]):
            gfrac = frac_grad_op(positions, mesh if batched else mesh.unsqueeze(0), batch_idx, cit, ctx.order)
            gpos, gc = _coordinate_grads(g.detach().to(positions.dtype), gfrac, positions.detach(), cit.detach(), batch_idx)
            gcit = _like_cell_inv_t(gc if (cell_inv_t is None or cell_inv_t.reshape(-1, 3, 3).shape[0] == gc.shape[0]) else gc.sum(0, keepdim=True), cell_inv_t)
            gcell = _cell_grad_without_cit(gc, cit, cell, cell_inv_t, need[cell_i])
        if batched:
            return _fit(need, (gpos if need[0] else None, gmesh, None, gcell, None, gcit if _n(need, 5) else None))
        return _fit(need, (gpos if need[0] else None, gmesh, gcell, None, gcit if _n(need, 4) else None))
    return backward


spline_gather_op = _op("_spline_gather", _spline_gather, _spline_gather_fake, _gather_backward(False), _gather_setup(False))
batch_spline_gather_op = _op("_batch_spline_gather", _batch_spline_gather, _batch_spline_gather_fake, _gather_backward(True), _gather_setup(True))


# ---- multi-channel spread / gather: values[N, C] <-> mesh[(B,) C, nx, ny, nz] (reference ops spline.py:2202-2580) ---------------------------
# One fused launch sequence per call (csrc/pme.hip: mi_spline_spread_channels / _gather_channels) instead of C scalar ops; argument lists
# are the reference's plus the optional `cell_inv_t` the scalar ops here carry.  Adjoints: the two ops are each other's (values / mesh
# branches, built from the ops themselves so they can be differentiated again); positions and cell come from the channel-weighted
# fractional gradient, an op of its own whose derivative is refused like `frac_grad_op`'s.
def _channels_impl(positions, batch_idx, cit):
    C.require_device(positions, cit)  # the ops are reachable from a trace over tensors that are not on the device: refuse, never dereference
    pos = positions.detach().contiguous()
    return pos, (None if batch_idx is None else C.i32(batch_idx)), cit.detach().to(pos.dtype).contiguous()


def _frac_grad_channels(positions: Tensor, mesh: Tensor, coef: Tensor, batch_idx: Optional[Tensor], cell_inv_t: Tensor, spline_order: int) -> Tensor:
    from nvalchemiops.spline import _launch_gather_channels

    pos, bi, cit = _channels_impl(positions, batch_idx, cell_inv_t)
    if pos.shape[0] == 0 or mesh.shape[1] == 0:
        return pos.new_zeros((pos.shape[0], 3))
    return _launch_gather_channels(pos, mesh.detach().to(pos.dtype).contiguous(), cit, bi, int(spline_order), coef=coef.detach().to(pos.dtype).contiguous())


frac_grad_channels_op = torch.library.custom_op("nvalchemiops::spline_gather_channels_frac_grad", _frac_grad_channels, mutates_args=())
frac_grad_channels_op.register_fake(lambda positions, mesh, coef, batch_idx, cell_inv_t, spline_order: positions.new_empty((positions.shape[0], 3)))
frac_grad_channels_op.register_autograd(lambda ctx, g: (_ for _ in ()).throw(NotImplementedError(_SECOND_ORDER.format(
    op="nvalchemiops::spline_gather_channels_frac_grad", what="position / cell gradient"))), setup_context=lambda ctx, inputs, output: None)


def _spread_channels_run(positions, values, batch_idx, cit, nsys, dims, order):
    from nvalchemiops.spline import _launch_spread_channels

    pos, bi, c = _channels_impl(positions, batch_idx, cit)
    if pos.shape[0] == 0 or values.shape[1] == 0:
        return pos.new_zeros((nsys, values.shape[1]) + tuple(dims))
    return _launch_spread_channels(pos, values.detach().to(pos.dtype).contiguous(), c, bi, nsys, dims, int(order), bi is not None)


def _gather_channels_run(positions, mesh, batch_idx, cit, order):
    from nvalchemiops.spline import _launch_gather_channels

    pos, bi, c = _channels_impl(positions, batch_idx, cit)
    if pos.shape[0] == 0 or mesh.shape[1] == 0:
        return pos.new_zeros((pos.shape[0], mesh.shape[1]))
    return _launch_gather_channels(pos, mesh.detach().to(pos.dtype).contiguous(), c, bi, int(order))


def _batch_cit(cell, cell_inv_t, dtype, nsys):
    cit = _cit(cell, cell_inv_t, dtype)
    return cit.expand(nsys, 3, 3) if cit.shape[0] == 1 and nsys > 1 else cit


def _spline_spread_channels(positions: Tensor, values: Tensor, cell: Tensor, num_channels: int, mesh_nx: int, mesh_ny: int, mesh_nz: int,
                            spline_order: int, cell_inv_t: Optional[Tensor] = None) -> Tensor:
    return _spread_channels_run(positions, values, None, _cit(cell, cell_inv_t, positions.dtype), 1, (mesh_nx, mesh_ny, mesh_nz), spline_order)[0]


def _spline_spread_channels_fake(positions, values, cell, num_channels, mesh_nx, mesh_ny, mesh_nz, spline_order, cell_inv_t=None):
    return positions.new_empty((num_channels, mesh_nx, mesh_ny, mesh_nz))


def _batch_spline_spread_channels(positions: Tensor, values: Tensor, batch_idx: Tensor, cell: Tensor, num_systems: int, num_channels: int,
                                  mesh_nx: int, mesh_ny: int, mesh_nz: int, spline_order: int, cell_inv_t: Optional[Tensor] = None) -> Tensor:
    return _spread_channels_run(positions, values, batch_idx, _batch_cit(cell, cell_inv_t, positions.dtype, num_systems), num_systems,
                                (mesh_nx, mesh_ny, mesh_nz), spline_order)


def _batch_spline_spread_channels_fake(positions, values, batch_idx, cell, num_systems, num_channels, mesh_nx, mesh_ny, mesh_nz, spline_order,
                                       cell_inv_t=None):
    return positions.new_empty((num_systems, num_channels, mesh_nx, mesh_ny, mesh_nz))


def _spline_gather_channels(positions: Tensor, mesh: Tensor, cell: Tensor, spline_order: int, cell_inv_t: Optional[Tensor] = None) -> Tensor:
    return _gather_channels_run(positions, mesh.unsqueeze(0), None, _cit(cell, cell_inv_t, positions.dtype), spline_order)


def _spline_gather_channels_fake(positions, mesh, cell, spline_order, cell_inv_t=None):
    return positions.new_empty((positions.shape[0], mesh.shape[0]))


def _batch_spline_gather_channels(positions: Tensor, mesh: Tensor, batch_idx: Tensor, cell: Tensor, spline_order: int,
                                  cell_inv_t: Optional[Tensor] = None) -> Tensor:
    return _gather_channels_run(positions, mesh, batch_idx, _batch_cit(cell, cell_inv_t, positions.dtype, mesh.shape[0]), spline_order)


def _batch_spline_gather_channels_fake(positions, mesh, batch_idx, cell, spline_order, cell_inv_t=None):
    return positions.new_empty((positions.shape[0], mesh.shape[1]))


def _channel_coordinate_grads(positions, mesh5, coef, batch_idx, cit, cell, cell_inv_t, order, need_cell):
    """Position / cell_inv_t / cell gradients shared by both adjoints: gfrac_i = sum_c coef_ic sum_g mesh_c[g] dW_i(g)/dfrac, then the
    chain rule of `_coordinate_grads` (the per-atom weights are inside gfrac already)."""
    gfrac = frac_grad_channels_op(positions, mesh5, coef, batch_idx, cit, order)
    gpos, gc = _coordinate_grads(None, gfrac, positions.detach(), cit.detach(), batch_idx)
    gcit = _like_cell_inv_t(gc if (cell_inv_t is None or cell_inv_t.reshape(-1, 3, 3).shape[0] == gc.shape[0]) else gc.sum(0, keepdim=True), cell_inv_t)
    return gpos, gcit, _cell_grad_without_cit(gc, cit, cell, cell_inv_t, need_cell)


def _spread_channels_setup(batched):
    def setup(ctx, inputs, output):
        if batched:
            positions, values, batch_idx, cell, num_systems, _, _, _, _, order, cell_inv_t = inputs
        else:
            positions, values, cell, _, _, _, _, order, cell_inv_t = inputs
            batch_idx, num_systems = None, 1
        ctx.save_for_backward(positions, values, cell, cell_inv_t, batch_idx)
        ctx.order, ctx.nsys = order, num_systems
    return setup


def _spread_channels_backward(batched):
    def backward(ctx, gmesh):
        positions, values, cell, cell_inv_t, batch_idx = ctx.saved_tensors
        need = ctx.needs_input_grad
        g = gmesh.contiguous()
        gvals = gpos = gcit = gcell = None
        ci, cell_i = (10, 3) if batched else (8, 2)
        if need[1]:  # d/dvalues = gather_channels(grad_mesh): the gather op, so this branch can be differentiated again
            if batched:
                gvals = torch.ops.alchemiops._batch_spline_gather_channels(positions, g, batch_idx, cell, ctx.order, cell_inv_t)
            else:
                gvals = torch.ops.alchemiops._spline_gather_channels(positions, g, cell, ctx.order, cell_inv_t)
        if need[0] or _n(need, ci) or (cell_inv_t is None and need[cell_i]):
            cit = _batch_cit(cell, cell_inv_t, positions.dtype, ctx.nsys if batched else 1)
            gpos, gcit, gcell = _channel_coordinate_grads(positions, g if batched else g.unsqueeze(0), values.to(positions.dtype), batch_idx, cit, cell,
                                                          cell_inv_t, ctx.order, need[cell_i])
        gpos = gpos if need[0] else None
        if batched:
            return _fit(need, (gpos, gvals, None, gcell, None, None, None, None, None, None, gcit if _n(need, ci) else None))
        return _fit(need, (gpos, gvals, gcell, None, None, None, None, None, gcit if _n(need, ci) else None))
    return backward


def _gather_channels_setup(batched):
    def setup(ctx, inputs, output):
        if batched:
            positions, mesh, batch_idx, cell, order, cell_inv_t = inputs
        else:
            positions, mesh, cell, order, cell_inv_t = inputs
            batch_idx = None
        ctx.save_for_backward(positions, mesh, cell, cell_inv_t, batch_idx)
        ctx.order = order
    return setup


def _gather_channels_backward(batched):
    def backward(ctx, gout):
        positions, mesh, cell, cell_inv_t, batch_idx = ctx.saved_tensors
        need = ctx.needs_input_grad
        nsys = mesh.shape[0] if batched else 1
        g = gout.contiguous()
        nch = mesh.shape[-4]
        nx, ny, nz = mesh.shape[-3:]
        gmesh = gpos = gcit = gcell = None
        ci, cell_i = (5, 3) if batched else (4, 2)
        if need[1]:  # d/dmesh = spread_channels(grad_out): the spread op, differentiable again
            if batched:
                gmesh = torch.ops.alchemiops._batch_spline_spread_channels(positions, g, batch_idx, cell, nsys, nch, nx, ny, nz, ctx.order, cell_inv_t)
            else:
                gmesh = torch.ops.alchemiops._spline_spread_channels(positions, g, cell, nch, nx, ny, nz, ctx.order, cell_inv_t)
        if need[0] or _n(need, ci) or (cell_inv_t is None and need[cell_i]):
            cit = _batch_cit(cell, cell_inv_t, positions.dtype, nsys)
            gpos, gcit, gcell = _channel_coordinate_grads(positions, mesh if batched else mesh.unsqueeze(0), g.to(positions.dtype), batch_idx, cit, cell,
                                                          cell_inv_t, ctx.order, need[cell_i])
        gpos = gpos if need[0] else None
        if batched:
            return _fit(need, (gpos, gmesh, None, gcell, None, gcit if _n(need, ci) else None))
        return _fit(need, (gpos, gmesh, gcell, None, gcit if _n(need, ci) else None))
    return backward


spline_spread_channels_op = _op("_spline_spread_channels", _spline_spread_channels, _spline_spread_channels_fake, _spread_channels_backward(False),
                                _spread_channels_setup(False))
batch_spline_spread_channels_op = _op("_batch_spline_spread_channels", _batch_spline_spread_channels, _batch_spline_spread_channels_fake,
                                      _spread_channels_backward(True), _spread_channels_setup(True))
spline_gather_channels_op = _op("_spline_gather_channels", _spline_gather_channels, _spline_gather_channels_fake, _gather_channels_backward(False),
                                _gather_channels_setup(False))
batch_spline_gather_channels_op = _op("_batch_spline_gather_channels", _batch_spline_gather_channels, _batch_spline_gather_channels_fake,
                                      _gather_channels_backward(True), _gather_channels_setup(True))


# ---- gather_vec3: out_i[c] = q_i sum_g mesh[g, c] w_i(g) -------------------------------------------------------------------------------
def _spline_gather_vec3(positions: Tensor, charges: Tensor, mesh: Tensor, cell: Tensor, spline_order: int,
                        cell_inv_t: Optional[Tensor] = None) -> Tensor:
    return _gather_vec3_impl(positions, charges, mesh.unsqueeze(0), None, _cit(cell, cell_inv_t, positions.dtype), spline_order)


def _vec3_fake(positions, *rest, **kw):
    return positions.new_empty((positions.shape[0], 3))


def _batch_spline_gather_vec3(positions: Tensor, charges: Tensor, mesh: Tensor, batch_idx: Tensor, cell: Tensor, spline_order: int,
                              cell_inv_t: Optional[Tensor] = None) -> Tensor:
    cit = _cit(cell, cell_inv_t, positions.dtype)
    if cit.shape[0] == 1 and mesh.shape[0] > 1:
        cit = cit.expand(mesh.shape[0], 3, 3)
    return _gather_vec3_impl(positions, charges, mesh, batch_idx, cit, spline_order)


def _vec3_setup(batched):
    def setup(ctx, inputs, output):
        if batched:
            positions, charges, mesh, batch_idx, cell, order, cell_inv_t = inputs
        else:
            positions, charges, mesh, cell, order, cell_inv_t = inputs
            batch_idx = None
        ctx.save_for_backward(positions, charges, mesh, cell, cell_inv_t, batch_idx)
        ctx.order = order
    return setup


def _vec3_backward(batched):
    """Adjoint of the force gather (the reference gets it from the tape of `_bspline_gather_vec3_kernel`, spline.py:1664-1747):
    with G = grad_out [N,3] and the three channel meshes M_c = mesh[..., c],
      d/dcharges_i = sum_c G_ic gather(M_c)_i ;  d/dmesh[..., c] = spread(q_i G_ic) ;  d/dr_i = sum_c q_i G_ic grad_r gather(M_c)_i."""
    def backward(ctx, gout):
        positions, charges, mesh, cell, cell_inv_t, batch_idx = ctx.saved_tensors
        need = ctx.needs_input_grad
        cit = _cit(cell, cell_inv_t, positions.dtype)
        nsys = mesh.shape[0] if batched else 1
        if batched and cit.shape[0] == 1 and nsys > 1:
            cit = cit.expand(nsys, 3, 3)
        g = gout.contiguous()
        q = charges.to(positions.dtype)
        nx, ny, nz = mesh.shape[-4:-1]
        ci = 6 if batched else 5
        gq = gmesh = gpos = gcit = None
        chan = [mesh[..., c].contiguous() for c in range(3)]
        if need[1]:
            per = [(torch.ops.alchemiops._batch_spline_gather(positions, chan[c], batch_idx, cell, ctx.order, cell_inv_t) if batched else
                    torch.ops.alchemiops._spline_gather(positions, chan[c], cell, ctx.order, cell_inv_t)) for c in range(3)]
            gq = (g * torch.stack(per, dim=-1)).sum(-1).to(charges.dtype)
        if need[2]:
            sp = []
            for c in range(3):
                w = (q * g[:, c]).contiguous()
                sp.append(torch.ops.alchemiops._batch_spline_spread(positions, w, batch_idx, cell, nsys, nx, ny, nz, ctx.order, cell_inv_t) if batched else
                          torch.ops.alchemiops._spline_spread(positions, w, cell, nx, ny, nz, ctx.order, cell_inv_t))
            gmesh = torch.stack(sp, dim=-1).to(mesh.dtype)
        cell_i = 4 if batched else 3
        gcell = None
        if need[0] or _n(need, ci) or (cell_inv_t is None and need[cell_i]):
            gpos = torch.zeros_like(positions)
            gc_tot = torch.zeros_like(cit)
            for c in range(3):
                gfrac = frac_grad_op(positions, chan[c] if batched else chan[c].unsqueeze(0), batch_idx, cit, ctx.order)
                gp, gc = _coordinate_grads((q * g[:, c]).detach(), gfrac, positions.detach(), cit.detach(), batch_idx)
                gpos = gpos + gp
                gc_tot = gc_tot + gc
            gcit = _like_cell_inv_t(gc_tot if (cell_inv_t is None or cell_inv_t.reshape(-1, 3, 3).shape[0] == gc_tot.shape[0]) else gc_tot.sum(0, keepdim=True), cell_inv_t)
            gcell = _cell_grad_without_cit(gc_tot, cit, cell, cell_inv_t, need[cell_i])
        if batched:
            return _fit(need, (gpos if need[0] else None, gq, gmesh, None, gcell, None, gcit if _n(need, 6) else None))
        return _fit(need, (gpos if need[0] else None, gq, gmesh, gcell, None, gcit if _n(need, 5) else None))
    return backward


spline_gather_vec3_op = _op("_spline_gather_vec3", _spline_gather_vec3, _vec3_fake, _vec3_backward(False), _vec3_setup(False))
batch_spline_gather_vec3_op = _op("_batch_spline_gather_vec3", _batch_spline_gather_vec3, _vec3_fake, _vec3_backward(True), _vec3_setup(True))


# ---- gather_gradient: F_i = -q_i sum_g mesh[g] grad_r w_i(g) (spline.py:1750-1840 / :2110-2200) -----------------------------------------
def _gather_gradient_impl(positions, charges, mesh, batch_idx, cit, order):
    gfrac = _gather_impl(positions, mesh, batch_idx, cit, order, grad=True)  # (forward implementation of an op: a raw launch is fine here)
    c = cit.detach().to(positions.dtype)
    cit_i = c[batch_idx.long()] if batch_idx is not None else c[0].expand(positions.shape[0], 3, 3)
    return -charges.detach().to(positions.dtype).unsqueeze(-1) * torch.einsum("na,nab->nb", gfrac, cit_i)


def _spline_gather_gradient(positions: Tensor, charges: Tensor, mesh: Tensor, cell: Tensor, spline_order: int,
                            cell_inv_t: Optional[Tensor] = None) -> Tensor:
    return _gather_gradient_impl(positions, charges, mesh.unsqueeze(0), None, _cit(cell, cell_inv_t, positions.dtype), spline_order)


def _batch_spline_gather_gradient(positions: Tensor, charges: Tensor, mesh: Tensor, batch_idx: Tensor, cell: Tensor, spline_order: int,
                                  cell_inv_t: Optional[Tensor] = None) -> Tensor:
    cit = _cit(cell, cell_inv_t, positions.dtype)
    if cit.shape[0] == 1 and mesh.shape[0] > 1:
        cit = cit.expand(mesh.shape[0], 3, 3)
    return _gather_gradient_impl(positions, charges, mesh, batch_idx, cit, spline_order)


def _no_second_order(op, what):
    def backward(ctx, *grads):
        raise NotImplementedError(_SECOND_ORDER.format(op=op, what=what))
    return backward


def _noop_setup(ctx, inputs, output):
    return None


# The adjoint of gather_gradient needs second derivatives of the spline weights: two more raw launches, ops for the same reason as
# `spline_gather_frac_grad`.
def _hess_dot(positions: Tensor, mesh: Tensor, batch_idx: Optional[Tensor], cell_inv_t: Tensor, vec: Tensor, spline_order: int) -> Tensor:
    """out_i[b] = sum_g mesh[g] sum_a vec_i[a] d^2 W_i(g) / dfrac_a dfrac_b  (`mi_spline_gather_hess_dot`); mesh is [B,nx,ny,nz]."""
    pos = positions.detach().contiguous()
    m, c, v = (t.detach().to(pos.dtype).contiguous() for t in (mesh, cell_inv_t, vec))
    bi = None if batch_idx is None else C.i32(batch_idx)
    nx, ny, nz = m.shape[-3:]
    out = torch.empty((pos.shape[0], 3), dtype=pos.dtype, device=pos.device)
    rc = C.lib().mi_spline_gather_hess_dot(C.ptr(pos), C.ptr(m), C.ptr(bi), C.ptr(c), C.ptr(v), pos.shape[0], c.shape[0], nx, ny, nz, C.spline_order_arg(spline_order),
                                           C.dtype_code(pos.dtype), C.ptr(out), C.stream_of(pos))
    C.check(rc, "mi_spline_gather_hess_dot")
    return out


def _spread_grad(positions: Tensor, vec: Tensor, batch_idx: Optional[Tensor], cell_inv_t: Tensor, num_systems: int, mesh_nx: int, mesh_ny: int,
                 mesh_nz: int, spline_order: int) -> Tensor:
    """mesh[s][g] = sum_{i in s} sum_a vec_i[a] d W_i(g) / dfrac_a  (`mi_spline_spread_grad`) -> [B,nx,ny,nz]."""
    pos = positions.detach().contiguous()
    c, v = (t.detach().to(pos.dtype).contiguous() for t in (cell_inv_t, vec))
    bi = None if batch_idx is None else C.i32(batch_idx)
    mesh = torch.empty((num_systems, mesh_nx, mesh_ny, mesh_nz), dtype=pos.dtype, device=pos.device)
    rc = C.lib().mi_spline_spread_grad(C.ptr(pos), C.ptr(v), C.ptr(bi), C.ptr(c), pos.shape[0], int(num_systems), mesh_nx, mesh_ny, mesh_nz,
                                       C.spline_order_arg(spline_order), C.dtype_code(pos.dtype), C.ptr(mesh), C.stream_of(pos))
    C.check(rc, "mi_spline_spread_grad")
    return mesh


hess_dot_op = torch.library.custom_op("nvalchemiops::spline_gather_hess_dot", _hess_dot, mutates_args=())
hess_dot_op.register_fake(lambda positions, mesh, batch_idx, cell_inv_t, vec, spline_order: positions.new_empty((positions.shape[0], 3)))
hess_dot_op.register_autograd(_no_second_order("nvalchemiops::spline_gather_hess_dot", "second-derivative gather"), setup_context=_noop_setup)
spread_grad_op = torch.library.custom_op("nvalchemiops::spline_spread_frac_grad", _spread_grad, mutates_args=())
spread_grad_op.register_fake(lambda positions, vec, batch_idx, cell_inv_t, num_systems, mesh_nx, mesh_ny, mesh_nz, spline_order:
                             positions.new_empty((num_systems, mesh_nx, mesh_ny, mesh_nz)))
spread_grad_op.register_autograd(_no_second_order("nvalchemiops::spline_spread_frac_grad", "gradient-weight spread"), setup_context=_noop_setup)


def _gather_gradient_setup(batched):
    def setup(ctx, inputs, output):
        if batched:
            positions, charges, mesh, batch_idx, cell, order, cell_inv_t = inputs
        else:
            positions, charges, mesh, cell, order, cell_inv_t = inputs
            batch_idx = None
        ctx.save_for_backward(positions, charges, mesh, cell, cell_inv_t, batch_idx)
        ctx.order = order
    return setup


def _gather_gradient_backward(batched):
    """Adjoint of F_i[b] = -q_i sum_a G_i[a] cit[a][b], G_i[a] = sum_g mesh[g] dW_i(g)/dfrac_a, for L = sum_i gF_i . F_i.  With
    v_i[a] = -q_i sum_b cit[a][b] gF_i[b]  (so L = sum_i v_i . G_i at fixed v):
      dL/dmesh = spread of v with the gradient weights;  dL/dq_i = -G_i . (cit gF_i);
      dL/dfrac_i = H_i v_i (second-derivative gather)  ->  dL/dr_i = cit^T dL/dfrac_i,  dL/dcit += dL/dfrac_i (x) r_i;
      dL/dcit[a][b] += sum_i -q_i G_i[a] gF_i[b]  (the explicit cit in F).
    The reference gets the same from the Warp tape of `_bspline_gather_gradient_kernel` (spline.py:678-755)."""
    def backward(ctx, gout):
        positions, charges, mesh, cell, cell_inv_t, batch_idx = ctx.saved_tensors
        need = ctx.needs_input_grad
        dt = positions.dtype
        cit = _cit(cell, cell_inv_t, dt)
        nsys = mesh.shape[0] if batched else 1
        if batched and cit.shape[0] == 1 and nsys > 1:
            cit = cit.expand(nsys, 3, 3)
        m = (mesh if batched else mesh.unsqueeze(0)).to(dt)
        nx, ny, nz = m.shape[-3:]
        g = gout.to(dt).contiguous()
        q = charges.to(dt)
        pos, c = positions.detach(), cit.detach()
        c_i = c[batch_idx.long()] if batch_idx is not None else c[0].expand(pos.shape[0], 3, 3)
        t = torch.einsum("nab,nb->na", c_i, g)                       # (cit gF)_i
        v = -q.unsqueeze(-1) * t
        ci = 6 if batched else 5
        cell_i = 4 if batched else 3
        want_c = _n(need, ci) or (cell_inv_t is None and need[cell_i])
        gq = gmesh = gpos = gcit = gcell = None
        if need[1] or want_c:
            gfr = frac_grad_op(pos, m, batch_idx, c, ctx.order)      # G_i
        if need[1]:
            gq = -(gfr * t).sum(-1).to(charges.dtype)
        if need[2]:
            gm = spread_grad_op(pos, v, batch_idx, c, nsys, nx, ny, nz, ctx.order)
            gmesh = (gm if batched else gm[0]).to(mesh.dtype)
        if need[0] or want_c:
            dfrac = hess_dot_op(pos, m, batch_idx, c, v, ctx.order)
            gpos, gc = _coordinate_grads(torch.ones_like(q), dfrac, pos, c, batch_idx)
            if want_c:
                direct = (-q).reshape(-1, 1, 1) * gfr.unsqueeze(-1) * g.unsqueeze(-2)
                gc = gc + (direct.sum(0, keepdim=True) if batch_idx is None else torch.zeros_like(c).index_add(0, batch_idx.long(), direct))
                gcit = _like_cell_inv_t(gc if (cell_inv_t is None or cell_inv_t.reshape(-1, 3, 3).shape[0] == gc.shape[0]) else gc.sum(0, keepdim=True), cell_inv_t)
                gcell = _cell_grad_without_cit(gc, cit, cell, cell_inv_t, need[cell_i])
        if batched:
            return _fit(need, (gpos if need[0] else None, gq, gmesh, None, gcell, None, gcit if _n(need, 6) else None))
        return _fit(need, (gpos if need[0] else None, gq, gmesh, gcell, None, gcit if _n(need, 5) else None))
    return backward


spline_gather_gradient_op = _op("_spline_gather_gradient", _spline_gather_gradient, _vec3_fake, _gather_gradient_backward(False),
                                _gather_gradient_setup(False))
batch_spline_gather_gradient_op = _op("_batch_spline_gather_gradient", _batch_spline_gather_gradient, _vec3_fake, _gather_gradient_backward(True),
                                      _gather_gradient_setup(True))


# =====================================================================================================================================
# PME: Green function / structure factor, energy corrections
# =====================================================================================================================================
def _green_sf_impl(k_squared, alpha, volume, nsys, nx, ny, nz, order):
    k2 = k_squared.detach().contiguous()
    dt, dev = k2.dtype, k2.device
    green = torch.empty_like(k2)
    sf2 = torch.empty((nx, ny, nz // 2 + 1), dtype=dt, device=dev)
    al = alpha.detach().to(dt).reshape(-1).contiguous()
    vol = volume.detach().to(dt).reshape(-1).contiguous()
    rc = C.lib().mi_pme_green_sf(C.ptr(k2), C.ptr(al), C.ptr(vol), int(nsys), nx, ny, nz, C.spline_order_arg(order), C.dtype_code(dt), C.ptr(green), C.ptr(sf2),
                                 C.stream_of(k2))
    C.check(rc, "mi_pme_green_sf")
    return green, sf2


def _pme_green_structure_factor(k_squared: Tensor, miller_x: Tensor, miller_y: Tensor, miller_z: Tensor, alpha: Tensor, volume: Tensor,
                                mesh_nx: int, mesh_ny: int, mesh_nz: int, spline_order: int) -> tuple[Tensor, Tensor]:
    return _green_sf_impl(k_squared, alpha, volume, 1, mesh_nx, mesh_ny, mesh_nz, spline_order)


def _batch_pme_green_structure_factor(k_squared: Tensor, miller_x: Tensor, miller_y: Tensor, miller_z: Tensor, alpha: Tensor, volumes: Tensor,
                                      mesh_nx: int, mesh_ny: int, mesh_nz: int, spline_order: int, num_systems: int) -> tuple[Tensor, Tensor]:
    return _green_sf_impl(k_squared, alpha, volumes, num_systems, mesh_nx, mesh_ny, mesh_nz, spline_order)


def _green_fake(k_squared, miller_x, miller_y, miller_z, alpha, volume, mesh_nx, mesh_ny, mesh_nz, spline_order, num_systems=1):
    return torch.empty_like(k_squared), k_squared.new_empty((mesh_nx, mesh_ny, mesh_nz // 2 + 1))


def _green_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[0], inputs[4], inputs[5], output[0])


def _green_backward(ctx, g_green, g_sf2):
    """G = 2 pi exp(-k^2 / 4 a^2) / (k^2 V): dG/dk^2 = -G (1/4a^2 + 1/k^2), dG/da = G k^2 / (2 a^3), dG/dV = -G / V (0 where G is masked)."""
    k2, alpha, volume, green = ctx.saved_tensors
    need = ctx.needs_input_grad
    if g_green is None:
        return (None,) * len(need)
    batched = k2.dim() == 4
    shape = (-1, 1, 1, 1) if batched else ()
    a = alpha.to(k2.dtype).reshape(shape) if batched else alpha.to(k2.dtype).reshape(-1)[0]
    v = volume.to(k2.dtype).reshape(shape) if batched else volume.to(k2.dtype).reshape(-1)[0]
    gg = g_green * green
    # G is masked to 0 where k^2 is (near) zero: keep 0 there instead of 0 * inf = NaN when a caller-supplied k_squared holds an exact zero
    gk2 = torch.where(green != 0, -gg * (0.25 / (a * a) + 1.0 / torch.where(green != 0, k2, torch.ones_like(k2))), torch.zeros_like(gg)) if need[0] else None
    ga = gg * k2 / (2.0 * a * a * a)
    gv = -gg / v
    red = (1, 2, 3) if batched else None
    galpha = (ga.sum(red) if batched else ga.sum()).reshape(alpha.shape).to(alpha.dtype) if need[4] else None
    gvol = (gv.sum(red) if batched else gv.sum()).reshape(volume.shape).to(volume.dtype) if need[5] else None
    return (gk2, None, None, None, galpha, gvol) + (None,) * (len(need) - 6)


pme_green_structure_factor_op = _op("_pme_green_structure_factor", _pme_green_structure_factor, _green_fake, _green_backward, _green_setup)
batch_pme_green_structure_factor_op = _op("_batch_pme_green_structure_factor", _batch_pme_green_structure_factor, _green_fake, _green_backward,
                                          _green_setup)


def _corrections_impl(raw, charges, batch_idx, volume, alpha, total_charge, want_cg):
    rawc = raw.detach().contiguous()
    dt = rawc.dtype
    q = charges.detach().to(dt).contiguous()
    bi = None if batch_idx is None else C.i32(batch_idx)
    vol = volume.detach().to(dt).reshape(-1).contiguous()
    al = alpha.detach().to(dt).reshape(-1).contiguous()
    qt = total_charge.detach().to(dt).reshape(-1).contiguous()
    e = torch.empty_like(rawc)
    cg = torch.empty_like(rawc) if want_cg else None
    rc = C.lib().mi_pme_corrections(C.ptr(rawc), C.ptr(q), C.ptr(bi), C.ptr(vol), C.ptr(al), C.ptr(qt), rawc.shape[0], C.dtype_code(dt), C.ptr(e),
                                    C.ptr(cg), C.stream_of(rawc))
    C.check(rc, "mi_pme_corrections")
    return (e, cg) if want_cg else e


def _pme_energy_corrections(raw_energies: Tensor, charges: Tensor, volume: Tensor, alpha: Tensor, total_charge: Tensor) -> Tensor:
    return _corrections_impl(raw_energies, charges, None, volume, alpha, total_charge, False)


def _batch_pme_energy_corrections(raw_energies: Tensor, charges: Tensor, batch_idx: Tensor, volumes: Tensor, alpha: Tensor,
                                  total_charges: Tensor) -> Tensor:
    return _corrections_impl(raw_energies, charges, batch_idx, volumes, alpha, total_charges, False)


def _pme_energy_corrections_with_charge_grad(raw_energies: Tensor, charges: Tensor, volume: Tensor, alpha: Tensor,
                                             total_charge: Tensor) -> tuple[Tensor, Tensor]:
    return _corrections_impl(raw_energies, charges, None, volume, alpha, total_charge, True)


def _batch_pme_energy_corrections_with_charge_grad(raw_energies: Tensor, charges: Tensor, batch_idx: Tensor, volumes: Tensor, alpha: Tensor,
                                                   total_charges: Tensor) -> tuple[Tensor, Tensor]:
    return _corrections_impl(raw_energies, charges, batch_idx, volumes, alpha, total_charges, True)


def _corr_fake(raw_energies, *rest):
    return torch.empty_like(raw_energies)


def _corr_cg_fake(raw_energies, *rest):
    return torch.empty_like(raw_energies), torch.empty_like(raw_energies)


def _corr_setup(batched):
    def setup(ctx, inputs, output):
        if batched:
            raw, q, bi, vol, al, qt = inputs
        else:
            raw, q, vol, al, qt = inputs
            bi = None
        ctx.save_for_backward(raw, q, vol, al, qt, bi)
    return setup


def _corr_backward(batched, with_cg):
    """E_i = q raw - q^2 a/sqrt(pi) - q pi Q/(2 a^2 V);  cg_i = 2 raw - 2 a q/sqrt(pi) - pi Q/(a^2 V)   (pme_kernels.py:340-657)."""
    rp = math.sqrt(math.pi)

    def backward(ctx, g_e, g_cg=None):
        raw, q, vol, al, qt, bi = ctx.saved_tensors
        dt = raw.dtype
        sel = bi.long() if bi is not None else torch.zeros(raw.shape[0], dtype=torch.long, device=raw.device)
        nsys = vol.reshape(-1).shape[0]
        a, v, qq = al.to(dt).reshape(-1)[sel], vol.to(dt).reshape(-1)[sel], qt.to(dt).reshape(-1)[sel]
        c = q.to(dt)
        ge = torch.zeros_like(raw) if g_e is None else g_e
        gc = torch.zeros_like(raw) if (not with_cg or g_cg is None) else g_cg
        g_raw = ge * c + 2.0 * gc
        g_q = ge * (raw - 2.0 * c * a / rp - math.pi * qq / (2.0 * a * a * v)) + gc * (-2.0 * a / rp)
        per_v = ge * c * math.pi * qq / (2.0 * a * a * v * v) + gc * math.pi * qq / (a * a * v * v)
        per_a = ge * (-c * c / rp + c * math.pi * qq / (a * a * a * v)) + gc * (-2.0 * c / rp + 2.0 * math.pi * qq / (a * a * a * v))
        per_q = ge * (-c * math.pi / (2.0 * a * a * v)) + gc * (-math.pi / (a * a * v))
        seg = lambda x, like: seg_sum(x, bi, nsys).reshape(like.shape).to(like.dtype)  # noqa: E731
        out = (g_raw, g_q.to(q.dtype)) + ((None,) if batched else ()) + (seg(per_v, vol), seg(per_a, al), seg(per_q, qt))
        return out
    return backward


pme_energy_corrections_op = _op("_pme_energy_corrections", _pme_energy_corrections, _corr_fake, _corr_backward(False, False), _corr_setup(False))
batch_pme_energy_corrections_op = _op("_batch_pme_energy_corrections", _batch_pme_energy_corrections, _corr_fake, _corr_backward(True, False),
                                      _corr_setup(True))
pme_energy_corrections_with_charge_grad_op = _op("_pme_energy_corrections_with_charge_grad", _pme_energy_corrections_with_charge_grad,
                                                 _corr_cg_fake, _corr_backward(False, True), _corr_setup(False))
batch_pme_energy_corrections_with_charge_grad_op = _op("_batch_pme_energy_corrections_with_charge_grad",
                                                       _batch_pme_energy_corrections_with_charge_grad, _corr_cg_fake,
                                                       _corr_backward(True, True), _corr_setup(True))


# =====================================================================================================================================
# Ewald real space: 12 ops = {single, batch} x {list, matrix} x {energy, +forces, +forces +charge_grad}
# =====================================================================================================================================
def _real_impl(positions, charges, cell, alpha, batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts,
               mask_value, forces, cgrad):
    from nvalchemiops.interactions.electrostatics.ewald import _real_space_inputs, _real_space_launch

    n, dt, dev = positions.shape[0], positions.dtype, positions.device
    p = _real_space_inputs(positions, charges, cell, alpha, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts,
                           batch_idx)
    if n == 0 or p["n_entries"] == 0:
        e, f, cg = torch.zeros(n, dtype=dt, device=dev), torch.zeros((n, 3), dtype=dt, device=dev), torch.zeros(n, dtype=dt, device=dev)
    else:
        e64, f, cg64 = _real_space_launch(p, mask_value, forces, cgrad)
        e, cg = e64.to(dt), (cg64.to(dt) if cg64 is not None else None)
    return (e,) + ((f,) if forces else ()) + ((cg,) if cgrad else ())


def _real_bwd(positions: Tensor, charges: Tensor, cell: Tensor, alpha: Tensor, batch_idx: Optional[Tensor], neighbor_list: Optional[Tensor],
              neighbor_ptr: Optional[Tensor], neighbor_shifts: Optional[Tensor], neighbor_matrix: Optional[Tensor],
              neighbor_matrix_shifts: Optional[Tensor], mask_value: int, grad_energies: Tensor) -> tuple[Tensor, Tensor, Tensor, Tensor]:
    """(dL/dpositions, dL/dcharges, dL/dcell [B,3,3] f64, dL/dalpha [B] f64) for L = sum_i g_i E_i: `mi_ewald_real_bwd`."""
    from nvalchemiops.interactions.electrostatics.ewald import _real_space_inputs

    p = _real_space_inputs(positions, charges, cell, alpha, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts,
                           batch_idx)
    pos, dt, dev = p["pos"], positions.dtype, positions.device
    n = pos.shape[0]
    gpos = torch.zeros((n, 3), dtype=dt, device=dev)
    gq = torch.zeros(n, dtype=dt, device=dev)
    gcell = torch.zeros(p["cells"].shape, dtype=torch.float64, device=dev)
    galpha = torch.zeros(p["alpha"].shape, dtype=torch.float64, device=dev)
    if n == 0 or p["n_entries"] == 0:
        return gpos, gq, gcell, galpha
    g = grad_energies.detach().to(dt).contiguous()
    nsys = int(p["cells"].shape[0])
    L = C.lib()
    L.mi_ewald_real_bwd_scratch_bytes.restype = ctypes.c_size_t
    sbytes = int(L.mi_ewald_real_bwd_scratch_bytes(nsys))
    sym = torch.empty(sbytes // 8, dtype=torch.int64, device=dev)
    rc = L.mi_ewald_real_bwd(C.ptr(pos), C.ptr(p["q"]), C.ptr(p["cells"]), C.ptr(p["alpha"]), C.ptr(p["bi"]), n, nsys, C.dtype_code(dt), C.ptr(p["idx"]),
                             C.ptr(p["sh"]), C.ptr(p["nptr"]), int(p["m"]), int(mask_value), C.ptr(g), C.ptr(gpos), C.ptr(gq), C.ptr(gcell),
                             C.ptr(galpha), C.ptr(sym), ctypes.c_size_t(sbytes), C.stream_of(pos))
    C.check(rc, "mi_ewald_real_bwd")
    return gpos, gq, gcell, galpha


def _real_bwd_fake(positions, charges, cell, alpha, batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts,
                   mask_value, grad_energies):
    nsys = cell.reshape(-1, 3, 3).shape[0]
    n = positions.shape[0]
    return (positions.new_empty((n, 3)), positions.new_empty((n,)), positions.new_empty((nsys, 3, 3), dtype=torch.float64),
            positions.new_empty((max(nsys, alpha.reshape(-1).shape[0]),), dtype=torch.float64))


real_bwd_op = torch.library.custom_op("nvalchemiops::ewald_real_space_backward", _real_bwd, mutates_args=())
real_bwd_op.register_fake(_real_bwd_fake)
real_bwd_op.register_autograd(lambda ctx, *g: (_ for _ in ()).throw(NotImplementedError(_SECOND_ORDER.format(
    op="nvalchemiops::ewald_real_space_backward", what="gradient"))), setup_context=lambda ctx, inputs, output: None)


def _real_forces_bwd(positions: Tensor, charges: Tensor, cell: Tensor, alpha: Tensor, batch_idx: Optional[Tensor], neighbor_list: Optional[Tensor],
                     neighbor_ptr: Optional[Tensor], neighbor_shifts: Optional[Tensor], neighbor_matrix: Optional[Tensor],
                     neighbor_matrix_shifts: Optional[Tensor], mask_value: int, grad_forces: Optional[Tensor],
                     grad_charge_grads: Optional[Tensor]) -> tuple[Tensor, Tensor, Tensor, Tensor]:
    """Float64 (dL/dpositions, dL/dcharges, dL/dcell [B,3,3], dL/dalpha [B]) for L = sum_k grad_forces_k . F_k + sum_k grad_charge_grads_k cg_k:
    `mi_ewald_real_forces_bwd` (second derivatives of the pair sum, entry-wise scatter); either weight may be None."""
    from nvalchemiops.interactions.electrostatics.ewald import _real_space_inputs

    p = _real_space_inputs(positions, charges, cell, alpha, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts,
                           batch_idx)
    pos, dt, dev = p["pos"], positions.dtype, positions.device
    n, nsys = pos.shape[0], p["cells"].shape[0]
    f64 = dict(dtype=torch.float64, device=dev)
    gpos, gq = torch.zeros((n, 3), **f64), torch.zeros(n, **f64)
    gcell, galpha = torch.zeros((nsys, 3, 3), **f64), torch.zeros(p["alpha"].shape[0], **f64)
    if n == 0 or p["n_entries"] == 0:
        return gpos, gq, gcell, galpha
    g = None if grad_forces is None else grad_forces.detach().to(dt).contiguous()
    gc = None if grad_charge_grads is None else grad_charge_grads.detach().to(dt).contiguous()
    if g is None and gc is None:
        return gpos, gq, gcell, galpha
    L = C.lib()
    L.mi_ewald_real_bwd_scratch_bytes.restype = ctypes.c_size_t
    sbytes = int(L.mi_ewald_real_bwd_scratch_bytes(int(nsys)))
    scratch = torch.empty(sbytes // 8, dtype=torch.int64, device=dev)
    rc = L.mi_ewald_real_forces_bwd(C.ptr(pos), C.ptr(p["q"]), C.ptr(p["cells"]), C.ptr(p["alpha"]), C.ptr(p["bi"]), n, nsys, C.dtype_code(dt),
                                    C.ptr(p["idx"]), C.ptr(p["sh"]), C.ptr(p["nptr"]), int(p["m"]), int(mask_value), C.ptr(g), C.ptr(gc),
                                    C.ptr(gpos), C.ptr(gq), C.ptr(gcell), C.ptr(galpha), C.ptr(scratch), ctypes.c_size_t(sbytes), C.stream_of(pos))
    C.check(rc, "mi_ewald_real_forces_bwd")
    return gpos, gq, gcell, galpha


def _real_forces_bwd_fake(positions, charges, cell, alpha, batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix,
                          neighbor_matrix_shifts, mask_value, grad_forces, grad_charge_grads):
    nsys = cell.reshape(-1, 3, 3).shape[0]
    n = positions.shape[0]
    f64 = dict(dtype=torch.float64)
    return (positions.new_empty((n, 3), **f64), positions.new_empty((n,), **f64), positions.new_empty((nsys, 3, 3), **f64),
            positions.new_empty((max(nsys, alpha.reshape(-1).shape[0]),), **f64))


real_forces_bwd_op = torch.library.custom_op("nvalchemiops::ewald_real_space_forces_backward", _real_forces_bwd, mutates_args=())
real_forces_bwd_op.register_fake(_real_forces_bwd_fake)
real_forces_bwd_op.register_autograd(lambda ctx, *g: (_ for _ in ()).throw(NotImplementedError(
    "nvalchemiops::ewald_real_space_forces_backward: third derivatives of the pair sum are not provided")), setup_context=lambda ctx, inputs, output: None)


def _real_setup(fmt, batched):
    def setup(ctx, inputs, output):
        positions, charges, cell, alpha = inputs[:4]
        rest = list(inputs[4:])
        batch_idx = rest.pop(0) if batched else None
        if fmt == "list":
            nl, nptr, nsh = rest
            ctx.save_for_backward(positions, charges, cell, alpha, batch_idx, nl, nptr, nsh)
            ctx.mask = 0
        else:
            nm, nmsh, mask = rest
            ctx.save_for_backward(positions, charges, cell, alpha, batch_idx, nm, nmsh)
            ctx.mask = mask
        ctx.fmt = fmt
        ctx.set_materialize_grads(False)
    return setup


def _real_backward(name, fmt, batched, n_out):
    def backward(ctx, *grads):
        # outputs: energies [, forces [, charge_gradients]]: all differentiable (first / second derivatives of the pair sum, two adjoint kernels)
        need = ctx.needs_input_grad
        n_in = len(need)
        g_e = grads[0]
        g_f = grads[1] if n_out >= 2 else None
        g_c = grads[2] if n_out >= 3 else None
        if g_e is None and g_f is None and g_c is None:
            return (None,) * n_in
        saved = ctx.saved_tensors
        positions, charges, cell, alpha, batch_idx = saved[:5]
        lists = (saved[5], saved[6], saved[7], None, None) if fmt == "list" else (None, None, None, saved[5], saved[6])
        gpos = gq = gcell = galpha = None
        if g_e is not None:
            gpos, gq, gcell, galpha = real_bwd_op(positions, charges, cell, alpha, batch_idx, *lists, int(ctx.mask), g_e)
            gpos, gq = gpos.double(), gq.double()
        if g_f is not None or g_c is not None:
            fp, fq, fc, fa = real_forces_bwd_op(positions, charges, cell, alpha, batch_idx, *lists, int(ctx.mask), g_f, g_c)
            gpos = fp if gpos is None else gpos + fp
            gq = fq if gq is None else gq + fq
            gcell = fc if gcell is None else gcell + fc
            galpha = fa if galpha is None else galpha + fa
        ga = None
        if need[3]:
            ga = (galpha.sum() if alpha.numel() == 1 and galpha.numel() > 1 else galpha[: alpha.numel()]).reshape(alpha.shape).to(alpha.dtype)
        return (gpos.to(positions.dtype) if need[0] else None, gq.to(charges.dtype) if need[1] else None,
                gcell.reshape(cell.shape).to(cell.dtype) if need[2] else None, ga) + (None,) * (n_in - 4)
    return backward


def _make_real_op(name, fmt, batched, forces, cgrad):
    n_out = 1 + int(forces) + int(cgrad)
    ret = "Tensor" if n_out == 1 else "tuple[" + ", ".join(["Tensor"] * n_out) + "]"
    args = "positions: Tensor, charges: Tensor, cell: Tensor, alpha: Tensor, " + ("batch_idx: Tensor, " if batched else "")
    args += ("neighbor_list: Tensor, neighbor_ptr: Tensor, neighbor_shifts: Tensor" if fmt == "list" else
             "neighbor_matrix: Tensor, neighbor_matrix_shifts: Tensor, mask_value: int")
    call = ("neighbor_list, neighbor_ptr, neighbor_shifts, None, None, 0" if fmt == "list" else "None, None, None, neighbor_matrix, neighbor_matrix_shifts, mask_value")
    src = (f"def {name}({args}) -> {ret}:\n"
           f"    out = _real_impl(positions, charges, cell, alpha, {'batch_idx' if batched else 'None'}, {call}, {forces}, {cgrad})\n"
           f"    return out[0] if len(out) == 1 else out\n")
    scope = {"_real_impl": _real_impl, "Tensor": Tensor}
    exec(src, scope)  # the op schema is inferred from the annotated signature, which must carry the reference's argument names

    def fake(positions, *rest):
        n = positions.shape[0]
        outs = (positions.new_empty((n,)),) + ((positions.new_empty((n, 3)),) if forces else ()) + ((positions.new_empty((n,)),) if cgrad else ())
        return outs[0] if n_out == 1 else outs
    return _op(name, scope[name], fake, _real_backward(name, fmt, batched, n_out), _real_setup(fmt, batched))


REAL_OPS = {}
for _b in (False, True):
    for _fmt in ("list", "matrix"):
        for _f, _c, _suffix in ((False, False, "energy"), (True, False, "energy_forces"), (True, True, "energy_forces_charge_grad")):
            _name = ("_batch" if _b else "") + "_ewald_real_space_" + _suffix + ("_matrix" if _fmt == "matrix" else "")
            REAL_OPS[(_b, _fmt, _f, _c)] = _make_real_op(_name, _fmt, _b, _f, _c)


def real_space_op(batched: bool, fmt: str, forces: bool, cgrad: bool):
    """The registered op for a configuration; (forces=False, cgrad=True) has no op of its own in the reference either (it runs the
    three-output op and drops the forces, ewald.py:2590-2620)."""
    return REAL_OPS[(batched, fmt, forces or cgrad, cgrad)]



# =====================================================================================================================================
# Ewald reciprocal space over explicit k-vectors: 6 ops = {single, batch} x {energy, +forces, +forces +charge_grad}
# =====================================================================================================================================
def _recip_bwd(positions: Tensor, charges: Tensor, cell: Tensor, k_vectors: Tensor, alpha: Tensor, batch_idx: Optional[Tensor],
               grad_energies: Tensor, need: int) -> tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """Float64 (dL/dpositions, dL/dcharges, dL/dcell [B,3,3], dL/dk_vectors [B,K,3], dL/dalpha [B]) for L = sum_i g_i E_i; `need` is a bit
    mask (1 atoms, 2 cell, 4 k_vectors, 8 alpha) of the gradients wanted, the others come back as zeros.  The cell enters through the
    volume only (k_vectors are an independent input): dL/dcell = dL/dV |det cell| cell^-T."""
    from nvalchemiops.interactions.electrostatics.ewald import _recip_adjoint, _recip_inputs

    p = _recip_inputs(positions, charges, cell, k_vectors, alpha, batch_idx)
    n, nsys, nk, dev = positions.shape[0], p["n_sys"], p["n_k"], positions.device
    f64 = dict(dtype=torch.float64, device=dev)
    if n == 0:
        return torch.zeros((n, 3), **f64), torch.zeros(n, **f64), torch.zeros((nsys, 3, 3), **f64), torch.zeros((nsys, nk, 3), **f64), torch.zeros(nsys, **f64)
    gpos, gq, gkv, gal, gvol = _recip_adjoint(p, grad_energies, bool(need & 1), bool(need & 4), bool(need & 8), bool(need & 2))
    gcell = None
    if gvol is not None:
        c64 = p["cells"].to(torch.float64)
        gcell = (gvol * torch.abs(torch.linalg.det(c64))).reshape(-1, 1, 1) * torch.linalg.inv(c64).transpose(-1, -2)
    return (gpos if gpos is not None else torch.zeros((n, 3), **f64), gq if gq is not None else torch.zeros(n, **f64),
            gcell if gcell is not None else torch.zeros((nsys, 3, 3), **f64), gkv if gkv is not None else torch.zeros((nsys, nk, 3), **f64),
            gal if gal is not None else torch.zeros(nsys, **f64))


def _recip_bwd_fake(positions, charges, cell, k_vectors, alpha, batch_idx, grad_energies, need):
    nsys = cell.reshape(-1, 3, 3).shape[0]
    n, nk = positions.shape[0], k_vectors.shape[-2]
    f64 = dict(dtype=torch.float64)
    return (positions.new_empty((n, 3), **f64), positions.new_empty((n,), **f64), positions.new_empty((nsys, 3, 3), **f64),
            positions.new_empty((nsys, nk, 3), **f64), positions.new_empty((nsys,), **f64))


recip_bwd_op = torch.library.custom_op("nvalchemiops::ewald_reciprocal_space_backward", _recip_bwd, mutates_args=())
recip_bwd_op.register_fake(_recip_bwd_fake)
recip_bwd_op.register_autograd(lambda ctx, *g: (_ for _ in ()).throw(NotImplementedError(_SECOND_ORDER.format(
    op="nvalchemiops::ewald_reciprocal_space_backward", what="gradient"))), setup_context=lambda ctx, inputs, output: None)


def _recip_out_bwd(positions: Tensor, charges: Tensor, cell: Tensor, k_vectors: Tensor, alpha: Tensor, batch_idx: Optional[Tensor],
                   grad_forces: Optional[Tensor], grad_charge_grads: Optional[Tensor], need: int) -> tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """Float64 (dL/dpositions, dL/dcharges, dL/dcell [B,3,3], dL/dalpha [B], dL/dk_vectors [B,K,3]) for L = sum_i grad_forces_i . F_i +
    sum_i grad_charge_grads_i cg_i of the explicit-k reciprocal sum (`_recip_outputs_adjoint`); `need` bits: 2 cell (through the volume),
    4 k_vectors, 8 alpha."""
    from nvalchemiops.interactions.electrostatics.ewald import _recip_inputs, _recip_outputs_adjoint

    p = _recip_inputs(positions, charges, cell, k_vectors, alpha, batch_idx)
    n, nsys, nk, dev = positions.shape[0], p["n_sys"], p["n_k"], positions.device
    f64 = dict(dtype=torch.float64, device=dev)
    zeros = (torch.zeros((n, 3), **f64), torch.zeros(n, **f64), torch.zeros((nsys, 3, 3), **f64), torch.zeros(nsys, **f64),
             torch.zeros((nsys, nk, 3), **f64))
    if n == 0 or nk == 0 or (grad_forces is None and grad_charge_grads is None):
        return zeros
    gpos, gq, gal, gvol, gkv = _recip_outputs_adjoint(p, grad_forces, grad_charge_grads, bool(need & 8), bool(need & 2), bool(need & 4))
    gcell = zeros[2]
    if gvol is not None:
        c64 = p["cells"].to(torch.float64)
        gcell = (gvol * torch.abs(torch.linalg.det(c64))).reshape(-1, 1, 1) * torch.linalg.inv(c64).transpose(-1, -2)
    return gpos, gq, gcell, gal if gal is not None else zeros[3], gkv if gkv is not None else zeros[4]


def _recip_out_bwd_fake(positions, charges, cell, k_vectors, alpha, batch_idx, grad_forces, grad_charge_grads, need):
    nsys = cell.reshape(-1, 3, 3).shape[0]
    n = positions.shape[0]
    f64 = dict(dtype=torch.float64)
    return (positions.new_empty((n, 3), **f64), positions.new_empty((n,), **f64), positions.new_empty((nsys, 3, 3), **f64),
            positions.new_empty((nsys,), **f64), positions.new_empty((nsys, k_vectors.shape[-2], 3), **f64))


recip_out_bwd_op = torch.library.custom_op("nvalchemiops::ewald_reciprocal_space_outputs_backward", _recip_out_bwd, mutates_args=())
recip_out_bwd_op.register_fake(_recip_out_bwd_fake)
recip_out_bwd_op.register_autograd(lambda ctx, *g: (_ for _ in ()).throw(NotImplementedError(
    "nvalchemiops::ewald_reciprocal_space_outputs_backward: third derivatives of the reciprocal sum are not provided")),
    setup_context=lambda ctx, inputs, output: None)


def _recip_setup(ctx, inputs, output):
    ctx.save_for_backward(*inputs)
    ctx.set_materialize_grads(False)


def _recip_backward(name, n_out):
    def backward(ctx, *grads):
        need = ctx.needs_input_grad
        g_e = grads[0]
        g_f = grads[1] if n_out >= 2 else None
        g_c = grads[2] if n_out >= 3 else None
        if g_e is None and g_f is None and g_c is None:
            return (None,) * len(need)
        positions, charges, cell, k_vectors, alpha, *rest = ctx.saved_tensors
        if k_vectors.shape[-2] == 0 and (rest or n_out > 1):  # the forward returned constant zeros (see `_recip_forward`)
            return tuple(torch.zeros_like(t) if w else None for t, w in zip((positions, charges, cell, k_vectors, alpha), need[:5])) + (None,) * (len(need) - 5)
        bi = rest[0] if rest else None
        gpos = gq = gcell = gkv = gal = None
        if g_e is not None:
            mask = (1 if need[0] or need[1] else 0) | (2 if need[2] else 0) | (4 if need[3] else 0) | (8 if need[4] else 0)
            gpos, gq, gcell, gkv, gal = recip_bwd_op(positions, charges, cell, k_vectors, alpha, bi, g_e, mask)
        if g_f is not None or g_c is not None:
            fp, fq, fc, fa, fk = recip_out_bwd_op(positions, charges, cell, k_vectors, alpha, bi, g_f, g_c,
                                                  (2 if need[2] else 0) | (4 if need[3] else 0) | (8 if need[4] else 0))
            gpos, gq, gcell, gal, gkv = (fp, fq, fc, fa, fk) if gpos is None else (gpos + fp, gq + fq, gcell + fc, gal + fa, gkv + fk)
        if need[3] and gkv.shape != k_vectors.shape:  # one [K,3] set shared by all systems (or a [1,K,3] one)
            gkv = gkv.sum(0).reshape(k_vectors.shape)
        if need[4]:
            gal = (gal.sum() if alpha.numel() == 1 and gal.numel() > 1 else gal[: alpha.numel()]).reshape(alpha.shape)
        return (gpos.to(positions.dtype) if need[0] else None, gq.to(charges.dtype) if need[1] else None,
                gcell.reshape(cell.shape).to(cell.dtype) if need[2] else None, gkv.to(k_vectors.dtype) if need[3] else None,
                gal.to(alpha.dtype) if need[4] else None) + (None,) * (len(need) - 5)
    return backward


def _make_recip_op(name, batched, forces, cgrad):
    from nvalchemiops.interactions.electrostatics.ewald import _recip_forward

    n_out = 1 + int(forces) + int(cgrad)
    ret = "Tensor" if n_out == 1 else "tuple[" + ", ".join(["Tensor"] * n_out) + "]"
    args = "positions: Tensor, charges: Tensor, cell: Tensor, k_vectors: Tensor, alpha: Tensor" + (", batch_idx: Tensor" if batched else "")
    src = (f"def {name}({args}) -> {ret}:\n"
           f"    out = _recip_forward(positions, charges, cell, k_vectors, alpha, {'batch_idx' if batched else 'None'}, {forces}, {cgrad})\n"
           f"    return out[0] if len(out) == 1 else out\n")
    scope = {"_recip_forward": _recip_forward, "Tensor": Tensor}
    exec(src, scope)  # as for the real-space ops: the schema must carry the reference's argument names (ewald.py:1603-2318)

    def fake(positions, *rest):
        n = positions.shape[0]
        outs = (positions.new_empty((n,)),) + ((positions.new_empty((n, 3)),) if forces else ()) + ((positions.new_empty((n,)),) if cgrad else ())
        return outs[0] if n_out == 1 else outs
    return _op(name, scope[name], fake, _recip_backward(name, n_out), _recip_setup)


RECIPROCAL_OPS = {}
for _b in (False, True):
    for _f, _c, _suffix in ((False, False, "energy"), (True, False, "energy_forces"), (True, True, "energy_forces_charge_grad")):
        RECIPROCAL_OPS[(_b, _f, _c)] = _make_recip_op(("_batch" if _b else "") + "_ewald_reciprocal_space_" + _suffix, _b, _f, _c)


def reciprocal_space_op(batched: bool, forces: bool, cgrad: bool):
    return RECIPROCAL_OPS[(batched, forces or cgrad, cgrad)]


# =====================================================================================================================================
# Cut-off Coulomb: 8 ops = {single, batch} x {list, matrix} x {energy, +forces}, registered as `nvalchemiops::` like the reference's
# (interactions/electrostatics/coulomb.py:716-1330); float64 in and out
# =====================================================================================================================================
def _coulomb_bwd(positions: Tensor, charges: Tensor, cell: Tensor, batch_idx: Optional[Tensor], neighbor_list: Optional[Tensor],
                 neighbor_ptr: Optional[Tensor], neighbor_shifts: Optional[Tensor], neighbor_matrix: Optional[Tensor],
                 neighbor_matrix_shifts: Optional[Tensor], fill_value: int, cutoff: float, alpha: float, with_forces: bool,
                 grad_energies: Tensor) -> tuple[Tensor, Tensor, Tensor]:
    """(dL/dpositions, dL/dcharges, dL/dcell [B,3,3]) for L = sum_i g_i E_i: `mi_coulomb_bwd`.  `with_forces` selects the energy prefactor
    of the op being differentiated (the energy-only matrix kernels carry no 1/2, coulomb.py:340)."""
    from nvalchemiops.interactions.electrostatics import coulomb

    return coulomb._backward(positions, charges, cell, batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix,
                             neighbor_matrix_shifts, fill_value, cutoff, alpha, with_forces, grad_energies)


def _coulomb_bwd_fake(positions, charges, cell, batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts,
                      fill_value, cutoff, alpha, with_forces, grad_energies):
    return torch.empty_like(positions), torch.empty_like(charges), cell.new_empty((cell.reshape(-1, 3, 3).shape[0], 3, 3))


coulomb_bwd_op = torch.library.custom_op("nvalchemiops::coulomb_backward", _coulomb_bwd, mutates_args=())
coulomb_bwd_op.register_fake(_coulomb_bwd_fake)
coulomb_bwd_op.register_autograd(lambda ctx, *g: (_ for _ in ()).throw(NotImplementedError(_SECOND_ORDER.format(
    op="nvalchemiops::coulomb_backward", what="gradient"))), setup_context=lambda ctx, inputs, output: None)


def _coulomb_forces_bwd(positions: Tensor, charges: Tensor, cell: Tensor, batch_idx: Optional[Tensor], neighbor_list: Optional[Tensor],
                        neighbor_ptr: Optional[Tensor], neighbor_shifts: Optional[Tensor], neighbor_matrix: Optional[Tensor],
                        neighbor_matrix_shifts: Optional[Tensor], fill_value: int, cutoff: float, alpha: float,
                        grad_forces: Tensor) -> tuple[Tensor, Tensor, Tensor]:
    """(dL/dpositions, dL/dcharges, dL/dcell [B,3,3]) for L = sum_k g_k . F_k: `mi_coulomb_forces_bwd`."""
    from nvalchemiops.interactions.electrostatics import coulomb

    return coulomb._forces_backward(positions, charges, cell, batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix,
                                    neighbor_matrix_shifts, fill_value, cutoff, alpha, grad_forces)


coulomb_forces_bwd_op = torch.library.custom_op("nvalchemiops::coulomb_forces_backward", _coulomb_forces_bwd, mutates_args=())
coulomb_forces_bwd_op.register_fake(lambda positions, charges, cell, batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix,
                                    neighbor_matrix_shifts, fill_value, cutoff, alpha, grad_forces:
                                    (torch.empty_like(positions), torch.empty_like(charges), cell.new_empty((cell.reshape(-1, 3, 3).shape[0], 3, 3))))
coulomb_forces_bwd_op.register_autograd(lambda ctx, *g: (_ for _ in ()).throw(NotImplementedError(
    "nvalchemiops::coulomb_forces_backward: third derivatives of the pair sum are not provided")), setup_context=lambda ctx, inputs, output: None)


def _coulomb_setup(fmt, batched):
    def setup(ctx, inputs, output):
        positions, charges, cell = inputs[:3]
        rest = list(inputs[3:])
        if fmt == "list":
            nl, nptr, nsh = rest[:3]
            rest = rest[3:]
            lists = (nl, nptr, nsh, None, None)
        else:
            nm, nmsh = rest[:2]
            rest = rest[2:]
            lists = (None, None, None, nm, nmsh)
        batch_idx = rest.pop(0) if batched else None
        ctx.cutoff, ctx.alpha = rest[0], rest[1]
        ctx.fill = rest[2] if fmt == "matrix" else 0
        ctx.save_for_backward(positions, charges, cell, batch_idx, *lists)
        ctx.set_materialize_grads(False)
    return setup


def _coulomb_backward(name, forces):
    def backward(ctx, *grads):
        need = ctx.needs_input_grad
        g_e, g_f = grads[0], (grads[1] if forces else None)
        if g_e is None and g_f is None:
            return (None,) * len(need)
        positions, charges, cell, batch_idx, *lists = ctx.saved_tensors
        gpos = gq = gcell = None
        if g_e is not None:
            gpos, gq, gcell = coulomb_bwd_op(positions, charges, cell, batch_idx, *lists, int(ctx.fill), float(ctx.cutoff), float(ctx.alpha), forces, g_e)
        if g_f is not None:  # the explicit forces are differentiable too (second derivatives of the pair term)
            fp, fq, fc = coulomb_forces_bwd_op(positions, charges, cell, batch_idx, *lists, int(ctx.fill), float(ctx.cutoff), float(ctx.alpha), g_f)
            gpos, gq, gcell = (fp, fq, fc) if gpos is None else (gpos + fp, gq + fq, gcell + fc)
        return (gpos if need[0] else None, gq if need[1] else None, gcell.reshape(cell.shape) if need[2] else None) + (None,) * (len(need) - 3)
    return backward


def _make_coulomb_op(name, fmt, batched, forces):
    from nvalchemiops.interactions.electrostatics import coulomb

    ret = "tuple[Tensor, Tensor]" if forces else "Tensor"
    lists = ("neighbor_list: Tensor, neighbor_ptr: Tensor, neighbor_shifts: Tensor" if fmt == "list" else
             "neighbor_matrix: Tensor, neighbor_matrix_shifts: Tensor")
    args = (f"positions: Tensor, charges: Tensor, cell: Tensor, {lists}, " + ("batch_idx: Tensor, " if batched else "") + "cutoff: float, alpha: float"
            + (", fill_value: int" if fmt == "matrix" else ""))
    call = ("neighbor_list, neighbor_ptr, neighbor_shifts, None, None, 0" if fmt == "list" else
            "None, None, None, neighbor_matrix, neighbor_matrix_shifts, fill_value")
    src = (f"def {name}({args}) -> {ret}:\n"
           f"    e, f = _forward(positions, charges, cell, {'batch_idx' if batched else 'None'}, {call}, cutoff, alpha, {forces})\n"
           f"    return {'(e, f)' if forces else 'e'}\n")
    scope = {"_forward": coulomb._forward, "Tensor": Tensor}
    exec(src, scope)  # the schema carries the reference's argument names and order

    def fake(positions, *rest):
        n = positions.shape[0]
        e = positions.new_empty((n,), dtype=torch.float64)
        return (e, positions.new_empty((n, 3), dtype=torch.float64)) if forces else e
    op = torch.library.custom_op(f"nvalchemiops::{name}", scope[name], mutates_args=())
    op.register_fake(fake)
    op.register_autograd(_coulomb_backward(name, forces), setup_context=_coulomb_setup(fmt, batched))
    return op


COULOMB_OPS = {}
for _b in (False, True):
    for _fmt in ("list", "matrix"):
        for _f in (False, True):
            COULOMB_OPS[(_b, _fmt, _f)] = _make_coulomb_op(("_batch" if _b else "") + "_coulomb_energy" + ("_forces" if _f else "") + "_" + _fmt,
                                                           _fmt, _b, _f)


def coulomb_op(batched: bool, fmt: str, forces: bool):
    return COULOMB_OPS[(batched, fmt, forces)]


# =====================================================================================================================================
# the fused reciprocal-space step as ONE op, for torch.compile (round 5)
# =====================================================================================================================================
# Outside a trace the reciprocal sum under autograd is the `pme._FusedReciprocal` node (inference kernels forward, hand-written adjoint).  A
# trace cannot look inside an autograd.Function that launches through ctypes, so until round 5 every `torch.compile` of PME took the op-by-op
# composition (2.7 x the forward).  These two ops are the same node in traceable form: the forward returns what its adjoint needs as extra
# outputs (the charge spectrum, the potential / field meshes, the per-system geometry), the backward is `pme._reciprocal_adjoint` behind a
# second op.  First order: the backward op raises for a second derivative (the eager node hands create_graph=True over to the composition;
# a compiled graph that needs it can set NVALCHEMIOPS_PME_FUSED_AUTOGRAD=0).
PME_FUSED_OP_CALLS = [0, 0]  # forward / backward launches of the traceable fused op (tests read it)


def _pme_fused_fwd(positions: Tensor, charges: Tensor, cells: Tensor, alpha: Tensor, batch_idx: Optional[Tensor], nx: int, ny: int, nz: int,
                   spline_order: int, compute_forces: bool) -> tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    from nvalchemiops.interactions.electrostatics.pme import _reciprocal_fused

    PME_FUSED_OP_CALLS[0] += 1

    dt = positions.dtype
    pos = positions.detach().contiguous()
    bi = None if batch_idx is None else C.i32(batch_idx)
    keep = {}
    e, f, cg = _reciprocal_fused(pos, charges.detach().to(dt).contiguous(), cells.detach().to(dt).contiguous(), alpha.detach().to(dt).reshape(-1).contiguous(),
                                 (int(nx), int(ny), int(nz)), int(spline_order), bi, bool(compute_forces), True, keep=keep)
    if f is None:
        f = pos.new_empty((0, 3))
    return e, f, cg, keep["spec"], keep["real"], keep["cit"].clone(), keep["recip"].clone(), keep["vol"].clone(), keep["qtot"].clone()


def _pme_fused_fwd_fake(positions, charges, cells, alpha, batch_idx, nx, ny, nz, spline_order, compute_forces):
    n, nsys, dt = positions.shape[0], cells.shape[0], positions.dtype
    cdt = torch.complex64 if dt == torch.float32 else torch.complex128
    new = positions.new_empty
    return (new((n,)), new((n, 3) if compute_forces else (0, 3)), new((n,)), new((nsys, nx, ny, nz // 2 + 1), dtype=cdt),
            new((nsys, 4 if compute_forces else 1, nx, ny, nz)), new((nsys, 3, 3)), new((nsys, 3, 3)), new((nsys,)), new((nsys,)))


def _pme_fused_bwd(positions: Tensor, charges: Tensor, cells: Tensor, alpha: Tensor, batch_idx: Optional[Tensor], spec: Tensor, real: Tensor, cg: Tensor,
                   cit: Tensor, recip: Tensor, vol: Tensor, qtot: Tensor, grad_energies: Optional[Tensor], grad_forces: Optional[Tensor],
                   grad_charge_grads: Optional[Tensor], nx: int, ny: int, nz: int, spline_order: int) -> tuple[Tensor, Tensor, Tensor, Tensor]:
    from nvalchemiops.interactions.electrostatics.pme import _reciprocal_adjoint

    PME_FUSED_OP_CALLS[1] += 1
    bi = None if batch_idx is None else C.i32(batch_idx)
    a = alpha.detach().reshape(-1)
    gp, gq, gc, ga = _reciprocal_adjoint((positions, charges, cells, a, spec, real, cg, cit, recip, vol, qtot), (True, True, True, True), grad_energies,
                                         grad_forces, (int(nx), int(ny), int(nz)), int(spline_order), bi, grad_charge_grads)
    z = torch.zeros_like
    return (z(positions) if gp is None else gp.to(positions.dtype), z(charges) if gq is None else gq.to(charges.dtype),
            z(cells) if gc is None else gc.to(cells.dtype), z(a) if ga is None else ga.reshape(a.shape).to(a.dtype))


pme_fused_op = torch.library.custom_op("nvalchemiops::pme_reciprocal_fused", _pme_fused_fwd, mutates_args=())
pme_fused_op.register_fake(_pme_fused_fwd_fake)
pme_fused_bwd_op = torch.library.custom_op("nvalchemiops::pme_reciprocal_fused_backward", _pme_fused_bwd, mutates_args=())
pme_fused_bwd_op.register_fake(lambda positions, charges, cells, alpha, *rest: (torch.empty_like(positions), torch.empty_like(charges), torch.empty_like(cells),
                                                                                 alpha.new_empty((alpha.numel(),))))
pme_fused_bwd_op.register_autograd(lambda ctx, *g: (_ for _ in ()).throw(NotImplementedError(
    "nvalchemiops::pme_reciprocal_fused_backward: second derivatives through the fused reciprocal op are not provided "
    "(NVALCHEMIOPS_PME_FUSED_AUTOGRAD=0 selects the differentiable op-by-op composition)")), setup_context=lambda ctx, inputs, output: None)


def _pme_fused_setup(ctx, inputs, output):
    positions, charges, cells, alpha, batch_idx, nx, ny, nz, order, compute_forces = inputs
    e, f, cg, spec, real, cit, recip, vol, qtot = output
    ctx.save_for_backward(positions, charges, cells, alpha, batch_idx, spec, real, cg, cit, recip, vol, qtot)
    ctx.meta = (int(nx), int(ny), int(nz), int(order), bool(compute_forces))


def _pme_fused_autograd(ctx, g_e, g_f, g_cg, *g_kept):
    positions, charges, cells, alpha, batch_idx, spec, real, cg, cit, recip, vol, qtot = ctx.saved_tensors
    nx, ny, nz, order, with_forces = ctx.meta
    gp, gq, gc, ga = pme_fused_bwd_op(positions, charges, cells, alpha, batch_idx, spec, real, cg, cit, recip, vol, qtot, g_e,
                                      g_f if with_forces else None, g_cg, nx, ny, nz, order)
    return gp, gq, gc, ga.reshape(alpha.shape), None, None, None, None, None, None


pme_fused_op.register_autograd(_pme_fused_autograd, setup_context=_pme_fused_setup)


# =====================================================================================================================================
# virials of the Ewald / PME sums (forward only)
# =====================================================================================================================================
# The `*_with_virial` functions return their sibling's outputs unchanged; when those go through autograd or a torch.compile trace, the virial
# comes from these ops: the same virial kernels on detached inputs.  The virial has no adjoint in this build: a loss that depends on it raises
# at backward (never a silent zero).
def _virial_no_adjoint(op):
    def backward(ctx, *grads):
        raise NotImplementedError(f"{op}: the virial is not differentiable in this build (training on stress is not supported); "
                                  "differentiate the energies, forces or charge gradients instead")
    return backward


def _ewald_real_virial(positions: Tensor, charges: Tensor, cells: Tensor, alpha: Tensor, batch_idx: Optional[Tensor], neighbor_list: Optional[Tensor],
                       neighbor_ptr: Optional[Tensor], neighbor_shifts: Optional[Tensor], neighbor_matrix: Optional[Tensor],
                       neighbor_matrix_shifts: Optional[Tensor], mask_value: int, num_systems: int) -> Tensor:
    from nvalchemiops.interactions.electrostatics.ewald import _real_virial

    return _real_virial(positions.detach(), charges.detach(), cells.detach(), alpha.detach(), neighbor_list, neighbor_ptr, neighbor_shifts,
                        neighbor_matrix, neighbor_matrix_shifts, int(mask_value), batch_idx, int(num_systems))


def _ewald_recip_virial(positions: Tensor, charges: Tensor, cells: Tensor, k_vectors: Tensor, alpha: Tensor, batch_idx: Optional[Tensor]) -> Tensor:
    from nvalchemiops.interactions.electrostatics.ewald import _recip_virial_only

    return _recip_virial_only(positions.detach(), charges.detach(), cells.detach(), k_vectors.detach(), alpha.detach(), batch_idx)


def _pme_recip_virial(positions: Tensor, charges: Tensor, cells: Tensor, alpha: Tensor, batch_idx: Optional[Tensor], nx: int, ny: int, nz: int,
                      spline_order: int, k_vectors: Optional[Tensor], k_squared: Optional[Tensor]) -> Tensor:
    from nvalchemiops.interactions.electrostatics.pme import _pme_virial_only

    return _pme_virial_only(positions.detach(), charges.detach(), cells.detach(), alpha.detach(), batch_idx, (int(nx), int(ny), int(nz)), int(spline_order),
                            None if k_vectors is None else k_vectors.detach(), None if k_squared is None else k_squared.detach())


def _noop_virial_setup(ctx, inputs, output):
    pass


ewald_real_virial_op = torch.library.custom_op("nvalchemiops::ewald_real_space_virial", _ewald_real_virial, mutates_args=())
ewald_real_virial_op.register_fake(lambda positions, *rest: positions.new_empty((int(rest[-1]), 3, 3)))
ewald_real_virial_op.register_autograd(_virial_no_adjoint("nvalchemiops::ewald_real_space_virial"), setup_context=_noop_virial_setup)
ewald_recip_virial_op = torch.library.custom_op("nvalchemiops::ewald_reciprocal_space_virial", _ewald_recip_virial, mutates_args=())
ewald_recip_virial_op.register_fake(lambda positions, charges, cells, *rest: positions.new_empty((cells.reshape(-1, 3, 3).shape[0], 3, 3)))
ewald_recip_virial_op.register_autograd(_virial_no_adjoint("nvalchemiops::ewald_reciprocal_space_virial"), setup_context=_noop_virial_setup)
pme_recip_virial_op = torch.library.custom_op("nvalchemiops::pme_reciprocal_space_virial", _pme_recip_virial, mutates_args=())
pme_recip_virial_op.register_fake(lambda positions, charges, cells, alpha, batch_idx, *rest:
                                  positions.new_empty((cells.reshape(-1, 3, 3).shape[0] if batch_idx is not None else 1, 3, 3)))
pme_recip_virial_op.register_autograd(_virial_no_adjoint("nvalchemiops::pme_reciprocal_space_virial"), setup_context=_noop_virial_setup)


# =====================================================================================================================================
# Gaussian-smeared charge correction: one op with optional tensors (single / batch, list / matrix, with / without a cell)
# =====================================================================================================================================
# Outputs are always the five of the public function; the ones not asked for are empty [0] tensors.  The energies are differentiable w.r.t.
# positions, charges, sigma and cell: the backward op runs the forward kernel with the incoming gradient as per-atom weights.
_GC_NAME = f"{_NS}::_gaussian_charge_correction"
_GC_OUTPUTS = ("energies", "forces", "charge_gradients", "sigma_gradients", "virial")


def _gaussian_fwd(positions: Tensor, charges: Tensor, sigma: Tensor, cell: Optional[Tensor], batch_idx: Optional[Tensor],
                  neighbor_list: Optional[Tensor], neighbor_ptr: Optional[Tensor], neighbor_shifts: Optional[Tensor],
                  neighbor_matrix: Optional[Tensor], neighbor_matrix_shifts: Optional[Tensor], mask_value: int, self_energy: bool,
                  neutralizing_background: bool, compute_forces: bool, compute_charge_gradients: bool, compute_sigma_gradients: bool,
                  compute_virial: bool) -> tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    from nvalchemiops.interactions.electrostatics.gaussian import _forward

    out = _forward(positions, charges, sigma, cell, batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts,
                   int(mask_value), self_energy, neutralizing_background, compute_forces, compute_charge_gradients, compute_sigma_gradients,
                   compute_virial)
    return tuple(positions.new_empty((0,)) if o is None else o for o in out)


def _gaussian_fwd_fake(positions, charges, sigma, cell, batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix,
                       neighbor_matrix_shifts, mask_value, self_energy, neutralizing_background, compute_forces, compute_charge_gradients,
                       compute_sigma_gradients, compute_virial):
    n = positions.shape[0]
    nsys = cell.reshape(-1, 3, 3).shape[0] if (cell is not None and batch_idx is not None) else 1
    empty = lambda: positions.new_empty((0,))  # noqa: E731
    return (positions.new_empty((n,)), positions.new_empty((n, 3)) if compute_forces else empty(),
            positions.new_empty((n,)) if compute_charge_gradients else empty(), positions.new_empty((n,)) if compute_sigma_gradients else empty(),
            positions.new_empty((nsys, 3, 3)) if compute_virial else empty())


def _gaussian_bwd(positions: Tensor, charges: Tensor, sigma: Tensor, cell: Optional[Tensor], batch_idx: Optional[Tensor],
                  neighbor_list: Optional[Tensor], neighbor_ptr: Optional[Tensor], neighbor_shifts: Optional[Tensor],
                  neighbor_matrix: Optional[Tensor], neighbor_matrix_shifts: Optional[Tensor], mask_value: int, self_energy: bool,
                  neutralizing_background: bool, grad_energies: Tensor) -> tuple[Tensor, Tensor, Tensor, Tensor]:
    """Float64 (dL/dpositions, dL/dcharges, dL/dsigma, dL/dcell [B,3,3] or [0]) for L = sum_i g_i E_i."""
    from nvalchemiops.interactions.electrostatics.gaussian import _adjoint

    gpos, gq, gs, gcell = _adjoint(positions, charges, sigma, cell, batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix,
                                   neighbor_matrix_shifts, int(mask_value), self_energy, neutralizing_background, grad_energies)
    return gpos, gq, gs, (gcell if gcell is not None else gpos.new_empty((0,)))


def _gaussian_bwd_fake(positions, charges, sigma, cell, batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix,
                       neighbor_matrix_shifts, mask_value, self_energy, neutralizing_background, grad_energies):
    n, f64 = positions.shape[0], dict(dtype=torch.float64)
    nsys = cell.reshape(-1, 3, 3).shape[0] if (cell is not None and batch_idx is not None) else 1
    return (positions.new_empty((n, 3), **f64), positions.new_empty((n,), **f64), positions.new_empty((n,), **f64),
            positions.new_empty((nsys, 3, 3), **f64) if cell is not None else positions.new_empty((0,), **f64))


gaussian_bwd_op = torch.library.custom_op("nvalchemiops::gaussian_charge_correction_backward", _gaussian_bwd, mutates_args=())
gaussian_bwd_op.register_fake(_gaussian_bwd_fake)
gaussian_bwd_op.register_autograd(lambda ctx, *g: (_ for _ in ()).throw(NotImplementedError(_SECOND_ORDER.format(
    op="nvalchemiops::gaussian_charge_correction_backward", what="gradient"))), setup_context=lambda ctx, inputs, output: None)


def _gaussian_setup(ctx, inputs, output):
    ctx.save_for_backward(*inputs[:10])
    ctx.mask, ctx.self_energy, ctx.background = inputs[10], inputs[11], inputs[12]
    ctx.set_materialize_grads(False)


def _gaussian_backward(ctx, g_e, *g_explicit):
    for what, g in zip(_GC_OUTPUTS[1:], g_explicit):
        if g is not None:
            raise NotImplementedError(_SECOND_ORDER.format(op=_GC_NAME, what=what))
    need = ctx.needs_input_grad
    if g_e is None:
        return (None,) * len(need)
    saved = ctx.saved_tensors
    positions, charges, sigma, cell = saved[:4]
    gpos, gq, gs, gcell = gaussian_bwd_op(*saved, int(ctx.mask), bool(ctx.self_energy), bool(ctx.background), g_e)
    return (gpos.to(positions.dtype) if need[0] else None, gq.to(charges.dtype) if need[1] else None, gs.to(sigma.dtype) if need[2] else None,
            gcell.reshape(cell.shape).to(cell.dtype) if (cell is not None and need[3]) else None) + (None,) * (len(need) - 4)


gaussian_charge_correction_op = _op("_gaussian_charge_correction", _gaussian_fwd, _gaussian_fwd_fake, _gaussian_backward, _gaussian_setup)


# =====================================================================================================================================
# point multipoles: nine operator halves and the bonded-pair scaling, one forward / backward op pair each, built from one table
# =====================================================================================================================================
# Outputs are always those of the public function (energies, forces, charge_gradients, dipole_gradients, the row's extra output, virial); the
# ones not asked for are empty [0] tensors.  The energies are differentiable w.r.t. the row's first inputs: the backward op runs the forward
# kernels with the incoming gradient as per-atom weights and returns float64 gradients.  Gradients of inputs without an adjoint (cell, alpha,
# k-vectors) are refused, never a silent zero: the virial is the strain derivative.  The ops are registered with an explicit schema string, so
# the implementations take *args in schema order.
_DP_NO_GRAD = ("{op}: gradients w.r.t. {what} are not provided by the point-dipole Ewald term (out of scope); use compute_virial for the "
               "strain derivative.")
_QD_NO_GRAD = ("{op}: gradients w.r.t. {what} are not provided by the point-quadrupole Ewald term (out of scope); use compute_virial for the "
               "strain derivative.")
_TH_NO_GRAD = ("{op}: gradients w.r.t. cell are not provided by the Thole damping term (out of scope); use "
               "compute_virial for the strain derivative.")
_CL_NO_GRAD = ("{op}: gradients w.r.t. cell are not provided by the bare multipole pair sums (out of scope); use compute_virial for the strain "
               "derivative.")
_PER_ATOM = {"positions": (3,), "charges": (), "dipoles": (3,), "quadrupoles": (3, 3), "polarizability": ()}  # shapes after [n]
_SCALARS = {"SymInt": int, "float": float, "bool": bool}  # schema type of a plain scalar -> the conversion `ctx.extra` and the launch functions get
_SYSTEMS = {  # the fake's number of systems, from (cell, batch_idx)
    "batch": lambda cell, batch_idx: cell.reshape(-1, 3, 3).shape[0] if batch_idx is not None else 1,
    "optional cell": lambda cell, batch_idx: cell.reshape(-1, 3, 3).shape[0] if (cell is not None and batch_idx is not None) else 1,
    "cell rows": lambda cell, batch_idx: cell.reshape(-1, 3, 3).shape[0],
}
_DP, _QD, _TH = ("positions", "charges", "dipoles"), ("positions", "charges", "dipoles", "quadrupoles"), ("positions", "charges", "dipoles",
                                                                                                            "polarizability")
_QG, _PG = ("quadrupole_gradients", (3, 3)), ("polarizability_gradients", ())
_LISTS = ("Tensor? batch_idx, Tensor? neighbor_list, Tensor? neighbor_ptr, Tensor? neighbor_shifts, Tensor? neighbor_matrix, "
          "Tensor? neighbor_matrix_shifts, SymInt mask_value")
_MESH = "Tensor cell, Tensor alpha, Tensor? batch_idx, SymInt nx, SymInt ny, SymInt nz, SymInt spline_order"
_KSUM = "Tensor cell, Tensor k_vectors, Tensor alpha, Tensor? batch_idx"
# op name: (module under interactions/electrostatics, its forward, its adjoint, differentiable inputs, middle arguments (a `Tensor` is saved
# for backward, a scalar travels in ctx.extra), extra output | None, system-count rule, inputs without an adjoint, refusal text)
_MULTIPOLE_OPS = {
    "ewald_dipole_real_space": ("dipole", "_real_forward", "_real_adjoint", _DP, f"Tensor cell, Tensor alpha, {_LISTS}", None, "batch",
                                ("cell", "alpha"), _DP_NO_GRAD),
    "ewald_dipole_reciprocal_space": ("dipole", "_recip_forward", "_recip_adjoint", _DP, _KSUM, None, "cell rows",
                                      ("cell", "k_vectors", "alpha"), _DP_NO_GRAD),
    "pme_dipole_reciprocal_space": ("pme_dipole", "_recip_forward", "_recip_adjoint", _DP, _MESH, None, "batch", ("cell", "alpha"), _DP_NO_GRAD),
    "thole_dipole_correction": ("thole", "_forward", "_adjoint", _TH, f"Tensor? cell, {_LISTS}, float thole", _PG, "optional cell", ("cell",),
                                _TH_NO_GRAD),
    "ewald_quadrupole_real_space": ("quadrupole", "_real_forward", "_real_adjoint", _QD, f"Tensor cell, Tensor alpha, {_LISTS}", _QG, "batch",
                                    ("cell", "alpha"), _QD_NO_GRAD),
    "ewald_quadrupole_reciprocal_space": ("quadrupole", "_recip_forward", "_recip_adjoint", _QD, _KSUM, _QG, "cell rows",
                                          ("cell", "k_vectors", "alpha"), _QD_NO_GRAD),
    "pme_quadrupole_reciprocal_space": ("pme_quadrupole", "_recip_forward", "_recip_adjoint", _QD, _MESH, _QG, "batch", ("cell", "alpha"),
                                        _QD_NO_GRAD),
    "coulomb_dipole_correction": ("cluster", "_dipole_forward", "_dipole_adjoint", _DP, f"Tensor? cell, {_LISTS}", None, "optional cell",
                                  ("cell",), _CL_NO_GRAD),
    "coulomb_quadrupole_correction": ("cluster", "_quadrupole_forward", "_quadrupole_adjoint", _QD, f"Tensor? cell, {_LISTS}", _QG,
                                      "optional cell", ("cell",), _CL_NO_GRAD),
    "pair_scale_correction": ("pair_scale", "_forward", "_adjoint", _QD, f"Tensor pair_scales, Tensor? cell, {_LISTS}, bool minimum_image", _QG,
                              "optional cell", ("cell",), _CL_NO_GRAD),
}


def _multipole_ops(name, module, forward, adjoint, diff, middle, extra, systems, no_adjoint, refusal):
    """(forward op `alchemiops::_<name>`, backward op `nvalchemiops::<name>_backward`) of one row of `_MULTIPOLE_OPS`, with their fakes, the
    second-order refusal on the backward op and the forward op's autograd."""
    fwd_name, bwd_name = f"{_NS}::_{name}", f"nvalchemiops::{name}_backward"
    mid = [a.split() for a in middle.split(", ")]  # [schema type, argument name]
    names = list(diff) + [a[1] for a in mid]
    n_diff, n_in = len(diff), len(names)
    k = n_diff + sum(t.startswith("Tensor") for t, _ in mid)  # the tensors lead, the plain scalars trail
    convert = [_SCALARS[t] for t, _ in mid[k - n_diff:]]
    outputs = (("energies", ()), ("forces", (3,)), ("charge_gradients", ()), ("dipole_gradients", (3,))) + ((extra,) if extra else ())
    i_cell, i_batch, nsys_of = names.index("cell"), names.index("batch_idx"), _SYSTEMS[systems]
    refused = {names.index(what): what for what in no_adjoint}
    inputs = ", ".join([f"Tensor {d}" for d in diff] + [middle])
    flags = ", ".join(f"bool compute_{o}" for o, _ in outputs[1:]) + ", bool compute_virial"

    def run(fn_name, args, tail):
        fn = getattr(importlib.import_module(f"nvalchemiops.interactions.electrostatics.{module}"), fn_name)
        return fn(*args[:k], *[c(v) for c, v in zip(convert, args[k:n_in])], *tail)

    def fwd(*args):
        return tuple(args[0].new_empty((0,)) if o is None else o for o in run(forward, args, args[n_in:]))

    def fwd_fake(*args):
        positions, want = args[0], (True,) + tuple(args[n_in:])
        shapes = [(positions.shape[0],) + s for _, s in outputs] + [(nsys_of(args[i_cell], args[i_batch]), 3, 3)]
        return tuple(positions.new_empty(s if w else (0,)) for s, w in zip(shapes, want))

    def bwd(*args):
        return run(adjoint, args, (args[n_in],))

    def bwd_fake(positions, *rest):
        return tuple(positions.new_empty((positions.shape[0],) + _PER_ATOM[d], dtype=torch.float64) for d in diff)

    def refuse_second_order(ctx, *grads):
        raise NotImplementedError(_SECOND_ORDER.format(op=bwd_name, what="gradient"))

    bwd_op = torch.library.custom_op(bwd_name, bwd, mutates_args=(),
                                     schema=f"({inputs}, Tensor grad_energies) -> ({', '.join(['Tensor'] * n_diff)})")
    bwd_op.register_fake(bwd_fake)
    bwd_op.register_autograd(refuse_second_order, setup_context=lambda ctx, inputs, output: None)

    def setup(ctx, inputs, output):
        ctx.save_for_backward(*inputs[:k])
        ctx.extra = tuple(c(v) for c, v in zip(convert, inputs[k:n_in]))
        ctx.set_materialize_grads(False)

    def backward(ctx, g_e, *g_explicit):
        for (what, _), g in zip(outputs[1:] + (("virial", None),), g_explicit):
            if g is not None:
                raise NotImplementedError(_SECOND_ORDER.format(op=fwd_name, what=what))
        need = ctx.needs_input_grad
        for i, what in refused.items():
            if need[i]:
                raise NotImplementedError(refusal.format(op=fwd_name, what=what))
        if g_e is None:
            return (None,) * len(need)
        saved = ctx.saved_tensors
        grads = bwd_op(*saved, *ctx.extra, g_e)
        return tuple(g.to(t.dtype) if w else None for g, t, w in zip(grads, saved[:n_diff], need[:n_diff])) + (None,) * (len(need) - n_diff)

    fwd_op = torch.library.custom_op(fwd_name, fwd, mutates_args=(),
                                     schema=f"({inputs}, {flags}) -> ({', '.join(['Tensor'] * (len(outputs) + 1))})")
    fwd_op.register_fake(fwd_fake)
    fwd_op.register_autograd(backward, setup_context=setup)
    return fwd_op, bwd_op


_MP = {name: _multipole_ops(name, *row) for name, row in _MULTIPOLE_OPS.items()}
ewald_dipole_real_space_op, ewald_dipole_real_bwd_op = _MP["ewald_dipole_real_space"]
ewald_dipole_reciprocal_space_op, ewald_dipole_recip_bwd_op = _MP["ewald_dipole_reciprocal_space"]
pme_dipole_reciprocal_space_op, pme_dipole_recip_bwd_op = _MP["pme_dipole_reciprocal_space"]
thole_dipole_correction_op, thole_dipole_bwd_op = _MP["thole_dipole_correction"]
ewald_quadrupole_real_space_op, ewald_quadrupole_real_bwd_op = _MP["ewald_quadrupole_real_space"]
ewald_quadrupole_reciprocal_space_op, ewald_quadrupole_recip_bwd_op = _MP["ewald_quadrupole_reciprocal_space"]
pme_quadrupole_reciprocal_space_op, pme_quadrupole_recip_bwd_op = _MP["pme_quadrupole_reciprocal_space"]
coulomb_dipole_correction_op, coulomb_dipole_bwd_op = _MP["coulomb_dipole_correction"]
coulomb_quadrupole_correction_op, coulomb_quadrupole_bwd_op = _MP["coulomb_quadrupole_correction"]
pair_scale_correction_op, pair_scale_bwd_op = _MP["pair_scale_correction"]


# =====================================================================================================================================
# local-frame multipoles: mu = R mu_loc, Q = R Q_loc R^T (nvalchemiops/interactions/electrostatics/frames.py)
# =====================================================================================================================================
# Both outputs are differentiable w.r.t. positions and the local multipoles; the backward op runs `mi_frame_adjoint` + `mi_frame_gather` and
# returns float64 gradients.  An output whose local input is None is an empty [0] tensor, and so is the gradient of an input that is None.
_FR_NO_GRAD = ("{op}: gradients w.r.t. cell are not provided by the local-frame rotation (out of scope); use compute_virial of "
               "multipole_frame_forces for the strain derivative.")
_FR_NAME = f"{_NS}::_rotate_multipoles"
_FR_INPUTS = ("Tensor positions, Tensor? local_dipoles, Tensor? local_quadrupoles, Tensor? cell, Tensor? batch_idx, Tensor frame_atoms, "
              "Tensor frame_kinds")


def _frames():
    return importlib.import_module("nvalchemiops.interactions.electrostatics.frames")


def _rotate_fwd(positions, local_dipoles, local_quadrupoles, cell, batch_idx, frame_atoms, frame_kinds, inverse_ptr, inverse_slots):
    mu, qd = _frames()._forward(positions, local_dipoles, local_quadrupoles, cell, batch_idx, frame_atoms, frame_kinds)
    return tuple(positions.new_empty((0,)) if o is None else o for o in (mu, qd))


def _rotate_fwd_fake(positions, local_dipoles, local_quadrupoles, cell, batch_idx, frame_atoms, frame_kinds, inverse_ptr, inverse_slots):
    n = positions.shape[0]
    return (positions.new_empty((n, 3) if local_dipoles is not None else (0,)),
            positions.new_empty((n, 3, 3) if local_quadrupoles is not None else (0,)))


def _rotate_bwd(positions, local_dipoles, local_quadrupoles, cell, batch_idx, frame_atoms, frame_kinds, inverse_ptr, inverse_slots, grad_dipoles,
                grad_quadrupoles):
    return _frames()._adjoint(positions, local_dipoles, local_quadrupoles, cell, batch_idx, frame_atoms, frame_kinds, inverse_ptr, inverse_slots,
                              grad_dipoles, grad_quadrupoles)


def _rotate_bwd_fake(positions, local_dipoles, local_quadrupoles, cell, batch_idx, frame_atoms, frame_kinds, inverse_ptr, inverse_slots,
                     grad_dipoles, grad_quadrupoles):
    n = positions.shape[0]
    f64 = lambda shape: positions.new_empty(shape, dtype=torch.float64)  # noqa: E731
    return f64((n, 3)), f64((n, 3) if local_dipoles is not None else (0,)), f64((n, 3, 3) if local_quadrupoles is not None else (0,))


def _rotate_refuse_second_order(ctx, *grads):
    raise NotImplementedError(_SECOND_ORDER.format(op="nvalchemiops::rotate_multipoles_backward", what="gradient"))


rotate_multipoles_bwd_op = torch.library.custom_op(
    "nvalchemiops::rotate_multipoles_backward", _rotate_bwd, mutates_args=(),
    schema=f"({_FR_INPUTS}, Tensor inverse_ptr, Tensor inverse_slots, Tensor? grad_dipoles, Tensor? grad_quadrupoles) -> (Tensor, Tensor, Tensor)")
rotate_multipoles_bwd_op.register_fake(_rotate_bwd_fake)
rotate_multipoles_bwd_op.register_autograd(_rotate_refuse_second_order, setup_context=lambda ctx, inputs, output: None)


def _rotate_setup(ctx, inputs, output):
    ctx.save_for_backward(*inputs)
    ctx.set_materialize_grads(False)


def _rotate_backward(ctx, g_mu, g_qd):
    need = ctx.needs_input_grad
    if need[3]:
        raise NotImplementedError(_FR_NO_GRAD.format(op=_FR_NAME))
    saved = ctx.saved_tensors
    if g_mu is not None and saved[1] is None:
        g_mu = None
    if g_qd is not None and saved[2] is None:
        g_qd = None
    if g_mu is None and g_qd is None:
        return (None,) * len(need)
    grads = rotate_multipoles_bwd_op(*saved, g_mu, g_qd)
    return tuple(g.to(t.dtype) if w else None for g, t, w in zip(grads, saved[:3], need[:3])) + (None,) * (len(need) - 3)


rotate_multipoles_op = torch.library.custom_op(_FR_NAME, _rotate_fwd, mutates_args=(),
                                               schema=f"({_FR_INPUTS}, Tensor inverse_ptr, Tensor inverse_slots) -> (Tensor, Tensor)")
rotate_multipoles_op.register_fake(_rotate_fwd_fake)
rotate_multipoles_op.register_autograd(_rotate_backward, setup_context=_rotate_setup)


__all__ = ["pair_scale_correction_op", "pair_scale_bwd_op", "rotate_multipoles_op", "rotate_multipoles_bwd_op", "coulomb_dipole_correction_op", "coulomb_dipole_bwd_op", "coulomb_quadrupole_correction_op", "coulomb_quadrupole_bwd_op",
           "pme_quadrupole_reciprocal_space_op", "pme_quadrupole_recip_bwd_op",
           "ewald_quadrupole_real_space_op", "ewald_quadrupole_reciprocal_space_op", "ewald_quadrupole_real_bwd_op",
           "ewald_quadrupole_recip_bwd_op", "thole_dipole_correction_op", "thole_dipole_bwd_op", "pme_dipole_reciprocal_space_op", "pme_dipole_recip_bwd_op", "ewald_dipole_real_space_op", "ewald_dipole_reciprocal_space_op", "ewald_dipole_real_bwd_op", "ewald_dipole_recip_bwd_op",
           "gaussian_charge_correction_op", "gaussian_bwd_op","spline_spread_op", "batch_spline_spread_op", "spline_gather_op", "batch_spline_gather_op", "spline_gather_vec3_op",
           "batch_spline_gather_vec3_op", "spline_gather_gradient_op", "batch_spline_gather_gradient_op", "pme_green_structure_factor_op",
           "batch_pme_green_structure_factor_op", "pme_energy_corrections_op", "batch_pme_energy_corrections_op",
           "pme_energy_corrections_with_charge_grad_op", "batch_pme_energy_corrections_with_charge_grad_op", "REAL_OPS", "real_space_op", "RECIPROCAL_OPS", "reciprocal_space_op", "COULOMB_OPS", "coulomb_op",
           "ewald_real_virial_op", "ewald_recip_virial_op", "pme_recip_virial_op"]
