"""The call layer the six dispersion operators (`dftd3`, `dftd3_zero`, `dftd3_atm`, `dftd3_zero_atm`, `dftd4`, `dftd4_atm`) and their twelve
custom ops share, each piece once: argument checks, the three-body parameter checks, system resolution and output allocation, the list
arguments of a launch, the launch prelude, the two parameter structs and the energy adjoint.  Plain functions on tuples: TorchDynamo inlines
them where a public function is traced, and the eager path pays a call, not an object, per piece.
"""
from __future__ import annotations

import torch

from nvalchemiops import _capi as C

FLOAT_TYPES = (torch.float32, torch.float64)
D4_INT_TABLES = ("n_ref", "ngw")
D4_TABLES = ("rcov", "en", "r4r2", "zeff", "gam", "n_ref", "ngw", "cn_ref", "q_ref", "c6_ref")  # `D4Parameters` order = `mi_d4_params` order


# ---- argument checks: list format, D3 tables, per-atom / neighbour data (the order a caller meets them in is the public functions') ----------

def check_lists(neighbor_matrix, neighbor_matrix_shifts, neighbor_list, neighbor_ptr, unit_shifts, cell, compute_virial, missing_functional) -> bool:
    """List-format checks of dftd3.py:2668-2726 of the reference, same order and messages; `missing_functional`: the message to raise when a
    required functional parameter is missing or out of range, or None.  Returns whether the list is a neighbour matrix."""
    use_matrix, use_list = neighbor_matrix is not None, neighbor_list is not None
    if use_matrix and use_list:
        raise ValueError("Cannot provide both neighbor_matrix and neighbor_list. Please provide only one neighbor representation format.")
    if not use_matrix and not use_list:
        raise ValueError("Must provide either neighbor_matrix or neighbor_list.")
    if use_matrix and unit_shifts is not None:
        raise ValueError("unit_shifts is for neighbor_list format. Use neighbor_matrix_shifts for neighbor_matrix format.")
    if use_list and neighbor_matrix_shifts is not None:
        raise ValueError("neighbor_matrix_shifts is for neighbor_matrix format. Use unit_shifts for neighbor_list format.")
    if use_list and neighbor_ptr is None:
        raise ValueError("neighbor_ptr must be provided when using neighbor_list format. "
                         "Obtain it from the neighbor list API by setting return_neighbor_list=True.")
    if missing_functional:
        raise ValueError(missing_functional)
    if compute_virial:
        need = "Virial computation requires periodic boundary conditions. "
        if cell is None:
            raise ValueError(need + "Please provide unit cell parameters (cell) and shifts (neighbor_matrix_shifts or unit_shifts) "
                             "when compute_virial=True or when passing a virial tensor.")
        if use_matrix and neighbor_matrix_shifts is None:
            raise ValueError(need + "Please provide neighbor_matrix_shifts along with cell when using neighbor_matrix format "
                             "and compute_virial=True or passing a virial tensor.")
        if use_list and unit_shifts is None:
            raise ValueError(need + "Please provide unit_shifts along with cell when using neighbor_list format "
                             "and compute_virial=True or passing a virial tensor.")
    return use_matrix


def d3_tables(d3_params, covalent_radii, r4r2, c6_reference, coord_num_ref):
    """(rcov, r4r2, c6ab, cn_ref) of a D3 call: explicit tensors win over `d3_params` entries (dftd3.py:2727-2757), a `D3Parameters` read
    by attribute and anything else by key; the three shapes are checked against rcov's length."""
    if covalent_radii is None or r4r2 is None or c6_reference is None or coord_num_ref is None:
        if d3_params is None:
            raise RuntimeError("DFT-D3 parameters must be explicitly provided. Either supply all individual parameters "
                               "(covalent_radii, r4r2, c6_reference, coord_num_ref), provide a D3Parameters instance, "
                               "or provide a d3_params dictionary. See the function docstring for details.")
        if hasattr(d3_params, "rcov"):  # a D3Parameters
            src = {"rcov": d3_params.rcov, "r4r2": d3_params.r4r2, "c6ab": d3_params.c6ab, "cn_ref": d3_params.cn_ref}
        else:
            src = d3_params
        covalent_radii = src["rcov"] if covalent_radii is None else covalent_radii
        r4r2 = src["r4r2"] if r4r2 is None else r4r2
        c6_reference = src["c6ab"] if c6_reference is None else c6_reference
        coord_num_ref = src["cn_ref"] if coord_num_ref is None else coord_num_ref
    nz = covalent_radii.size(0)
    if tuple(r4r2.shape) != (nz,):
        raise ValueError(f"r4r2 must have shape [{nz}] to match rcov, got {tuple(r4r2.shape)}")
    if c6_reference.dim() != 4 or tuple(c6_reference.shape[:2]) != (nz, nz):
        raise ValueError(f"c6ab must have shape {(nz, nz, 5, 5)}, got {tuple(c6_reference.shape)}")
    if tuple(coord_num_ref.shape) != tuple(c6_reference.shape):
        raise ValueError(f"cn_ref must have shape {tuple(c6_reference.shape)}, got {tuple(coord_num_ref.shape)}")
    return covalent_radii, r4r2, c6_reference, coord_num_ref


def d3_cutoff_radii(d3_params, cutoff_radii, nz):
    """The pair cutoff radii r0ab[Z+1, Z+1] of the zero damping: explicit tensor, else key "r0ab" of a `d3_params` dict (`D3Parameters` does
    not carry them), checked against rcov's length `nz`.  A caller runs this after `check_atoms`: that is where these errors have come."""
    if cutoff_radii is None and isinstance(d3_params, dict):
        cutoff_radii = d3_params.get("r0ab")
    if cutoff_radii is None:
        raise RuntimeError("DFT-D3 zero-damping pair cutoff radii must be explicitly provided. Either supply cutoff_radii (r0ab[max_Z+1, max_Z+1], "
                           'in Bohr) or provide a d3_params dictionary with the key "r0ab"; a D3Parameters instance does not carry them.')
    if not isinstance(cutoff_radii, torch.Tensor):
        raise TypeError(f"Parameter 'cutoff_radii' must be a torch.Tensor, got {type(cutoff_radii)}")
    if cutoff_radii.dtype not in FLOAT_TYPES:
        raise TypeError(f"Parameter 'cutoff_radii' must be float32 or float64, got {cutoff_radii.dtype}")
    if tuple(cutoff_radii.shape) != (nz, nz):
        raise ValueError(f"cutoff_radii must have shape [{nz}, {nz}] to match rcov, got {tuple(cutoff_radii.shape)}")
    return cutoff_radii


def check_atoms(positions, numbers, batch_idx, num_systems, neighbor_matrix, neighbor_matrix_shifts, neighbor_list, neighbor_ptr, unit_shifts,
                cell) -> None:
    """Neighbour data, per-atom tensors and cells against the number of atoms and systems (`_capi.check_neighbor_data`: host-side shape
    reads, before the device check and before any launch -- the kernels see bare pointers and these integers)."""
    if num_systems is None and batch_idx is None:
        num_systems = 1
    if positions.size(0) > 0:  # (no atoms: nothing is launched, and the reference's empty-input contract reads batch_idx on its own)
        shifts = neighbor_matrix_shifts if neighbor_matrix is not None else unit_shifts
        C.check_neighbor_data(positions.size(0), neighbor_matrix=neighbor_matrix, neighbor_matrix_shifts=neighbor_matrix_shifts,
                              neighbor_list=neighbor_list, neighbor_ptr=neighbor_ptr, neighbor_shifts=unit_shifts, shifts_name="unit_shifts",
                              cell=cell if shifts is not None else None, num_systems=num_systems, numbers=numbers, batch_idx=batch_idx)


def three_body_missing(three_body_cutoff, alpha):
    """The `missing_functional` message of a three-body call after its operator's own head, or None."""
    if three_body_cutoff is None:
        return "three_body_cutoff must be provided: the distance below which all three sides of a triple must lie."
    if not three_body_cutoff > 0:
        return f"three_body_cutoff must be positive, got {three_body_cutoff}"
    if not alpha > 0:
        return f"alpha must be positive, got {alpha}"
    return None


# ---- systems and outputs: (energy, forces, k per-atom vectors, virial), all float32 -----------------------------------------------------------

def empty_result(positions, batch_idx, k, compute_virial):
    """What a call without atoms returns (the reference's empty-input contract, dftd3.py:2759-2775): the systems are those `batch_idx`
    names, whatever `num_systems` and `cell` say."""
    f32 = dict(dtype=torch.float32, device=positions.device)
    nsys = infer_num_systems(None, None if batch_idx is None or batch_idx.numel() == 0 else batch_idx, None)
    out = (torch.zeros(nsys, **f32), torch.zeros((0, 3), **f32)) + tuple([torch.zeros((0,), **f32) for _ in range(k)])
    return out + (torch.zeros((0, 3, 3), **f32),) if compute_virial else out


def infer_num_systems(num_systems, batch_idx, cell) -> int:
    if num_systems is not None:
        return num_systems
    if batch_idx is None:
        return 1
    if cell is not None:
        return cell.size(0)
    return int(batch_idx.max().item()) + 1


def allocate(positions, num_systems, k, compute_virial):
    """(energy[num_systems], forces[N,3], k x [N], virial[num_systems,3,3] or the (0,3,3) placeholder); the launch writes every element."""
    dev, n, f32 = positions.device, positions.size(0), torch.float32
    out = [torch.empty(num_systems, dtype=f32, device=dev), torch.empty((n, 3), dtype=f32, device=dev)]
    for _ in range(k):
        out.append(torch.empty(n, dtype=f32, device=dev))
    out.append(torch.empty((num_systems, 3, 3), dtype=f32, device=dev) if compute_virial else torch.zeros((0, 3, 3), dtype=f32, device=dev))
    return tuple(out)


def select(out, compute_virial):
    """The tuple a public function returns: the placeholder virial is not part of it."""
    return out if compute_virial else out[:-1]


# ---- launch arguments -------------------------------------------------------------------------------------------------------------------------

def list_args(n, neighbor_matrix=None, neighbor_matrix_shifts=None, fill_value=None, neighbor_list=None, neighbor_ptr=None, unit_shifts=None,
              idx_j=None):
    """(idx, shifts, nptr, max_neighbors, fill_value) as every launch function takes them, from a padded matrix (`fill_value` None: n) or
    from a CSR list, `neighbor_list` [2, P] or its second row `idx_j` (width and fill value are not read).  `idx is neighbor_matrix` tells a
    caller that no conversion took place."""
    if neighbor_matrix is not None:
        nm = C.i32(neighbor_matrix)
        return nm, neighbor_matrix_shifts, None, nm.size(1), n if fill_value is None else fill_value
    return C.i32(idx_j if neighbor_list is None else neighbor_list[1]), unit_shifts, C.i32(neighbor_ptr), 0, 0


def f32_on(t, dev):
    return t.detach().to(device=dev, dtype=torch.float32).contiguous()  # (dftd3.py:1912-1915)


def prelude(positions, numbers, shifts, cell, batch_idx):
    """(pos, dtype code, z, cell_t, sh, bi) of a launch; cell_t and sh are None unless the call is periodic (cell and shifts given).  The
    caller holds the tuple until the launch is enqueued: the allocator may otherwise reuse the converted tensors' blocks."""
    dev = positions.device
    pos = positions.detach().contiguous()
    code = C.dtype_code(pos.dtype)
    periodic = cell is not None and shifts is not None
    cell_t = cell.detach().to(dtype=pos.dtype, device=dev).reshape(-1, 3, 3).contiguous() if periodic else None
    sh = C.i32(shifts.to(dev)) if periodic else None
    bi = None if batch_idx is None else C.i32(batch_idx)
    return pos, code, C.i32(numbers), cell_t, sh, bi


def d3_struct(dev, tables, scalars):
    """`mi_d3_params` of (rcov, r4r2, c6ab, cn_ref) and the scalars' dict, with the float32 tensors it points into (keep them referenced)."""
    keep = tuple(f32_on(t, dev) for t in tables)
    if keep[2].shape[-1] != 5 or keep[2].shape[-2] != 5:
        raise ValueError("this build supports the standard 5x5 CN interpolation mesh only")
    par = C.MiD3Params(rcov=keep[0].data_ptr(), r4r2=keep[1].data_ptr(), c6ab=keep[2].data_ptr(), cn_ref=keep[3].data_ptr(),
                       nz=keep[0].shape[0], **{k: float(v) for k, v in scalars.items()})
    return par, keep


def d4_struct(dev, tables, scalars):
    """`mi_d4_params` of the ten tables in `D4_TABLES` order and the scalars' dict, with the converted tensors it points into."""
    keep = {k: (C.i32(t.detach().to(dev)) if k in D4_INT_TABLES else f32_on(t, dev)) for k, t in zip(D4_TABLES, tables)}
    par = C.MiD4Params(**{k: t.data_ptr() for k, t in keep.items()}, nz=keep["rcov"].shape[0], **{k: float(v) for k, v in scalars.items()})
    return par, keep


# ---- autograd -----------------------------------------------------------------------------------------------------------------------------------

class EnergyAdjoint(torch.autograd.Function):
    """`energy` = run()[0] with a hand-written first-order adjoint: d(sum_s g_s E_s)/d(positions) = -g[batch] forces and, where `charges` is
    given, /d(charges) = g[batch] dE/dq; run() returns (energy, forces, ...) with dE/dq at index 3."""

    @staticmethod
    def forward(ctx, positions, charges, batch_idx, run):
        out = run()
        ctx.save_for_backward(out[1], None if charges is None else out[3])
        ctx.batch_idx = batch_idx
        ctx.dtypes = (positions.dtype, None if charges is None else charges.dtype)
        ctx.mark_non_differentiable(*out[1:])
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, *_unused):
        forces, charge_grad = ctx.saved_tensors
        ga = g.expand(forces.shape[0]) if ctx.batch_idx is None else g[ctx.batch_idx.long()]
        gp = (-ga[:, None] * forces).to(ctx.dtypes[0]) if ctx.needs_input_grad[0] else None
        gq = (ga * charge_grad).to(ctx.dtypes[1]) if ctx.needs_input_grad[1] else None
        return gp, gq, None, None
