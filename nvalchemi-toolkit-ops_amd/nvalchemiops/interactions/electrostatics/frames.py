"""Local-frame multipoles: the rotation of per-atom local dipoles and quadrupoles into the laboratory frame, and the torque forces.

Every multipole operator of this package (`ewald_dipole_correction`, `ewald_quadrupole_correction`, `pme_*`, `coulomb_*`, `thole_*`, the
induced-dipole solvers) takes Cartesian laboratory-frame tensors and holds them fixed in space.  AMOEBA-class force fields, and learned
potentials that predict equivariant multipoles, define an atom's permanent multipoles in a local frame built from two or three bonded
neighbours: the laboratory-frame tensors are then a function of the positions, and the torque on a multipole becomes forces on the atoms that
define its frame.  This module is that link:

    LocalFrames               the frame table of a topology (built once) with the inverse map the adjoint needs
    rotate_multipoles         mu = R mu_loc, Q = R Q_loc R^T, differentiable w.r.t. positions and the local multipoles
    multipole_frame_forces    the same adjoint without an autograd graph: torque forces, local gradients, virial term

Frames are Tinker / OpenMM's axis types.  With d_a = r_a - r_i for frame atom a of atom i and n(v) = v / |v|:

    kind             e_z                                x-like vector before orthogonalising
    FRAME_Z_ONLY     n(d_z)                             lab x if |e_z . x^| < 0.866, else lab y
    FRAME_Z_THEN_X   n(d_z)                             d_x
    FRAME_BISECTOR   n(n(d_z) + n(d_x))                 d_x
    FRAME_Z_BISECT   n(d_z)                             n(n(d_x) + n(d_y))
    FRAME_THREE_FOLD n(n(d_z) + n(d_x) + n(d_y))        d_x

e_x is the x-like vector orthogonalised against e_z and normalised, e_y = e_z x e_x and R = [e_x e_y e_z] as columns.  FRAME_NONE is R = I:
that atom's multipoles are laboratory-frame already and carry no torque force.  A FRAME_Z_THEN_X atom with a y atom is a chiral centre: if
d_y . (d_z x d_x) < 0 the local y axis is mirrored (mu_y, Q_xy and Q_yz change sign); the gradient treats the sign as a constant.

The kernels are csrc/frames.hip (`mi_frame_rotate`, `mi_frame_adjoint`, `mi_frame_gather`): one thread per atom, float64 arithmetic whatever
the positions dtype, outputs rounded once, no floating-point atomics, so two calls, and a call on a side stream, are bit-identical.  The
reference package has no counterpart."""
from __future__ import annotations

import ctypes

import torch

from nvalchemiops import _capi as C
from nvalchemiops.interactions.electrostatics import _pairs as P

FRAME_NONE, FRAME_Z_ONLY, FRAME_Z_THEN_X, FRAME_BISECTOR, FRAME_Z_BISECT, FRAME_THREE_FOLD = 0, 1, 2, 3, 4, 5
_KIND_NAMES = ("FRAME_NONE", "FRAME_Z_ONLY", "FRAME_Z_THEN_X", "FRAME_BISECTOR", "FRAME_Z_BISECT", "FRAME_THREE_FOLD")
_SLOT_NAMES = ("z", "x", "y")
# per kind and slot (z, x, y): 2 = required, 1 = used when given (the chirality atom of Z_THEN_X), 0 = not looked at
_SLOT_USE = ((0, 0, 0), (2, 0, 0), (2, 2, 1), (2, 2, 0), (2, 2, 2), (2, 2, 2))

_GEOMETRY = """d_a is the minimum image when `cell` is given ([3, 3], or [num_systems, 3, 3] with `batch_idx`; rows are lattice vectors): valid for
    frame atoms closer than half the smallest cell height, which is NOT checked; wrapped and unwrapped coordinates then give the same
    result.  With `cell=None` nothing is wrapped.  Degenerate geometry (a zero or collinear pair of frame vectors) is the caller's
    responsibility: it yields non-finite values for that atom and the atoms it names, and for no other atom."""


class LocalFrames:
    """The local frames of a topology: a plain container of tensors, built once.

    `frame_atoms` int32 [N, 3] holds the indices of the (z, x, y) atoms of every atom, -1 for an unused slot; `frame_kinds` int32 [N] one of
    FRAME_NONE, FRAME_Z_ONLY (z), FRAME_Z_THEN_X (z, x; a y atom makes it a chiral centre), FRAME_BISECTOR (z, x), FRAME_Z_BISECT (z, x, y),
    FRAME_THREE_FOLD (z, x, y).  A slot its kind does not look at is stored as -1, whatever was passed.  `batch_idx` [N] is only read by the
    validation.

    The constructor also builds the inverse map the adjoint needs: `inverse_ptr` int32 [N + 1] and `inverse_slots` int32 [E], a CSR over
    atoms of the (atom j, slot) pairs that name each atom, stored as codes 4 j + 1 + slot in ascending order.

    With `validate=True` the tables are checked once, on the host (one device read), and a ValueError names the first offending atom: an index
    outside [-1, N), a required slot that holds -1, an atom that names itself, a frame atom that appears twice, an unknown kind, and with
    `batch_idx` a frame atom in another system.  `validate=False` skips the read; the kernels then treat an index outside [0, N) as an
    unused slot (non-finite values for that atom, never an out-of-bounds access).

    `to(device)` returns a copy on another device."""

    def __init__(self, frame_atoms: torch.Tensor, frame_kinds: torch.Tensor, *, batch_idx: torch.Tensor | None = None, validate: bool = True):
        if not isinstance(frame_atoms, torch.Tensor) or frame_atoms.dim() != 2 or frame_atoms.shape[1] != 3:
            raise ValueError(f"frame_atoms must have shape [num_atoms, 3], got {tuple(getattr(frame_atoms, 'shape', ()))}")
        n = frame_atoms.shape[0]
        if not isinstance(frame_kinds, torch.Tensor) or tuple(frame_kinds.shape) != (n,):
            raise ValueError(f"frame_kinds must have one entry per atom: expected shape [{n}], got {tuple(getattr(frame_kinds, 'shape', ()))}")
        for name, t in (("frame_atoms", frame_atoms), ("frame_kinds", frame_kinds)):
            if t.dtype not in (torch.int32, torch.int64):
                raise ValueError(f"{name} must be an int32 (or int64) tensor, got {t.dtype}")
        if frame_kinds.device != frame_atoms.device:
            raise ValueError(f"tensors on different devices: {frame_atoms.device} vs {frame_kinds.device}")
        if n > (1 << 29):
            raise ValueError(f"at most 2^29 atoms, got {n}")
        C.check_per_atom(n, batch_idx=batch_idx)
        if validate:
            _validate(frame_atoms, frame_kinds, batch_idx)
        dev = frame_atoms.device
        kinds = frame_kinds.to(torch.int32)
        known = (kinds >= 0) & (kinds <= FRAME_THREE_FOLD)
        use = torch.tensor(_SLOT_USE, dtype=torch.int32, device=dev)[torch.where(known, kinds, 0).long()]  # [N, 3]
        atoms = frame_atoms.to(torch.int32)
        atoms = torch.where((use > 0) & (atoms >= 0) & (atoms < n), atoms, -1).contiguous()
        codes = 4 * torch.arange(n, dtype=torch.int64, device=dev)[:, None] + torch.arange(1, 4, dtype=torch.int64, device=dev)[None, :]
        named = atoms >= 0
        target, code = atoms[named].long(), codes[named]
        order = torch.argsort(target * (4 * max(n, 1)) + code)  # by the atom named, then by code: all keys are distinct
        ptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        if n:
            ptr[1:] = torch.cumsum(torch.bincount(target, minlength=n), 0)
        self.num_atoms = n
        self.frame_atoms = atoms
        self.frame_kinds = torch.where(known, kinds, 0).contiguous()
        self.inverse_ptr = ptr.to(torch.int32).contiguous()
        self.inverse_slots = code[order].to(torch.int32).contiguous()

    def to(self, device) -> "LocalFrames":
        other = object.__new__(LocalFrames)
        other.num_atoms = self.num_atoms
        for name in ("frame_atoms", "frame_kinds", "inverse_ptr", "inverse_slots"):
            setattr(other, name, getattr(self, name).to(device))
        return other

    @property
    def device(self) -> torch.device:
        return self.frame_atoms.device

    def __repr__(self) -> str:
        return f"LocalFrames(num_atoms={self.num_atoms}, entries={self.inverse_slots.shape[0]}, device={self.device})"


def _validate(frame_atoms, frame_kinds, batch_idx) -> None:
    """Every ValueError of the tables' VALUES, on the host."""
    atoms, kinds = frame_atoms.detach().cpu().long(), frame_kinds.detach().cpu().long()
    n = atoms.shape[0]

    def first(mask):  # (atom, slot) of the first True of an [N, 3] mask, (atom,) of an [N] mask
        return tuple(int(v) for v in torch.nonzero(mask)[0])

    bad = (kinds < 0) | (kinds > FRAME_THREE_FOLD)
    if bool(bad.any()):
        (i,) = first(bad)
        raise ValueError(f"atom {i}: unknown frame kind {int(kinds[i])} (the kinds are {', '.join(f'{k} = {v}' for v, k in enumerate(_KIND_NAMES))})")
    bad = (atoms < -1) | (atoms >= n)
    if bool(bad.any()):
        i, s = first(bad)
        raise ValueError(f"atom {i}: frame atom index {int(atoms[i, s])} in slot {_SLOT_NAMES[s]} is outside [-1, {n})")
    use = torch.tensor(_SLOT_USE)[kinds]
    bad = (use == 2) & (atoms < 0)
    if bool(bad.any()):
        i, s = first(bad)
        raise ValueError(f"atom {i}: kind {_KIND_NAMES[int(kinds[i])]} requires a {_SLOT_NAMES[s]} atom, but slot {_SLOT_NAMES[s]} holds -1")
    used = torch.where(use > 0, atoms, -1)
    bad = used == torch.arange(n)[:, None]
    if bool(bad.any()):
        i, s = first(bad)
        raise ValueError(f"atom {i}: names itself as its {_SLOT_NAMES[s]} atom")
    z, x, y = used.unbind(-1)
    bad = ((z >= 0) & ((z == x) | (z == y))) | ((x >= 0) & (x == y))
    if bool(bad.any()):
        (i,) = first(bad)
        raise ValueError(f"atom {i}: a frame atom appears twice in {used[i].tolist()}")
    if batch_idx is not None:
        bi = batch_idx.detach().cpu().long()
        bad = (used >= 0) & (bi[used.clamp(min=0)] != bi[:, None])
        if bool(bad.any()):
            i, s = first(bad)
            raise ValueError(f"atom {i} (system {int(bi[i])}): its {_SLOT_NAMES[s]} atom {int(used[i, s])} is in another system "
                             f"({int(bi[used[i, s]])})")


# ---- argument checks --------------------------------------------------------------------------------------------------------------------------
def _check(positions, local_dipoles, local_quadrupoles, frames, cell, batch_idx, compute_virial=False):
    """Every argument error, before anything is launched.  Returns the number of systems."""
    if positions.dim() != 2 or positions.shape[1] != 3:
        raise ValueError(f"positions must have shape [num_atoms, 3], got {tuple(positions.shape)}")
    C.dtype_code(positions.dtype)
    n = positions.shape[0]
    if not isinstance(frames, LocalFrames):
        raise TypeError(f"frames must be a LocalFrames, got {type(frames)}")
    if frames.num_atoms != n:
        raise ValueError(f"frames describes {frames.num_atoms} atoms but positions has {n}")
    if local_dipoles is not None and tuple(local_dipoles.shape) != (n, 3):
        raise ValueError(f"local_dipoles must have one vector per atom: expected shape [{n}, 3], got {tuple(local_dipoles.shape)}")
    if local_quadrupoles is not None and tuple(local_quadrupoles.shape) != (n, 3, 3):
        raise ValueError(f"local_quadrupoles must have one 3 x 3 tensor per atom: expected shape [{n}, 3, 3], got {tuple(local_quadrupoles.shape)}")
    for name, t in (("local_dipoles", local_dipoles), ("local_quadrupoles", local_quadrupoles)):
        if t is not None and not t.dtype.is_floating_point:
            raise ValueError(f"{name} must be a floating-point tensor, got {t.dtype}")
    C.check_per_atom(n, batch_idx=batch_idx)
    if cell is None:
        if compute_virial:
            raise ValueError("compute_virial needs a cell")
        return 1
    if cell.dim() not in (2, 3) or tuple(cell.shape[-2:]) != (3, 3):
        raise ValueError(f"cell must have shape [3, 3] or [num_systems, 3, 3], got {tuple(cell.shape)}")
    n_cells = cell.shape[0] if cell.dim() == 3 else 1
    if batch_idx is None and n_cells != 1:
        raise ValueError(f"cell holds {n_cells} systems: batch_idx is required")
    return n_cells


def _inputs(positions, local_dipoles, local_quadrupoles, cell, batch_idx, frame_atoms, frame_kinds):
    """Detached contiguous launch tensors in the positions dtype (device check included; shapes were checked before)."""
    dt = positions.dtype
    C.require_device(positions, local_dipoles, local_quadrupoles, cell, batch_idx, frame_atoms, frame_kinds)
    conv = lambda t: None if t is None else t.detach().to(dt).contiguous()  # noqa: E731
    cells = None if cell is None else conv(cell.reshape(-1, 3, 3))
    batched = batch_idx is not None and cells is not None
    nsys = cells.shape[0] if batched else 1
    if cells is not None:
        cells = cells[:nsys].contiguous()
    return dict(pos=positions.detach().contiguous(), mu=conv(local_dipoles), qd=conv(local_quadrupoles), cells=cells,
                bi=C.i32(batch_idx) if batched else None, nsys=nsys, code=C.dtype_code(dt), atoms=C.i32(frame_atoms), kinds=C.i32(frame_kinds))


# ---- launches ---------------------------------------------------------------------------------------------------------------------------------
def _forward(positions, local_dipoles, local_quadrupoles, cell, batch_idx, frame_atoms, frame_kinds):
    """(dipoles | None, quadrupoles | None) in the positions dtype, no autograd graph: what the eager call and the `alchemiops::_rotate_multipoles`
    op both run."""
    n, dt, dev = positions.shape[0], positions.dtype, positions.device
    mu = torch.empty((n, 3), dtype=dt, device=dev) if local_dipoles is not None else None
    qd = torch.empty((n, 3, 3), dtype=dt, device=dev) if local_quadrupoles is not None else None
    if n == 0 or (mu is None and qd is None):
        return mu, qd
    p = _inputs(positions, local_dipoles, local_quadrupoles, cell, batch_idx, frame_atoms, frame_kinds)
    rc = C.lib().mi_frame_rotate(C.ptr(p["pos"]), C.ptr(p["mu"]), C.ptr(p["qd"]), C.ptr(p["atoms"]), C.ptr(p["kinds"]), C.ptr(p["cells"]),
                                 C.ptr(p["bi"]), n, p["nsys"], p["code"], C.ptr(mu), C.ptr(qd), C.stream_of(positions))
    C.check(rc, "mi_frame_rotate")
    return mu, qd


def _adjoint_launch(positions, local_dipoles, local_quadrupoles, cell, batch_idx, frame_atoms, frame_kinds, inverse_ptr, inverse_slots,
                    dipole_grads, quadrupole_grads, out_dtype, sign, local, virial):
    """`mi_frame_adjoint` + `mi_frame_gather`: (sign * dL/dpositions in `out_dtype`, float64 dL/dlocal_dipoles | None, float64
    dL/dlocal_quadrupoles | None, float64 virial [nsys, 3, 3] | None)."""
    n, dev = positions.shape[0], positions.device
    p = _inputs(positions, local_dipoles, local_quadrupoles, cell, batch_idx, frame_atoms, frame_kinds)
    C.require_device(positions, dipole_grads, quadrupole_grads, inverse_ptr, inverse_slots)
    dt = positions.dtype
    g_mu = None if (dipole_grads is None or p["mu"] is None) else dipole_grads.detach().to(dt).contiguous()
    g_qd = None if (quadrupole_grads is None or p["qd"] is None) else quadrupole_grads.detach().to(dt).contiguous()
    f64 = dict(dtype=torch.float64, device=dev)
    rec = torch.empty((n, 4, 3), **f64)
    lmu = torch.empty((n, 3), **f64) if (local and g_mu is not None) else None
    lqd = torch.empty((n, 3, 3), **f64) if (local and g_qd is not None) else None
    vrow = torch.empty((n, 9), **f64) if virial else None
    L, st = C.lib(), C.stream_of(positions)
    rc = L.mi_frame_adjoint(C.ptr(p["pos"]), C.ptr(p["mu"]), C.ptr(p["qd"]), C.ptr(p["atoms"]), C.ptr(p["kinds"]), C.ptr(p["cells"]), C.ptr(p["bi"]),
                            C.ptr(g_mu), C.ptr(g_qd), n, p["nsys"], p["code"], C.ptr(rec), C.ptr(lmu), C.ptr(lqd), C.ptr(vrow), st)
    C.check(rc, "mi_frame_adjoint")
    out = torch.empty((n, 3), dtype=out_dtype, device=dev)
    part = torch.empty((p["nsys"], int(L.mi_frame_blocks()), 9), **f64) if virial else None
    iptr, islots = C.i32(inverse_ptr), C.i32(inverse_slots)
    rc = L.mi_frame_gather(C.ptr(rec), C.ptr(iptr), C.ptr(islots), ctypes.c_longlong(islots.shape[0]), C.ptr(vrow), C.ptr(p["bi"]), n, p["nsys"],
                           C.dtype_code(out_dtype), C.cdouble(sign), C.ptr(out), C.ptr(part), st)
    C.check(rc, "mi_frame_gather")
    return out, lmu, lqd, C.fold_virial9(part) if virial else None


def _adjoint(positions, local_dipoles, local_quadrupoles, cell, batch_idx, frame_atoms, frame_kinds, inverse_ptr, inverse_slots, grad_dipoles,
             grad_quadrupoles):
    """Float64 (dL/dpositions, dL/dlocal_dipoles, dL/dlocal_quadrupoles) for the incoming gradients of the two outputs (None: zero); an input
    that was not given gets an empty [0] tensor."""
    n, dev = positions.shape[0], positions.device
    f64 = dict(dtype=torch.float64, device=dev)
    none = torch.zeros((0,), **f64)
    if n == 0:
        return (torch.zeros((0, 3), **f64), none if local_dipoles is None else torch.zeros((0, 3), **f64),
                none if local_quadrupoles is None else torch.zeros((0, 3, 3), **f64))
    gp, lmu, lqd, _ = _adjoint_launch(positions, local_dipoles, local_quadrupoles, cell, batch_idx, frame_atoms, frame_kinds, inverse_ptr,
                                      inverse_slots, grad_dipoles, grad_quadrupoles, torch.float64, 1.0, True, False)
    if lmu is None:
        lmu = none if local_dipoles is None else torch.zeros((n, 3), **f64)
    if lqd is None:
        lqd = none if local_quadrupoles is None else torch.zeros((n, 3, 3), **f64)
    return gp, lmu, lqd


# ---- public functions ---------------------------------------------------------------------------------------------------------------------------
@C.traceable
def rotate_multipoles(positions: torch.Tensor, local_dipoles: torch.Tensor | None, local_quadrupoles: torch.Tensor | None, frames: LocalFrames,
                      cell: torch.Tensor | None = None, *, batch_idx: torch.Tensor | None = None):
    """Laboratory-frame multipoles of atoms whose permanent multipoles are defined in local frames:

        dipoles [N, 3] = R mu_loc,    quadrupoles [N, 3, 3] = R Q_loc R^T,    Q_loc = 1/2 (Q + Q^T) of `local_quadrupoles`

    in the positions dtype (float64 arithmetic, rounded once), ready to pass to every `*_dipole_*` and `*_quadrupole_*` operator of this
    package.  R = [e_x e_y e_z] is the rotation of the atom's frame in `frames` (a `LocalFrames`; the module docstring has the table of kinds,
    FRAME_NONE is R = I).  `local_dipoles=None` or `local_quadrupoles=None` returns None in that place.

    GEOMETRY

    The result is differentiable once w.r.t. `positions`, `local_dipoles` and `local_quadrupoles`, for any upstream gradient: the call then
    goes through the `alchemiops::_rotate_multipoles` op with a hand-written adjoint (`mi_frame_adjoint` + `mi_frame_gather`), as it does
    under `torch.compile`, so `energies.sum().backward()` through any multipole operator gives the complete forces, torque terms included:
    -positions.grad.  Second-order gradients and a gradient w.r.t. `cell` raise NotImplementedError: the strain derivative is
    `multipole_frame_forces(compute_virial=True)`.  The chirality sign and the lab axis of FRAME_Z_ONLY are constants for the gradient.  CPU
    tensors raise NativeLibraryError: there is no fallback."""
    _check(positions, local_dipoles, local_quadrupoles, frames, cell, batch_idx)
    dt = positions.dtype
    if P.needs_op(positions, local_dipoles, local_quadrupoles, cell):
        from nvalchemiops import _eops

        mu, qd = _eops.rotate_multipoles_op(positions, None if local_dipoles is None else local_dipoles.to(dt),
                                            None if local_quadrupoles is None else local_quadrupoles.to(dt), cell, batch_idx, frames.frame_atoms,
                                            frames.frame_kinds, frames.inverse_ptr, frames.inverse_slots)
        return mu if local_dipoles is not None else None, qd if local_quadrupoles is not None else None
    return _forward(positions, local_dipoles, local_quadrupoles, cell, batch_idx, frames.frame_atoms, frames.frame_kinds)


@C.eager
def multipole_frame_forces(positions: torch.Tensor, local_dipoles: torch.Tensor | None, local_quadrupoles: torch.Tensor | None, frames: LocalFrames,
                           dipole_grads: torch.Tensor | None, quadrupole_grads: torch.Tensor | None, cell: torch.Tensor | None = None, *,
                           batch_idx: torch.Tensor | None = None, compute_local_gradients: bool = False, compute_virial: bool = False):
    """The torque forces of local-frame multipoles, on the explicit-gradient path (no autograd graph).

    `dipole_grads` [N, 3] and `quadrupole_grads` [N, 3, 3] are the caller's summed dE/dmu and dE/dQ of whatever corrections are in use
    (`compute_dipole_gradients=True`, `compute_quadrupole_gradients=True`), evaluated at the laboratory-frame multipoles of
    `rotate_multipoles`; a gradient whose local input is None is not read.  Those operators hold the multipoles fixed in space: their forces
    lack the term through which the multipoles follow the frame atoms,

        forces [N, 3] = -(dmu/dr . dE/dmu + dQ/dr : dE/dQ)

    which is returned here and has to be ADDED to the corrections' own forces.  It is the torque mu x (-dE/dmu) (and its quadrupole analogue)
    turned into forces on the frame-defining atoms: per molecule the torque forces sum to zero, and their moment balances that torque.

    Returns ``forces``, or a tuple with what was asked for, in this order: forces; with `compute_local_gradients` local_dipole_grads [N, 3] =
    dE/dmu_loc = R^T dE/dmu and local_quadrupole_grads [N, 3, 3] = dE/dQ_loc = R^T 1/2 (g + g^T) R (None where the local input is None); with
    `compute_virial` the term virial [num_systems, 3, 3] = -dE/d(strain) that has to be ADDED to the corrections' fixed-multipole virials (it
    needs a cell: ValueError without one, as the cluster operators).  All in the positions dtype (float64 arithmetic, rounded once).  The
    kernels are those of the adjoint of `rotate_multipoles`.

    GEOMETRY

    CPU tensors raise NativeLibraryError: there is no fallback."""
    nsys = _check(positions, local_dipoles, local_quadrupoles, frames, cell, batch_idx, compute_virial)
    n, dt, dev = positions.shape[0], positions.dtype, positions.device
    for name, g, shape in (("dipole_grads", dipole_grads, (n, 3)), ("quadrupole_grads", quadrupole_grads, (n, 3, 3))):
        if g is not None and tuple(g.shape) != shape:
            raise ValueError(f"{name} must have shape {list(shape)}, got {tuple(g.shape)}")
    if local_dipoles is not None and dipole_grads is None:
        raise ValueError("dipole_grads is required when local_dipoles is given")
    if local_quadrupoles is not None and quadrupole_grads is None:
        raise ValueError("quadrupole_grads is required when local_quadrupoles is given")
    if n == 0:
        z = lambda *shape: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
        f, lmu, lqd, vir = z(0, 3), None if local_dipoles is None else z(0, 3), None if local_quadrupoles is None else z(0, 3, 3), z(nsys, 3, 3)
    else:
        with torch.no_grad():
            f, lmu, lqd, vir = _adjoint_launch(positions, local_dipoles, local_quadrupoles, cell, batch_idx, frames.frame_atoms, frames.frame_kinds,
                                               frames.inverse_ptr, frames.inverse_slots, dipole_grads, quadrupole_grads, dt, -1.0,
                                               compute_local_gradients, compute_virial)
        lmu = None if lmu is None else lmu.to(dt)
        lqd = None if lqd is None else lqd.to(dt)
        vir = None if vir is None else vir.to(dt)
    out = (f,) + ((lmu, lqd) if compute_local_gradients else ()) + ((vir,) if compute_virial else ())
    return out if len(out) > 1 else out[0]


for _fn in (rotate_multipoles, multipole_frame_forces):
    _fn.__doc__ = _fn.__doc__.replace("GEOMETRY", _GEOMETRY)
del _fn

__all__ = ["LocalFrames", "rotate_multipoles", "multipole_frame_forces", "FRAME_NONE", "FRAME_Z_ONLY", "FRAME_Z_THEN_X", "FRAME_BISECTOR",
           "FRAME_Z_BISECT", "FRAME_THREE_FOLD"]
