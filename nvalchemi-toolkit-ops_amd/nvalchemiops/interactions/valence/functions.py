"""The valence (bonded) terms of a force field: bond stretch, angle bend, stretch-bend, out-of-plane bend and Fourier torsion, and the
coupled torsion terms stretch-torsion, angle-torsion and pi-torsion (torsion-torsion: tortor.py).

The electrostatics and vdw packages cover every non-bonded term of an AMOEBA-class model; this module is the bonded energy.  The definitions
are Tinker's (angles in radians, no 1/2 in front of a force constant).  All functions run on one HIP kernel family (csrc/valence.hip,
`mi_valence`): a term pass with one thread per term writes the term energy, a gradient record, the parameter gradients and the virial words;
a gather pass with one thread per atom sums the atom's slots in a fixed order.  All arithmetic is float64 whatever the positions dtype, there
are no atomics, and forward and adjoint are the same launch without and with per-atom weights, so every output is bit-reproducible.  The
reference package has no counterpart."""
from __future__ import annotations

import ctypes
import functools

import torch

from nvalchemiops import _capi as C
from nvalchemiops.interactions.electrostatics import _pairs as P
from nvalchemiops.interactions.valence.terms import ValenceTerms

BOND, ANGLE, STRETCH_BEND, OUT_OF_PLANE, TORSION, STRETCH_TORSION, ANGLE_TORSION, PI_TORSION = range(8)
PLANES = {"wdc": 0, "allinger": 1}
VALENCE_FORCES, VALENCE_PARAMETER_GRAD, VALENCE_VIRIAL, VALENCE_TERM_MAJOR = 1, 2, 4, 8
_NAMES = ("bond_stretch", "angle_bend", "stretch_bend", "out_of_plane_bend", "torsion", "stretch_torsion", "angle_torsion", "pi_torsion")
_ARITY = (2, 3, 3, 4, 4, 4, 4, 6)
_PARAMS = (2, 2, 5, 1, None, 15, 11, 1)  # columns of `parameters`; a torsion takes 2 F, F in 1..6

_COMMON_DOC = """`terms` is a `ValenceTerms` built once from the atom tuples; `parameters` [T, P] holds one row per term, float32 or float64, converted to
    the positions dtype.  With `cell` ([3, 3], or [num_systems, 3, 3] with `batch_idx`; rows are lattice vectors) every difference vector is
    reduced to its minimum image in float64, so molecules wrapped atom by atom and whole molecules agree.  The image is found by rounding the
    fractional coordinates: exact for vectors shorter than half the smallest cell height, as bonded vectors are, but not the shortest image
    in a strongly skewed cell.  With `cell=None` the system is a
    cluster and `compute_virial` raises ValueError.

    Returns ``energies`` [N], or a tuple (energies, forces [N, 3], parameter_grads [T, P], virial [num_systems, 3, 3]) holding only the items
    asked for, all in the positions dtype.  energies are atom shares, E_i = sum over the terms that name i of E_t / A: summing over atoms,
    or folding with `batch_idx`, gives the total.  forces = -dE/dr; parameter_grads = dE_total/dparameters; virial = -dE/d(strain) with cell and
    positions strained together, the sum over the difference vectors v of a term of -(dE/dv) (x) v.  Zero terms or zero atoms give zeros of
    the right shapes.  Energies are differentiable once w.r.t. positions and parameters (the same kernels with per-atom weights); the call then
    goes through its `alchemiops::` op, as it does under `torch.compile`.  Differentiating the explicit forces, parameter gradients or virial
    raises NotImplementedError; the cell has no gradient.  CPU tensors raise NativeLibraryError: there is no fallback."""


def _check(kind, positions, terms, parameters, cell, batch_idx, compute_virial):
    """Every argument error, before anything is launched.  Returns the number of systems.  `kind` None: a table without parameters, whose
    type the caller has checked (torsion_torsion)."""
    if positions.dim() != 2 or positions.shape[1] != 3:
        raise ValueError(f"positions must have shape [num_atoms, 3], got {tuple(positions.shape)}")
    C.dtype_code(positions.dtype)
    n = positions.shape[0]
    if not isinstance(terms, ValenceTerms):
        raise TypeError(f"terms must be a ValenceTerms, got {type(terms)}")
    if terms.num_atoms != n:
        raise ValueError(f"terms describes {terms.num_atoms} atoms but positions has {n}")
    if kind is not None:
        _check_parameters(kind, terms, parameters)
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
    return n_cells if batch_idx is not None else 1


def _check_parameters(kind, terms, parameters):
    name = _NAMES[kind]
    if terms.arity != _ARITY[kind]:
        raise ValueError(f"{name} takes terms of {_ARITY[kind]} atoms, got a table of {terms.arity}")
    if not isinstance(parameters, torch.Tensor) or parameters.dim() != 2 or parameters.shape[0] != terms.num_terms:
        raise ValueError(f"parameters must have shape [{terms.num_terms}, P] (one row per term), got {tuple(getattr(parameters, 'shape', ()))}")
    if parameters.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"parameters must be float32 or float64, got {parameters.dtype}")
    p = parameters.shape[1]
    if kind == TORSION:
        if p % 2 or not 2 <= p <= 12:
            raise ValueError(f"torsion parameters hold V_1..V_F and gamma_1..gamma_F: P = 2 F with F in 1..6, got P = {p}")
    elif p != _PARAMS[kind]:
        raise ValueError(f"{name} takes {_PARAMS[kind]} parameters per term, got P = {p}")


def _launch(kind, positions, parameters, cell, batch_idx, atoms, slot_ptr, slot_idx, consts, plane, flags, weights=None, energies=True):
    """One `mi_valence` launch: (energies | None and forces | None in the positions dtype, float64 parameter gradients | None, float64 virial
    [nsys, 3, 3] | None).  VALENCE_TERM_MAJOR in `flags` selects the other layout of the gradient record (tools/valence_bench.py times it)."""
    C.require_device(positions, parameters, cell, batch_idx, atoms, slot_ptr, slot_idx, weights)
    dt, dev, n, t = positions.dtype, positions.device, positions.shape[0], atoms.shape[0]
    conv = lambda x: None if x is None else x.detach().to(dt).contiguous()  # noqa: E731
    pos, par, cells = positions.detach().contiguous(), conv(parameters), None if cell is None else conv(cell.reshape(-1, 3, 3))
    batched = batch_idx is not None and cells is not None
    nsys = cells.shape[0] if batched else 1
    bi = C.i32(batch_idx) if batched else None
    atoms, slot_ptr, slot_idx = C.i32(atoms), C.i32(slot_ptr), C.i32(slot_idx)
    L = C.lib()
    f64 = dict(dtype=torch.float64, device=dev)
    e = torch.empty(n, dtype=dt, device=dev) if energies else None
    f = torch.empty((n, 3), dtype=dt, device=dev) if flags & VALENCE_FORCES else None
    pg = torch.empty((t, par.shape[1]), **f64) if flags & VALENCE_PARAMETER_GRAD else None
    part = torch.empty((nsys, int(L.mi_valence_blocks()), 9), **f64) if flags & VALENCE_VIRIAL else None
    nbytes = int(L.mi_valence_scratch_bytes(int(kind), t, int(flags)))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    rc = L.mi_valence(int(kind), C.ptr(pos), C.ptr(atoms), C.ptr(par), par.shape[1], C.ptr(cells), C.ptr(bi), C.ptr(weights), C.ptr(slot_ptr),
                      C.ptr(slot_idx), ctypes.c_longlong(slot_idx.shape[0]), n, t, nsys, C.dtype_code(dt), *(C.cdouble(c) for c in consts),
                      int(plane), int(flags), C.ptr(e), C.ptr(f), C.ptr(pg), C.ptr(part), C.ptr(scratch), ctypes.c_size_t(nbytes),
                      C.stream_of(pos))
    C.check(rc, "mi_valence")
    return e, f, pg, C.fold_virial9(part) if part is not None else None


def _forward(kind, positions, parameters, cell, batch_idx, atoms, slot_ptr, slot_idx, cubic, quartic, pentic, sextic, plane, forces, pgrads,
             virial):
    """(energies, forces | None, parameter_grads | None, virial | None) in the positions dtype, no autograd graph: what the eager call and
    the op both run."""
    dt = positions.dtype
    flags = (VALENCE_FORCES if forces else 0) | (VALENCE_PARAMETER_GRAD if pgrads else 0) | (VALENCE_VIRIAL if virial else 0)
    e, f, pg, vir = _launch(kind, positions, parameters, cell, batch_idx, atoms, slot_ptr, slot_idx, (cubic, quartic, pentic, sextic), plane, flags)
    return e, f, pg.to(dt) if pgrads else None, vir.to(dt) if virial else None


def _adjoint(kind, positions, parameters, cell, batch_idx, atoms, slot_ptr, slot_idx, cubic, quartic, pentic, sextic, plane, grad_energies):
    """Float64 (dL/dpositions, dL/dparameters) of L = sum_i g_i E_i: the forward kernels with weights."""
    g = grad_energies.detach().to(torch.float64).contiguous()
    _, f, pg, _ = _launch(kind, positions, parameters, cell, batch_idx, atoms, slot_ptr, slot_idx, (cubic, quartic, pentic, sextic), plane,
                          VALENCE_FORCES | VALENCE_PARAMETER_GRAD, weights=g, energies=False)
    return -f.to(torch.float64), pg


def _call(kind, positions, terms, parameters, cell, consts, plane, batch_idx, compute_forces, compute_parameter_gradients, compute_virial):
    nsys = _check(kind, positions, terms, parameters, cell, batch_idx, compute_virial)
    n, dev, dt = positions.shape[0], positions.device, positions.dtype
    want = (True, compute_forces, compute_parameter_gradients, compute_virial)
    if n == 0 or terms.num_terms == 0:
        z = lambda *shape: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
        return P.select((z(n), z(n, 3), z(*parameters.shape), z(nsys, 3, 3)), want)
    args = (positions, parameters.to(dt), cell, batch_idx, terms.atoms, terms.slot_ptr, terms.slot_idx, *(float(c) for c in consts), int(plane),
            bool(compute_forces), bool(compute_parameter_gradients), bool(compute_virial))
    return P.dispatch("VALENCE_OPS", functools.partial(_forward, kind), args, (positions, parameters), want, kind)


@C.traceable
def bond_stretch(positions: torch.Tensor, terms: ValenceTerms, parameters: torch.Tensor, cell: torch.Tensor | None = None, *, cubic: float = 0.0,
                 quartic: float = 0.0, batch_idx: torch.Tensor | None = None, compute_forces: bool = False,
                 compute_parameter_gradients: bool = False, compute_virial: bool = False):
    """Anharmonic bond stretching over the terms (a, b), `parameters` [T, 2] = (k, r0):

        E_t = k D^2 (1 + cubic D + quartic D^2),    D = |r_a - r_b| - r0

    THE ENERGY HAS NO 1/2: this is Tinker's convention, a caller whose force constant belongs to 1/2 k D^2 passes k / 2.  A Urey-Bradley term
    is this function on the 1-3 pairs.

    COMMON"""
    return _call(BOND, positions, terms, parameters, cell, (cubic, quartic, 0.0, 0.0), 0, batch_idx, compute_forces, compute_parameter_gradients,
                 compute_virial)


@C.traceable
def angle_bend(positions: torch.Tensor, terms: ValenceTerms, parameters: torch.Tensor, cell: torch.Tensor | None = None, *, cubic: float = 0.0,
               quartic: float = 0.0, pentic: float = 0.0, sextic: float = 0.0, batch_idx: torch.Tensor | None = None, compute_forces: bool = False,
               compute_parameter_gradients: bool = False, compute_virial: bool = False):
    """Anharmonic angle bending over the terms (a, b, c) with b the vertex, `parameters` [T, 2] = (k, theta0), radians:

        E_t = k D^2 (1 + cubic D + quartic D^2 + pentic D^3 + sextic D^4),    D = theta - theta0,  theta = angle(r_a - r_b, r_c - r_b)

    No 1/2 in front of k (Tinker's convention).  A straight angle (theta = 0 or pi) has no defined gradient.

    COMMON"""
    return _call(ANGLE, positions, terms, parameters, cell, (cubic, quartic, pentic, sextic), 0, batch_idx, compute_forces,
                 compute_parameter_gradients, compute_virial)


@C.traceable
def stretch_bend(positions: torch.Tensor, terms: ValenceTerms, parameters: torch.Tensor, cell: torch.Tensor | None = None, *,
                 batch_idx: torch.Tensor | None = None, compute_forces: bool = False, compute_parameter_gradients: bool = False,
                 compute_virial: bool = False):
    """Stretch-bend coupling over the terms (a, b, c) with b the vertex, `parameters` [T, 5] = (k1, k2, r1_0, r2_0, theta0), radians:

        E_t = (k1 (|r_a - r_b| - r1_0) + k2 (|r_c - r_b| - r2_0)) (theta - theta0)

    COMMON"""
    return _call(STRETCH_BEND, positions, terms, parameters, cell, (0.0,) * 4, 0, batch_idx, compute_forces, compute_parameter_gradients,
                 compute_virial)


@C.traceable
def out_of_plane_bend(positions: torch.Tensor, terms: ValenceTerms, parameters: torch.Tensor, cell: torch.Tensor | None = None, *,
                      cubic: float = 0.0, quartic: float = 0.0, pentic: float = 0.0, sextic: float = 0.0, plane: str = "wdc",
                      batch_idx: torch.Tensor | None = None, compute_forces: bool = False, compute_parameter_gradients: bool = False,
                      compute_virial: bool = False):
    """Out-of-plane bending at a trigonal centre over the terms (a, b, c, d) with b the centre and d the atom out of the plane,
    `parameters` [T, 1] = (k).  With u = r_a - r_b, v = r_c - r_b, w = r_d - r_b and V = w . (u x v):

        E_t = k X^2 (1 + cubic X + quartic X^2 + pentic X^3 + sextic X^4),    X = asin(|V| / sqrt(cc |w|^2)) >= 0
        plane="wdc"       cc = |u|^2 |v|^2 - (u . v)^2                 the angle of b-d to the plane a-b-c (Wilson-Decius-Cross)
        plane="allinger"  cc = |p|^2 |q|^2 - (p . q)^2, p = r_a - r_d, q = r_c - r_d    the height of b over the plane a-c-d

    (any other `plane` raises ValueError).  A planar term, V == 0, contributes an exact zero to the forces.

    COMMON"""
    if plane not in PLANES:
        raise ValueError(f"unknown plane {plane!r}: expected one of {sorted(PLANES)}")
    return _call(OUT_OF_PLANE, positions, terms, parameters, cell, (cubic, quartic, pentic, sextic), PLANES[plane], batch_idx, compute_forces,
                 compute_parameter_gradients, compute_virial)


@C.traceable
def torsion(positions: torch.Tensor, terms: ValenceTerms, parameters: torch.Tensor, cell: torch.Tensor | None = None, *,
            batch_idx: torch.Tensor | None = None, compute_forces: bool = False, compute_parameter_gradients: bool = False,
            compute_virial: bool = False):
    """Fourier torsions over the terms (a, b, c, d), `parameters` [T, 2 F] = (V_1 .. V_F, gamma_1 .. gamma_F) with F in 1..6, radians:

        E_t = sum_{n = 1..F} V_n (1 + cos(n phi - gamma_n)),    phi = atan2(|b2| b1 . (b2 x b3), (b1 x b2) . (b2 x b3))

    with b1 = r_b - r_a, b2 = r_c - r_b, b3 = r_d - r_c: the IUPAC dihedral, trans is pi.  The amplitudes carry no 1/2.  Improper torsions are
    this function on other atom tuples.  A table with odd P, or P outside 2..12, raises ValueError.

    COMMON"""
    return _call(TORSION, positions, terms, parameters, cell, (0.0,) * 4, 0, batch_idx, compute_forces, compute_parameter_gradients, compute_virial)


@C.traceable
def stretch_torsion(positions: torch.Tensor, terms: ValenceTerms, parameters: torch.Tensor, cell: torch.Tensor | None = None, *,
                    batch_idx: torch.Tensor | None = None, compute_forces: bool = False, compute_parameter_gradients: bool = False,
                    compute_virial: bool = False):
    """Stretch-torsion coupling over the terms (a, b, c, d), `parameters` [T, 15] = (k_11 k_12 k_13 k_21 .. k_33, r0_1 r0_2 r0_3,
    gamma_1 gamma_2 gamma_3), radians:

        E_t = sum_{m = 1..3} (r_m - r0_m) sum_{n = 1..3} k_mn (1 + cos(n phi - gamma_n))

    with r_1 = |r_b - r_a|, r_2 = |r_c - r_b|, r_3 = |r_d - r_c| and phi the dihedral of `torsion`.  AMOEBA's term has gamma = (0, pi, 0); a
    force field that couples the central bond only leaves the rows m = 1 and 3 zero.

    COMMON"""
    return _call(STRETCH_TORSION, positions, terms, parameters, cell, (0.0,) * 4, 0, batch_idx, compute_forces, compute_parameter_gradients,
                 compute_virial)


@C.traceable
def angle_torsion(positions: torch.Tensor, terms: ValenceTerms, parameters: torch.Tensor, cell: torch.Tensor | None = None, *,
                  batch_idx: torch.Tensor | None = None, compute_forces: bool = False, compute_parameter_gradients: bool = False,
                  compute_virial: bool = False):
    """Angle-torsion coupling over the terms (a, b, c, d), `parameters` [T, 11] = (k_11 k_12 k_13 k_21 k_22 k_23, theta0_1 theta0_2,
    gamma_1 gamma_2 gamma_3), radians:

        E_t = sum_{m = 1, 2} (theta_m - theta0_m) sum_{n = 1..3} k_mn (1 + cos(n phi - gamma_n))

    with theta_1 = angle(a, b, c), theta_2 = angle(b, c, d) and phi the dihedral of `torsion`.  A straight angle has no defined gradient.

    COMMON"""
    return _call(ANGLE_TORSION, positions, terms, parameters, cell, (0.0,) * 4, 0, batch_idx, compute_forces, compute_parameter_gradients,
                 compute_virial)


@C.traceable
def pi_torsion(positions: torch.Tensor, terms: ValenceTerms, parameters: torch.Tensor, cell: torch.Tensor | None = None, *,
               batch_idx: torch.Tensor | None = None, compute_forces: bool = False, compute_parameter_gradients: bool = False,
               compute_virial: bool = False):
    """Pi-orbital torsions about the bond c-d of two trigonal centres over the terms (a, b, c, d, e, f) of a `WideValenceTerms`, a and b
    bonded to c, e and f bonded to d, `parameters` [T, 1] = (k):

        E_t = k (1 - cos 2 phi),    phi = dihedral of the points (c + p, c, d, d + q),  p = (r_a - r_d) x (r_b - r_d),  q = (r_e - r_c) x (r_f - r_c)

    The minimum-imaged vectors are r_a - r_d, r_b - r_d, r_e - r_c, r_f - r_c and r_d - r_c, and the virial is the sum over these five.

    COMMON"""
    return _call(PI_TORSION, positions, terms, parameters, cell, (0.0,) * 4, 0, batch_idx, compute_forces, compute_parameter_gradients, compute_virial)


for _fn in (bond_stretch, angle_bend, stretch_bend, out_of_plane_bend, torsion, stretch_torsion, angle_torsion, pi_torsion):
    _fn.__doc__ = _fn.__doc__.replace("COMMON", _COMMON_DOC)
del _fn

__all__ = ["bond_stretch", "angle_bend", "stretch_bend", "out_of_plane_bend", "torsion", "stretch_torsion", "angle_torsion", "pi_torsion"]
