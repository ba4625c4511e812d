"""The raw-pointer boundary, GPU half: every public entry point gives the same result whatever the LAYOUT of its tensor arguments.

Every kernel is reached through `_capi.ptr(t)` = the bare `data_ptr()`; dtype, strides, storage offset and shape stay behind in Python.
Whether pointer and integers agree is decided by the `.contiguous()` / `.to()` / `C.i32()` calls of the entry points; a missing one is
silent (wrong numbers, no fault).  Each test here calls an entry point once with canonical arguments (checked once against the oracle of
the op's own parity module, so that two equally wrong results cannot agree), then again with ONE argument at a time replaced by an
equal-valued variant:

    off   offset view       big[1:] of an [n+1, ...] buffer: contiguous, non-zero storage offset ([N,3] fp32 is then only 4-byte aligned)
    col   column-strided    wide[..., 3:3+k] (1-D tensors: column 1 of an [n, 3] buffer)
    row   row-strided       double[::2]
    T     transposed        storage in reversed dimension order, permuted back (posT.t())
    F     Fortran cell      cell.transpose(-1, -2).contiguous().transpose(-1, -2)
    x0    stride-0          base[:1].expand(B, ...) of a [B, ...] buffer (cell, pbc, alpha of a batch whose systems share the value)
    i64   int64 for int32   what torch users have by default
    flt   other float       float64 next to float32 positions and the reverse (every fixture value is exactly representable in float32)
    grad  gradient layouts  grad outputs as a stride-0 expansion (out.sum()), row-strided, transposed and offset views (what (w * out).sum() gives)

Which variant goes to which argument (no tensor argument of a listed entry point is skipped; `-` = does not apply):

    argument class                                   off col row  T   F   x0  i64 flt
    positions [N,3] (also reference/current, k-vectors, math points)
                                                      x   x   x   x   -   -   -   (math points, current_positions: x)
    dipoles [N,3], k_vectors [K,3] / [B,K,3] of the
      point-dipole operators                          x   x   x   x   -   -   -   x
    quadrupoles [N,3,3]                               x   x   x   x   x   -   -   x      (T: the atom axis stored last; F: the two tensor
                                                                                          axes swapped in storage)
    k_vectors [B,K,3] of a batch in ONE cell          also as [1,K,3], as an offset view of that, and as x0
    external_field, initial_dipoles [N,3]             x   x   x   x   -   -   -   x
    cell [3,3] / [B,3,3]                              x   -   x*  -   x   x*  -   x      (* batch forms)
    pbc [3] / [B,3] (bool)                            x   -   x*  -   -   x*  -   -
    charges, values, raw energies, alpha [B]          x   x   x   -   -   x*  -   x      (values [N,C] also T)
    numbers, batch_idx, batch_ptr, neighbor_ptr,
      num_neighbors, cells_per_dimension              x   x   x   -   -   -   x   -
    neighbor_matrix, atom_to_cell_mapping             x   x   x   x   -   -   x   -
    neighbor_matrix_shifts, unit/neighbor_shifts      x   x   x   x   -   -   x   -
    neighbor_list [2,P]                               x   x   x   x   -   -   x   -
    D3 tables rcov, r4r2, c6ab, cn_ref, r0ab          x   x   x   T(c6ab, cn_ref, r0ab)  -   -   -   x
    D4 tables rcov, en, r4r2, zeff, gam, cn_ref,
      q_ref, c6_ref                                   x   x   x   T(cn_ref, q_ref, c6_ref) -   -   -   x
    D4 tables n_ref, ngw                              x   x   x   T(ngw)  -   -   x   -
    sigma, electronegativity, hardness, polarizability,
      initial_charges, total_charge [B]               x   x   x   -   -   -   -   x      (polarizability also as a Python number)
    meshes, k_squared                                 x   x   x   x   -   -   -   x*     (* not k_squared)
    pair_scales [N,M] beside a matrix                 x   x   x   x   -   -   -   x      (float32 or float64 WHATEVER the positions dtype:
    pair_scales [nnz] beside a list                   x   x   x   -   -   -   -   x       flt is the dtype the positions do not have)
    frame_atoms [N,3] (through `LocalFrames`)         x   x   x   x   -   -   x   -
    frame_kinds [N] (through `LocalFrames`)           x   x   x   -   -   -   x   -
    local_dipoles, dipole_grads [N,3]                 x   x   x   x   -   -   -   x      (the caller's gradients of `multipole_frame_forces`
    local_quadrupoles, quadrupole_grads [N,3,3]       x   x   x   x   x   -   -   x       are of any float dtype and layout)

`flt` goes to every float argument but the one whose dtype IS the dtype of the call and of its outputs: positions, and where there are
none `k_squared` (pme_green_structure_factor) and `raw_energies` (pme_energy_corrections_with_charge_grad).

Memory-safety rule of this file: every variant is built so that, from its `data_ptr()`, the storage holds at least as many BYTES as the
canonical tensor (`_variant` asserts it), index tensors are padded with 0 (a valid index) and float tensors with 0.5 (a point inside the
box).  A code path that ignored strides or dtype would read wrong values but stay inside the allocation: nothing here can cause an
out-of-bounds access, even against a broken library.  Everything that COULD go out of bounds is in tests/test_arg_contract_cpu.py, behind
a launch guard.  Shapes: 130 atoms (more than two waves, no multiple of 64) in a triclinic cell of 12 Bohr, a batch of 70 + 60 atoms,
cutoff 5 Bohr (20 - 60 neighbours), meshes (12, 10, 14) and (16, 8, 24), tables with 4 species present.  `dftd4`, `dftd4_atm`,
`gaussian_charge_correction`, `charge_equilibration` and the point-dipole operators have fixtures of their own (tests/layout_cases.py, which
says why); tests/test_layout_sensitivity_cpu.py checks without a GPU that an argument of theirs read one row off moves the result by 100 bars.

MEASURED on one MI355X for those four ops (variants run, all in one run; every sweep prints its line under `pytest -s`): dftd4 single
system 69 (matrix, `D4Parameters`) + 73 (CSR, tables as a dict) + 11 (float64 positions), batch 75 + 78 + 12; dftd4_atm 65 + 69 + 11,
44 + 44 (the tables on the compact block) and 71 + 74 + 12; gaussian_charge_correction 25 (matrix) + 29 (CSR) single, 31 + 34 batch, in float32 and in float64; charge_equilibration
33 + 37 (cluster batch), 50 + 54 (periodic Ewald batch) + 1 (stride-0 cell).  Worst |variant - canonical| / bar: 0 in every sweep, the
periodic solves included: every variant gave the bits of the canonical call.

Point-dipole operators, in float32 and in float64 alike (variants run; single system / batch): ewald_dipole_reciprocal_space 25 / 32,
pme_dipole_reciprocal_space 20 / 27, ewald_dipole_real_space 30 (matrix) + 34 (CSR) / 37 + 39, ewald_dipole_correction 35 + 39 / 42 + 44,
pme_dipole_correction 30 + 34 / 37 + 39: 1 088 variants.  The explicit sums gave the bits of the canonical call in every variant.  The mesh
term stayed within 0.0015 of its 1e-12 bar in float64 (float64 atomic adds in the spread) and gave the bits of the canonical call in
float32, where the spread adds in float64 and rounds once; so did `pme_dipole_correction` (0.0004 in float64).  DESIGN.md section 3.21.

Point quadrupoles, Thole damping and induced dipoles (fixtures `quadrupole`, `thole`, `induced` of tests/layout_cases.py; variants run,
single system / batch).  In float32 and in float64 alike: ewald_quadrupole_reciprocal_space 31 / 38 (+ 2 stride-0 and 2 [1, K, 3] forms on
the batch in one cell), ewald_quadrupole_real_space 36 (matrix) + 40 (CSR) / 43 + 45, ewald_quadrupole_correction 41 + 45 / 48 + 50,
thole_dipole_correction 30 + 34 / 36 + 39 (+ a Python number against a constant tensor in each): 1 120 variants.  In float64:
induced_dipoles and thole_induced_dipoles, each 44 + 48 / 49 + 53 with reciprocal="ewald" and 39 / 44 with reciprocal="pme": 554
variants.  Every variant of the explicit sums and of the "ewald" solves gave the BITS of the canonical call (dipoles and iteration
counts), and so did the "pme" solves, whose bar is twice `_check_solution`'s bound.  Gradient layouts: 10 ops in float32 and 14 in float64
(the four solves are float64 only), four grad-output layouts each, every gradient bit-identical to the contiguous backward.  With the
`.contiguous()` of `quadrupoles` taken out of the real-space launch (a patched `launch_inputs`, not committed) the col, row and T variants
of `ewald_quadrupole_real_space` and `ewald_quadrupole_correction` fail in every sweep; F does not and cannot: it hands the kernel Q
transposed, and 1/2 (Q + Q^T) is what the kernel uses.  DESIGN.md section 3.25.

Point quadrupoles on the mesh (fixture `pme_quadrupole`: the quadrupole fixture on mesh (12, 10, 14) at order 6; variants run, single system /
batch, in float32 and in float64 alike): pme_quadrupole_reciprocal_space 26 (+ 4 forms with a [3, 3] cell, a 0-d alpha and a Python number) /
33, pme_quadrupole_correction 36 (matrix) + 40 (CSR) (+ 2) / 43 + 45: 446 variants and 12 forms.  In float32 every variant gave the BITS of the
canonical call (the spread adds in float64 and rounds once); in float64 they stayed within 0.0034 of the 1e-12 bar of two runs.  Gradient
layouts of both entry points: bit-identical in float32, within that bar in float64.  DESIGN.md section 3.28.

Cluster multipoles, scaled pairs and local frames (fixtures `pair_scale`, `frames`, `cluster_induced` of tests/layout_cases.py; variants run,
single system / batch, in float32 and in float64 alike): coulomb_dipole_correction 26 (matrix) + 30 (CSR) + 18 (`cell=None`: the first
system as a cluster, a matrix without shifts whose rows hold padding between live entries) / 32 + 35 + 18, coulomb_quadrupole_correction
32 + 36 + 24 / 38 + 41 + 24, pair_scale_correction 37 + 40 with shifts and 32 + 35 under `minimum_image` / 43 + 45 and 37 + 40 (+ three
`None` forms per list against zero tensors), LocalFrames + rotate_multipoles + multipole_frame_forces 38 / 43 (+ `LocalFrames.to()`);
cluster_induced_dipoles (float64, cluster batch, undamped and Thole) 31 + 35 each (+ a Python number against a constant tensor): 1 620
variants, every one the BITS of the canonical call -- for the frames also `torch.equal` tables, for the solves dipoles and iteration counts.
Gradient layouts: 14 ops (the two cluster corrections and pair_scale_correction in both list forms, rotate_multipoles with both outputs;
single system and batch) x 4 grad-output layouts in each dtype, every gradient bit-identical to the contiguous backward.
With the `.contiguous()` of `pair_scales` taken out of `pair_scale._inputs` and the one of `dipole_grads` out of
`frames._adjoint_launch` (patched in a scratch run, not committed) all eight sweeps of `test_pair_scale_correction` and `test_local_frames`
fail: `pair_scales` col and row (both list forms) and T (matrix) in float64, where `.to(float64)` is the tensor itself, and T alone in
float32, where `.to()` copies a strided view into contiguous storage but keeps the strides of a dense transposed one; `dipole_grads` col,
row and T in both dtypes (the torque forces move by about 10).  `off` and `flt` do not and cannot fail: an offset view is contiguous from
its own pointer, and a dtype change copies.  DESIGN.md section 3.33."""
import functools
import re
import types

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import layout_cases as LC
from tests import systems as S
from tests import test_coulomb_gpu as TC
from tests import test_d3_atm_gpu as TATM
from tests import test_d3_gpu as TD3
from tests import test_d3_zero_atm_gpu as TZA
from tests import test_d3_zero_gpu as TZ
from tests import test_d4_atm_gpu as TD4A
from tests import test_d4_gpu as TD4
from tests import test_dipole_gpu as TDP
from tests import test_gaussian_charges_gpu as TG
from tests import test_induced_gpu as TI
from tests import test_math_gpu as TM
from tests import test_pme_dipole_gpu as TPD
from tests import test_pme_gpu as TP
from tests import test_qeq_gpu as TQ
from tests import test_quadrupole_gpu as TQD
from tests import test_thole_gpu as TTH

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, NA, NB = 130, 70, 60
RC, M = 5.0, 64
MESHES = [(12, 10, 14), (16, 8, 24)]
F32, F64, I32, I64 = torch.float32, torch.float64, torch.int32, torch.int64
_FAULT = []  # a HIP error was seen: nothing more is started on the device in this session


@pytest.fixture(autouse=True)
def _stop_after_a_device_fault():
    if _FAULT:
        pytest.exit(f"a device error was reported earlier ({_FAULT[0]}): no further GPU work in this session", returncode=3)
    yield


def _t(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


# ---- systems (tests/systems.py) ----------------------------------------------------------------------------------------------------------

_system = LC.system  # the lattice builder, in tests/layout_cases.py so that the CPU suite can build the same fixtures


@functools.lru_cache(maxsize=None)
def _fx(dtype_name, batch=False):
    """Canonical inputs (numpy + device) and the canonical neighbour data of the single system / the batch, built once per dtype."""
    from nvalchemiops.neighborlist import batch_cell_list, cell_list

    dt = np.dtype(dtype_name).type
    f = types.SimpleNamespace(dtype=dt, tdtype=F32 if dt == np.float32 else F64, batch=batch)
    if not batch:
        pos, cell, q, z = _system(N, 7, 12.0)
        f.n, f.pos, f.cell, f.q, f.z, f.pbc, f.bi, f.alpha = N, pos.astype(dt), cell.astype(dt)[None], q.astype(dt), z, np.ones((1, 3), bool), None, np.array([0.4], np.float32).astype(dt)
    else:
        a, b = _system(NA, 8, 12.0), _system(NB, 9, 11.0)
        f.n = NA + NB
        f.pos, f.cell = np.concatenate([a[0], b[0]]).astype(dt), np.stack([a[1], b[1]]).astype(dt)
        f.q, f.z = np.concatenate([a[2], b[2]]).astype(dt), np.concatenate([a[3], b[3]])
        f.pbc, f.bi, f.alpha = np.ones((2, 3), bool), np.repeat(np.arange(2, dtype=np.int32), [NA, NB]), np.array([0.4, 0.375], np.float32).astype(dt)
        f.bptr = np.array([0, NA, NA + NB], np.int32)
    f.P, f.C, f.Q, f.Zt, f.PBC, f.AL = _t(f.pos), _t(f.cell), _t(f.q), _t(f.z), _t(f.pbc), _t(f.alpha)
    f.BI = None if f.bi is None else _t(f.bi)
    if not batch:
        f.nm, f.num, f.sh = cell_list(f.P, RC, f.C[0], f.PBC[0], max_neighbors=M)
        f.lst, f.ptr, f.lsh = cell_list(f.P, RC, f.C[0], f.PBC[0], max_neighbors=M, return_neighbor_list=True)
        onm, onum, osh = O.cell_list(f.pos, RC, f.cell[0], [True] * 3, max_neighbors=M)
    else:
        f.nm, f.num, f.sh = batch_cell_list(f.P, RC, f.C, f.PBC, f.BI, max_neighbors=M)
        f.lst, f.ptr, f.lsh = batch_cell_list(f.P, RC, f.C, f.PBC, f.BI, max_neighbors=M, return_neighbor_list=True)
        onm, onum, osh = O.cell_list(f.pos, RC, f.cell, f.pbc, batch_idx=f.bi, max_neighbors=M)
    assert 20 <= int(onum.max()) <= M and np.array_equal(f.num.cpu().numpy(), onum)
    assert np.array_equal(O.canonical_pairs(f.nm.cpu().numpy(), onum, f.sh.cpu().numpy()), O.canonical_pairs(onm, onum, osh))
    f.nm_np, f.sh_np, f.lst_np, f.ptr_np, f.lsh_np = (t.cpu().numpy() for t in (f.nm, f.sh, f.lst, f.ptr, f.lsh))
    return f


# ---- variants ----------------------------------------------------------------------------------------------------------------------------

def _junk(t):
    return 0.5 if t.dtype.is_floating_point else (False if t.dtype == torch.bool else 0)


def _buffer(shape, like, dtype=None):
    return torch.full(tuple(shape), _junk(like), dtype=dtype or like.dtype, device=like.device)


def _offset(t):
    big = _buffer((t.shape[0] + 1,) + tuple(t.shape[1:]), t)
    big[1:] = t
    return big[1:]


def _rowstride(t):
    big = _buffer((2 * t.shape[0],) + tuple(t.shape[1:]), t)
    big[::2] = t
    return big[::2]


def _colstride(t):
    if t.dim() == 1:
        big = _buffer((t.shape[0], 3), t)
        big[:, 1] = t
        return big[:, 1]
    k = t.shape[-1]
    big = _buffer(tuple(t.shape[:-1]) + (k + 6,), t)
    big[..., 3:3 + k] = t
    return big[..., 3:3 + k]


def _transposed(t):
    perm = tuple(reversed(range(t.dim())))
    return t.permute(perm).contiguous().permute(perm)


def _fortran(t):
    return t.transpose(-1, -2).contiguous().transpose(-1, -2)


def _expand0(t):
    assert bool((t == t[:1]).all()), "stride-0 expansion needs a batch whose systems share the value"
    base = t[:1].repeat((t.shape[0],) + (1,) * (t.dim() - 1)).contiguous()  # a full [B, ...] buffer behind the pointer, not one row
    return base[:1].expand(t.shape)


def _int64(t):
    return t.to(I64)


def _otherfloat(t):
    dt = F32 if t.dtype == F64 else F64
    buf = torch.full((2 * t.numel() + 2,), 0.5, dtype=dt, device=t.device)  # twice the elements: as many bytes as the wider of the two
    v = buf[:t.numel()].view(t.shape)
    v.copy_(t)
    return v


KINDS = {"off": _offset, "col": _colstride, "row": _rowstride, "T": _transposed, "F": _fortran, "x0": _expand0, "i64": _int64, "flt": _otherfloat}
POS = "off col row T"
VEC = "off col row flt"       # float [N]
IDX = "off col row i64"       # int [N]
MAT = "off col row T i64"     # int [N, M] / [N, M, 3] / [2, P] / [P, 3]
CELL1 = "off F flt"           # one cell
CELLB = "off row F flt"       # [B, 3, 3]
TAB = "off col row flt"


def _same_values(a, b):
    """torch.equal, with NaN equal to NaN (the D4 tables hold NaN in the entries no kernel may read)."""
    if not a.dtype.is_floating_point:
        return torch.equal(a, b)
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))


def _variant(t, kind):
    v = KINDS[kind](t)
    assert v.shape == t.shape and _same_values(v.to(t.dtype), t), kind
    assert v.dtype != t.dtype or v.stride() != t.stride() or v.storage_offset() != 0, f"{kind}: not a different layout"
    behind = v.untyped_storage().nbytes() - v.storage_offset() * v.element_size()
    assert behind >= t.numel() * t.element_size(), f"{kind}: the storage behind the pointer is shorter than the canonical tensor"
    return v


def _tuple(out):
    return tuple(out) if isinstance(out, (tuple, list)) else (out,)


def _compare(out, ref, close, what):
    assert len(out) == len(ref), f"{what}: {len(out)} outputs, canonical call has {len(ref)}"
    for i, (o, r) in enumerate(zip(out, ref)):
        if r is None or not isinstance(r, torch.Tensor):
            assert o == r, f"{what} out{i}"
            continue
        assert tuple(o.shape) == tuple(r.shape), f"{what} out{i}: shape {tuple(o.shape)} vs {tuple(r.shape)}"
        if r.dtype.is_floating_point:
            assert o.dtype == r.dtype, f"{what} out{i}: dtype {o.dtype} vs {r.dtype}"
            close(o, r.detach().cpu().numpy(), f"{what} out{i}", i)
        else:  # integer outputs equal the canonical call's exactly
            assert torch.equal(o.to(r.dtype), r), f"{what} out{i}: integer output differs from the canonical call's"
    return True


def _guarded(fn, what, fails):
    """Run one variant; a mismatch or a refusal is collected (all variants of a test are reported together), a device error ends the session."""
    try:
        fn()
    except (AssertionError, ValueError, TypeError, IndexError, KeyError, NotImplementedError) as e:
        fails.append(f"{what}: {type(e).__name__}: {str(e)[:400]}")
    except RuntimeError as e:
        if re.search(r"(?i)hip|illegal|fault|abort|device-side", str(e)):
            _FAULT.append(f"{what}: {str(e)[:200]}")
            raise
        fails.append(f"{what}: {type(e).__name__}: {str(e)[:400]}")


def _sweep(what, call, kw, plan, close=None, ref=None):
    """call(**kw) once (or `ref`), then once per (argument, variant) of `plan`; every output against the canonical call's."""
    ref = _tuple(call(**kw)) if ref is None else ref
    fails, done = [], 0
    for arg, kinds in plan.items():
        for kind in kinds.split():
            def one(arg=arg, kind=kind):
                v = _variant(kw[arg], kind)
                _compare(_tuple(call(**{**kw, arg: v})), ref, close, f"{what}[{arg}:{kind}]")
            _guarded(one, f"{what}[{arg}:{kind}]", fails)
            done += 1
    if fails:  # reported when the test ends (`_collecting`), so that one run shows every sweep of a test
        _PENDING.append(f"{what}: {len(fails)} of {done} variants differ:\n  " + "\n  ".join(fails))
    return ref


_PENDING = []


def _collecting(test):
    """A test made of several sweeps fails once, at its end, with the differing variants of ALL its sweeps (and its own first error, if any)."""
    @functools.wraps(test)
    def run(*args, **kwargs):
        del _PENDING[:]
        try:
            test(*args, **kwargs)
        except AssertionError as e:
            _PENDING.append(f"{type(e).__name__}: {str(e)[:1500]}")
        found, _PENDING[:] = list(_PENDING), []
        assert not found, "\n".join(found)
    return run


def _sweep_shared(what, call, kw, shared, close=None):
    """Stride-0 expansion: the canonical call is the one with the value REPEATED for every system (a contiguous [B, ...] tensor)."""
    rep = {k: kw[k][:1].repeat((kw[k].shape[0],) + (1,) * (kw[k].dim() - 1)).contiguous() for k in shared}
    base = {**kw, **rep}
    return _sweep(what, call, base, {k: "x0" for k in shared}, close)


# ---- closeness: the functions and constants of each op's own oracle-parity module --------------------------------------------------------

def _close_d3(extras):
    def close(o, r, what, i):
        TD3._close(o, r, 1e-6, 1e-6 + extras[i] * (np.abs(r).max() if r.size else 0.0), what)  # tests/test_d3_gpu.py::_check
    return close


CLOSE_D3 = _close_d3([0.0, 5e-6, 0.0, 2e-7])   # energy, forces, coord_num, virial
CLOSE_ATM = _close_d3([0.0, 5e-6, 2e-7])       # energy, forces, virial (tests/test_d3_atm_gpu.py::_judge's extras)


def _close_pme(dtype):
    return lambda o, r, what, i: TP._close(o, r, dtype, what)  # tests/test_pme_gpu.py::_close


def CLOSE_COULOMB(o, r, what, i):
    TC._close(o, r, what)  # tests/test_coulomb_gpu.py::_close, rel = 1e-11


def CLOSE_MATH(o, r, what, i):
    np.testing.assert_allclose(o.cpu().numpy(), r, err_msg=what, **TM.TOL)  # tests/test_math_gpu.py::TOL


DTYPES = pytest.mark.parametrize("dtype", ["float32", "float64"])


# ==== neighbour lists =====================================================================================================================

def _pairs(nm, num, sh):
    return O.canonical_pairs(nm.cpu().numpy(), num.cpu().numpy(), sh.cpu().numpy())


@DTYPES
@pytest.mark.parametrize("coo", [False, True])
@_collecting
def test_cell_list_and_naive(dtype, coo):
    from nvalchemiops.neighborlist import cell_list, naive_neighbor_list, neighbor_list

    f = _fx(dtype)
    kw = dict(positions=f.P, cell=f.C[0], pbc=f.PBC[0])
    plan = dict(positions=POS, cell=CELL1, pbc="off")
    ref = _sweep("cell_list", lambda **a: cell_list(a["positions"], RC, a["cell"], a["pbc"], max_neighbors=M, return_neighbor_list=coo), kw, plan)
    if not coo:  # canonical vs oracle (the fixture did the same for its own call)
        onm, onum, osh = O.cell_list(f.pos, RC, f.cell[0], [True] * 3, max_neighbors=M)
        assert np.array_equal(_pairs(ref[0], ref[1], ref[2]), O.canonical_pairs(onm, onum, osh))
    _sweep("neighbor_list(cell_list)", lambda **a: neighbor_list(a["positions"], RC, cell=a["cell"], pbc=a["pbc"], method="cell_list", max_neighbors=M,
                                                                 return_neighbor_list=coo), kw, plan, ref=ref)
    # [1, 3, 3] cell and [1, 3] pbc, as the batch-minded caller passes them
    _sweep("cell_list[B=1]", lambda **a: cell_list(a["positions"], RC, a["cell"], a["pbc"], max_neighbors=M, return_neighbor_list=coo),
           dict(positions=f.P, cell=f.C, pbc=f.PBC), dict(cell="off F flt", pbc="off"), ref=ref)
    nref = _sweep("naive", lambda **a: naive_neighbor_list(a["positions"], RC, cell=a["cell"], pbc=a["pbc"], max_neighbors=M, return_neighbor_list=coo),
                  kw, plan)
    _sweep("neighbor_list(naive)", lambda **a: neighbor_list(a["positions"], RC, cell=a["cell"], pbc=a["pbc"], method="naive", max_neighbors=M,
                                                             return_neighbor_list=coo), kw, plan, ref=nref)
    fref = _sweep("naive free space", lambda **a: naive_neighbor_list(a["positions"], RC, max_neighbors=M, return_neighbor_list=coo),
                  dict(positions=f.P), dict(positions=POS))
    if not coo:
        onm, onum, osh = O.naive(f.pos, RC, f.cell[0], [True] * 3, max_neighbors=M)
        assert np.array_equal(_pairs(nref[0], nref[1], nref[2]), O.canonical_pairs(onm, onum, osh))
        onm, onum = O.naive(f.pos, RC, max_neighbors=M)
        assert np.array_equal(fref[1].cpu().numpy(), onum) and np.array_equal(np.sort(fref[0].cpu().numpy(), 1), np.sort(onm, 1))


@DTYPES
@pytest.mark.parametrize("coo", [False, True])
@_collecting
def test_batch_cell_list_and_batch_naive(dtype, coo):
    from nvalchemiops.neighborlist import batch_cell_list, batch_naive_neighbor_list, neighbor_list

    f = _fx(dtype, batch=True)
    kw = dict(positions=f.P, cell=f.C, pbc=f.PBC, batch_idx=f.BI)
    plan = dict(positions=POS, cell=CELLB, pbc="off row", batch_idx=IDX)
    bcl = lambda **a: batch_cell_list(a["positions"], RC, a["cell"], a["pbc"], a["batch_idx"], max_neighbors=M, return_neighbor_list=coo)  # noqa: E731
    ref = _sweep("batch_cell_list", bcl, kw, plan)
    _sweep("neighbor_list(batch_cell_list)", lambda **a: neighbor_list(a["positions"], RC, cell=a["cell"], pbc=a["pbc"], batch_idx=a["batch_idx"],
                                                                       method="batch_cell_list", max_neighbors=M, return_neighbor_list=coo), kw, plan, ref=ref)
    _sweep_shared("batch_cell_list", bcl, kw, ("cell", "pbc"))
    bptr = _t(f.bptr)
    bn = lambda **a: batch_naive_neighbor_list(a["positions"], RC, batch_idx=a["batch_idx"], batch_ptr=a["batch_ptr"], pbc=a["pbc"], cell=a["cell"],  # noqa: E731
                                               max_neighbors=M, return_neighbor_list=coo)
    nref = _sweep("batch_naive", bn, dict(kw, batch_ptr=bptr), dict(plan, batch_ptr="off row i64"))
    _sweep("neighbor_list(batch_naive)", lambda **a: neighbor_list(a["positions"], RC, cell=a["cell"], pbc=a["pbc"], batch_idx=a["batch_idx"],
                                                                   batch_ptr=a["batch_ptr"], method="batch_naive", max_neighbors=M,
                                                                   return_neighbor_list=coo), dict(kw, batch_ptr=bptr), dict(plan, batch_ptr="off row i64"), ref=nref)
    _sweep_shared("batch_naive", bn, dict(kw, batch_ptr=bptr), ("cell", "pbc"))
    _sweep("batch_naive free space", lambda **a: batch_naive_neighbor_list(a["positions"], RC, batch_idx=a["batch_idx"], max_neighbors=M,
                                                                           return_neighbor_list=coo), dict(positions=f.P, batch_idx=f.BI),
           dict(positions=POS, batch_idx=IDX))
    if not coo:
        onm, onum, osh = O.cell_list(f.pos, RC, f.cell, f.pbc, batch_idx=f.bi, max_neighbors=M)
        assert np.array_equal(_pairs(ref[0], ref[1], ref[2]), O.canonical_pairs(onm, onum, osh))
        off = 0
        for s, n in enumerate((NA, NB)):  # the naive semantics system by system (the oracle's naive search is single-system)
            onm, onum, osh = O.naive(f.pos[off:off + n], RC, f.cell[s], [True] * 3, max_neighbors=M, fill_value=f.n)
            got = _pairs(nref[0][off:off + n] - off, nref[1][off:off + n], nref[2][off:off + n])
            want = O.canonical_pairs(np.where(onm == f.n, f.n - off, onm), onum, osh)
            assert np.array_equal(got, want), f"batch_naive system {s}"
            off += n


@DTYPES
@_collecting
def test_dual_cutoff_forms(dtype):
    from nvalchemiops.neighborlist import batch_naive_neighbor_list_dual_cutoff, naive_neighbor_list_dual_cutoff, neighbor_list

    f = _fx(dtype)
    rc1 = 3.5
    kw = dict(positions=f.P, cell=f.C[0], pbc=f.PBC[0])
    plan = dict(positions=POS, cell=CELL1, pbc="off")
    ref = _sweep("naive_dual_cutoff", lambda **a: naive_neighbor_list_dual_cutoff(a["positions"], rc1, RC, pbc=a["pbc"], cell=a["cell"], max_neighbors1=M,
                                                                                  max_neighbors2=M), kw, plan)
    _sweep("neighbor_list(naive_dual_cutoff)", lambda **a: neighbor_list(a["positions"], rc1, cell=a["cell"], pbc=a["pbc"], cutoff2=RC,
                                                                         method="naive_dual_cutoff", max_neighbors1=M, max_neighbors2=M), kw, plan, ref=ref)
    for (nm, num, sh), rc in ((ref[:3], rc1), (ref[3:], RC)):
        onm, onum, osh = O.naive(f.pos, rc, f.cell[0], [True] * 3, max_neighbors=M, image_range_cutoff=RC)
        assert np.array_equal(_pairs(nm, num, sh), O.canonical_pairs(onm, onum, osh)), f"cutoff {rc}"
    b = _fx(dtype, batch=True)
    kwb = dict(positions=b.P, cell=b.C, pbc=b.PBC, batch_idx=b.BI)
    planb = dict(positions=POS, cell=CELLB, pbc="off row", batch_idx=IDX)
    dual = lambda **a: batch_naive_neighbor_list_dual_cutoff(a["positions"], rc1, RC, batch_idx=a["batch_idx"], pbc=a["pbc"], cell=a["cell"],  # noqa: E731
                                                             max_neighbors1=M, max_neighbors2=M)
    bref = _sweep("batch_naive_dual_cutoff", dual, kwb, planb)
    _sweep_shared("batch_naive_dual_cutoff", dual, kwb, ("cell", "pbc"))
    for (nm, num, sh), rc in ((bref[:3], rc1), (bref[3:], RC)):
        off = 0
        for s, n in enumerate((NA, NB)):
            onm, onum, osh = O.naive(b.pos[off:off + n], rc, b.cell[s], [True] * 3, max_neighbors=M, fill_value=b.n, image_range_cutoff=RC)
            want = O.canonical_pairs(np.where(onm == b.n, b.n - off, onm), onum, osh)
            assert np.array_equal(_pairs(nm[off:off + n] - off, num[off:off + n], sh[off:off + n]), want), f"batch dual, cutoff {rc}, system {s}"
            off += n


@DTYPES
@_collecting
def test_build_query_rebuild_detection_and_coo_conversion(dtype):
    from nvalchemiops.neighborlist import (allocate_cell_list, batch_build_cell_list, batch_query_cell_list, build_cell_list, cell_list_needs_rebuild,
                                           estimate_batch_cell_list_sizes, estimate_cell_list_sizes, get_neighbor_list_from_neighbor_matrix,
                                           neighbor_list_needs_rebuild, query_cell_list)

    f = _fx(dtype)
    ncell, radius = estimate_cell_list_sizes(f.C[0], f.PBC[0], RC)

    def build(**a):
        cache = allocate_cell_list(f.n, ncell, radius, f.P.device)
        build_cell_list(a["positions"], RC, a["cell"], a["pbc"], *cache)
        return (cache[0],) + tuple(cache[2:])

    kw = dict(positions=f.P, cell=f.C[0], pbc=f.PBC[0])
    plan = dict(positions=POS, cell=CELL1, pbc="off")
    cref = _sweep("build_cell_list", build, kw, plan)
    want = O.build_cell_cache(f.pos, RC, f.cell[0], [True] * 3, ncell)
    for got, w in zip(cref, want):
        assert np.array_equal(got.cpu().numpy().reshape(w.shape), w)
    cache = allocate_cell_list(f.n, ncell, radius, f.P.device)
    build_cell_list(f.P, RC, f.C[0], f.PBC[0], *cache)

    def query(**a):
        nm, sh, num = torch.full((f.n, M), f.n, dtype=I32, device=DEV), torch.zeros((f.n, M, 3), dtype=I32, device=DEV), torch.zeros(f.n, dtype=I32, device=DEV)
        query_cell_list(a["positions"], RC, a["cell"], a["pbc"], *cache, nm, sh, num)
        return nm, num, sh

    qref = _sweep("query_cell_list", query, kw, plan)
    assert np.array_equal(_pairs(*qref), _pairs(f.nm, f.num, f.sh))  # (the fixture's list is oracle-checked)
    # rebuild detection: unchanged positions (False) and a configuration in which atoms changed cells / moved beyond the skin (True)
    moved = f.P.clone()
    moved[::7] += 0.45 * f.C[0, 0]
    moved = moved.float().to(f.tdtype)  # (float32 numbers, like every fixture value: the other-float variant is equal-valued)
    for cur, label in ((f.P, "still"), (moved, "moved")):
        rkw = dict(current_positions=cur, atom_to_cell_mapping=cache[3], cells_per_dimension=cache[0], cell=f.C[0], pbc=f.PBC[0])
        r = _sweep(f"cell_list_needs_rebuild {label}", lambda **a: cell_list_needs_rebuild(**a), rkw,
                   dict(current_positions=POS, atom_to_cell_mapping=MAT, cells_per_dimension="off col row i64", cell=CELL1, pbc="off"))
        assert bool(r[0].item()) == O.cells_changed(cur.cpu().numpy(), f.cell[0], cache[3].cpu().numpy(), cache[0].cpu().numpy(), [True] * 3) == (label == "moved")
        r = _sweep(f"neighbor_list_needs_rebuild {label}", lambda **a: neighbor_list_needs_rebuild(a["reference_positions"], a["current_positions"], 0.5),
                   dict(reference_positions=f.P, current_positions=cur), dict(reference_positions=POS, current_positions=POS + " flt"))
        assert bool(r[0].item()) == O.moved_beyond_skin(f.pos, cur.cpu().numpy(), 0.5) == (label == "moved")
    # matrix -> COO
    coo = _sweep("get_neighbor_list_from_neighbor_matrix",
                 lambda **a: get_neighbor_list_from_neighbor_matrix(a["neighbor_matrix"], a["num_neighbors"], a["neighbor_shift_matrix"], fill_value=f.n),
                 dict(neighbor_matrix=f.nm, num_neighbors=f.num, neighbor_shift_matrix=f.sh), dict(neighbor_matrix=MAT, num_neighbors=IDX, neighbor_shift_matrix=MAT))
    olst, optr, olsh = O.matrix_to_coo(f.nm_np, f.num.cpu().numpy(), f.sh_np, fill_value=f.n)
    assert np.array_equal(coo[0].cpu().numpy(), olst) and np.array_equal(coo[1].cpu().numpy(), optr) and np.array_equal(coo[2].cpu().numpy(), olsh)
    # the batch build / query pair
    b = _fx(dtype, batch=True)
    bncell, bradius = estimate_batch_cell_list_sizes(b.C, b.PBC, RC)

    def bbuild(**a):
        c = allocate_cell_list(b.n, bncell, bradius, b.P.device)
        batch_build_cell_list(a["positions"], RC, a["cell"], a["pbc"], a["batch_idx"], *c)
        return (c[0],) + tuple(c[2:])

    kwb = dict(positions=b.P, cell=b.C, pbc=b.PBC, batch_idx=b.BI)
    planb = dict(positions=POS, cell=CELLB, pbc="off row", batch_idx=IDX)
    bcref = _sweep("batch_build_cell_list", bbuild, kwb, planb)
    for got, w in zip(bcref, O.build_cell_cache(b.pos, RC, b.cell, b.pbc, bncell, batch_idx=b.bi)):
        assert np.array_equal(got.cpu().numpy().reshape(w.shape), w)
    bcache = allocate_cell_list(b.n, bncell, bradius, b.P.device)
    batch_build_cell_list(b.P, RC, b.C, b.PBC, b.BI, *bcache)

    def bquery(**a):
        nm, sh, num = torch.full((b.n, M), b.n, dtype=I32, device=DEV), torch.zeros((b.n, M, 3), dtype=I32, device=DEV), torch.zeros(b.n, dtype=I32, device=DEV)
        batch_query_cell_list(a["positions"], a["cell"], a["pbc"], RC, a["batch_idx"], *bcache, nm, sh, num)
        return nm, num, sh

    bqref = _sweep("batch_query_cell_list", bquery, kwb, planb)
    assert np.array_equal(_pairs(*bqref), _pairs(b.nm, b.num, b.sh))


# ==== dispersion ==========================================================================================================================

def _r0ab(t):
    """A symmetric table of pair cutoff radii for the zero damping, float32 values (the sum rule of tests/test_d3_zero_gpu.py's tables)."""
    r = (t["rcov"].astype(np.float64) * 1.6 + 0.9).astype(np.float32)
    r0 = (r[:, None] + r[None, :]).astype(np.float32)
    r0[0, :] = r0[:, 0] = 0.0
    return r0


D3_BJ = dict(a1=0.4, a2=4.0, s8=0.8)
D3_CALLS = ("dftd3", "dftd3_zero", "dftd3_atm", "dftd3_zero_atm")
RC3 = 4.0


def _d3_call(name):
    from nvalchemiops.interactions import dispersion as D

    fn = getattr(D, name)
    extra = {"dftd3": D3_BJ, "dftd3_zero": TZ.ZERO, "dftd3_atm": dict(a1=0.4, a2=4.0, three_body_cutoff=RC3), "dftd3_zero_atm": dict(three_body_cutoff=RC3)}[name]

    def call(positions, numbers, **a):
        if "zero" not in name:
            a.pop("cutoff_radii")
        return fn(positions, numbers, **extra, compute_virial=True, **a)
    return call


def _d3_oracle(name, f, ref, t, r0, csr=False):
    """The canonical call against the reference of the op's own parity module, at that module's bar."""
    cell = f.cell if f.batch else f.cell[0]
    if name == "dftd3":
        # tests/test_d3_gpu.py::_check, its bars unchanged, against the float64 restatement of the same sum (tests/atm_reference.py, term
        # "two_body": the reference tests/test_d3_atm_gpu.py is built on).  It is the more accurate of the two host references and knows
        # nothing of the kernel: the wide-sum oracle of test_d3_gpu does its pair arithmetic in float32 and is itself 2.3e-6 away from it
        # in the forces of this dense fixture (52 neighbours on average), more than the forces' bar of 1.3e-6.  The distance to that
        # oracle is printed, not asserted.
        r64 = TATM.R.reference(f.pos, f.z, t, D3_BJ["a1"], D3_BJ["a2"], RC, s6=1.0, s8=D3_BJ["s8"], cell=cell, batch_idx=f.bi, term="two_body")
        want = tuple(r64[k].reshape(tuple(o.shape)) for k, o in zip(("energy", "forces", "cn", "virial"), ref))
        lists = dict(idx_j=f.lst_np[1], neighbor_ptr=f.ptr_np, unit_shifts=f.lsh_np) if csr else dict(neighbor_matrix=f.nm_np, neighbor_matrix_shifts=f.sh_np)
        wide = TD3._wide(f.pos, f.z, t, cell=f.cell, batch_idx=f.bi, compute_virial=True, num_systems=f.cell.shape[0], **lists, **TD3.FP)
        for key, o, w64, w32 in zip(("energy", "forces", "coord_num", "virial"), ref, want, wide):
            o = o.detach().cpu().numpy().astype(np.float64)
            print(f"[layouts dftd3{' csr' if csr else ''}{' batch' if f.batch else ''}] {key:9s} kernel vs float64 restatement {np.abs(o - w64).max():.3e}  "
                  f"kernel vs wide-sum oracle {np.abs(o - w32).max():.3e}  oracle vs restatement {np.abs(w32 - w64).max():.3e}  max|ref| {np.abs(w64).max():.3e}")
        TD3._check(ref, want, virial=True)
    elif name == "dftd3_zero":
        TZ._judge("layouts", ref, *TZ._references(f.pos, f.z, t, r0, RC, cell=cell, batch_idx=f.bi))
    elif name == "dftd3_atm":
        TATM._judge("layouts", ref, *TATM._references(f.pos, f.z, t, RC, RC3, cell=cell, batch_idx=f.bi))
    else:
        TZA._judge("layouts", ref, *TZA._references(f.pos, f.z, t, r0, RC, RC3, cell=cell, batch_idx=f.bi))


@pytest.mark.parametrize("name", D3_CALLS)
@pytest.mark.parametrize("batch", [False, True])
@_collecting
def test_dftd3_family(name, batch):
    f = _fx("float32", batch=batch)
    t = S.d3_test_tables(17)
    r0 = _r0ab(t)
    call = _d3_call(name)
    close = CLOSE_D3 if "atm" not in name else CLOSE_ATM
    tabs = dict(covalent_radii=_t(t["rcov"]), r4r2=_t(t["r4r2"]), c6_reference=_t(t["c6ab"]), coord_num_ref=_t(t["cn_ref"]), cutoff_radii=_t(r0))
    tplan = dict(covalent_radii=TAB, r4r2=TAB, c6_reference=TAB + " T", coord_num_ref=TAB + " T")
    if "zero" in name:
        tplan["cutoff_radii"] = TAB + " T"  # (a symmetric table: its transpose holds the same values)
    sysk = dict(positions=f.P, numbers=f.Zt, cell=f.C, **tabs)
    splan = dict(positions=POS, numbers=IDX, cell=CELLB if batch else CELL1, **tplan)
    if batch:
        sysk["batch_idx"], splan["batch_idx"] = f.BI, IDX
    ref = _sweep(f"{name} matrix", call, dict(sysk, neighbor_matrix=f.nm, neighbor_matrix_shifts=f.sh),
                 dict(splan, neighbor_matrix=MAT, neighbor_matrix_shifts=MAT), close)
    _d3_oracle(name, f, ref, t, r0)
    csr = _sweep(f"{name} csr", call, dict(sysk, neighbor_list=f.lst, neighbor_ptr=f.ptr, unit_shifts=f.lsh),
                 dict(positions=POS, numbers=IDX, cell=splan["cell"], neighbor_list=MAT, neighbor_ptr=IDX, unit_shifts=MAT), close)
    _d3_oracle(name, f, csr, t, r0, csr=True)
    if batch:
        _sweep_shared(f"{name} matrix", call, dict(sysk, neighbor_matrix=f.nm, neighbor_matrix_shifts=f.sh), ("cell",), close)
    # float64 positions with the float32 tables and cell of the call above (D3 outputs are float32 whatever the positions' dtype)
    g = _fx("float64", batch=batch)
    k64 = dict(sysk, positions=g.P, cell=g.C, neighbor_matrix=g.nm, neighbor_matrix_shifts=g.sh)
    _sweep(f"{name} matrix f64", call, k64, dict(positions=POS, cell=splan["cell"], neighbor_matrix="off i64", neighbor_matrix_shifts="off i64"), close)


# ---- DFT-D4 (its own fixture: tests/layout_cases.py says why) ------------------------------------------------------------------------------

RC4, RC43, M4 = LC.D4_RC, LC.D4_RC3, 128
_WORST = [0.0]  # largest error / bar of the sweep in progress (the closeness functions of the four newer ops record it)


def _count(plan):
    return sum(len(kinds.split()) for kinds in plan.values())


def _swept(what, call, kw, plan, close, ref=None, shared=()):
    """`_sweep` (+ `_sweep_shared` for the arguments in `shared`); prints the number of variants run and the worst error / bar among them."""
    _WORST[0] = 0.0
    ref = _sweep(what, call, kw, plan, close, ref=ref)
    if shared:
        _sweep_shared(what, call, kw, shared, close)
    print(f"[layouts] {what:44s} {_count(plan) + len(shared):3d} variants, worst error / bar {_WORST[0]:.3g}")
    return ref


def _close_bars(bars, keys):
    """Elementwise |variant - canonical| <= the bar of tests/test_d4_gpu.py::_bars / tests/test_d4_atm_gpu.py::_bars for that output."""
    def close(o, r, what, i):
        err, bar = np.abs(o.detach().cpu().numpy().astype(np.float64) - r.astype(np.float64)), bars[keys[i]][0]
        _WORST[0] = max(_WORST[0], float((err / bar).max()) if err.size else 0.0)
        assert (err <= bar).all(), f"{what}: max err {err.max():.3e}, worst err / bar {(err / bar).max():.3g}"
    return close


@functools.lru_cache(maxsize=None)
def _d4fx(batch, dtype_name="float32", compact=False):
    """A D4 fixture of tests/layout_cases.py on the device with both list layouts (cutoff 9 Bohr); tables and charges are float32."""
    from nvalchemiops.neighborlist import batch_cell_list, cell_list

    c, dt = LC.d4(batch, compact), np.dtype(dtype_name).type
    f = types.SimpleNamespace(batch=batch, n=len(c["pos"]), c=c)
    f.P, f.C, f.Q, f.Zt = _t(c["pos"].astype(dt)), _t(c["cell"].astype(dt)), _t(c["q"]), _t(c["z"])
    f.BI = None if not batch else _t(c["batch_idx"])
    pbc = torch.ones((f.C.shape[0], 3), dtype=torch.bool, device=DEV)
    if not batch:
        f.nm, f.num, f.sh = cell_list(f.P, RC4, f.C[0], pbc[0], max_neighbors=M4)
        f.lst, f.ptr, f.lsh = cell_list(f.P, RC4, f.C[0], pbc[0], max_neighbors=M4, return_neighbor_list=True)
    else:
        f.nm, f.num, f.sh = batch_cell_list(f.P, RC4, f.C, pbc, f.BI, max_neighbors=M4)
        f.lst, f.ptr, f.lsh = batch_cell_list(f.P, RC4, f.C, pbc, f.BI, max_neighbors=M4, return_neighbor_list=True)
    assert 8 <= int(f.num.max()) <= M4, "the rows of the neighbour matrix must hold every neighbour inside the list cutoff"
    f.tabs = {k: _t(c["tables"][k]) for k in LC.R.TABLE_KEYS}
    return f


D4_TPLAN = dict(rcov=TAB, en=TAB, r4r2=TAB, zeff=TAB, gam=TAB, n_ref=IDX, ngw=MAT, cn_ref=TAB + " T", q_ref=TAB + " T", c6_ref=TAB + " T")


def _d4_call(name, as_params, s9=None):
    from nvalchemiops.interactions.dispersion import D4Parameters, dftd4, dftd4_atm

    def call(positions, numbers, **a):
        tab = {k: a.pop(k) for k in LC.R.TABLE_KEYS}
        params = D4Parameters(**tab) if as_params else tab
        if name == "dftd4":
            return dftd4(positions, numbers, a.pop("charges"), **TD4.BJ, d4_params=params, compute_virial=True, **a)
        return dftd4_atm(positions, numbers, **TD4A.BJ, three_body_cutoff=RC43, s9=s9, d4_params=params, compute_virial=True, **a)
    return call


@pytest.mark.parametrize("name", ["dftd4", "dftd4_atm"])
@pytest.mark.parametrize("batch", [False, True])
@_collecting
def test_dftd4_family(name, batch):
    """Matrix layout with the tables as a `D4Parameters`, CSR with the tables as a dict; every argument in both."""
    f = _d4fx(batch)
    if name == "dftd4":
        r64, r32 = LC.d4_references(batch)
        bars, keys, judge, s9 = TD4._bars(r64, r32), TD4.KEYS, TD4._judge, None
        assert all(np.array_equal(bars[k][0], LC.d4_bar(r64, r32, k)) for k in keys)  # the bar the CPU suite measured the fixture against
    else:
        s9 = LC.d4_atm_s9(batch)
        assert (batch or s9 == 10.0) and RC43 <= RC4
        r64, r32 = LC.d4_atm_references(batch)
        bars, keys, judge = TD4A._bars(r64, r32), TD4A.KEYS, TD4A._judge
    close = _close_bars(bars, keys)
    sysk = dict(positions=f.P, numbers=f.Zt, cell=f.C, **f.tabs)
    splan = dict(positions=POS, numbers=IDX, cell=CELLB if batch else CELL1, **D4_TPLAN)
    if name == "dftd4":
        sysk["charges"], splan["charges"] = f.Q, VEC
    if batch:
        sysk["batch_idx"], splan["batch_idx"] = f.BI, IDX
    tag = f"{name}{' batch' if batch else ''}"
    mk = dict(sysk, neighbor_matrix=f.nm, neighbor_matrix_shifts=f.sh)
    ref = _tuple(_d4_call(name, True, s9)(**mk))
    judge(f"layouts {tag} matrix", ref, r64, r32)  # the canonical call against the op's own reference, at its own module's bar
    _swept(f"{tag} matrix, D4Parameters", _d4_call(name, True, s9), mk, dict(splan, neighbor_matrix=MAT, neighbor_matrix_shifts=MAT), close, ref=ref,
           shared=("cell",) if batch else ())
    ck = dict(sysk, neighbor_list=f.lst, neighbor_ptr=f.ptr, unit_shifts=f.lsh)
    csr = _tuple(_d4_call(name, False, s9)(**ck))
    judge(f"layouts {tag} csr", csr, r64, r32)
    _swept(f"{tag} csr, tables as a dict", _d4_call(name, False, s9), ck, dict(splan, neighbor_list=MAT, neighbor_ptr=IDX, unit_shifts=MAT), close, ref=csr)
    # float64 positions and cell with the float32 tables and charges of the calls above (D4 outputs are float32 whatever the positions' dtype)
    g = _d4fx(batch, "float64")
    k64 = dict(sysk, positions=g.P, cell=g.C, neighbor_matrix=g.nm, neighbor_matrix_shifts=g.sh)
    r = _tuple(_d4_call(name, True, s9)(**k64))
    judge(f"layouts {tag} matrix f64", r, r64, r32)
    _swept(f"{tag} matrix f64", _d4_call(name, True, s9), k64, dict(positions=POS, cell=splan["cell"], neighbor_matrix="off i64", neighbor_matrix_shifts="off i64"),
           close, ref=r)
    if name == "dftd4_atm" and not batch:
        # The tables once more on the compact 130-atom block: on the single system above rolled `en` moves the three-body term by 66 bars
        # only, on this one every table moves it by more than 100 (tests/test_layout_sensitivity_cpu.py).
        f, s9 = _d4fx(False, compact=True), LC.d4_atm_s9(False, True)
        r64, r32 = LC.d4_atm_references(False, True)
        close = _close_bars(TD4A._bars(r64, r32), keys)
        sysk = dict(positions=f.P, numbers=f.Zt, cell=f.C, **f.tabs)
        for label, as_params, lists in (("matrix, D4Parameters", True, dict(neighbor_matrix=f.nm, neighbor_matrix_shifts=f.sh)),
                                        ("csr, tables as a dict", False, dict(neighbor_list=f.lst, neighbor_ptr=f.ptr, unit_shifts=f.lsh))):
            ref = _tuple(_d4_call(name, as_params, s9)(**sysk, **lists))
            judge(f"layouts {name} compact {label}", ref, r64, r32)
            _swept(f"{name} compact {label}", _d4_call(name, as_params, s9), dict(sysk, **lists), D4_TPLAN, close, ref=ref)


# ==== electrostatics ======================================================================================================================

@pytest.fixture(params=["tile", "auto"])
def spread_path(request, monkeypatch):
    """Both spread / gather pipelines, as tests/test_pme_gpu.py's autouse fixture: the tile kernels forced wherever the mesh allows them, and
    the library's own policy (small systems: zero-fill + atomic spread + per-atom gather)."""
    from nvalchemiops import spline

    monkeypatch.setattr(spline, "_SPREAD_PATH", request.param)
    return request.param


@DTYPES
@pytest.mark.parametrize("batch", [False, True])
@_collecting
def test_ewald_real_space_and_coulomb(dtype, batch):
    from nvalchemiops.interactions.electrostatics import ewald_real_space, ewald_real_space_with_virial
    from nvalchemiops.interactions.electrostatics.coulomb import coulomb_energy, coulomb_energy_forces, coulomb_forces

    f = _fx(dtype, batch=batch)
    close = _close_pme(f.dtype)
    sysk = dict(positions=f.P, charges=f.Q, cell=f.C, alpha=f.AL)
    splan = dict(positions=POS, charges=VEC, cell=CELLB if batch else CELL1, alpha="off row flt")
    if batch:
        sysk["batch_idx"], splan["batch_idx"] = f.BI, IDX
    okw = dict(batch_idx=f.bi, compute_forces=True, compute_charge_gradients=True)
    ocell, oalpha = (f.cell, f.alpha) if batch else (f.cell[0], float(f.alpha[0]))
    for fn, label in ((ewald_real_space, "ewald_real_space"), (ewald_real_space_with_virial, "ewald_real_space_with_virial")):
        mat = lambda fn=fn, **a: fn(mask_value=f.n, compute_forces=True, compute_charge_gradients=True, **a)  # noqa: E731
        ref = _sweep(f"{label} matrix", mat, dict(sysk, neighbor_matrix=f.nm, neighbor_matrix_shifts=f.sh),
                     dict(splan, neighbor_matrix=MAT, neighbor_matrix_shifts=MAT), close)
        want = O.ewald_real_space(f.pos, f.q, ocell, oalpha, neighbor_matrix=f.nm_np, neighbor_matrix_shifts=f.sh_np, mask_value=f.n, **okw)
        for o, r, w in zip(ref, want, ("energies", "forces", "charge_grads")):
            TP._close(o, r, f.dtype, f"{label} {w} vs oracle")
        lst = lambda fn=fn, **a: fn(compute_forces=True, compute_charge_gradients=True, **a)  # noqa: E731
        csr = _sweep(f"{label} csr", lst, dict(sysk, neighbor_list=f.lst, neighbor_ptr=f.ptr, neighbor_shifts=f.lsh),
                     dict(positions=POS, charges=VEC, neighbor_list=MAT, neighbor_ptr=IDX, neighbor_shifts=MAT), close)
        _compare(csr, ref, close, f"{label} csr vs matrix")
        if batch:
            _sweep_shared(f"{label} matrix", mat, dict(sysk, neighbor_matrix=f.nm, neighbor_matrix_shifts=f.sh), ("cell", "alpha"), close)
    if dtype != "float64":
        return  # the cut-off Coulomb ops compute in float64 and round to the input dtype: their 1e-11 bar is a float64 bar
    ck = dict(positions=f.P, charges=f.Q, cell=f.C)
    cplan = dict(positions=POS, charges=VEC, cell=CELLB if batch else CELL1)
    if batch:
        ck["batch_idx"], cplan["batch_idx"] = f.BI, IDX
    for fn in (coulomb_energy, coulomb_forces, coulomb_energy_forces):
        run = lambda fn=fn, **a: fn(a.pop("positions"), a.pop("charges"), a.pop("cell"), 4.5, 0.3, **a)  # noqa: E731
        mref = _sweep(f"{fn.__name__} matrix", run, dict(ck, neighbor_matrix=f.nm, neighbor_matrix_shifts=f.sh),
                      dict(cplan, neighbor_matrix=MAT, neighbor_matrix_shifts=MAT), CLOSE_COULOMB)
        lref = _sweep(f"{fn.__name__} list", run, dict(ck, neighbor_list=f.lst, neighbor_ptr=f.ptr, neighbor_shifts=f.lsh),
                      dict(cplan, neighbor_list=MAT, neighbor_ptr=IDX, neighbor_shifts=MAT), CLOSE_COULOMB)
        oe, of = O.coulomb(f.pos, f.q, f.cell, 4.5, 0.3, neighbor_list=f.lst_np, neighbor_ptr=f.ptr_np, neighbor_shifts=f.lsh_np, batch_idx=f.bi)
        oem, ofm = O.coulomb(f.pos, f.q, f.cell, 4.5, 0.3, neighbor_matrix=f.nm_np, neighbor_matrix_shifts=f.sh_np, batch_idx=f.bi,
                             compute_forces=fn is not coulomb_energy)
        for got, want in ((lref, (oe, of)), (mref, (oem, ofm))):
            want = {"coulomb_energy": (want[0],), "coulomb_forces": (want[1],), "coulomb_energy_forces": want}[fn.__name__]
            for o, r in zip(got, want):
                TC._close(o, r, f"{fn.__name__} vs oracle")
        if batch:
            _sweep_shared(f"{fn.__name__} matrix", run, dict(ck, neighbor_matrix=f.nm, neighbor_matrix_shifts=f.sh), ("cell",), CLOSE_COULOMB)


@DTYPES
@_collecting
def test_ewald_reciprocal_space_and_summation(dtype):
    from nvalchemiops.interactions.electrostatics import (ewald_real_space, ewald_reciprocal_space, ewald_summation,
                                                          generate_k_vectors_ewald_summation)

    f = _fx(dtype)
    close = _close_pme(f.dtype)
    kv = generate_k_vectors_ewald_summation(f.C[0], 2.0)
    kw = dict(positions=f.P, charges=f.Q, cell=f.C[0], k_vectors=kv, alpha=f.AL)
    plan = dict(positions=POS, charges=VEC, cell=CELL1, k_vectors=POS, alpha="off row flt")
    ref = _sweep("ewald_reciprocal_space", lambda **a: ewald_reciprocal_space(compute_forces=True, compute_charge_gradients=True, **a), kw, plan, close)
    for o, r, w in zip(ref, O.ewald_reciprocal_space(f.pos, f.q, f.cell[0], kv.cpu().numpy(), float(f.alpha[0])), ("energies", "forces", "charge_grads")):
        TP._close(o, r, f.dtype, f"ewald_reciprocal_space {w} vs oracle")
    skw = dict(positions=f.P, charges=f.Q, cell=f.C[0], alpha=f.AL, k_vectors=kv, neighbor_matrix=f.nm, neighbor_matrix_shifts=f.sh)
    sref = _sweep("ewald_summation", lambda **a: ewald_summation(mask_value=f.n, compute_forces=True, **a), skw,
                  dict(plan, neighbor_matrix=MAT, neighbor_matrix_shifts=MAT), close)
    real = ewald_real_space(f.P, f.Q, f.C, f.AL, neighbor_matrix=f.nm, neighbor_matrix_shifts=f.sh, mask_value=f.n, compute_forces=True)
    _compare(sref, (real[0] + ref[0], real[1] + ref[1]), close, "ewald_summation = real + reciprocal (both oracle-checked)")
    b = _fx(dtype, batch=True)
    bkv = generate_k_vectors_ewald_summation(b.C, 2.0)
    bkw = dict(positions=b.P, charges=b.Q, cell=b.C, k_vectors=bkv, alpha=b.AL, batch_idx=b.BI)
    bref = _sweep("ewald_reciprocal_space batch", lambda **a: ewald_reciprocal_space(compute_forces=True, **a), bkw,
                  dict(positions=POS, charges=VEC, cell=CELLB, k_vectors="off row T", alpha="off row flt", batch_idx=IDX), close)
    off = 0
    for s, n in enumerate((NA, NB)):
        oe, of, _ = O.ewald_reciprocal_space(b.pos[off:off + n], b.q[off:off + n], b.cell[s], bkv[s].cpu().numpy(), float(b.alpha[s]))
        TP._close(bref[0][off:off + n], oe, b.dtype, f"batch energies {s}")
        TP._close(bref[1][off:off + n], of, b.dtype, f"batch forces {s}")
        off += n


@DTYPES
@pytest.mark.parametrize("dims", MESHES)
@_collecting
def test_pme(dtype, dims, spread_path):
    from nvalchemiops.interactions.electrostatics import (particle_mesh_ewald, particle_mesh_ewald_with_virial, pme_reciprocal_space,
                                                          pme_reciprocal_space_with_virial)

    f = _fx(dtype)
    close = _close_pme(f.dtype)
    kw = dict(positions=f.P, charges=f.Q, cell=f.C[0], alpha=f.AL)
    plan = dict(positions=POS, charges=VEC, cell=CELL1, alpha="off row flt")
    flags = dict(mesh_dimensions=dims, spline_order=4, compute_forces=True, compute_charge_gradients=True)
    want = O.pme_reciprocal_space(f.pos, f.q, f.cell[0], float(f.alpha[0]), dims, 4, compute_forces=True, compute_charge_gradients=True)
    for fn in (pme_reciprocal_space, pme_reciprocal_space_with_virial):
        ref = _sweep(fn.__name__, lambda fn=fn, **a: fn(**a, **flags), kw, plan, close)
        for o, r, w in zip(ref, want, ("energies", "forces", "charge_grads")):
            TP._close(o, r, f.dtype, f"{fn.__name__} {w} vs oracle")
        _sweep(fn.__name__ + " [1,3,3] cell", lambda fn=fn, **a: fn(**a, **flags), dict(kw, cell=f.C), dict(cell=CELL1), close, ref=ref)
    want = O.particle_mesh_ewald(f.pos, f.q, f.cell[0], float(f.alpha[0]), dims, 4, neighbor_matrix=f.nm_np, neighbor_matrix_shifts=f.sh_np,
                                 mask_value=f.n, compute_forces=True, compute_charge_gradients=True)
    for fn in (particle_mesh_ewald, particle_mesh_ewald_with_virial):
        ref = _sweep(fn.__name__ + " matrix", lambda fn=fn, **a: fn(mask_value=f.n, **a, **flags), dict(kw, neighbor_matrix=f.nm, neighbor_matrix_shifts=f.sh),
                     dict(plan, neighbor_matrix=MAT, neighbor_matrix_shifts=MAT), close)
        for o, r, w in zip(ref, want, ("energies", "forces", "charge_grads")):
            TP._close(o, r, f.dtype, f"{fn.__name__} {w} vs oracle")
        csr = _sweep(fn.__name__ + " csr", lambda fn=fn, **a: fn(**a, **flags), dict(kw, neighbor_list=f.lst, neighbor_ptr=f.ptr, neighbor_shifts=f.lsh),
                     dict(neighbor_list=MAT, neighbor_ptr=IDX, neighbor_shifts=MAT), close)
        _compare(csr, ref, close, fn.__name__ + " csr vs matrix")


@DTYPES
@_collecting
def test_pme_batch(dtype, spread_path):
    from nvalchemiops.interactions.electrostatics import particle_mesh_ewald, pme_reciprocal_space

    b = _fx(dtype, batch=True)
    close = _close_pme(b.dtype)
    dims = MESHES[0]
    kw = dict(positions=b.P, charges=b.Q, cell=b.C, alpha=b.AL, batch_idx=b.BI)
    plan = dict(positions=POS, charges=VEC, cell=CELLB, alpha="off row flt", batch_idx=IDX)
    flags = dict(mesh_dimensions=dims, spline_order=4, compute_forces=True)
    rec = lambda **a: pme_reciprocal_space(**a, **flags)  # noqa: E731
    ref = _sweep("pme_reciprocal_space batch", rec, kw, plan, close)
    want = O.pme_reciprocal_space(b.pos, b.q, b.cell, b.alpha, dims, 4, batch_idx=b.bi, compute_forces=True)
    for o, r, w in zip(ref, want, ("energies", "forces")):
        TP._close(o, r, b.dtype, f"batch {w} vs oracle")
    _sweep_shared("pme_reciprocal_space batch", rec, kw, ("cell", "alpha"), close)
    full = lambda **a: particle_mesh_ewald(mask_value=b.n, **a, **flags)  # noqa: E731
    ref = _sweep("particle_mesh_ewald batch", full, dict(kw, neighbor_matrix=b.nm, neighbor_matrix_shifts=b.sh),
                 dict(plan, neighbor_matrix=MAT, neighbor_matrix_shifts=MAT), close)
    want = O.particle_mesh_ewald(b.pos, b.q, b.cell, b.alpha, dims, 4, batch_idx=b.bi, neighbor_matrix=b.nm_np, neighbor_matrix_shifts=b.sh_np,
                                 mask_value=b.n, compute_forces=True)
    for o, r, w in zip(ref, want, ("energies", "forces")):
        TP._close(o, r, b.dtype, f"batch PME {w} vs oracle")
    _sweep_shared("particle_mesh_ewald batch", full, dict(kw, neighbor_matrix=b.nm, neighbor_matrix_shifts=b.sh), ("cell", "alpha"), close)


@DTYPES
@_collecting
def test_pme_green_structure_factor_and_corrections(dtype):
    from nvalchemiops.interactions.electrostatics import generate_k_vectors_pme, pme_energy_corrections_with_charge_grad, pme_green_structure_factor

    f = _fx(dtype)
    close = _close_pme(f.dtype)
    for dims in MESHES:
        _, k2 = generate_k_vectors_pme(f.C[0], dims)
        _, ok2 = O.generate_k_vectors_pme(f.cell[0], dims)
        ref = _sweep(f"pme_green_structure_factor {dims}", lambda **a: pme_green_structure_factor(a["k_squared"], dims, a["alpha"], a["cell"], 4),
                     dict(k_squared=k2, alpha=f.AL, cell=f.C[0]), dict(k_squared="off col row T", alpha="off row flt", cell=CELL1), close)
        for o, r, w in zip(ref, O.pme_green_structure_factor(ok2, dims, float(f.alpha[0]), f.cell[0], 4), ("green", "sf2")):
            TP._close(o, r, f.dtype, w)
    raw = np.random.default_rng(2).normal(size=f.n).astype(np.float32).astype(f.dtype)
    ref = _sweep("pme_energy_corrections_with_charge_grad", lambda **a: pme_energy_corrections_with_charge_grad(**a),
                 dict(raw_energies=_t(raw), charges=f.Q, cell=f.C[0], alpha=f.AL), dict(raw_energies="off col row", charges=VEC, cell=CELL1, alpha="off row flt"), close)
    for o, r, w in zip(ref, O.pme_energy_corrections(raw, f.q, f.cell[0], float(f.alpha[0]), with_charge_grad=True), ("corrections", "charge grad")):
        TP._close(o, r, f.dtype, w)
    b = _fx(dtype, batch=True)
    rawb = np.random.default_rng(3).normal(size=b.n).astype(np.float32).astype(b.dtype)
    bkw = dict(raw_energies=_t(rawb), charges=b.Q, cell=b.C, alpha=b.AL, batch_idx=b.BI)
    ref = _sweep("pme_energy_corrections_with_charge_grad batch", lambda **a: pme_energy_corrections_with_charge_grad(**a), bkw,
                 dict(raw_energies="off col row", charges=VEC, cell=CELLB, alpha="off row flt", batch_idx=IDX), close)
    for o, r, w in zip(ref, O.pme_energy_corrections(rawb, b.q, b.cell, b.alpha, batch_idx=b.bi, with_charge_grad=True), ("corrections", "charge grad")):
        TP._close(o, r, b.dtype, "batch " + w)
    _sweep_shared("pme_energy_corrections_with_charge_grad batch", lambda **a: pme_energy_corrections_with_charge_grad(**a), bkw, ("cell", "alpha"), close)


# ---- Gaussian-smeared charges and charge equilibration --------------------------------------------------------------------------------------

MG = 192


@functools.lru_cache(maxsize=None)
def _gfx(dtype_name, batch):
    """The Gaussian fixture of tests/layout_cases.py on the device (cutoff 7 Bohr: 90 - 130 neighbours) and its reference, computed once."""
    from nvalchemiops.neighborlist import batch_cell_list, cell_list

    c, dt = LC.gaussian(batch), np.dtype(dtype_name).type
    f = types.SimpleNamespace(batch=batch, n=len(c["pos"]), tdtype=F32 if dt == np.float32 else F64)
    f.P, f.C, f.Q, f.S = (_t(c[k].astype(dt)) for k in ("pos", "cell", "q", "sigma"))
    f.BI = None if not batch else _t(c["batch_idx"])
    pbc = torch.ones((f.C.shape[0], 3), dtype=torch.bool, device=DEV)
    if not batch:
        f.nm, f.num, f.sh = cell_list(f.P, LC.GC_RC, f.C[0], pbc[0], max_neighbors=MG)
        f.lst, f.ptr, f.lsh = cell_list(f.P, LC.GC_RC, f.C[0], pbc[0], max_neighbors=MG, return_neighbor_list=True)
    else:
        f.nm, f.num, f.sh = batch_cell_list(f.P, LC.GC_RC, f.C, pbc, f.BI, max_neighbors=MG)
        f.lst, f.ptr, f.lsh = batch_cell_list(f.P, LC.GC_RC, f.C, pbc, f.BI, max_neighbors=MG, return_neighbor_list=True)
    assert 64 < int(f.num.max()) <= MG
    f.rel = 1e-11 if dt == np.float64 else 1e-6  # tests/test_gaussian_charges_gpu.py: test_parity_fp64_matrix_and_csr / test_fp32_inputs
    f.ref = TG._ref(f.P, f.Q, f.S, f.C, TG.R.entries_from_matrix(f.nm, f.sh, f.n), batch_idx=f.BI, distance_dtype=f.tdtype)
    return f


def _close_gaussian(rel):
    def close(o, r, what, i):
        _WORST[0] = max(_WORST[0], TG._close(o, r, what, rel) / rel)
    return close


@DTYPES
@pytest.mark.parametrize("batch", [False, True])
@_collecting
def test_gaussian_charge_correction(dtype, batch):
    from nvalchemiops.interactions.electrostatics import gaussian_charge_correction as gcc

    f = _gfx(dtype, batch)
    close = _close_gaussian(f.rel)
    call = lambda positions, charges, sigma, cell, **a: gcc(positions, charges, sigma, cell, **a, **TG.ALL)  # noqa: E731
    sysk = dict(positions=f.P, charges=f.Q, sigma=f.S, cell=f.C)
    splan = dict(positions=POS, charges=VEC, sigma=VEC, cell=CELLB if batch else CELL1)
    if batch:
        sysk["batch_idx"], splan["batch_idx"] = f.BI, IDX
    tag = f"gaussian {dtype}{' batch' if batch else ''}"
    for label, lists, lplan in (("matrix", dict(neighbor_matrix=f.nm, neighbor_matrix_shifts=f.sh, mask_value=f.n), dict(neighbor_matrix=MAT, neighbor_matrix_shifts=MAT)),
                                ("csr", dict(neighbor_list=f.lst, neighbor_ptr=f.ptr, neighbor_shifts=f.lsh), dict(neighbor_list=MAT, neighbor_ptr=IDX, neighbor_shifts=MAT))):
        ref = _tuple(call(**sysk, **lists))
        assert len(ref) == 5
        for name, o in zip(TG.NAMES, ref):  # the canonical call against the float64 restatement, at the module's bar
            assert o.dtype == f.tdtype
            TG._close(o, f.ref[name], f"{tag} {label} {name} vs the restatement", f.rel)
        _swept(f"{tag} {label}", call, dict(sysk, **lists), dict(splan, **lplan), close, ref=ref, shared=("cell",) if batch and label == "matrix" else ())


def _qeq_lists(c):
    nm, sh = TQ._lists(*c["ent"], c["n"], c["width"], c["n"])
    lst, ptr, lsh = TQ._csr(nm, sh, c["n"])
    return nm, sh, lst, ptr, lsh


def _exact(o, r, what, i):
    assert np.array_equal(o.detach().cpu().numpy(), r), f"{what}: not bit-identical to the canonical call (max difference {np.abs(o.detach().cpu().numpy() - r).max():.3e})"


@_collecting
def test_charge_equilibration_cluster_batch():
    """No cell: the solve is free of atomics, so every variant gives the BITS of the canonical call -- charges, chemical potentials,
    iteration counts -- from a warm start and per-system total charges."""
    from nvalchemiops.interactions.electrostatics import charge_equilibration as qeq

    c = LC.qeq_cluster()
    nm, sh, lst, ptr, lsh = _qeq_lists(c)
    h, chi, total, bi = LC.qeq_dense(c, DEV)

    def call(positions, electronegativity, hardness, sigma, **a):
        out = qeq(positions, electronegativity, hardness, sigma, tolerance=LC.QEQ_TOL, return_info=True, **a)
        return out.charges, out.chemical_potential, out.iterations

    sysk = dict(positions=_t(c["pos"]), electronegativity=chi, hardness=_t(c["hard"]), sigma=_t(c["sigma"]), initial_charges=_t(c["q0"]), total_charge=total,
                batch_idx=bi)
    splan = dict(positions=POS, electronegativity=VEC, hardness=VEC, sigma=VEC, initial_charges=VEC, total_charge=VEC, batch_idx=IDX)
    for label, lists, lplan in (("matrix", dict(neighbor_matrix=nm, mask_value=c["n"]), dict(neighbor_matrix=MAT)),
                                ("csr", dict(neighbor_list=lst, neighbor_ptr=ptr), dict(neighbor_list=MAT, neighbor_ptr=IDX))):
        out = qeq(sysk["positions"], chi, sysk["hardness"], sysk["sigma"], tolerance=LC.QEQ_TOL, return_info=True,
                  **{k: sysk[k] for k in ("initial_charges", "total_charge", "batch_idx")}, **lists)
        TQ._check_solution(out, h, chi, total, bi, c["nsys"], LC.QEQ_TOL, 200, f"layouts cluster batch {label}")
        assert int(out.iterations.min()) > 0
        _swept(f"charge_equilibration cluster {label}", call, dict(sysk, **lists), dict(splan, **lplan), _exact,
               ref=(out.charges, out.chemical_potential, out.iterations))


@pytest.mark.parametrize("same_cell", [False, True], ids=["two_cells", "x0"])
@_collecting
def test_charge_equilibration_periodic_ewald_batch(same_cell):
    """reciprocal="ewald" with given k-vectors and one alpha per system.  Reciprocal space adds with atomics in arrival order, so a variant
    is within TWICE the bound `_check_solution` derives from the dense operator for the distance of a converged solve to the exact charges
    (each of the two calls is within once of them); chemical potentials within ||H|| times that.  `x0`: both systems in the same cell, which
    is then a stride-0 expansion."""
    from nvalchemiops.interactions.electrostatics import charge_equilibration as qeq

    c = LC.qeq_periodic(same_cell)
    nm, sh, lst, ptr, lsh = _qeq_lists(c)
    h, chi, total, bi = LC.qeq_dense(c, DEV)
    bound = torch.tensor(LC.qeq_charge_bound(h, chi, total, bi, c["nsys"]), dtype=F64, device=DEV)
    hmax = torch.stack([torch.linalg.eigvalsh(h[bi == s][:, bi == s]).abs().max() for s in range(c["nsys"])])
    bars = ((2.0 * bound)[bi.long()].cpu().numpy(), (2.0 * bound * hmax).cpu().numpy())

    def close(o, r, what, i):
        err = np.abs(o.detach().cpu().numpy() - r)
        _WORST[0] = max(_WORST[0], float((err / bars[i]).max()))
        assert (err <= bars[i]).all(), f"{what}: max err {err.max():.3e}, worst err / bar {(err / bars[i]).max():.3g}"

    def call(positions, electronegativity, hardness, sigma, cell, **a):
        out = qeq(positions, electronegativity, hardness, sigma, cell, reciprocal="ewald", tolerance=LC.QEQ_TOL, return_info=True, **a)
        return out.charges, out.chemical_potential

    sysk = dict(positions=_t(c["pos"]), electronegativity=chi, hardness=_t(c["hard"]), sigma=_t(c["sigma"]), cell=_t(c["cell"]), initial_charges=_t(c["q0"]),
                total_charge=total, alpha=_t(c["alpha"]), k_vectors=_t(c["kv"]), batch_idx=bi)
    splan = dict(positions=POS, electronegativity=VEC, hardness=VEC, sigma=VEC, cell=CELLB, initial_charges=VEC, total_charge=VEC, alpha=VEC, k_vectors=POS,
                 batch_idx=IDX)
    for label, lists, lplan in (("matrix", dict(neighbor_matrix=nm, neighbor_matrix_shifts=sh, mask_value=c["n"]), dict(neighbor_matrix=MAT, neighbor_matrix_shifts=MAT)),
                                ("csr", dict(neighbor_list=lst, neighbor_ptr=ptr, neighbor_shifts=lsh), dict(neighbor_list=MAT, neighbor_ptr=IDX, neighbor_shifts=MAT))):
        if same_cell and label == "csr":
            continue  # (the whole plan runs on the two-cell batch; here only `cell` is swept, once)
        a = {k: v for k, v in sysk.items() if k not in ("positions", "electronegativity", "hardness", "sigma", "cell")}
        out = qeq(sysk["positions"], chi, sysk["hardness"], sysk["sigma"], sysk["cell"], reciprocal="ewald", tolerance=LC.QEQ_TOL, return_info=True, **a, **lists)
        TQ._check_solution(out, h, chi, total, bi, c["nsys"], LC.QEQ_TOL, 200, f"layouts periodic ewald batch {label}")
        _swept(f"charge_equilibration ewald {'x0 ' if same_cell else ''}{label}", call, dict(sysk, **lists), {} if same_cell else dict(splan, **lplan), close,
               ref=(out.charges, out.chemical_potential), shared=("cell",) if same_cell else ())


# ---- point dipoles: explicit Ewald sum and particle-mesh Ewald ---------------------------------------------------------------------------------

DIP = POS + " flt"  # dipoles [N, 3], k_vectors [K, 3] / [B, K, 3]


@functools.lru_cache(maxsize=None)
def _dfx(dtype_name, batch):
    """The dipole fixture of tests/layout_cases.py on the device with both list layouts (cutoff 7 Bohr) and its restatements, computed once:
    the explicit sum (total, real-space half, reciprocal half) on the stored entries and the fixture's k set, the mesh term in float64 and
    -- for the float32 bar -- in the restatement's float32 mode."""
    from nvalchemiops.neighborlist import batch_cell_list, cell_list

    c, dt = LC.dipole(batch), np.dtype(dtype_name).type
    f = types.SimpleNamespace(batch=batch, n=len(c["pos"]), tdtype=F32 if dt == np.float32 else F64)
    f.P, f.C, f.Q, f.MU, f.AL, f.KV = (_t(c[k].astype(dt)) for k in ("pos", "cell", "q", "mu", "alpha", "kv"))
    f.BI = None if not batch else _t(c["batch_idx"])
    pbc = torch.ones((f.C.shape[0], 3), dtype=torch.bool, device=DEV)
    if not batch:
        f.nm, f.num, f.sh = cell_list(f.P, LC.GC_RC, f.C[0], pbc[0], max_neighbors=MG)
        f.lst, f.ptr, f.lsh = cell_list(f.P, LC.GC_RC, f.C[0], pbc[0], max_neighbors=MG, return_neighbor_list=True)
    else:
        f.nm, f.num, f.sh = batch_cell_list(f.P, LC.GC_RC, f.C, pbc, f.BI, max_neighbors=MG)
        f.lst, f.ptr, f.lsh = batch_cell_list(f.P, LC.GC_RC, f.C, pbc, f.BI, max_neighbors=MG, return_neighbor_list=True)
    assert 64 < int(f.num.max()) <= MG and f.KV.shape[-2] > 256
    f.rel = 1e-11 if dt == np.float64 else 1e-6  # tests/test_dipole_gpu.py: test_parity_fp64_matrix_and_csr / test_parity_fp32_inputs
    ent = TDP.R.entries_from_matrix(f.nm, f.sh, f.n)
    ev = lambda entries, kv: TDP.R.evaluate(f.P, f.Q, f.MU, f.C, f.AL, entries, kv, batch_idx=f.BI, distance_dtype=f.tdtype)  # noqa: E731
    f.ref = dict(total=ev(ent, f.KV), real=ev(ent, None), recip=ev(None, f.KV), mesh=LC.dipole_reference(batch, "pme"))
    if dt == np.float32:
        low = LC.dipole_reference(batch, "pme", dtype=F32)
        f.mesh_rel = {k: 4.0 * float(np.abs(low[k] - f.ref["mesh"][k]).max() / np.abs(f.ref["mesh"][k]).max()) for k in LC.DP_NAMES}  # tests/test_pme_dipole_gpu.py
    else:
        f.mesh_rel = {k: 1e-10 for k in LC.DP_NAMES}
    f.two_runs = 1e-12 if dt == np.float64 else 1e-6  # two device results of the mesh term (float atomics in the spread)
    return f


def _close_two_runs(rel):
    """|variant - canonical| <= rel x max |canonical| per output: the mesh term's spread adds with float atomics."""
    def close(o, r, what, i):
        err, scale = np.abs(o.detach().cpu().numpy().astype(np.float64) - r.astype(np.float64)).max(), np.abs(r).max()
        if err / (rel * scale) > _WORST[0]:
            _WORST[0] = float(err / (rel * scale))
            print(f"    {what}: {_WORST[0]:.3g} of the bar")
        assert err <= rel * scale, f"{what}: max err {err:.3e} > {rel * scale:.3e}"
    return close


@DTYPES
@pytest.mark.parametrize("batch", [False, True])
@_collecting
def test_point_dipole_operators(dtype, batch):
    """`ewald_dipole_correction`, `ewald_dipole_real_space`, `ewald_dipole_reciprocal_space`, `pme_dipole_reciprocal_space` and
    `pme_dipole_correction`, all outputs.  The explicit sums use no atomics: every variant must give the BITS of the canonical call (the
    `flt` variants too: every fixture value is a float32 number).  The mesh term, and the correction that contains it, within 1e-12
    (float64) / 1e-6 (float32) of the largest canonical value per output."""
    from nvalchemiops.interactions.electrostatics import (ewald_dipole_correction, ewald_dipole_real_space, ewald_dipole_reciprocal_space,
                                                          pme_dipole_correction, pme_dipole_reciprocal_space)

    f = _dfx(dtype, batch)
    mesh = dict(mesh_dimensions=LC.DP_MESH, spline_order=LC.DP_ORDER)
    two_runs = _close_two_runs(f.two_runs)
    tag = f"{dtype}{' batch' if batch else ''}"
    atoms = dict(positions=f.P, charges=f.Q, dipoles=f.MU, cell=f.C, alpha=f.AL)
    aplan = dict(positions=POS, charges=VEC, dipoles=DIP, cell=CELLB if batch else CELL1, alpha=VEC)
    if batch:
        atoms["batch_idx"], aplan["batch_idx"] = f.BI, IDX
    shared = ("cell", "alpha") if batch else ()

    def against_restatement(out, ref, rel, what):
        assert len(out) == 5
        for name, o in zip(LC.DP_NAMES, out):
            assert o.dtype == f.tdtype
            if isinstance(rel, dict):
                TPD._close(o.reshape(ref[name].shape), ref[name], f"{what} {name} vs the restatement", rel[name])
            else:
                TDP._close(o, ref[name], f"{what} {name} vs the restatement", rel)

    # the halves that take no list
    call = lambda **a: ewald_dipole_reciprocal_space(**a, **TDP.ALL)  # noqa: E731
    kw = dict(atoms, k_vectors=f.KV)
    ref = _tuple(call(**kw))
    against_restatement(ref, f.ref["recip"], f.rel, f"ewald_dipole_reciprocal_space {tag}")
    _swept(f"ewald_dipole_reciprocal_space {tag}", call, kw, dict(aplan, k_vectors=DIP), _exact, ref=ref, shared=shared)
    call = lambda **a: pme_dipole_reciprocal_space(**a, **mesh, **TDP.ALL)  # noqa: E731
    rec = _tuple(call(**atoms))
    against_restatement(rec, f.ref["mesh"], f.mesh_rel, f"pme_dipole_reciprocal_space {tag}")
    _swept(f"pme_dipole_reciprocal_space {tag}", call, atoms, aplan, two_runs, ref=rec, shared=shared)
    # the entry points that take a list, in both list formats
    for label, lists, lplan in (("matrix", dict(neighbor_matrix=f.nm, neighbor_matrix_shifts=f.sh, mask_value=f.n), dict(neighbor_matrix=MAT, neighbor_matrix_shifts=MAT)),
                                ("csr", dict(neighbor_list=f.lst, neighbor_ptr=f.ptr, neighbor_shifts=f.lsh), dict(neighbor_list=MAT, neighbor_ptr=IDX, neighbor_shifts=MAT))):
        sh = shared if label == "matrix" else ()
        call = lambda **a: ewald_dipole_real_space(**a, **TDP.ALL)  # noqa: E731
        real = _tuple(call(**atoms, **lists))
        against_restatement(real, f.ref["real"], f.rel, f"ewald_dipole_real_space {tag} {label}")
        _swept(f"ewald_dipole_real_space {tag} {label}", call, dict(atoms, **lists), dict(aplan, **lplan), _exact, ref=real, shared=sh)
        call = lambda **a: ewald_dipole_correction(**a, **TDP.ALL)  # noqa: E731
        kw = dict(atoms, k_vectors=f.KV, **lists)
        ref = _tuple(call(**kw))
        against_restatement(ref, f.ref["total"], f.rel, f"ewald_dipole_correction {tag} {label}")
        _swept(f"ewald_dipole_correction {tag} {label}", call, kw, dict(aplan, k_vectors=DIP, **lplan), _exact, ref=ref, shared=sh)
        call = lambda **a: pme_dipole_correction(**a, **mesh, **TDP.ALL)  # noqa: E731
        ref = _tuple(call(**atoms, **lists))
        for i, name in enumerate(LC.DP_NAMES):  # its halves were checked against their restatements above: the sum of the two canonical calls
            two_runs(ref[i], (real[i] + rec[i]).cpu().numpy(), f"pme_dipole_correction {tag} {label} {name} vs real space + mesh", i)
        _swept(f"pme_dipole_correction {tag} {label}", call, dict(atoms, **lists), dict(aplan, **lplan), two_runs, ref=ref, shared=sh)


# ---- point quadrupoles, Thole damping, induced dipoles -------------------------------------------------------------------------------------

QUAD = "off col row T F flt"  # quadrupoles [N, 3, 3]: col = a view of a wider last dimension, T = the atom axis stored last, F = the two tensor axes swapped in storage


@functools.lru_cache(maxsize=None)
def _mfx(dtype_name, batch):
    """The dipole fixture on the device (`_dfx`: positions, charges, dipoles, cells, alpha, k set, both list layouts) with the quadrupoles and
    polarisabilities of tests/layout_cases.py, and the restatements of the quadrupole term (real-space half, reciprocal half, their sum) and
    of the Thole correction on the stored entries, computed once."""
    d, dt = _dfx(dtype_name, batch), np.dtype(dtype_name).type
    f = types.SimpleNamespace(**vars(d))
    f.QD, f.POL = _t(LC.quadrupole(batch)["qd"].astype(dt)), _t(LC.thole(batch)["polar"].astype(dt))
    ent = TDP.R.entries_from_matrix(f.nm, f.sh, f.n)
    ev = lambda entries, kv: TQD.R.evaluate(f.P, f.Q, f.MU, f.QD, f.C, f.AL, entries, kv, batch_idx=f.BI, distance_dtype=f.tdtype)  # noqa: E731
    f.qref = dict(real=ev(ent, None), recip=ev(None, f.KV))
    f.qref["total"] = TQD._sum(f.qref["real"], f.qref["recip"])
    f.tref = TTH.TR.evaluate(f.P, f.Q, f.MU, f.POL, f.C, LC.THOLE, ent, batch_idx=f.BI, distance_dtype=f.tdtype)
    return f


def _list_forms(f):
    return (("matrix", dict(neighbor_matrix=f.nm, neighbor_matrix_shifts=f.sh, mask_value=f.n), dict(neighbor_matrix=MAT, neighbor_matrix_shifts=MAT)),
            ("csr", dict(neighbor_list=f.lst, neighbor_ptr=f.ptr, neighbor_shifts=f.lsh), dict(neighbor_list=MAT, neighbor_ptr=IDX, neighbor_shifts=MAT)))


@DTYPES
@pytest.mark.parametrize("batch", [False, True])
@_collecting
def test_point_quadrupole_operators(dtype, batch):
    """`ewald_quadrupole_reciprocal_space`, `ewald_quadrupole_real_space` and `ewald_quadrupole_correction`, all six outputs: the canonical
    call against the restatement at the bars of tests/test_quadrupole_gpu.py, every variant against the BITS of the canonical call (nothing in
    csrc/quadrupole.hip adds with atomics; the `flt` variants too, every fixture value being a float32 number).  On the batch the reciprocal
    half is run once more with both systems in the cell of the first: `k_vectors` as [1, K, 3] and as a stride-0 expansion must give the
    bits of the contiguous [B, K, 3] set."""
    from nvalchemiops.interactions.electrostatics import ewald_quadrupole_correction, ewald_quadrupole_real_space, ewald_quadrupole_reciprocal_space

    f = _mfx(dtype, batch)
    tag = f"{dtype}{' batch' if batch else ''}"
    atoms = dict(positions=f.P, charges=f.Q, dipoles=f.MU, quadrupoles=f.QD, cell=f.C, alpha=f.AL)
    aplan = dict(positions=POS, charges=VEC, dipoles=DIP, quadrupoles=QUAD, cell=CELLB if batch else CELL1, alpha=VEC)
    if batch:
        atoms["batch_idx"], aplan["batch_idx"] = f.BI, IDX
    shared = ("cell", "alpha") if batch else ()

    def against_restatement(out, ref, what):
        assert len(out) == 6
        for name, o in zip(TQD.NAMES, out):
            assert o.dtype == f.tdtype
            TQD._close(o, ref[name], f"{what} {name} vs the restatement", f.rel)

    call = lambda **a: ewald_quadrupole_reciprocal_space(**a, **TQD.ALL)  # noqa: E731
    kw = dict(atoms, k_vectors=f.KV)
    ref = _tuple(call(**kw))
    against_restatement(ref, f.qref["recip"], f"ewald_quadrupole_reciprocal_space {tag}")
    _swept(f"ewald_quadrupole_reciprocal_space {tag}", call, kw, dict(aplan, k_vectors=DIP), _exact, ref=ref, shared=shared)
    if batch:  # one cell and one k set for both systems
        same = dict(kw, cell=f.C[:1].repeat(2, 1, 1).contiguous(), k_vectors=f.KV[:1].repeat(2, 1, 1).contiguous())
        ref = _swept(f"ewald_quadrupole_reciprocal_space {tag} x0", call, same, {}, _exact, shared=("cell", "k_vectors"))
        assert not torch.equal(ref[0], _tuple(call(**kw))[0])
        _compare(_tuple(call(**dict(same, k_vectors=f.KV[:1]))), ref, _exact, "ewald_quadrupole_reciprocal_space[k_vectors:[1, K, 3]]")
        _compare(_tuple(call(**dict(same, k_vectors=_variant(f.KV[:1], "off")))), ref, _exact, "ewald_quadrupole_reciprocal_space[k_vectors:[1, K, 3] off]")
    for label, lists, lplan in _list_forms(f):
        sh = shared if label == "matrix" else ()
        call = lambda **a: ewald_quadrupole_real_space(**a, **TQD.ALL)  # noqa: E731
        ref = _tuple(call(**atoms, **lists))
        against_restatement(ref, f.qref["real"], f"ewald_quadrupole_real_space {tag} {label}")
        _swept(f"ewald_quadrupole_real_space {tag} {label}", call, dict(atoms, **lists), dict(aplan, **lplan), _exact, ref=ref, shared=sh)
        call = lambda **a: ewald_quadrupole_correction(**a, **TQD.ALL)  # noqa: E731
        kw = dict(atoms, k_vectors=f.KV, **lists)
        ref = _tuple(call(**kw))
        against_restatement(ref, f.qref["total"], f"ewald_quadrupole_correction {tag} {label}")
        _swept(f"ewald_quadrupole_correction {tag} {label}", call, kw, dict(aplan, k_vectors=DIP, **lplan), _exact, ref=ref, shared=sh)


@DTYPES
@pytest.mark.parametrize("batch", [False, True])
@_collecting
def test_pme_quadrupole_operators(dtype, batch):
    """`pme_quadrupole_reciprocal_space` and `pme_quadrupole_correction` (matrix and CSR lists) on the fixture `pme_quadrupole` of
    tests/layout_cases.py (mesh (12, 10, 14), order 6), all six outputs.  The canonical call of the mesh half against the restatement at the
    bars of tests/test_pme_quadrupole_gpu.py (1e-10 of max |ref| in float64, 4 x the restatement's float32-mode deviation in float32), the
    canonical correction against real-space half + mesh half.  Variants: in float32 the BITS of the canonical call (the spread adds in float64
    and rounds once; every fixture value is a float32 number), in float64 the 1e-12 bar of two runs (float64 atomic adds in the spread).
    On the single system also the forms no plan holds: a [3, 3] cell, alpha as a 0-d tensor and as a Python number; [B] alpha and an int64
    `batch_idx` are in the plans."""
    from nvalchemiops.interactions.electrostatics import ewald_quadrupole_real_space, pme_quadrupole_correction, pme_quadrupole_reciprocal_space

    f = _mfx(dtype, batch)
    mesh = dict(mesh_dimensions=LC.DP_MESH, spline_order=LC.PQ_ORDER)
    close = _exact if dtype == "float32" else _close_two_runs(1e-12)
    tag = f"{dtype}{' batch' if batch else ''}"
    atoms = dict(positions=f.P, charges=f.Q, dipoles=f.MU, quadrupoles=f.QD, cell=f.C, alpha=f.AL)
    aplan = dict(positions=POS, charges=VEC, dipoles=DIP, quadrupoles=QUAD, cell=CELLB if batch else CELL1, alpha=VEC)
    if batch:
        atoms["batch_idx"], aplan["batch_idx"] = f.BI, IDX
    shared = ("cell", "alpha") if batch else ()
    r64, r32 = LC.pme_quadrupole_references(batch)
    call = lambda **a: pme_quadrupole_reciprocal_space(**a, **mesh, **TQD.ALL)  # noqa: E731
    rec = _tuple(call(**atoms))
    assert len(rec) == 6
    for name, o in zip(LC.QD_NAMES, rec):
        assert o.dtype == f.tdtype
        rel = 1e-10 if dtype == "float64" else 4.0 * float(np.abs(r32[name] - r64[name]).max() / np.abs(r64[name]).max())
        TPD._close(o.reshape(r64[name].shape), r64[name], f"pme_quadrupole_reciprocal_space {tag} {name} vs the restatement", rel)
    _swept(f"pme_quadrupole_reciprocal_space {tag}", call, atoms, aplan, close, ref=rec, shared=shared)
    if not batch:
        for what, form in (("cell:[3, 3]", dict(cell=f.C[0])), ("alpha:0-d", dict(alpha=f.AL[0])), ("alpha:number", dict(alpha=float(f.AL[0]))),
                           ("cell:[3, 3] alpha:number", dict(cell=f.C[0], alpha=float(f.AL[0])))):
            _compare(_tuple(call(**dict(atoms, **form))), rec, close, f"pme_quadrupole_reciprocal_space[{what}]")
    for label, lists, lplan in _list_forms(f):
        sh = shared if label == "matrix" else ()
        real = _tuple(ewald_quadrupole_real_space(**atoms, **lists, **TQD.ALL))
        call = lambda **a: pme_quadrupole_correction(**a, **mesh, **TQD.ALL)  # noqa: E731
        ref = _tuple(call(**atoms, **lists))
        for i, name in enumerate(LC.QD_NAMES):  # the real-space half has its own sweep and restatement above: the sum of the two canonical calls
            close(ref[i], (real[i] + rec[i]).cpu().numpy(), f"pme_quadrupole_correction {tag} {label} {name} vs real space + mesh", i)
        _swept(f"pme_quadrupole_correction {tag} {label}", call, dict(atoms, **lists), dict(aplan, **lplan), close, ref=ref, shared=sh)
        if not batch:
            _compare(_tuple(call(**dict(atoms, cell=f.C[0], alpha=float(f.AL[0])), **lists)), ref, close, f"pme_quadrupole_correction {label}[cell:[3, 3] alpha:number]")


@DTYPES
@pytest.mark.parametrize("batch", [False, True])
@_collecting
def test_thole_dipole_correction(dtype, batch):
    """All six outputs; `polarizability` gets the plan of `sigma`.  One kernel, no atomics: every variant gives the bits of the canonical call,
    and a Python number gives the bits of a constant tensor."""
    from nvalchemiops.interactions.electrostatics import thole_dipole_correction as th

    f = _mfx(dtype, batch)
    tag = f"thole_dipole_correction {dtype}{' batch' if batch else ''}"
    call = lambda **a: th(**a, thole=LC.THOLE, **TTH.ALL)  # noqa: E731
    atoms = dict(positions=f.P, charges=f.Q, dipoles=f.MU, polarizability=f.POL, cell=f.C)
    aplan = dict(positions=POS, charges=VEC, dipoles=DIP, polarizability=VEC, cell=CELLB if batch else CELL1)
    if batch:
        atoms["batch_idx"], aplan["batch_idx"] = f.BI, IDX
    for label, lists, lplan in _list_forms(f):
        ref = _tuple(call(**atoms, **lists))
        assert len(ref) == 6
        for name, o in zip(TTH.NAMES, ref):
            assert o.dtype == f.tdtype
            TTH._close(o, f.tref[name], f"{tag} {label} {name} vs the restatement", f.rel)
        _swept(f"{tag} {label}", call, dict(atoms, **lists), dict(aplan, **lplan), _exact, ref=ref, shared=("cell",) if batch and label == "matrix" else ())
        number = _tuple(call(**dict(atoms, polarizability=2.5), **lists))
        _compare(_tuple(call(**dict(atoms, polarizability=torch.full_like(f.POL, 2.5)), **lists)), number, _exact, f"{tag} {label}[polarizability: number]")
        assert not torch.equal(number[0], ref[0])


@functools.lru_cache(maxsize=None)
def _ifx(batch):
    """An induced-dipole fixture of tests/layout_cases.py on the device (float64 arrays of float32 numbers) with both list layouts and the
    dense restatements, undamped and damped, computed once."""
    c = LC.induced(batch)
    f = types.SimpleNamespace(batch=batch, n=c["n"], nsys=c["nsys"], c=c)
    f.P, f.Q, f.C, f.AL, f.KV, f.F, f.X0 = (_t(c[k]) for k in ("pos", "q", "cell", "alpha", "kv", "field", "start"))
    f.BI = None if not batch else _t(c["batch_idx"])
    f.nm, f.sh = TQ._lists(*c["ent"], c["n"], c["width"], c["n"])
    f.lst, f.ptr, f.lsh = TQ._csr(f.nm, f.sh, c["n"])
    f.dense = {th: LC.induced_dense(c, th, DEV) for th in (None, LC.THOLE)}
    return f


def _within_twice_the_bound(bound_per_row):
    def close(o, r, what, i):
        err = np.abs(o.detach().cpu().numpy() - r)
        _WORST[0] = max(_WORST[0], float((err / bound_per_row).max()))
        assert (err <= bound_per_row).all(), f"{what}: max err {err.max():.3e}, worst err / (2 x bound) {(err / bound_per_row).max():.3g}"
    return close


@pytest.mark.parametrize("damped", [False, True], ids=["undamped", "thole"])
@pytest.mark.parametrize("batch", [False, True])
@_collecting
def test_induced_dipoles_explicit_ewald_and_pme(batch, damped):
    """`induced_dipoles` / `thole_induced_dipoles` with reciprocal="ewald", given k-vectors, one alpha per system, an external field and a warm
    start: the canonical call against the dense solve by `_check_solution`, and every variant against the BITS of the canonical dipoles and
    iteration counts, as the docstring of `induced_dipoles` promises for this path.  Then one pass with reciprocal="pme" (matrix list), whose
    mesh spread adds with atomics: each variant within TWICE `_check_solution`'s bound of the canonical pme call (each of the two converged
    solves is within once of the exact solution of its operator)."""
    from nvalchemiops.interactions.electrostatics import induced_dipoles, thole_induced_dipoles

    f = _ifx(batch)
    thole = LC.THOLE if damped else None
    d = f.dense[thole]
    extra = dict(thole=thole) if damped else {}
    fn = thole_induced_dipoles if damped else induced_dipoles
    tag = f"{'thole_' if damped else ''}induced_dipoles{' batch' if batch else ''}"

    def call(positions, charges, polarizability, cell, **a):
        out = fn(positions, charges, polarizability, cell, tolerance=LC.IND_TOL, return_info=True, **extra, **a)
        return out.dipoles, out.iterations

    atoms = dict(positions=f.P, charges=f.Q, polarizability=d["polar"], cell=f.C, alpha=f.AL, external_field=f.F, initial_dipoles=f.X0)
    aplan = dict(positions=POS, charges=VEC, polarizability=VEC, cell=CELLB if batch else CELL1, alpha=VEC, external_field=DIP, initial_dipoles=DIP)
    if batch:
        atoms["batch_idx"], aplan["batch_idx"] = f.BI, IDX
    for label, lists, lplan in _list_forms(f):
        kw = dict(atoms, reciprocal="ewald", k_vectors=f.KV, **lists)
        a = {k: v for k, v in kw.items() if k not in ("positions", "charges", "polarizability", "cell")}
        out = fn(f.P, f.Q, d["polar"], f.C, tolerance=LC.IND_TOL, return_info=True, **extra, **a)
        TI._check_solution(out, d["H"], d["b"], d["polar"], f.BI, f.nsys, LC.IND_TOL, f"layouts {tag} {label}", x0=f.X0)
        assert int(out.iterations.min()) > 0
        _swept(f"{tag} ewald {label}", call, kw, dict(aplan, k_vectors=DIP, **lplan), _exact, ref=(out.dipoles, out.iterations))
    label, lists, lplan = _list_forms(f)[0]
    bound = np.asarray(LC.induced_bound(d, f.nsys))
    rows = 2.0 * bound[np.zeros(f.n, np.int64) if f.BI is None else f.c["batch_idx"]][:, None]
    kw = dict(atoms, reciprocal="pme", mesh_dimensions=(32, 32, 32), spline_order=5, **lists)
    _swept(f"{tag} pme {label}", lambda **a: call(**a)[:1], kw, dict(aplan, **lplan), _within_twice_the_bound(rows))


# ---- cluster multipoles, scaled pairs, local frames ------------------------------------------------------------------------------------------

def _cluster_lists(f):
    """The first system of the fixture as a cluster: its rows of the stored matrix with every entry that carries a shift, or that lies in
    another system, turned into padding -- padding BETWEEN live entries -- and no shifts."""
    n1 = f.n if f.BI is None else int((f.BI == 0).sum())
    nm = f.nm[:n1].clone()
    nm[(f.sh[:n1] != 0).any(-1) | (nm >= n1)] = n1
    return n1, nm.contiguous()


@DTYPES
@pytest.mark.parametrize("batch", [False, True])
@_collecting
def test_cluster_multipole_corrections(dtype, batch):
    """`coulomb_dipole_correction` and `coulomb_quadrupole_correction`, every output: as periodic cut-off sums on the quadrupole fixture
    (both list forms, a stride-0 cell on the batch's matrix form) and once more with `cell=None` on the first system as a cluster, a matrix
    without shifts whose rows hold padding between live entries.  The canonical call against tests/cluster_multipole_reference.py on the
    stored entries at the bars of tests/test_cluster_multipole_gpu.py, every variant against the BITS of the canonical call."""
    from nvalchemiops.interactions.electrostatics import coulomb_dipole_correction, coulomb_quadrupole_correction
    from tests import cluster_multipole_reference as CR
    from tests import test_cluster_multipole_gpu as TCM

    f = _mfx(dtype, batch)
    tag = f"{dtype}{' batch' if batch else ''}"
    ent = TDP.R.entries_from_matrix(f.nm, f.sh, f.n)
    n1, nm1 = _cluster_lists(f)
    ent1 = TDP.R.entries_from_matrix(nm1, torch.zeros(tuple(nm1.shape) + (3,), dtype=I32, device=DEV), n1)
    assert 0 < ent1[0].shape[0] < ent[0].shape[0] and bool(((nm1 == n1)[:, :-1] & (nm1 != n1)[:, 1:]).any()), "padding between live entries"
    for which, fn, evaluate, extra, eplan in (("dipole", coulomb_dipole_correction, CR.dipole_evaluate, {}, {}),
                                              ("quadrupole", coulomb_quadrupole_correction, CR.quadrupole_evaluate, dict(quadrupoles=f.QD), dict(quadrupoles=QUAD))):
        call = lambda fn=fn, which=which, **a: fn(**a, **{k: v for k, v in TCM.ALL[which].items() if a.get("cell") is not None or k != "compute_virial"})  # noqa: E731
        atoms = dict(positions=f.P, charges=f.Q, dipoles=f.MU, **extra, cell=f.C)
        aplan = dict(positions=POS, charges=VEC, dipoles=DIP, **eplan, cell=CELLB if batch else CELL1)
        if batch:
            atoms["batch_idx"], aplan["batch_idx"] = f.BI, IDX
        ref64 = evaluate(*[atoms[k] for k in ("positions", "charges", "dipoles") + tuple(extra)], ent, cell=f.C, batch_idx=f.BI, distance_dtype=f.tdtype)
        for label, lists, lplan in _list_forms(f):
            ref = _tuple(call(**atoms, **lists))
            assert len(ref) == len(TCM.NAMES[which])
            for name, o in zip(TCM.NAMES[which], ref):
                assert o.dtype == f.tdtype
                TCM._close(o, ref64[name], f"coulomb_{which}_correction {tag} {label} {name} vs the restatement", f.rel)
            _swept(f"coulomb_{which}_correction {tag} {label}", call, dict(atoms, **lists), dict(aplan, **lplan), _exact, ref=ref,
                   shared=("cell",) if batch and label == "matrix" else ())
        # the first system as a cluster
        catoms = {k: (v[:n1].contiguous() if k != "cell" else None) for k, v in atoms.items() if k != "batch_idx"}
        cplan = {k: v for k, v in aplan.items() if k not in ("cell", "batch_idx")}
        lists = dict(neighbor_matrix=nm1, mask_value=n1)
        ref = _tuple(call(**catoms, **lists))
        ref64 = evaluate(*[catoms[k] for k in ("positions", "charges", "dipoles") + tuple(extra)], ent1, distance_dtype=f.tdtype)
        for name, o in zip([k for k in TCM.NAMES[which] if k != "virial"], ref):
            TCM._close(o, ref64[name], f"coulomb_{which}_correction {tag} cluster {name} vs the restatement", f.rel)
        _swept(f"coulomb_{which}_correction {tag} cluster", call, dict(catoms, **lists), dict(cplan, neighbor_matrix=MAT), _exact, ref=ref)


SCL_M = "off col row T flt"   # pair_scales [N, M]: float32 or float64 whatever the positions dtype
SCL_L = "off col row flt"     # pair_scales [nnz]


def _matrix_of(entries, values, n, fill):
    """Padded [n, M] matrix (+ shifts and per-slot values, 0.5 on padding) of entries sorted by row."""
    i, j, S = entries
    counts = torch.bincount(i, minlength=n)
    col = torch.arange(i.shape[0], device=DEV) - (torch.cumsum(counts, 0) - counts)[i]
    m = int(counts.max()) + 2
    nm = torch.full((n, m), fill, dtype=I32, device=DEV)
    sh = torch.zeros((n, m, 3), dtype=I32, device=DEV)
    val = torch.full((n, m), 0.5, dtype=values.dtype, device=DEV)
    nm[i, col], sh[i, col], val[i, col] = j.to(I32), S.to(I32), values
    ptr = torch.zeros(n + 1, dtype=I32, device=DEV)
    ptr[1:] = torch.cumsum(counts, 0)
    return nm, sh, val, torch.stack([i, j]).to(I32).contiguous(), ptr, S.to(I32).contiguous()


def _stored_pair_scales(f):
    """(pair_scales [N, M] beside the stored matrix with 0.5 on its padding, pair_scales [nnz] beside the stored CSR list) in the positions dtype."""
    live = (f.nm >= 0) & (f.nm < f.n)
    snm = torch.full(tuple(f.nm.shape), 0.5, dtype=f.tdtype, device=DEV)
    snm[live] = LC.distance_class_scales(f.P, f.C, f.BI, *TDP.R.entries_from_matrix(f.nm, f.sh, f.n)).to(f.tdtype)
    scsr = LC.distance_class_scales(f.P, f.C, f.BI, f.lst[0].long(), f.lst[1].long(), f.lsh.long()).to(f.tdtype)
    return snm.contiguous(), scsr.contiguous()


@DTYPES
@pytest.mark.parametrize("batch", [False, True])
@_collecting
def test_pair_scale_correction(dtype, batch):
    """All six outputs on the quadrupole fixture with one scale per stored entry from its distance class (tests/layout_cases.py: symmetric by
    construction, one class exactly 1, 0.5 on the padding of the matrix).  `pair_scales` is an argument class of its own: [N, M] beside a
    matrix, [nnz] beside a list, float32 or float64 whatever the positions dtype, so `flt` is the float dtype the positions do NOT have.
    With shifts; then with `minimum_image=True` on the sub-list of the pairs whose stored shift already is the minimum image (fractional
    components at most 0.45), without shifts, where the call with shifts and the call without meet the same restatement; then
    `dipoles=None`, `quadrupoles=None` and both against the bits of zero tensors."""
    from nvalchemiops.interactions.electrostatics import pair_scale_correction
    from tests import pair_scale_reference as PSR
    from tests import test_pair_scale_gpu as TPS

    f = _mfx(dtype, batch)
    tag = f"pair_scale_correction {dtype}{' batch' if batch else ''}"
    ent = TDP.R.entries_from_matrix(f.nm, f.sh, f.n)
    scales = LC.distance_class_scales(f.P, f.C, f.BI, *ent)
    assert sorted(set(scales.tolist())) == sorted(LC.PS_SCALES)
    call = lambda **a: pair_scale_correction(**a, **TPS.ALL)  # noqa: E731
    atoms = dict(positions=f.P, charges=f.Q, dipoles=f.MU, quadrupoles=f.QD, cell=f.C)
    aplan = dict(positions=POS, charges=VEC, dipoles=DIP, quadrupoles=QUAD, cell=CELLB if batch else CELL1)
    if batch:
        atoms["batch_idx"], aplan["batch_idx"] = f.BI, IDX

    def against_restatement(out, ref, what):
        assert len(out) == 6
        for name, o in zip(TPS.NAMES, out):
            assert o.dtype == f.tdtype
            TPS._close(o, ref[name], f"{what} {name} vs the restatement", f.rel)

    # the whole list, explicit shifts; the stored matrix and the stored CSR list hold the same entries in the same row order
    ref64 = PSR.evaluate(f.P, f.Q, f.MU, f.QD, scales, ent, cell=f.C, batch_idx=f.BI, distance_dtype=f.tdtype)
    snm, scsr = _stored_pair_scales(f)
    for (label, lists, lplan), s, splan in zip(_list_forms(f), (snm, scsr), (SCL_M, SCL_L)):
        kw = dict(atoms, pair_scales=s, **lists)
        ref = _tuple(call(**kw))
        against_restatement(ref, ref64, f"{tag} {label}")
        _swept(f"{tag} {label}", call, kw, dict(aplan, pair_scales=splan, **lplan), _exact, ref=ref, shared=("cell",) if batch and label == "matrix" else ())
        for absent in (("dipoles",), ("quadrupoles",), ("dipoles", "quadrupoles")):
            none = _tuple(call(**dict(kw, **{k: None for k in absent})))
            _compare(_tuple(call(**dict(kw, **{k: torch.zeros_like(kw[k]) for k in absent}))), none, _exact, f"{tag} {label}[{' '.join(absent)}: None]")
            assert not torch.equal(none[0], ref[0])
    # minimum image on the pairs whose stored shift already is the minimum image
    keep = LC.minimum_image_entries(f.P, f.C, f.BI, *ent)
    sub = tuple(e[keep] for e in ent)
    assert 0 < int(keep.sum()) < keep.shape[0] and bool((sub[2] != 0).any())
    ref64 = PSR.evaluate(f.P, f.Q, f.MU, f.QD, scales[keep], sub, cell=f.C, batch_idx=f.BI, distance_dtype=f.tdtype, minimum_image=True)
    nm, sh, snm, lst, ptr, lsh = _matrix_of(sub, scales[keep].to(f.tdtype), f.n, f.n)
    for label, lists, shifts, s, lplan, splan in (
            ("matrix", dict(neighbor_matrix=nm, mask_value=f.n), dict(neighbor_matrix_shifts=sh), snm, dict(neighbor_matrix=MAT), SCL_M),
            ("csr", dict(neighbor_list=lst, neighbor_ptr=ptr), dict(neighbor_shifts=lsh), scales[keep].to(f.tdtype).contiguous(),
             dict(neighbor_list=MAT, neighbor_ptr=IDX), SCL_L)):
        against_restatement(_tuple(call(**atoms, pair_scales=s, **lists, **shifts)), ref64, f"{tag} {label} sub-list with shifts")
        kw = dict(atoms, pair_scales=s, **lists)
        mcall = lambda **a: pair_scale_correction(**a, minimum_image=True, **TPS.ALL)  # noqa: E731
        ref = _tuple(mcall(**kw))
        against_restatement(ref, ref64, f"{tag} {label} minimum image")
        _swept(f"{tag} {label} minimum image", mcall, kw, dict(aplan, pair_scales=splan, **lplan), _exact, ref=ref)


@functools.lru_cache(maxsize=None)
def _ffx(dtype_name, batch):
    c, dt = LC.frames(batch), np.dtype(dtype_name).type
    f = types.SimpleNamespace(batch=batch, n=c["n"], c=c, tdtype=F32 if dt == np.float32 else F64, rel=1e-11 if dt == np.float64 else 1e-6)
    f.P, f.MU, f.QD, f.WMU, f.WQ, f.C = (_t(c[k].astype(dt)) for k in ("pos", "mu", "quad", "w_mu", "w_q", "cell"))
    f.ATOMS, f.KINDS = _t(c["atoms"]), _t(c["kinds"])
    f.BI = None if not batch else _t(c["batch_idx"])
    f.ref = LC.frames_reference(batch)
    return f


@DTYPES
@pytest.mark.parametrize("batch", [False, True])
@_collecting
def test_local_frames(dtype, batch):
    """`LocalFrames`, `rotate_multipoles` and `multipole_frame_forces(compute_local_gradients=True, compute_virial=True)` on the fixture
    `frames` of tests/layout_cases.py.  `frame_atoms` and `frame_kinds` go through the constructor in every layout and as int64; the four
    tensors of the resulting object must equal the canonical object's.  The local multipoles and the caller's gradients get the plans of
    dipoles and quadrupoles, `flt` included (`multipole_frame_forces` takes gradients of any float dtype).  The canonical call against
    tests/local_frames_reference.py at the bars of tests/test_local_frames_gpu.py, every variant against the BITS of the canonical call.  A
    `LocalFrames` built on the CPU and moved with `.to()` gives the bits of the device-built one."""
    from nvalchemiops.interactions.electrostatics import LocalFrames, multipole_frame_forces, rotate_multipoles
    from tests import test_local_frames_gpu as TLF

    f = _ffx(dtype, batch)
    tag = f"local frames {dtype}{' batch' if batch else ''}"

    def run(fr, positions, local_dipoles, local_quadrupoles, dipole_grads, quadrupole_grads, cell, batch_idx=None):
        mu, qd = rotate_multipoles(positions, local_dipoles, local_quadrupoles, fr, cell, batch_idx=batch_idx)
        out = multipole_frame_forces(positions, local_dipoles, local_quadrupoles, fr, dipole_grads, quadrupole_grads, cell, batch_idx=batch_idx,
                                     compute_local_gradients=True, compute_virial=True)
        return (mu, qd) + tuple(out) + (fr.frame_atoms, fr.frame_kinds, fr.inverse_ptr, fr.inverse_slots)

    def call(frame_atoms, frame_kinds, **a):
        return run(LocalFrames(frame_atoms, frame_kinds, batch_idx=a.get("batch_idx")), **a)

    kw = dict(frame_atoms=f.ATOMS, frame_kinds=f.KINDS, positions=f.P, local_dipoles=f.MU, local_quadrupoles=f.QD, dipole_grads=f.WMU,
              quadrupole_grads=f.WQ, cell=f.C)
    plan = dict(frame_atoms=MAT, frame_kinds=IDX, positions=POS, local_dipoles=DIP, local_quadrupoles=QUAD, dipole_grads=DIP, quadrupole_grads=QUAD,
                cell=CELLB if batch else CELL1)
    if batch:
        kw["batch_idx"], plan["batch_idx"] = f.BI, IDX
    ref = call(**kw)
    assert len(ref) == 10 and all(o.dtype == f.tdtype for o in ref[:6]) and all(o.dtype == I32 for o in ref[6:])
    for name, o, sign in zip(LC.FR_NAMES, ref, (1.0, 1.0, -1.0, 1.0, 1.0, 1.0)):  # the third output is the torque force, -dL/dr
        TLF._close(sign * o, f.ref[name], f"{tag} {name} vs the restatement", f.rel)
    _swept(tag, call, kw, plan, _exact, ref=ref)
    moved = LocalFrames(f.ATOMS.cpu(), f.KINDS.cpu(), batch_idx=None if f.BI is None else f.BI.cpu()).to(DEV)
    _compare(run(moved, **{k: v for k, v in kw.items() if not k.startswith("frame_")}), ref, _exact, f"{tag}[LocalFrames.to()]")


@pytest.mark.parametrize("damped", [False, True], ids=["undamped", "thole"])
@_collecting
def test_cluster_induced_dipoles(damped):
    """`cluster_induced_dipoles` on the batch of three clusters of tests/layout_cases.py (`cluster_induced`), an external field and a warm
    start, float64: the canonical call against the dense solve by `_check_solution` of tests/test_induced_gpu.py, every variant against
    the BITS of the canonical dipoles and iteration counts; a Python number for the polarisability against a constant tensor."""
    from nvalchemiops.interactions.electrostatics import cluster_induced_dipoles
    from tests import test_cluster_multipole_gpu as TCM

    c = LC.cluster_induced()
    thole = LC.THOLE if damped else None
    d = LC.cluster_induced_dense(thole, DEV)
    lf = TCM._lists(*c["entries"], c["n"], False)
    tag = f"cluster_induced_dipoles {'thole' if damped else 'undamped'}"

    def call(**a):
        out = cluster_induced_dipoles(thole=thole, num_systems=c["nsys"], tolerance=LC.IND_TOL, return_info=True, **a)
        return out.dipoles, out.iterations

    atoms = dict(positions=_t(c["pos"]), charges=_t(c["q"]), polarizability=d["polar"], external_field=_t(c["field"]), initial_dipoles=_t(c["start"]),
                 batch_idx=_t(c["batch_idx"]))
    aplan = dict(positions=POS, charges=VEC, polarizability=VEC, external_field=DIP, initial_dipoles=DIP, batch_idx=IDX)
    for label, lists, lplan in (("matrix", dict(neighbor_matrix=lf["nm"], mask_value=c["n"]), dict(neighbor_matrix=MAT)),
                                ("csr", dict(neighbor_list=lf["nl"], neighbor_ptr=lf["ptr"]), dict(neighbor_list=MAT, neighbor_ptr=IDX))):
        kw = dict(atoms, **lists)
        out = cluster_induced_dipoles(thole=thole, num_systems=c["nsys"], tolerance=LC.IND_TOL, return_info=True, **kw)
        TI._check_solution(out, d["H"], d["b"], d["polar"], atoms["batch_idx"], c["nsys"], LC.IND_TOL, f"layouts {tag} {label}", x0=atoms["initial_dipoles"])
        assert int(out.iterations.max()) > 0
        _swept(f"{tag} {label}", call, kw, dict(aplan, **lplan), _exact, ref=(out.dipoles, out.iterations))
        number = call(**dict(kw, polarizability=0.0625))
        _compare(call(**dict(kw, polarizability=torch.full_like(d["polar"], 0.0625))), number, _exact, f"{tag} {label}[polarizability: number]")
        assert not torch.equal(number[0], out.dipoles)


# ==== splines =============================================================================================================================

MESH = "off col row T flt"


@DTYPES
@pytest.mark.parametrize("dims", MESHES)
@_collecting
def test_splines(dtype, dims, spread_path):
    from nvalchemiops.spline import (spline_gather, spline_gather_channels, spline_gather_gradient, spline_gather_vec3, spline_spread,
                                     spline_spread_channels)

    g = np.random.default_rng(11)
    rnd = lambda *shape: g.normal(size=shape).astype(np.float32)  # noqa: E731
    for f in (_fx(dtype), _fx(dtype, batch=True)):
        close, dt = _close_pme(f.dtype), f.dtype
        nb = f.cell.shape[0]
        lead = (nb,) if f.batch else ()
        cell = f.C if f.batch else f.C[0]
        ocell = f.cell if f.batch else f.cell[0]
        base = dict(positions=f.P, cell=cell)
        bplan = dict(positions=POS, cell=CELLB if f.batch else CELL1)
        if f.batch:
            base["batch_idx"], bplan["batch_idx"] = f.BI, IDX
        tag = " batch" if f.batch else ""
        field, vfield = rnd(*lead, *dims).astype(dt), rnd(*lead, *dims, 3).astype(dt)
        vals, cmesh = rnd(f.n, 5).astype(dt), rnd(*lead, 5, *dims).astype(dt)
        ref = _sweep("spline_spread" + tag, lambda **a: spline_spread(a.pop("positions"), a.pop("values"), a.pop("cell"), dims, 4, **a),
                     dict(base, values=f.Q), dict(bplan, values=VEC), close)
        TP._close(ref[0], O.spline_spread(f.pos, f.q, ocell, dims, 4, batch_idx=f.bi), dt, "spread vs oracle")
        ref = _sweep("spline_gather" + tag, lambda **a: spline_gather(a.pop("positions"), a.pop("mesh"), a.pop("cell"), 4, **a),
                     dict(base, mesh=_t(field)), dict(bplan, mesh=MESH), close)
        TP._close(ref[0], O.spline_gather(f.pos, field, ocell, 4, batch_idx=f.bi), dt, "gather vs oracle")
        ref = _sweep("spline_gather_vec3" + tag, lambda **a: spline_gather_vec3(a.pop("positions"), a.pop("charges"), a.pop("mesh"), a.pop("cell"), 4, **a),
                     dict(base, charges=f.Q, mesh=_t(vfield)), dict(bplan, charges=VEC, mesh=MESH), close)
        TP._close(ref[0], O.spline_gather_vec3(f.pos, f.q, vfield, ocell, 4, batch_idx=f.bi), dt, "gather_vec3 vs oracle")
        gref = _sweep("spline_gather_gradient" + tag,
                      lambda **a: spline_gather_gradient(a.pop("positions"), a.pop("charges"), a.pop("mesh"), a.pop("cell"), 4, **a),
                      dict(base, charges=f.Q, mesh=_t(field)), dict(bplan, charges=VEC, mesh=MESH), close)
        # the gradient's reference: autograd of the (oracle-checked) gather with respect to the positions -- the adjoint kernels, not the
        # kernel under test.  (Central differences, as tests/test_pme_gpu.py uses on 40 atoms, are no reference here: with 130 atoms some
        # sit within h of a knot of the cubic spline, where the third derivative jumps.)
        bkw = dict(batch_idx=f.BI) if f.batch else {}
        x = f.P.clone().requires_grad_(True)
        dgdx, = torch.autograd.grad(spline_gather(x, _t(field), cell, 4, **bkw).sum(), x)
        TP._close(gref[0], (-f.Q[:, None] * dgdx).cpu().numpy(), dt, "gather_gradient vs autograd of the gather")
        ref = _sweep("spline_spread_channels" + tag, lambda **a: spline_spread_channels(a.pop("positions"), a.pop("values"), a.pop("cell"), dims, 4, **a),
                     dict(base, values=_t(vals)), dict(bplan, values="off col row T flt"), close)
        for ch in range(5):
            TP._close(ref[0][(slice(None), ch) if f.batch else ch], O.spline_spread(f.pos, vals[:, ch], ocell, dims, 4, batch_idx=f.bi), dt, f"channel {ch} vs oracle")
        ref = _sweep("spline_gather_channels" + tag, lambda **a: spline_gather_channels(a.pop("positions"), a.pop("mesh"), a.pop("cell"), 4, **a),
                     dict(base, mesh=_t(cmesh)), dict(bplan, mesh=MESH), close)
        for ch in range(5):
            plane = cmesh[:, ch] if f.batch else cmesh[ch]
            TP._close(ref[0][:, ch], O.spline_gather(f.pos, np.ascontiguousarray(plane), ocell, 4, batch_idx=f.bi), dt, f"gather channel {ch} vs oracle")


# ==== math ================================================================================================================================

@_collecting
def test_math_functions():
    from nvalchemiops.math import (eval_gto_density_pytorch, eval_gto_fourier_pytorch, eval_spherical_harmonics_gradient_pytorch,
                                   eval_spherical_harmonics_pytorch)

    pts = (np.random.default_rng(0).normal(size=(2 * N, 3)) * 3.0).astype(np.float32).astype(np.float64)
    pts = pts[np.linalg.norm(pts, axis=1) > 0.5][:N]  # (as tests/test_math_gpu.py: the gradients are singular at the origin)
    P = _t(pts)
    plan = dict(positions=POS + " flt")
    ref = _sweep("eval_spherical_harmonics_pytorch", lambda **a: eval_spherical_harmonics_pytorch(a["positions"], 2), dict(positions=P), plan, CLOSE_MATH)
    np.testing.assert_allclose(ref[0].cpu().numpy(), TM._ylm(pts), **TM.TOL)
    gref = _sweep("eval_spherical_harmonics_gradient_pytorch", lambda **a: eval_spherical_harmonics_gradient_pytorch(a["positions"], 2), dict(positions=P),
                  plan, CLOSE_MATH)
    x = P.clone().requires_grad_(True)
    y = TM._ylm(x, lib=torch)
    for c in range(9):  # the closed forms, differentiated by autograd
        np.testing.assert_allclose(gref[0][:, c].cpu().numpy(), torch.autograd.grad(y[:, c].sum(), x, retain_graph=True)[0].cpu().numpy(), **TM.TOL)
    sigma = 0.75
    dref = _sweep("eval_gto_density_pytorch", lambda **a: eval_gto_density_pytorch(a["positions"], sigma, 2), dict(positions=P), plan, CLOSE_MATH)
    r2 = (pts ** 2).sum(1)
    want = np.sqrt(4 * np.pi) / (2 * np.pi * sigma ** 2) ** 1.5 * TM._ylm(pts) * np.exp(-r2 / (2 * sigma ** 2))[:, None]
    np.testing.assert_allclose(dref[0].cpu().numpy(), want, **TM.TOL)
    fref = _sweep("eval_gto_fourier_pytorch", lambda **a: eval_gto_fourier_pytorch(a["k_vectors"], sigma, 2), dict(k_vectors=P),
                  dict(k_vectors=POS + " flt"), CLOSE_MATH)
    env, ylm = np.exp(-r2 * sigma ** 2 / 2)[:, None], TM._ylm(pts) * np.sqrt(4 * np.pi)
    real = np.concatenate([env, np.zeros((N, 3)), -0.25 * ylm[:, 4:] * env], 1)
    imag = np.concatenate([np.zeros((N, 1)), 0.5 * ylm[:, 1:4] * env, np.zeros((N, 5))], 1)
    np.testing.assert_allclose(fref[0].cpu().numpy(), real, **TM.TOL)
    np.testing.assert_allclose(fref[1].cpu().numpy(), imag, **TM.TOL)


# ==== gradient layouts ====================================================================================================================

@DTYPES
def test_gradient_layouts(dtype, spread_path):
    """The adjoint kernels receive the grad outputs as raw pointers too.  For every autograd-capable op -- energies AND explicit forces where
    the op returns them -- the backward is taken with grad outputs of equal values in four layouts, handed over as they are
    (`torch.autograd.grad(..., grad_outputs=...)`): contiguous (the canonical one), a stride-0 expansion (what `out.sum().backward()`
    produces), a row-strided view and transposed / column-strided storage (what `(w * out).sum()` produces when w is such a view and
    autograd keeps its layout).  Gradients with respect to positions, charges and cell must agree with the canonical backward's."""
    from nvalchemiops.interactions.electrostatics import (ewald_real_space, ewald_reciprocal_space, ewald_summation, generate_k_vectors_ewald_summation,
                                                          particle_mesh_ewald, pme_reciprocal_space)
    from nvalchemiops.interactions.electrostatics.coulomb import coulomb_energy, coulomb_energy_forces
    from nvalchemiops.spline import spline_gather, spline_gather_channels, spline_gather_vec3, spline_spread, spline_spread_channels

    f = _fx(dtype)
    close = _close_pme(f.dtype)
    dims = MESHES[0]
    kv = generate_k_vectors_ewald_summation(f.C[0], 2.0)
    g = np.random.default_rng(5)
    field = _t(g.normal(size=dims).astype(np.float32).astype(f.dtype))
    vfield = _t(g.normal(size=dims + (3,)).astype(np.float32).astype(f.dtype))
    cmesh = _t(g.normal(size=(3,) + dims).astype(np.float32).astype(f.dtype))
    vals = _t(g.normal(size=(f.n, 3)).astype(np.float32).astype(f.dtype))
    nb = dict(neighbor_matrix=f.nm, neighbor_matrix_shifts=f.sh)
    ops = {
        "ewald_real_space": lambda p, q, c: ewald_real_space(p, q, c, f.AL, mask_value=f.n, **nb),
        "ewald_real_space +forces": lambda p, q, c: ewald_real_space(p, q, c, f.AL, mask_value=f.n, compute_forces=True, **nb),
        "ewald_reciprocal_space": lambda p, q, c: ewald_reciprocal_space(p, q, c[0], kv, f.AL),
        "ewald_reciprocal_space +forces": lambda p, q, c: ewald_reciprocal_space(p, q, c[0], kv, f.AL, compute_forces=True),
        "ewald_summation": lambda p, q, c: ewald_summation(p, q, c[0], alpha=f.AL, k_vectors=kv, mask_value=f.n, **nb),
        "pme_reciprocal_space": lambda p, q, c: pme_reciprocal_space(p, q, c[0], f.AL, mesh_dimensions=dims, spline_order=4),
        "particle_mesh_ewald": lambda p, q, c: particle_mesh_ewald(p, q, c[0], f.AL, mesh_dimensions=dims, spline_order=4, mask_value=f.n, **nb),
        "spline_spread": lambda p, q, c: spline_spread(p, q, c[0], dims, 4),
        "spline_gather": lambda p, q, c: spline_gather(p, field, c[0], 4) * q,
        "spline_gather_vec3": lambda p, q, c: spline_gather_vec3(p, q, vfield, c[0], 4),
        "spline_spread_channels": lambda p, q, c: spline_spread_channels(p, vals * q[:, None], c[0], dims, 4),
        "spline_gather_channels": lambda p, q, c: spline_gather_channels(p, cmesh, c[0], 4) * q[:, None],
    }
    if dtype == "float64":  # (the cut-off Coulomb ops compute in float64: their 1e-11 bar is a float64 bar)
        ops["coulomb_energy"] = lambda p, q, c: coulomb_energy(p, q, c, 4.5, 0.3, **nb)
        ops["coulomb_energy_forces"] = lambda p, q, c: coulomb_energy_forces(p, q, c, 4.5, 0.3, **nb)
    _check_gradient_layouts({name: (op, (f.P, f.Q, f.C), ("positions", "charges", "cell"), CLOSE_COULOMB if name.startswith("coulomb") else close)
                             for name, op in ops.items()})


def _check_gradient_layouts(ops):
    """ops: name -> (op(*leaves) -> output(s), the tensors to differentiate with respect to, their names, closeness).  Every grad-output
    layout against the canonical (contiguous) backward of the same op."""
    fails = []
    for name, (op, inputs, args, close) in ops.items():
        def grads(layout, op=op, inputs=inputs):
            leaves = [t.clone().requires_grad_(True) for t in inputs]
            outs = _tuple(op(*leaves))
            gs = []
            for i, o in enumerate(outs):
                w = _t(np.random.default_rng(9 + i).uniform(0.5, 1.5, tuple(o.shape)).astype(np.float32)).to(o.dtype)
                if layout == "x0":  # every element the same value: ones, canonical = contiguous ones
                    w = torch.ones((), dtype=o.dtype, device=o.device).expand(o.shape)
                elif layout == "ones":
                    w = torch.ones_like(o)
                elif layout == "T":
                    w = _variant(w, "T" if w.dim() > 1 else "col")
                elif layout != "contiguous":
                    w = _variant(w, layout)
                gs.append(w)
            return torch.autograd.grad(outs, leaves, grad_outputs=gs, allow_unused=True)

        def one(name=name, grads=grads, args=args, close=close):
            ref_w, ref_1 = grads("contiguous"), grads("ones")
            for layout, ref in (("x0", ref_1), ("row", ref_w), ("T", ref_w), ("off", ref_w)):
                for gt, rf, arg in zip(grads(layout), ref, args):
                    assert (gt is None) == (rf is None), f"{name} grad output {layout}: d/d{arg}"
                    if rf is not None:
                        close(gt, rf.cpu().numpy(), f"{name} grad output {layout}: d/d{arg}", args.index(arg))
        _guarded(one, name, fails)
    assert not fails, "\n".join(fails)


@DTYPES
def test_gradient_layouts_of_the_dispersion_and_charge_ops(dtype):
    """The same for the four adjoint paths of `gaussian_charge_correction` (energies, with respect to positions, charges, sigma and cell),
    `dftd4` (positions and charges) and `dftd4_atm` (positions) on the two-system batch -- so that the [B] grad output has a layout -- and
    the charges of `charge_equilibration` on the cluster batch (positions, chi, hardness, sigma, total charge; float64 only).  Each against
    its own contiguous backward: `dftd4`, `dftd4_atm` and the solver part of the cluster solve (chi, hardness, total charge) are free of
    atomics, so the bits must be equal; the Gaussian energies, and the position and sigma gradients of the solve, at their modules' bars."""
    from nvalchemiops.interactions.dispersion import dftd4, dftd4_atm
    from nvalchemiops.interactions.electrostatics import charge_equilibration as qeq, gaussian_charge_correction as gcc

    ops = {}
    for batch in (False, True):
        g = _gfx(dtype, batch)
        bkw = dict(batch_idx=g.BI) if batch else {}
        ops[f"gaussian_charge_correction{' batch' if batch else ''}"] = (
            lambda p, q, s, c, g=g, bkw=bkw: gcc(p, q, s, c, neighbor_matrix=g.nm, neighbor_matrix_shifts=g.sh, mask_value=g.n, **bkw),
            (g.P, g.Q, g.S, g.C), ("positions", "charges", "sigma", "cell"), lambda o, r, what, i, g=g: TG._close(o, r, what, g.rel))
        ops[f"gaussian_charge_correction csr{' batch' if batch else ''}"] = (
            lambda p, q, s, c, g=g, bkw=bkw: gcc(p, q, s, c, neighbor_list=g.lst, neighbor_ptr=g.ptr, neighbor_shifts=g.lsh, **bkw),
            (g.P, g.Q, g.S, g.C), ("positions", "charges", "sigma", "cell"), lambda o, r, what, i, g=g: TG._close(o, r, what, g.rel))
    f = _d4fx(True, dtype)
    params = TD4._params(f.c["tables"])
    lists = dict(neighbor_matrix=f.nm, neighbor_matrix_shifts=f.sh, cell=f.C, batch_idx=f.BI)
    ops["dftd4 batch"] = (lambda p, q: dftd4(p, f.Zt, q, **TD4.BJ, d4_params=params, **lists)[0], (f.P, f.Q.to(f.P.dtype)), ("positions", "charges"), _exact)
    s9 = LC.d4_atm_s9(True)
    ops["dftd4_atm batch"] = (lambda p: dftd4_atm(p, f.Zt, **TD4A.BJ, three_body_cutoff=RC43, s9=s9, d4_params=params, **lists)[0], (f.P,), ("positions",), _exact)
    if dtype == "float64":
        c = LC.qeq_cluster()
        nm, _, _, _, _ = _qeq_lists(c)
        bi = _t(c["batch_idx"])
        solve = lambda p, chi, j, s, tot: qeq(p, chi, j, s, total_charge=tot, batch_idx=bi, neighbor_matrix=nm, mask_value=c["n"], tolerance=1e-12)  # noqa: E731
        inputs = tuple(_t(c[k]) for k in ("pos", "chi", "hard", "sigma", "total"))
        # chi, hardness and total charge come out of the solver's own kernels (no atomics): equal bits.  The gradients with respect to
        # positions and sigma are assembled by the adjoints of the public energy functions, which add with atomics (measured: 1.1e-16
        # between two equal backward passes): those two at the relative bars of tests/test_qeq_gpu.py::GRAD_BARS.  The bars are relative
        # to the largest component of the gradient of a loss with random weights: for the stride-0 layout (every weight 1) the loss is
        # sum_i q_i = sum_s Q_s, whose gradient with respect to positions and sigma is zero up to rounding and gives no scale.
        leaves = [t.clone().requires_grad_(True) for t in inputs]
        w = _t(np.random.default_rng(9).uniform(0.5, 1.5, c["n"]).astype(np.float32)).to(F64)
        scale = [float(g.abs().max()) for g in torch.autograd.grad((w * solve(*leaves)).sum(), leaves)]
        rel = {0: TQ.GRAD_BARS["cluster"]["pos"], 3: TQ.GRAD_BARS["cluster"]["sigma"]}

        def close_qeq(o, r, what, i):
            if i not in rel:
                return _exact(o, r, what, i)
            err = np.abs(o.detach().cpu().numpy() - r).max()
            assert err <= rel[i] * scale[i], f"{what}: max err {err:.3e} on {scale[i]:.3e}"

        ops["charge_equilibration cluster batch"] = (solve, inputs, ("positions", "chi", "hardness", "sigma", "total_charge"), close_qeq)
    _check_gradient_layouts(ops)


@DTYPES
def test_gradient_layouts_of_the_point_dipole_ops(dtype):
    """The same for `ewald_dipole_correction` (matrix and CSR), `ewald_dipole_reciprocal_space` and `pme_dipole_reciprocal_space` on the single
    system and the batch, with respect to positions, charges and dipoles.  The adjoints of the explicit sums are the forward kernels with
    weights and use no atomics: equal bits.  The mesh term at the bar of two device results."""
    from nvalchemiops.interactions.electrostatics import ewald_dipole_correction, ewald_dipole_reciprocal_space, pme_dipole_reciprocal_space

    ops = {}
    for batch in (False, True):
        f = _dfx(dtype, batch)
        bkw = dict(batch_idx=f.BI) if batch else {}
        tag = " batch" if batch else ""
        leaves, names = (f.P, f.Q, f.MU), ("positions", "charges", "dipoles")
        ops[f"ewald_dipole_correction{tag}"] = (
            lambda p, q, m, f=f, bkw=bkw: ewald_dipole_correction(p, q, m, f.C, f.AL, f.KV, neighbor_matrix=f.nm, neighbor_matrix_shifts=f.sh, mask_value=f.n, **bkw),
            leaves, names, _exact)
        ops[f"ewald_dipole_correction csr{tag}"] = (
            lambda p, q, m, f=f, bkw=bkw: ewald_dipole_correction(p, q, m, f.C, f.AL, f.KV, neighbor_list=f.lst, neighbor_ptr=f.ptr, neighbor_shifts=f.lsh, **bkw),
            leaves, names, _exact)
        ops[f"ewald_dipole_reciprocal_space{tag}"] = (lambda p, q, m, f=f, bkw=bkw: ewald_dipole_reciprocal_space(p, q, m, f.C, f.KV, f.AL, **bkw), leaves, names, _exact)
        ops[f"pme_dipole_reciprocal_space{tag}"] = (
            lambda p, q, m, f=f, bkw=bkw: pme_dipole_reciprocal_space(p, q, m, f.C, f.AL, mesh_dimensions=LC.DP_MESH, spline_order=LC.DP_ORDER, **bkw),
            leaves, names, _close_two_runs(f.two_runs))
    _check_gradient_layouts(ops)


@DTYPES
def test_gradient_layouts_of_the_quadrupole_thole_and_induced_dipole_ops(dtype):
    """The same for `ewald_quadrupole_correction` (matrix and CSR) and `ewald_quadrupole_reciprocal_space` with respect to positions, charges,
    dipoles and quadrupoles, `thole_dipole_correction` with respect to positions, charges, dipoles and polarizability -- on the single system
    and the batch -- and the dipoles of `induced_dipoles` / `thole_induced_dipoles` (reciprocal="ewald", float64 only) with respect to
    positions, charges, polarizability and the external field.  The adjoints are the forward kernels with weights; the backward of the solve
    is one more solve with the stored operator and two calls of the public energy functions: no atomics anywhere, equal bits.  And
    `pme_quadrupole_reciprocal_space` / `pme_quadrupole_correction` (mesh (12, 10, 14), order 6) with respect to positions, charges, dipoles
    and quadrupoles: the four-mesh adjoint adds with float64 atomics in the spread, so equal bits in float32 (rounded once) and the bar of
    two runs, 1e-12 of the largest component, in float64."""
    from nvalchemiops.interactions.electrostatics import (ewald_quadrupole_correction, ewald_quadrupole_reciprocal_space, induced_dipoles,
                                                          pme_quadrupole_correction, pme_quadrupole_reciprocal_space, thole_dipole_correction,
                                                          thole_induced_dipoles)

    mesh = dict(mesh_dimensions=LC.DP_MESH, spline_order=LC.PQ_ORDER)
    mesh_close = _exact if dtype == "float32" else _close_two_runs(1e-12)

    ops = {}
    for batch in (False, True):
        f = _mfx(dtype, batch)
        bkw = dict(batch_idx=f.BI) if batch else {}
        tag = " batch" if batch else ""
        leaves, names = (f.P, f.Q, f.MU, f.QD), ("positions", "charges", "dipoles", "quadrupoles")
        for label, lists, _ in _list_forms(f):
            ops[f"ewald_quadrupole_correction {label}{tag}"] = (
                lambda p, q, m, t, f=f, bkw=bkw, lists=lists: ewald_quadrupole_correction(p, q, m, t, f.C, f.AL, f.KV, **lists, **bkw), leaves, names, _exact)
            ops[f"thole_dipole_correction {label}{tag}"] = (
                lambda p, q, m, a, f=f, bkw=bkw, lists=lists: thole_dipole_correction(p, q, m, a, f.C, thole=LC.THOLE, **lists, **bkw),
                (f.P, f.Q, f.MU, f.POL), ("positions", "charges", "dipoles", "polarizability"), _exact)
        ops[f"ewald_quadrupole_reciprocal_space{tag}"] = (
            lambda p, q, m, t, f=f, bkw=bkw: ewald_quadrupole_reciprocal_space(p, q, m, t, f.C, f.KV, f.AL, **bkw), leaves, names, _exact)
        ops[f"pme_quadrupole_reciprocal_space{tag}"] = (
            lambda p, q, m, t, f=f, bkw=bkw: pme_quadrupole_reciprocal_space(p, q, m, t, f.C, f.AL, **mesh, **bkw), leaves, names, mesh_close)
        lists = _list_forms(f)[int(batch)][1]  # the matrix on the single system, CSR on the batch
        ops[f"pme_quadrupole_correction{tag}"] = (
            lambda p, q, m, t, f=f, bkw=bkw, lists=lists: pme_quadrupole_correction(p, q, m, t, f.C, f.AL, **mesh, **lists, **bkw), leaves, names, mesh_close)
        if dtype == "float64":
            g = _ifx(batch)
            gkw = dict(batch_idx=g.BI) if batch else {}
            common = dict(reciprocal="ewald", alpha=g.AL, k_vectors=g.KV, tolerance=1e-12, neighbor_matrix=g.nm, neighbor_matrix_shifts=g.sh, mask_value=g.n)
            ops[f"induced_dipoles{tag}"] = (lambda p, q, a, e, g=g, gkw=gkw, common=common: induced_dipoles(p, q, a, g.C, external_field=e, **common, **gkw),
                                           (g.P, g.Q, g.dense[None]["polar"], g.F), ("positions", "charges", "polarizability", "external_field"), _exact)
            ops[f"thole_induced_dipoles{tag}"] = (
                lambda p, q, a, e, g=g, gkw=gkw, common=common: thole_induced_dipoles(p, q, a, g.C, thole=LC.THOLE, external_field=e, **common, **gkw),
                (g.P, g.Q, g.dense[LC.THOLE]["polar"], g.F), ("positions", "charges", "polarizability", "external_field"), _exact)
    _check_gradient_layouts(ops)
    print(f"[layouts] gradient layouts {dtype}: {len(ops)} ops x 4 grad-output layouts, every gradient bit-identical to the contiguous backward"
          + (" (the four mesh ops: within the bar of two runs)" if dtype == "float64" else ""))


@DTYPES
def test_gradient_layouts_of_the_cluster_pair_scale_and_local_frame_ops(dtype):
    """The same for `coulomb_dipole_correction`, `coulomb_quadrupole_correction` and `pair_scale_correction` (matrix and CSR, periodic cut-off
    sums on the quadrupole fixture) with respect to positions, charges, dipoles and quadrupoles, and for BOTH outputs of `rotate_multipoles`
    on the fixture `frames` with respect to positions and the local multipoles, on the single system and the batch.  Every adjoint is the
    forward kernel with weights, or `mi_frame_adjoint` + `mi_frame_gather`: no atomics, equal bits."""
    from nvalchemiops.interactions.electrostatics import (LocalFrames, coulomb_dipole_correction, coulomb_quadrupole_correction, pair_scale_correction,
                                                          rotate_multipoles)

    ops = {}
    for batch in (False, True):
        f = _mfx(dtype, batch)
        bkw = dict(batch_idx=f.BI) if batch else {}
        tag = " batch" if batch else ""
        leaves, names = (f.P, f.Q, f.MU, f.QD), ("positions", "charges", "dipoles", "quadrupoles")
        for (label, lists, _), s in zip(_list_forms(f), _stored_pair_scales(f)):
            ops[f"coulomb_dipole_correction {label}{tag}"] = (
                lambda p, q, m, f=f, bkw=bkw, lists=lists: coulomb_dipole_correction(p, q, m, f.C, **lists, **bkw), leaves[:3], names[:3], _exact)
            ops[f"coulomb_quadrupole_correction {label}{tag}"] = (
                lambda p, q, m, t, f=f, bkw=bkw, lists=lists: coulomb_quadrupole_correction(p, q, m, t, f.C, **lists, **bkw), leaves, names, _exact)
            ops[f"pair_scale_correction {label}{tag}"] = (
                lambda p, q, m, t, f=f, bkw=bkw, lists=lists, s=s: pair_scale_correction(p, q, m, t, s, f.C, **lists, **bkw), leaves, names, _exact)
        g = _ffx(dtype, batch)
        fr = LocalFrames(g.ATOMS, g.KINDS, batch_idx=g.BI)
        ops[f"rotate_multipoles{tag}"] = (lambda p, m, t, g=g, fr=fr: rotate_multipoles(p, m, t, fr, g.C, batch_idx=g.BI), (g.P, g.MU, g.QD),
                                          ("positions", "local_dipoles", "local_quadrupoles"), _exact)
    _check_gradient_layouts(ops)
    print(f"[layouts] gradient layouts {dtype}: {len(ops)} ops x 4 grad-output layouts, every gradient bit-identical to the contiguous backward")


# ==== caller-owned output buffers =========================================================================================================

SENTINEL = -7


def _owned_searches(f):
    """name -> (call(nm, sh, num) -> returned tuple | None, pre-fill the call expects in the rows it writes | None)."""
    from nvalchemiops.neighborlist import (allocate_cell_list, batch_build_cell_list, batch_cell_list, batch_naive_neighbor_list, batch_query_cell_list,
                                           build_cell_list, cell_list, estimate_batch_cell_list_sizes, estimate_cell_list_sizes, naive_neighbor_list,
                                           query_cell_list)

    out = dict(neighbor_matrix=None, neighbor_matrix_shifts=None, num_neighbors=None)
    if not f.batch:
        ncell, radius = estimate_cell_list_sizes(f.C[0], f.PBC[0], RC)
        cache = allocate_cell_list(f.n, ncell, radius, f.P.device)
        build_cell_list(f.P, RC, f.C[0], f.PBC[0], *cache)
        return {
            "cell_list": (lambda nm, sh, num: cell_list(f.P, RC, f.C[0], f.PBC[0], **dict(out, neighbor_matrix=nm, neighbor_matrix_shifts=sh, num_neighbors=num)), False),
            "naive_neighbor_list": (lambda nm, sh, num: naive_neighbor_list(f.P, RC, cell=f.C[0], pbc=f.PBC[0], neighbor_matrix=nm, neighbor_matrix_shifts=sh,
                                                                            num_neighbors=num), False),
            "query_cell_list": (lambda nm, sh, num: query_cell_list(f.P, RC, f.C[0], f.PBC[0], *cache, nm, sh, num), True),
            "op neighbor_search": (lambda nm, sh, num: torch.ops.nvalchemiops.neighbor_search(f.P, f.C, f.PBC, None, RC, 0, f.n, nm, sh, num, None), False),
        }
    ncell, radius = estimate_batch_cell_list_sizes(f.C, f.PBC, RC)
    cache = allocate_cell_list(f.n, ncell, radius, f.P.device)
    batch_build_cell_list(f.P, RC, f.C, f.PBC, f.BI, *cache)
    return {
        "batch_cell_list": (lambda nm, sh, num: batch_cell_list(f.P, RC, f.C, f.PBC, f.BI, neighbor_matrix=nm, neighbor_matrix_shifts=sh, num_neighbors=num), False),
        "batch_naive_neighbor_list": (lambda nm, sh, num: batch_naive_neighbor_list(f.P, RC, batch_idx=f.BI, pbc=f.PBC, cell=f.C, neighbor_matrix=nm,
                                                                                    neighbor_matrix_shifts=sh, num_neighbors=num), False),
        "batch_query_cell_list": (lambda nm, sh, num: batch_query_cell_list(f.P, f.C, f.PBC, RC, f.BI, *cache, nm, sh, num), True),
        "op neighbor_search": (lambda nm, sh, num: torch.ops.nvalchemiops.neighbor_search(f.P, f.C, f.PBC, f.BI, RC, 0, f.n, nm, sh, num, None), False),
    }


def _fresh(f, prefilled, rows=None, width=M, dtype=I32):
    rows = f.n if rows is None else rows
    mk = lambda shape, v: torch.full(shape, v, dtype=dtype, device=DEV)  # noqa: E731
    if prefilled:  # the query entry points write hits only: the caller pre-fills (fill value N, zero shifts, zero counts)
        return mk((rows, width), f.n), mk((rows, width, 3), 0), mk((rows,), 0)
    return mk((rows, width), SENTINEL), mk((rows, width, 3), SENTINEL), mk((rows,), SENTINEL)


@pytest.mark.parametrize("batch", [False, True])
def test_row_slices_of_a_taller_buffer_are_legal_outputs(batch):
    """buf[:n] and buf[k:k+n] are contiguous: results equal the canonical call's, rows outside the slice keep the sentinel, and what the
    entry point returns is the caller's own storage."""
    f = _fx("float32", batch=batch)
    fails = []
    for name, (call, prefilled) in _owned_searches(f).items():
        def one(name=name, call=call, prefilled=prefilled):
            canon = _fresh(f, prefilled)
            ret = call(*canon)
            assert np.array_equal(_pairs(canon[0], canon[2], canon[1]), _pairs(f.nm, f.num, f.sh)), f"{name}: canonical call vs the oracle-checked list"
            if ret is not None:  # same-storage returns: (matrix, counts, shifts) ARE the caller's tensors
                assert [r.data_ptr() for r in ret] == [canon[0].data_ptr(), canon[2].data_ptr(), canon[1].data_ptr()], f"{name}: returned tensors are not the caller's storage"
            for k in (0, 3):
                tall = [torch.full((f.n + 5,) + tuple(c.shape[1:]), SENTINEL, dtype=I32, device=DEV) for c in canon]
                views = [t[k:k + f.n] for t in tall]
                if prefilled:
                    for v, c in zip(views, _fresh(f, True)):
                        v.copy_(c)
                ret = call(*views)
                for v, c, t, what in zip(views, canon, tall, ("neighbor_matrix", "neighbor_matrix_shifts", "num_neighbors")):
                    assert torch.equal(v, c), f"{name} buf[{k}:{k}+n] {what}: differs from the canonical call"
                    assert bool((t[:k] == SENTINEL).all()) and bool((t[k + f.n:] == SENTINEL).all()), f"{name} buf[{k}:{k}+n] {what}: rows outside the slice were written"
                if ret is not None:
                    assert [r.data_ptr() for r in ret] == [views[0].data_ptr(), views[2].data_ptr(), views[1].data_ptr()], f"{name}: returned tensors are not the caller's storage"
        _guarded(one, name, fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("batch", [False, True])
def test_illegal_outputs_are_refused_and_left_untouched(batch):
    """A non-contiguous output (buf[:, :m]) and an int64 output raise ValueError naming the argument -- the rule the dual-cutoff entry points
    always had, now the package's one rule -- and the whole buffer keeps its sentinel.  (Both stay inside the allocation whatever the
    library does: the column slice has N * (M + 8) elements behind it, the int64 buffer twice the bytes.)"""
    f = _fx("float32", batch=batch)
    names = ("neighbor_matrix", "neighbor_matrix_shifts", "num_neighbors")
    fails = []
    for name, (call, prefilled) in _owned_searches(f).items():
        for bad in range(3):
            for kind in ("column slice", "int64"):
                if kind == "column slice" and bad == 2:
                    continue  # num_neighbors has no columns; its strided form is in tests/test_arg_contract_cpu.py

                def one(name=name, call=call, bad=bad, kind=kind):
                    bufs = list(_fresh(f, False))
                    whole = bufs[bad]
                    if kind == "int64":
                        whole = bufs[bad] = torch.full(tuple(bufs[bad].shape), SENTINEL, dtype=I64, device=DEV)
                    else:
                        whole = torch.full((f.n, M + 8) + tuple(bufs[bad].shape[2:]), SENTINEL, dtype=I32, device=DEV)
                        bufs[bad] = whole[:, :M]
                    try:
                        call(*bufs)
                    except ValueError as e:
                        assert names[bad] in str(e), f"{name}: the ValueError does not name {names[bad]}: {e}"
                    else:
                        raise AssertionError(f"{name}: {names[bad]} ({kind}) was accepted")
                    torch.cuda.synchronize()
                    assert bool((whole == SENTINEL).all()), f"{name}: {names[bad]} ({kind}) was written before it was refused"
                    for i, b in enumerate(bufs):
                        assert bool((b == SENTINEL).all()), f"{name}: {names[i]} was written although {names[bad]} ({kind}) was refused"
                _guarded(one, f"{name} {names[bad]} {kind}", fails)
    assert not fails, "\n".join(fails)
