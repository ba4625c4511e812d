"""Sizes beyond one trip of the per-system folds of `dftd4`, `dftd4_atm`, `gaussian_charge_correction`, `charge_equilibration`,
`ewald_dipole_real_space`, `ewald_real_space_with_virial`, `ewald_quadrupole_real_space`, `thole_dipole_correction`, `induced_dipoles`,
`thole_induced_dipoles`, `pair_scale_correction`, `rotate_multipoles` / `multipole_frame_forces`, `coulomb_dipole_correction`,
`coulomb_quadrupole_correction` (as periodic cut-off sums) and `cluster_induced_dipoles`.

Every per-system sum of these ops is the fixed-order fold of csrc/pair_row.h (`mi_system_fold`) on a grid of (blocks, systems) blocks of
256 threads, each looping `r += blocks * 256` over ALL N rows and keeping those of its system: `d4_fold_kernel` (also `dftd4_atm`'s),
`gc_fold_kernel`, `gc_system_sums_kernel`, `qeq_fold_kernel`, `dp_fold_kernel` (also as `mi_thole_dipole` launches it),
`ew_virial_fold_kernel`, `qd_fold_kernel`, `ind_dot_kernel`, `ps_fold_kernel`, `fr_fold_kernel` (and `dp_fold_kernel` / `qd_fold_kernel` once
more as `mi_coulomb_dipole` / `mi_coulomb_quadrupole` launch them from their own scratch layout); `qeq_cg_update_kernel`, `qeq_cg_direction_kernel`, `ind_cg_update_kernel` and
`ind_cg_direction_kernel` walk the same grid.  The parity modules stop at a few hundred atoms; the second trip of these loops
(N > 256 * blocks = 16 384) and the batched form at that size are compared here.

No large reference is needed.  These ops take the pairs from the list, so K copies of a small system with the small list repeated
blockwise (indices + k n0, fill value N) are K independent systems, even at identical positions; the small call is judged against its
float64 reference in the same test.  K is the smallest number of copies with K n0 >= 1.5 * 256 * blocks (the second trip holds at least
a third of the rows) and K n0 no multiple of 64.

  (a) all copies as ONE system (periodic: one shared cell).  Per-atom outputs equal the tiled small call's bit for bit: the kernels are
      owner-computes with fixed-order sums and a row's arithmetic does not depend on N.  Per-system outputs:
      |X_big - K X_small| <= 2^-22 max|X_big| -- two float32 roundings with a factor 2; the float64 reordering error is negligible.  One
      lost row of 24 640 is 4e-5.
  (b) the copies as a BATCH of K systems (periodic: K cells, and once more as a stride-0 expansion of one cell).  Every system's energy
      and virial within 2^-22 max|X_small| of the small call's, per-atom outputs bit-identical again.
  Gaussian background term: the per-system charge sum feeds every atom.  In (a) Q = K Q_small, so the expectation is the small call
      without background plus K x (K^2 x for the virial) the closed-form background part of the small system, compared with the
      module's rel = 1e-11 `_close`, as are the per-atom outputs of (b) with the background switched on.
  ewald_dipole_real_space (nine-word virial) and ewald_real_space_with_virial (six words): (a) and (b) as above on the small systems of
      `test_dipole_gpu._single()` (judged against tests/dipole_reference.py at that module's rel = 1e-11) and of
      `test_electrostatic_virial_gpu._real_inputs` (judged against the strain derivative at that module's 1e-10).  The per-atom energies
      and forces of `ewald_real_space_with_virial` are asserted bit-identical too: that held on the commit before the folds were shared
      (the tiled list is a new tensor, so the big calls take the symmetry-checksum path while the small matrix call takes the trusted
      one: same bits), so the module's looser rtol 1e-12 / atol 1e-14 of its scatter path is not needed.
  charge_equilibration (cluster): the operator is block-diagonal with identical blocks, so the exact solution is the small dense KKT
      solution tiled:  max|q - q_ref| <= sqrt(K) (10 tol ||b_small|| / lambda_min + 1e-14) for the single system (||b|| grows as sqrt(K)),
      without the sqrt(K) per system of the batch -- `_check_solution`'s bound with the small block's spectrum; tol = 1e-10.
  ewald_quadrupole_real_space and thole_dipole_correction: (a) and (b) on `test_quadrupole_gpu._single()` (300 atoms) and on the single
      periodic case of tests/test_thole_gpu.py (27 atoms, rows of about 210 entries, its three non-polarisable atoms; the list padded
      with the mask value alone), every flag, both formats, the small call judged against its restatement at the module's 1e-11.
  induced_dipoles and thole_induced_dipoles: reciprocal="ewald" with an EMPTY k set -- `k_vectors` [0, 3] is accepted, as
      `ewald_dipole_reciprocal_space` accepts it, and leaves the self term alone, so the copies do not couple -- on the 27-atom lattice
      with a list cutoff of 6 (`thole_cases.fold_case()`; tests/test_induced_reference_cpu.py asserts that this truncated H is positive
      definite).  The bound is the QEq one, with `_check_solution` of tests/test_induced_gpu.py for the small call.  `mi_induced_dot` and
      the `partial` output of `mi_induced_apply` on K n0 random rows against float64 torch sums per system, at the fold bar.
  pair_scale_correction: with explicit shifts (the `MIN = false` kernels) on the 24-atom triclinic box of tests/pair_scale_cases.py, and
      with `minimum_image=True` (the `MIN = true` kernels) on its three wrapped molecules -- (b) is their batch of three cells tiled to
      3 K systems, (a) the 9-atom chain alone in its cell -- every flag, both formats.  The matrices keep all three kinds of padding
      (`_tile_padded_matrix`: a -1 slot stays -1) and NaN scales on the padding; `pair_scales` is tiled like the shifts.
  rotate_multipoles + multipole_frame_forces(compute_local_gradients, compute_virial): the "triclinic" case of
      tests/test_local_frames_gpu.py (25 atoms, every kind, wrapped positions); `LocalFrames` is built from the tiled tables.  Dipoles,
      quadrupoles, torque forces and both local gradients bit for bit; the virial term of `fr_fold_kernel` at the fold bar.
  coulomb_dipole_correction / coulomb_quadrupole_correction with a cell: the periodic problem of tests/cluster_multipole_reference.py
      (96 atoms) with its list cut to the entries within 7.0 plus every self image (the shortest lattice vector is 8.87, so a plain cutoff
      below it would hold none): rows of 130 - 145 entries, 3.4 M entries tiled.  The first periodic BATCH of the bare kind.
  cluster_induced_dipoles: K copies of the 150-atom cluster over its all-pairs list (3.7 M entries), undamped and thole = 0.39, as one
      system and with num_systems = K; the bound of the induced-dipole test above, and the iteration count equal to the small call's.

MEASURED on one MI355X (each test prints its figures under `pytest -s`; matrix and CSR agree to the digits shown).  Per-atom outputs:
bit-identical wherever that is asserted.  Worst |X_big - K X_small| / bar as ONE system:
  dftd4      molecule70 (K 353, N 24 710)      E 0.215                 triclinic_f32 (K 1366, N 24 588)  E 0.352  V 0.107
  dftd4_atm  molecule70                        E 0.104                 triclinic_f32                     E 0.148  V 0.052
  gaussian   300 atoms (K 82, N 24 600)        V 8.7e-10 (without background); with background, relative to max|ref| against the bar
             1e-11: energies 1.4e-16, forces 0, charge gradients 3.1e-16, sigma gradients 2.1e-16, virial 3.6e-16
As a BATCH of K systems: every energy and virial of dftd4 and dftd4_atm EQUAL to the small call's (error 0), with K cells and with the
stride-0 cell; gaussian virial 3.6e-15 and 5.3e-15 absolute (1.1e-9 and 1.8e-9 of the bar).
  dipole real space  300 atoms (K 82, N 24 600): small call against the reference 6.0e-16 / 1.3e-15 / 1.3e-16 / 8.9e-16 / 1.8e-14
             (energies / forces / charge / dipole gradients / virial, bar 1e-11); virial as one system 3.6e-12 (5.7e-10 of the bar), in the
             batch 1.1e-13 (1.5e-9 of the bar) with K cells and with the stride-0 cell
  ewald real space   160 atoms (K 155, N 24 800): virial as one system 2.3e-13 (1.5e-9 of the bar), in the batch 8.9e-16 (8.8e-10 of the
             bar), both cell forms; energies and forces bit-identical, here and at the commit before the folds were shared
  charge_equilibration  60 atoms (K 410, N 24 600): max|q - q_ref| 2.9e-11 as one system (bar 1.3e-7) and in the worst system of the batch
             (bar 6.2e-9); 19 iterations in the small call, the single system and all 410 systems of the batch.
  quadrupole real space  300 atoms (K 82, N 24 600): small call against the reference 1.4e-15 / 1.3e-15 / 3.7e-16 / 7.1e-16 / 6.6e-16 /
             6.0e-14 (energies / forces / charge / dipole / quadrupole gradients / virial, bar 1e-11); virial as one system 2.3e-10
             (3.7e-10 of the bar), in the batch 7.3e-12 (9.6e-10 of the bar) with K cells and with the stride-0 cell.  With
             `qd_fold_kernel` cut to its first trip (a scratch build) the one-system virial is off by 2.1e6 bars, and
             tests/test_quadrupole_gpu.py still passes.
  thole      27 atoms (K 911, N 24 597): small call 1.1e-15 at worst (bar 1e-11); virial as one system 2.8e-14 (6.2e-10 of the bar), in
             the batch 2.8e-17 (5.5e-10 of the bar), both cell forms
  induced_dipoles  27 atoms (K 911, N 24 597), empty k set: max|mu - mu_ref| 3.0e-12 undamped and 1.0e-12 damped, as one system (bars
             2.1e-8 and 1.9e-8) and in the worst system of the batch (bars 6.9e-10 and 6.2e-10), both cell forms; 10 iterations in the
             small call, the single system and all 911 systems of the batch (reference PCG: 10)
  mi_induced_dot / mi_induced_apply partial  24 597 random rows: 1.2e-9 / 0 of the bar as one system, 8.8e-10 / 1.2e-9 as 911 systems
  pair_scale  24 atoms (K 1025, N 24 600), shifts: small call 1.1e-15 at worst (bar 1e-11); virial as one system 1.8e-12 (8.8e-10 of the
             bar), in the batch 1.8e-15 (8.8e-10 of the bar), both cell forms.  Minimum image: the batch of 17 atoms in three cells (K 1446,
             4338 systems, N 24 582) small call 1.3e-15, every system's virial 1.8e-15 (9.0e-10 of the bar); the chain (K 2731, N 24 579) as
             one system 3.6e-12 (6.8e-10 of the bar).  With `ps_fold_kernel` cut to its first trip (a scratch build, all reads in range) the
             one-system virial is off by 2.1e6 bars and the virials of the minimum-image batch by 4.2e6 bars -- all four tests fail -- and
             tests/test_pair_scale_gpu.py still passes (35 tests).
  local frames  25 atoms (K 984, N 24 600): virial term as one system 3.6e-12 (7.0e-10 of the bar), in the batch 3.6e-15 (6.8e-10 of the
             bar), both cell forms.  With `fr_fold_kernel` cut to its first trip the one-system virial term is off by 2.1e6 bars, and
             tests/test_local_frames_gpu.py still passes (45 tests).
  cluster dipole / quadrupole, periodic  96 atoms (K 257, N 24 672, 3.4 M entries): small call 2.7e-15 / 3.7e-15 at worst (bar 1e-11);
             virial as one system 2.3e-13 / 4.5e-13 (6.9e-10 / 6.2e-10 of the bar), in the batch 8.9e-16 / 2.7e-15 (6.9e-10 / 9.3e-10 of
             the bar), both cell forms
  cluster_induced_dipoles  150 atoms (K 164, N 24 600): max|mu - mu_ref| 6.1e-12 undamped and 2.7e-11 damped, as one system (bars 1.4e-7)
             and in the worst system of the batch (bars 1.1e-8); 8 / 15 iterations in the small call, the single system and all 164
             systems of the batch (reference PCG: 8 / 15)
Matrix and CSR agree to the digits shown; per-atom outputs bit-identical wherever that is asserted."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import cluster_multipole_reference as CR
from tests import d4_atm_cases as K3
from tests import d4_cases as K4
from tests import pair_scale_reference as PR
from tests import qeq_reference as QR
from tests import test_cluster_multipole_gpu as TCM
from tests import test_d4_atm_gpu as TD4A
from tests import test_d4_gpu as TD4
from tests import test_dipole_gpu as TDP
from tests import test_electrostatic_virial_gpu as TV
from tests import test_gaussian_charges_gpu as TG
from tests import test_induced_gpu as TI
from tests import test_local_frames_gpu as TLF
from tests import test_pair_scale_gpu as TPS
from tests import test_qeq_gpu as TQ
from tests import test_quadrupole_gpu as TQD
from tests import test_thole_gpu as TTH
from tests import thole_cases as TC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64
FOLD = 2.0 ** -22


def _copies(n0, blocks):
    k = math.ceil(1.5 * 256 * blocks / n0)
    while (k * n0) % 64 == 0:
        k += 1
    assert 3 * (k * n0 - 256 * blocks) >= k * n0, "the second trip must hold at least a third of the rows"
    return k


def _tile_matrix(nm, sh, k):
    """[n0, M] with fill value n0 -> [k n0, M] with fill value k n0: block b holds the small list shifted by b n0."""
    n0 = nm.shape[0]
    off = (torch.arange(k, device=nm.device, dtype=nm.dtype) * n0)[:, None, None]
    big = torch.where(nm[None] == n0, torch.full_like(nm[None], k * n0), nm[None] + off).reshape(k * n0, -1).contiguous()
    return big, None if sh is None else sh.repeat(k, 1, 1).contiguous()


def _tile_padded_matrix(nm, k):
    """`_tile_matrix` for a matrix that holds all three kinds of padding (the mask value n0, -1 and n0 + 7): a -1 slot stays -1, a value
    >= n0 moves up by (k - 1) n0, so the mask value becomes k n0 and n0 + 7 becomes k n0 + 7, outside [0, k n0) again."""
    n0 = nm.shape[0]
    off = (torch.arange(k, device=nm.device, dtype=nm.dtype) * n0)[:, None, None]
    pad = torch.where(nm < 0, nm, nm + (k - 1) * n0)
    return torch.where(((nm >= 0) & (nm < n0))[None], nm[None] + off, pad[None]).reshape(k * n0, -1).contiguous()


def _tile_csr(lst, ptr, lsh, k):
    n0, p0 = ptr.shape[0] - 1, lst.shape[1]
    off = torch.arange(k, device=lst.device, dtype=lst.dtype)
    big = (lst[:, None, :] + (off * n0)[None, :, None]).reshape(2, k * p0).contiguous()
    bptr = torch.cat([(ptr[None, :-1] + (off * p0)[:, None]).reshape(-1), ptr.new_tensor([k * p0])]).contiguous()
    return big, bptr, None if lsh is None else lsh.repeat(k, 1).contiguous()


def _fold_close(big, small_times_k, scale, what):
    err = float((big.double() - small_times_k.double()).abs().max())
    bar = FOLD * float(scale.double().abs().max())
    print(f"[fold] {what:58s} max error {err:.3e}  bar {bar:.3e}  error / bar {err / bar if bar else 0.0:.3g}")
    assert err <= bar, f"{what}: {err:.3e} > {bar:.3e}"


def _bitwise(big, small, k, what):
    tiled = small.repeat((k,) + (1,) * (small.dim() - 1))
    assert torch.equal(big, tiled), f"{what}: per-atom output differs from the tiled small call's by up to {float((big - tiled).abs().max()):.3e}"


# ---- dftd4 / dftd4_atm ---------------------------------------------------------------------------------------------------------------------

def _d4_blocks():
    from nvalchemiops import _capi as C

    return int(C.lib().mi_d4_fold_blocks())


@pytest.mark.parametrize("name", ["molecule70", "triclinic_f32"])
@pytest.mark.parametrize("op", ["dftd4", "dftd4_atm"])
def test_d4_copies_as_one_system_and_as_a_batch(op, name):
    from nvalchemiops.interactions.dispersion import dftd4, dftd4_atm

    if op == "dftd4":
        c, args, kw, m, l, _ = TD4._inputs(name)
        fn, judge, refs, per_atom = dftd4, TD4._judge, K4.references(name), (1, 2, 3)
    else:
        c, args, kw, m, l, _ = TD4A._inputs(name)
        fn, judge, refs, per_atom = dftd4_atm, TD4A._judge, K3.references(name), (1,)
    n0, periodic = len(c["pos"]), c["cell"] is not None
    k = _copies(n0, _d4_blocks())
    n = k * n0
    assert n > 256 * _d4_blocks() and n % 64 != 0
    big_args = tuple(a.repeat((k,) + (1,) * (a.dim() - 1)) for a in args)
    bi = torch.arange(k, device=DEV, dtype=torch.int32).repeat_interleave(n0)
    nm, sh = _tile_matrix(m["neighbor_matrix"], m.get("neighbor_matrix_shifts"), k)
    lst, ptr, lsh = _tile_csr(l["neighbor_list"], l["neighbor_ptr"], l.get("unit_shifts"), k)
    layouts = (("matrix", m, dict(neighbor_matrix=nm, **(dict(neighbor_matrix_shifts=sh) if periodic else {}))),
               ("csr", l, dict(neighbor_list=lst, neighbor_ptr=ptr, **(dict(unit_shifts=lsh) if periodic else {}))))
    for tag, small_lists, big_lists in layouts:
        small = fn(*args, **kw, **small_lists)
        judge(f"fold sizes {op} {name} {tag}: the small call", small, *refs)
        per_system = (0, len(small) - 1) if periodic else (0,)
        # (a) one system of K n0 atoms
        one = fn(*big_args, **kw, **big_lists)
        for i in per_atom:
            _bitwise(one[i], small[i], k, f"{op} {name} {tag} one system, output {i}")
        for i in per_system:
            _fold_close(one[i], k * small[i].double(), one[i], f"{op} {name} {tag} one system of {n} atoms, output {i}")
        # (b) a batch of K systems
        cells = [None]
        if periodic:
            full = kw["cell"].repeat(k, 1, 1).contiguous()
            cells = [full, kw["cell"][:1].expand(k, 3, 3)]
            assert cells[1].stride(0) == 0
        for cell in cells:
            bkw = dict(kw, batch_idx=bi, num_systems=k, **({} if cell is None else dict(cell=cell)))
            many = fn(*big_args, **bkw, **big_lists)
            for i in per_atom:
                _bitwise(many[i], small[i], k, f"{op} {name} {tag} batch, output {i}")
            for i in per_system:
                assert many[i].shape[0] == k
                _fold_close(many[i], small[i].double().expand_as(many[i]), small[i],
                            f"{op} {name} {tag} batch of {k}{'' if cell is None or cell.stride(0) else ' (stride-0 cell)'}, output {i}")


# ---- gaussian_charge_correction --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", ["matrix", "list"])
def test_gaussian_copies_as_one_system_and_as_a_batch(fmt):
    from nvalchemiops import _capi as C
    from nvalchemiops.interactions.electrostatics import gaussian_charge_correction as gcc

    f = TG._single()
    n0, blocks = f["n"], int(C.lib().mi_gaussian_charges_blocks())
    k = _copies(n0, blocks)
    n = k * n0
    assert n > 256 * blocks and n % 64 != 0
    P, Q, S = (f[x].repeat((k,) + (1,) * (f[x].dim() - 1)) for x in ("P", "Q", "S"))
    if fmt == "matrix":
        nm, sh = _tile_matrix(f["nm"], f["sh"], k)
        big = dict(neighbor_matrix=nm, neighbor_matrix_shifts=sh, mask_value=n)
    else:
        lst, ptr, lsh = _tile_csr(f["nl"], f["ptr"], f["lsh"], k)
        big = dict(neighbor_list=lst, neighbor_ptr=ptr, neighbor_shifts=lsh)
    small = gcc(f["P"], f["Q"], f["S"], f["C"], **TG._fmt_kw(f, fmt), **TG.ALL)
    for name, o in zip(TG.NAMES, small):
        TG._close(o, f["ref"][name], f"fold sizes gaussian {fmt}: the small call, {name}")
    plain = gcc(f["P"], f["Q"], f["S"], f["C"], **TG._fmt_kw(f, fmt), neutralizing_background=False, **TG.ALL)
    # the closed-form background part of the small system: (2 pi / V) Q q_i s_i and its derivatives
    s = torch.clamp(f["S"], min=0.0) ** 2
    pref = 2.0 * math.pi / float(torch.linalg.det(f["C"][0]).abs())
    qsum, qssum = f["Q"].sum(), (f["Q"] * s).sum()
    bg = (pref * qsum * f["Q"] * s, None, pref * qssum + pref * qsum * s, 2.0 * pref * qsum * f["Q"] * torch.clamp(f["S"], min=0.0),
          (pref * qsum * qssum) * torch.eye(3, dtype=F64, device=DEV)[None])
    # (a) one system: without background bit for bit and the virial fold; with background the expectation above
    one = gcc(P, Q, S, f["C"], **big, neutralizing_background=False, **TG.ALL)
    for i in range(4):
        _bitwise(one[i], plain[i], k, f"gaussian {fmt} one system without background, {TG.NAMES[i]}")
    _fold_close(one[4], k * plain[4], one[4], f"gaussian {fmt} one system of {n} atoms without background, virial")
    one = gcc(P, Q, S, f["C"], **big, **TG.ALL)
    for i, name in enumerate(TG.NAMES):
        want = plain[i] if bg[i] is None else plain[i] + k * bg[i]
        want = want.repeat((k,) + (1,) * (want.dim() - 1)) if i < 4 else k * plain[4] + k * k * bg[4]
        print(f"[fold] gaussian {fmt} one system with background, {name:13s} relative error {TG._close(one[i], want, f'gaussian {fmt} one system, {name}'):.3e}  (bar 1e-11)")
    # (b) a batch of K systems: K cells, and one cell as a stride-0 expansion
    bi = torch.arange(k, device=DEV, dtype=torch.int32).repeat_interleave(n0)
    for cell in (f["C"].repeat(k, 1, 1).contiguous(), f["C"][:1].expand(k, 3, 3)):
        label = f"gaussian {fmt} batch of {k}{'' if cell.stride(0) else ' (stride-0 cell)'}"
        many = gcc(P, Q, S, cell, batch_idx=bi, **big, neutralizing_background=False, **TG.ALL)
        for i in range(4):
            _bitwise(many[i], plain[i], k, f"{label} without background, {TG.NAMES[i]}")
        _fold_close(many[4], plain[4].expand_as(many[4]), plain[4], f"{label} without background, virial")
        many = gcc(P, Q, S, cell, batch_idx=bi, **big, **TG.ALL)
        for i in range(4):
            TG._close(many[i], small[i].repeat((k,) + (1,) * (small[i].dim() - 1)), f"{label}, {TG.NAMES[i]}")
        _fold_close(many[4], small[4].expand_as(many[4]), small[4], f"{label}, virial")


# ---- ewald_dipole_real_space / ewald_real_space_with_virial --------------------------------------------------------------------------------

def _check_copies(label, small, one, many, k, per_atom, vir):
    """`small`: the outputs of the small call; `one`: of its K copies as one system; `many`: [(tag, outputs)] of the copies as a batch."""
    for i in per_atom:
        _bitwise(one[i], small[i], k, f"{label} one system, output {i}")
    _fold_close(one[vir], k * small[vir].double(), one[vir], f"{label} one system of {k * small[0].shape[0]} atoms, virial")
    for tag, out in many:
        for i in per_atom:
            _bitwise(out[i], small[i], k, f"{label} batch{tag}, output {i}")
        assert out[vir].shape[0] == k
        _fold_close(out[vir], small[vir].expand_as(out[vir]), small[vir], f"{label} batch of {k}{tag}, virial")


def _tiled_lists(fmt, nm, sh, nl, ptr, lsh, k, n):
    if fmt == "matrix":
        nm, sh = _tile_matrix(nm, sh, k)
        return dict(neighbor_matrix=nm, neighbor_matrix_shifts=sh, mask_value=n)
    lst, ptr, lsh = _tile_csr(nl, ptr, lsh, k)
    return dict(neighbor_list=lst, neighbor_ptr=ptr, neighbor_shifts=lsh)


@pytest.mark.parametrize("fmt", ["matrix", "list"])
def test_dipole_real_space_copies_as_one_system_and_as_a_batch(fmt):
    from nvalchemiops import _capi as C
    from nvalchemiops.interactions.electrostatics import ewald_dipole_real_space as real

    f = TDP._single()
    n0, blocks = f["n"], int(C.lib().mi_ewald_dipole_blocks())
    k = _copies(n0, blocks)
    n = k * n0
    assert n > 256 * blocks and n % 64 != 0
    small = real(f["P"], f["Q"], f["M"], f["C"], f["A"], **TDP._fmt_kw(f, fmt), **TDP.ALL)
    for name, o in zip(TDP.NAMES, small):
        TDP._close(o, f["ref_real"][name], f"fold sizes dipole {fmt}: the small call, {name}")
    P, Q, M = (f[x].repeat((k,) + (1,) * (f[x].dim() - 1)) for x in ("P", "Q", "M"))
    big = _tiled_lists(fmt, f["nm"], f["sh"], f["nl"], f["ptr"], f["lsh"], k, n)
    one = real(P, Q, M, f["C"], f["A"], **big, **TDP.ALL)
    bi = torch.arange(k, device=DEV, dtype=torch.int32).repeat_interleave(n0)
    many = [(tag, real(P, Q, M, cell, TDP.ALPHA, batch_idx=bi, **big, **TDP.ALL))
            for tag, cell in (("", f["C"].repeat(k, 1, 1).contiguous()), (" (stride-0 cell)", f["C"][:1].expand(k, 3, 3)))]
    _check_copies(f"dipole real space {fmt}", small, one, many, k, per_atom=(0, 1, 2, 3), vir=4)


@pytest.mark.parametrize("kind", ["matrix", "csr"])
def test_ewald_real_space_virial_copies_as_one_system_and_as_a_batch(kind):
    from nvalchemiops import _capi as C
    from nvalchemiops.interactions.electrostatics import ewald_real_space, ewald_real_space_with_virial as real

    P0, Cc, Q0, nl = TV._real_inputs(kind)
    n0, blocks = P0.shape[0], int(C.lib().mi_ewald_virial_blocks())
    k = _copies(n0, blocks)
    n = k * n0
    assert n > 256 * blocks and n % 64 != 0
    alpha = torch.tensor([0.35], dtype=F64, device=DEV)
    small = real(P0, Q0, Cc[None], alpha, compute_forces=True, **nl)
    TV._close(small[2], TV._strain_derivative(lambda p, c: ewald_real_space(p, Q0, c, alpha, **nl), P0, Cc), 1e-10,
              f"fold sizes ewald {kind}: the small call, virial")
    P, Q = P0.repeat(k, 1), Q0.repeat(k)
    big = _tiled_lists(kind, nl.get("neighbor_matrix"), nl.get("neighbor_matrix_shifts"), nl.get("neighbor_list"), nl.get("neighbor_ptr"),
                       nl.get("neighbor_shifts"), k, n)
    one = real(P, Q, Cc[None], alpha, compute_forces=True, **big)
    bi = torch.arange(k, device=DEV, dtype=torch.int32).repeat_interleave(n0)
    many = [(tag, real(P, Q, cell, alpha.expand(k).contiguous(), batch_idx=bi, compute_forces=True, **big))
            for tag, cell in (("", Cc[None].repeat(k, 1, 1).contiguous()), (" (stride-0 cell)", Cc[None].expand(k, 3, 3)))]
    _check_copies(f"ewald real space {kind}", small, one, many, k, per_atom=(0, 1), vir=2)


# ---- charge_equilibration ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", ["matrix", "csr"])
def test_charge_equilibration_copies_as_one_system_and_as_a_batch(fmt):
    from nvalchemiops import _capi as C
    from nvalchemiops.interactions.electrostatics import charge_equilibration as qeq

    tol, total, max_iterations = 1e-10, -0.7, 200
    f = TQ._cluster((60,), 33)
    n0, blocks = f["n"], int(C.lib().mi_qeq_blocks())
    k = _copies(n0, blocks)
    n = k * n0
    assert n > 256 * blocks and n % 64 != 0
    h = QR.dense_operator(f["pos"], f["sigma"], f["hard"], None, None, None, *f["ent"])
    out = qeq(f["pos"], f["chi"], f["hard"], f["sigma"], total_charge=total, tolerance=tol, return_info=True, **TQ._kw(f, fmt, shifts=False))
    q_ref, _ = TQ._check_solution(out, h, f["chi"], total, None, 1, tol, max_iterations, f"fold sizes qeq {fmt}: the small call")
    b_norm = float(QR.projected_residual(h, f["chi"], torch.full((n0,), total / n0, dtype=F64, device=DEV))[0])
    dq = 10.0 * tol * b_norm / float(torch.linalg.eigvalsh(h).min()) + 1e-14
    pos, chi, hard, sigma = (f[x].repeat((k,) + (1,) * (f[x].dim() - 1)) for x in ("pos", "chi", "hard", "sigma"))
    if fmt == "matrix":
        nm, _ = _tile_matrix(f["nm"], None, k)
        big = dict(neighbor_matrix=nm, mask_value=n)
    else:
        lst, ptr, _ = _tile_csr(f["nl"], f["ptr"], None, k)
        big = dict(neighbor_list=lst, neighbor_ptr=ptr)
    want = q_ref.repeat(k)
    # one system of K n0 atoms with total charge K Q
    one = qeq(pos, chi, hard, sigma, total_charge=k * total, tolerance=tol, max_iterations=max_iterations, return_info=True, **big)
    err = float((one.charges - want).abs().max())
    print(f"[fold] qeq {fmt} one system of {n} atoms: max|q - q_ref| {err:.3e}  bar {math.sqrt(k) * dq:.3e}  iterations {one.iterations.tolist()}")
    assert err <= math.sqrt(k) * dq
    assert abs(float(one.charges.sum()) - k * total) <= 1e-12 * n and int(one.iterations[0]) <= max_iterations
    # a batch of K systems
    bi = torch.arange(k, device=DEV, dtype=torch.int32).repeat_interleave(n0)
    many = qeq(pos, chi, hard, sigma, total_charge=torch.full((k,), total, dtype=F64, device=DEV), batch_idx=bi, tolerance=tol,
               max_iterations=max_iterations, return_info=True, **big)
    err = (many.charges - want).abs().reshape(k, n0).max(1).values
    print(f"[fold] qeq {fmt} batch of {k}: worst system max|q - q_ref| {float(err.max()):.3e}  bar {dq:.3e}  iterations {int(many.iterations.min())} - "
          f"{int(many.iterations.max())}")
    assert bool((err <= dq).all())
    assert bool(((many.charges.reshape(k, n0).sum(1) - total).abs() <= 1e-12 * n0).all()) and bool((many.iterations <= max_iterations).all())


# ---- ewald_quadrupole_real_space / thole_dipole_correction ---------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", ["matrix", "list"])
def test_quadrupole_real_space_copies_as_one_system_and_as_a_batch(fmt):
    from nvalchemiops import _capi as C
    from nvalchemiops.interactions.electrostatics import ewald_quadrupole_real_space as real

    f = TQD._single()
    n0, blocks = f["n"], int(C.lib().mi_ewald_quadrupole_blocks())
    k = _copies(n0, blocks)
    n = k * n0
    assert n > 256 * blocks and n % 64 != 0
    small = real(f["P"], f["Q"], f["M"], f["T"], f["C"], f["A"], **TQD._fmt_kw(f, fmt), **TQD.ALL)
    for name, o in zip(TQD.NAMES, small):
        TQD._close(o, f["ref_real"][name], f"fold sizes quadrupole {fmt}: the small call, {name}")
    P, Q, M, T = (f[x].repeat((k,) + (1,) * (f[x].dim() - 1)) for x in ("P", "Q", "M", "T"))
    big = _tiled_lists(fmt, f["nm"], f["sh"], f["nl"], f["ptr"], f["lsh"], k, n)
    one = real(P, Q, M, T, f["C"], f["A"], **big, **TQD.ALL)
    bi = torch.arange(k, device=DEV, dtype=torch.int32).repeat_interleave(n0)
    many = [(tag, real(P, Q, M, T, cell, TQD.ALPHA, batch_idx=bi, **big, **TQD.ALL))
            for tag, cell in (("", f["C"].repeat(k, 1, 1).contiguous()), (" (stride-0 cell)", f["C"][:1].expand(k, 3, 3)))]
    _check_copies(f"quadrupole real space {fmt}", small, one, many, k, per_atom=(0, 1, 2, 3, 4), vir=5)


@pytest.mark.parametrize("fmt", ["matrix", "list"])
def test_thole_dipole_correction_copies_as_one_system_and_as_a_batch(fmt):
    """The single periodic case of tests/test_thole_gpu.py (27 atoms, rows of about 210 entries, atoms with a = 0, a < 0 and a = NaN) over a
    list padded with the mask value alone: the other two kinds of padding of that case (-1, N + 7) would turn into indices of other copies
    when the list is tiled."""
    from nvalchemiops import _capi as C
    from nvalchemiops.interactions.electrostatics import thole_dipole_correction as th

    c = TTH._abi_case("single")
    n0, blocks = c["n"], int(C.lib().mi_thole_dipole_blocks())
    f = TTH._lists(*c["ent"], n0)
    k = _copies(n0, blocks)
    n = k * n0
    assert n > 256 * blocks and n % 64 != 0
    p0, q0, m0, a0, cell = (TTH._t(c[x]) for x in ("pos", "q", "mu", "polar", "cells"))
    small = th(p0, q0, m0, a0, cell, **TTH._kw(f, fmt), **TTH.ALL)
    ref = TTH._abi_reference("single", F64)
    for name, o in zip(TTH.NAMES, small):
        TTH._close(o, ref[name], f"fold sizes thole {fmt}: the small call, {name}", 1e-11)
    P, Q, M, A = (x.repeat((k,) + (1,) * (x.dim() - 1)) for x in (p0, q0, m0, a0))
    big = _tiled_lists(fmt, f["nm"], f["sh"], f["nl"], f["ptr"], f["lsh"], k, n)
    one = th(P, Q, M, A, cell, **big, **TTH.ALL)
    bi = torch.arange(k, device=DEV, dtype=torch.int32).repeat_interleave(n0)
    many = [(tag, th(P, Q, M, A, cells, batch_idx=bi, **big, **TTH.ALL))
            for tag, cells in (("", cell.repeat(k, 1, 1).contiguous()), (" (stride-0 cell)", cell[:1].expand(k, 3, 3)))]
    _check_copies(f"thole {fmt}", small, one, many, k, per_atom=(0, 1, 2, 3, 4), vir=5)


# ---- induced_dipoles / thole_induced_dipoles -----------------------------------------------------------------------------------------------

def _induced_copies():
    """(case, small lists, K, blocks) of `thole_cases.fold_case()`: 27 atoms, so K = 911 and N = 24 597."""
    from nvalchemiops import _capi as C

    case = TC.fold_case()
    blocks = int(C.lib().mi_induced_blocks())
    k = _copies(case["n"], blocks)
    assert k * case["n"] > 256 * blocks and (k * case["n"]) % 64 != 0
    return case, TTH._lists(*case["entries"], case["n"]), k, blocks


@pytest.mark.parametrize("thole", [None, TC.THOLE], ids=["undamped", "thole"])
@pytest.mark.parametrize("fmt", ["matrix", "list"])
def test_induced_dipoles_copies_as_one_system_and_as_a_batch(fmt, thole):
    """reciprocal="ewald" with an EMPTY k set: the reciprocal term is the self term alone, the operator of the copies is block-diagonal with
    identical blocks and the exact solution is the small dense solution tiled.  `_check_solution`'s bound with the small block's spectrum:
    max|mu - mu_ref| <= 10 tol ||b_small|| / lambda_min + 1e-14 per system of the batch, times sqrt(K) for the single system (||b|| grows as
    sqrt(K)), as for `charge_equilibration` above."""
    from nvalchemiops.interactions.electrostatics import induced_dipoles, thole_induced_dipoles

    tol = 1e-10
    case, f, k, _ = _induced_copies()
    n0, n = case["n"], k * case["n"]
    d = TC.dense(case, thole, DEV)
    assert d["kv"].shape == (0, 3)
    solve = induced_dipoles if thole is None else (lambda *a, **kw: thole_induced_dipoles(*a, thole=thole, **kw))
    common = dict(reciprocal="ewald", k_vectors=d["kv"], tolerance=tol, return_info=True)
    p0, q0, cell = TTH._t(case["pos"]), TTH._t(case["q"]), TTH._t(case["cell"]).reshape(1, 3, 3)
    label = f"{'induced' if thole is None else 'thole induced'} {fmt}"
    out = solve(p0, q0, d["polar"], cell, alpha=case["alpha"], **common, **TTH._kw(f, fmt))
    mu_ref = TI._check_solution(out, d["H"], d["b"], d["polar"], None, 1, tol, f"fold sizes {label}: the small call")
    dmu = 10.0 * tol * float(d["b"].norm()) / float(torch.linalg.eigvalsh(d["H"]).min()) + 1e-14
    P, Q, A = p0.repeat(k, 1), q0.repeat(k), d["polar"].repeat(k)
    big = _tiled_lists(fmt, f["nm"], f["sh"], f["nl"], f["ptr"], f["lsh"], k, n)
    want = mu_ref.repeat(k, 1)
    # one system of K n0 atoms
    one = solve(P, Q, A, cell, alpha=case["alpha"], **common, **big)
    err = float((one.dipoles - want).abs().max())
    print(f"[fold] {label} one system of {n} atoms: max|mu - mu_ref| {err:.3e}  bar {math.sqrt(k) * dmu:.3e}  iterations {one.iterations.tolist()} "
          f"(small call {out.iterations.tolist()})")
    assert err <= math.sqrt(k) * dmu and float(one.residual[0]) <= tol
    # a batch of K systems: K cells, and one cell as a stride-0 expansion
    bi = torch.arange(k, device=DEV, dtype=torch.int32).repeat_interleave(n0)
    for tag, cells in (("", cell.repeat(k, 1, 1).contiguous()), (" (stride-0 cell)", cell[:1].expand(k, 3, 3))):
        many = solve(P, Q, A, cells, alpha=torch.full((k,), case["alpha"], dtype=F64, device=DEV), batch_idx=bi, **common, **big)
        err = (many.dipoles - want).abs().reshape(k, -1).max(1).values
        print(f"[fold] {label} batch of {k}{tag}: worst system max|mu - mu_ref| {float(err.max()):.3e}  bar {dmu:.3e}  iterations "
              f"{int(many.iterations.min())} - {int(many.iterations.max())}")
        assert bool((err <= dmu).all()) and bool((many.residual <= tol).all())
        energy = many.polarization_energy
        assert bool(((energy - out.polarization_energy).abs() <= 100.0 * tol * out.polarization_energy.abs() + 1e-14).all())


@pytest.mark.parametrize("fmt", ["matrix", "csr"])
def test_induced_dot_and_apply_partials_beyond_one_trip(fmt):
    """`mi_induced_dot` and the `partial` output of `mi_induced_apply` on K n0 random rows against float64 torch sums per system, as one
    system and as a batch of K; the products themselves equal the tiled small product bit for bit."""
    from nvalchemiops import _capi as C

    case, f, k, blocks = _induced_copies()
    n0, n = case["n"], k * case["n"]
    g = torch.Generator(device="cpu").manual_seed(41)
    x, y = (torch.randn((n, 3), dtype=F64, generator=g).to(DEV) for _ in range(2))
    bi = torch.arange(k, device=DEV, dtype=torch.int32).repeat_interleave(n0)
    p0, a0, cell, al = TTH._t(case["pos"]), TTH._t(case["polar"]), TTH._t(case["cell"]).reshape(1, 3, 3), TTH._t(np.array([case["alpha"]]))
    if fmt == "matrix":
        nm, sh = _tile_matrix(f["nm"], f["sh"], k)
        idx, nptr, m = nm, None, nm.shape[1]
        small_lay = (f["nm"], f["sh"], None, f["nm"].shape[1])
    else:
        lst, nptr, sh = _tile_csr(f["nl"], f["ptr"], f["lsh"], k)
        idx, m = lst[1].contiguous(), 0
        small_lay = (f["nl"][1].contiguous(), f["lsh"], f["ptr"], 0)
    ten0, nbr0, diag0, _ = TI._tensors(p0, a0, cell, al, None, 1, *small_lay, n0)
    P, A = p0.repeat(k, 1), a0.repeat(k)
    for label, b, nsys, cells, alpha in (("one system", None, 1, cell, al), (f"batch of {k}", bi, k, cell.repeat(k, 1, 1).contiguous(), al.repeat(k))):
        part = torch.full((nsys, blocks), float("nan"), dtype=F64, device=DEV)
        C.check(C.lib().mi_induced_dot(C.ptr(x), C.ptr(y), C.ptr(b), n, nsys, C.ptr(part), C.stream_of(x)), "mi_induced_dot")
        want = (x * y).sum(1).reshape(nsys, -1).sum(1)
        _fold_close(part.sum(1), want, want, f"mi_induced_dot {label} of {n} rows")
        ten, nbr, diag, _ = TI._tensors(P, A, cells, alpha, b, nsys, idx, sh, nptr, m, n)
        hx, part = TI._apply(ten, nbr, diag, x, None, b, nsys, nptr, m)
        want = (x * hx).sum(1).reshape(nsys, -1).sum(1)
        _fold_close(part.sum(1), want, want, f"mi_induced_apply {fmt} partial, {label}")
        for s in (0, k // 2, k - 1):  # the product of a copy is the small product on that copy's rows
            rows = slice(s * n0, (s + 1) * n0)
            assert torch.equal(hx[rows], TI._apply(ten0, nbr0, diag0, x[rows].contiguous(), None, None, 1, small_lay[2], small_lay[3], want_partial=False)[0])


# ---- pair_scale_correction -----------------------------------------------------------------------------------------------------------------

def _pair_scale_copies(n0):
    from nvalchemiops import _capi as C

    blocks = int(C.lib().mi_pair_scale_blocks())
    k = _copies(n0, blocks)
    assert k * n0 > 256 * blocks and (k * n0) % 64 != 0
    return k


def _tiled_scaled_lists(f, fmt, k, shifts):
    """The lists of `test_pair_scale_gpu._lists` (matrix: all three kinds of padding, NaN scales on the padding) repeated blockwise, the scales
    and the shifts tiled alike."""
    if fmt == "matrix":
        return dict(pair_scales=f["snm"].repeat(k, 1), neighbor_matrix=_tile_padded_matrix(f["nm"], k),
                    neighbor_matrix_shifts=f["sh"].repeat(k, 1, 1).contiguous() if shifts else None, mask_value=k * f["n"])
    lst, ptr, lsh = _tile_csr(f["nl"], f["ptr"], f["lsh"] if shifts else None, k)
    return dict(pair_scales=f["scsr"].repeat(k), neighbor_list=lst, neighbor_ptr=ptr, neighbor_shifts=lsh)


def _tiled_atoms(args, k):
    return [a.repeat((k,) + (1,) * (a.dim() - 1)) for a in args]


@pytest.mark.parametrize("fmt", ["matrix", "list"])
def test_pair_scale_copies_as_one_system_and_as_a_batch(fmt):
    """Explicit shifts (the `MIN = false` kernels and `ps_fold_kernel`): the 24-atom triclinic box of tests/pair_scale_cases.py, every flag."""
    fn, f = TPS._fn(), TPS._case("periodic")
    n0 = f["n"]
    k = _pair_scale_copies(n0)
    args, cell, ref = TPS._inputs(f), TPS._cells(f), TPS._reference("periodic")
    small = fn(*args, cell=cell, **TPS._kw(f, fmt), **TPS.ALL)
    for name, o in zip(TPS.NAMES, small):
        TPS._close(o, ref[name], f"fold sizes pair scale {fmt}: the small call, {name}", 1e-11)
    big_args, big = _tiled_atoms(args, k), _tiled_scaled_lists(f, fmt, k, True)
    one = fn(*big_args, cell=cell, **big, **TPS.ALL)
    bi = torch.arange(k, device=DEV, dtype=torch.int32).repeat_interleave(n0)
    many = [(tag, fn(*big_args, cell=cells, batch_idx=bi, **big, **TPS.ALL))
            for tag, cells in (("", cell.repeat(k, 1, 1).contiguous()), (" (stride-0 cell)", cell[:1].expand(k, 3, 3)))]
    _check_copies(f"pair scale {fmt}", small, one, many, k, per_atom=(0, 1, 2, 3, 4), vir=5)


@pytest.mark.parametrize("fmt", ["matrix", "list"])
def test_pair_scale_minimum_image_copies_as_one_system_and_as_a_batch(fmt):
    """`minimum_image=True` on a list without shifts (the `MIN = true` kernels): the three wrapped molecules of tests/pair_scale_cases.py,
    their batch of three cells tiled to 3 K systems (the cells repeated; 3 K stays below the 65 535 of the grid), and the 9-atom chain alone
    in its cell as one system of K copies."""
    fn, f = TPS._fn(), TPS._case("molecules")
    args, cells, ref = TPS._inputs(f), TPS._cells(f), TPS._reference("molecules")
    # (b) the batch of three systems, K times
    n0 = f["n"]
    k = _pair_scale_copies(n0)
    assert 3 * k <= 65535
    small = fn(*args, cell=cells, batch_idx=f["bi"], minimum_image=True, **TPS._kw(f, fmt, shifts=False), **TPS.ALL)
    for name, o in zip(TPS.NAMES, small):
        TPS._close(o, ref[name], f"fold sizes pair scale minimum image {fmt}: the small batch, {name}", 1e-11)
    bi = (3 * torch.arange(k, device=DEV, dtype=torch.int32)[:, None] + f["bi"][None, :].to(torch.int32)).reshape(-1).contiguous()
    many = fn(*_tiled_atoms(args, k), cell=cells.repeat(k, 1, 1).contiguous(), batch_idx=bi, minimum_image=True,
              **_tiled_scaled_lists(f, fmt, k, False), **TPS.ALL)
    for i in range(5):
        _bitwise(many[i], small[i], k, f"pair scale minimum image {fmt} batch, output {i}")
    assert many[5].shape[0] == 3 * k
    _fold_close(many[5], small[5].repeat(k, 1, 1), small[5], f"pair scale minimum image {fmt} batch of {3 * k}, virial")
    # (a) the chain alone in its cell: one system of K copies
    p = f["problem"]
    sel = p["entries"][0] < 9
    assert bool((p["entries"][1][sel] < 9).all())
    c = TPS._lists(tuple(e[sel] for e in p["entries"]), p["scales"][sel.numpy()], 9, True)
    k = _pair_scale_copies(9)
    chain, cell = [a[:9].contiguous() for a in args], cells[:1].contiguous()
    small = fn(*chain, cell=cell, minimum_image=True, **TPS._kw(c, fmt, shifts=False), **TPS.ALL)
    ref = PR.evaluate(*chain, c["s"], c["ent"], cell=cell, minimum_image=True)
    for name, o in zip(TPS.NAMES, small):
        TPS._close(o, ref[name], f"fold sizes pair scale minimum image {fmt}: the chain, {name}", 1e-11)
    one = fn(*_tiled_atoms(chain, k), cell=cell, minimum_image=True, **_tiled_scaled_lists(c, fmt, k, False), **TPS.ALL)
    _check_copies(f"pair scale minimum image {fmt}", small, one, [], k, per_atom=(0, 1, 2, 3, 4), vir=5)


# ---- rotate_multipoles / multipole_frame_forces --------------------------------------------------------------------------------------------

def test_local_frames_copies_as_one_system_and_as_a_batch():
    """The "triclinic" case of tests/test_local_frames_gpu.py (every kind, wrapped positions, molecules that straddle faces); `LocalFrames` is
    built from the tiled tables (indices + k n0, a -1 slot stays -1).  Dipoles, quadrupoles, torque forces and both local gradients bit for
    bit, the virial term of `fr_fold_kernel` at the fold bar."""
    from nvalchemiops import _capi as C

    LocalFrames, rotate, frame_forces = TLF._api()
    c = TLF._case("triclinic")
    n0, blocks = c["n"], int(C.lib().mi_frame_blocks())
    k = _copies(n0, blocks)
    n = k * n0
    assert n > 256 * blocks and n % 64 != 0
    small = TLF._check_all("triclinic", F64)  # (forces, local_dipole_grads, local_quadrupole_grads, virial), judged against the reference
    d = TLF._device_inputs(c, F64)
    small = tuple(rotate(d["pos"], d["mu"], d["quad"], d["frames"], d["cell"])) + tuple(small)
    P, MU, QD, WMU, WQ = _tiled_atoms([d[x] for x in ("pos", "mu", "quad", "w_mu", "w_q")], k)
    off = (torch.arange(k, dtype=torch.int32) * n0)[:, None, None]
    atoms = torch.where(c["atoms"][None] >= 0, c["atoms"][None] + off, c["atoms"][None]).reshape(n, 3).to(DEV)
    kinds = c["kinds"].repeat(k).to(DEV)
    assert int(atoms.min()) == -1 and int(atoms.max()) < n

    def run(frames, cell, bi):
        out = frame_forces(P, MU, QD, frames, WMU, WQ, cell, batch_idx=bi, compute_local_gradients=True, compute_virial=True)
        return tuple(rotate(P, MU, QD, frames, cell, batch_idx=bi)) + tuple(out)

    one = run(LocalFrames(atoms, kinds), d["cell"], None)
    bi = torch.arange(k, device=DEV, dtype=torch.int32).repeat_interleave(n0)
    frames = LocalFrames(atoms, kinds, batch_idx=bi)
    many = [(tag, run(frames, cells, bi))
            for tag, cells in (("", d["cell"][None].repeat(k, 1, 1).contiguous()), (" (stride-0 cell)", d["cell"][None].expand(k, 3, 3)))]
    _check_copies("local frames", small, one, many, k, per_atom=(0, 1, 2, 3, 4), vir=5)


# ---- coulomb_dipole_correction / coulomb_quadrupole_correction as periodic cut-off sums ---------------------------------------------------------

CLUSTER_FOLD_CUTOFF = 7.0


@functools.lru_cache(maxsize=None)
def _cluster_periodic_case():
    """The periodic problem of tests/cluster_multipole_reference.py (96 atoms, cutoff 9.0, rows of about 290 entries) with its list cut to
    the entries within `CLUSTER_FOLD_CUTOFF` plus every self image (i, i, S != 0) it holds: K = 257 copies then store about 3.4 M entries
    where the full list would store 7.2 M.  The shortest lattice vector is 8.87 long, so a plain cutoff that short would hold no self image;
    the cut list is still full (an entry and its mirror have the same length) and rows still hold more than 64 entries."""
    p = CR.periodic_problem()
    i, j, S = p["entries"]
    pos, cell = torch.as_tensor(p["pos"]), torch.as_tensor(p["cell"])
    r = (pos[j] + S.to(F64) @ cell - pos[i]).norm(dim=1)
    keep = (r < CLUSTER_FOLD_CUTOFF) | (i == j)
    i, j, S = i[keep], j[keep], S[keep]
    counts = torch.bincount(i, minlength=p["n"])
    assert int(counts.min()) > 64 and bool((counts % 64 != 0).any()) and bool(((i == j) & (S != 0).any(-1)).any())
    f = TCM._lists(i, j, S, p["n"], True)
    f.update(cells=p["cell"][None], **{x: p[x] for x in ("pos", "q", "mu", "Q")})
    return f


@pytest.mark.parametrize("fmt", ["matrix", "list"])
@pytest.mark.parametrize("which", ["dipole", "quadrupole"])
def test_cluster_corrections_periodic_copies_as_one_system_and_as_a_batch(which, fmt):
    """`mi_coulomb_dipole` / `mi_coulomb_quadrupole` launch the shared `dp_fold_kernel` / `qd_fold_kernel` from their own scratch layout; this
    is the second trip of those launches and the first periodic BATCH of the bare kind, every flag."""
    from nvalchemiops import _capi as C

    fn, f = TCM._api(which), _cluster_periodic_case()
    n0, blocks = f["n"], int(getattr(C.lib(), f"mi_coulomb_{which}_blocks")())
    k = _copies(n0, blocks)
    n = k * n0
    assert n > 256 * blocks and n % 64 != 0 and k * f["nl"].shape[1] <= 4_200_000
    args, cell = [TCM._t(f[x]) for x in TCM.INPUTS[which]], TCM._t(f["cells"])
    small = fn(*args, cell, **TCM._kw(f, fmt), **TCM.ALL[which])
    evaluate = CR.dipole_evaluate if which == "dipole" else CR.quadrupole_evaluate
    ref = evaluate(*args, f["ent"], cell=cell)
    for name, o in zip(TCM.NAMES[which], small):
        TCM._close(o, ref[name], f"fold sizes cluster {which} {fmt}: the small call, {name}", 1e-11)
    if fmt == "matrix":
        big = dict(neighbor_matrix=_tile_padded_matrix(f["nm"], k), neighbor_matrix_shifts=f["sh"].repeat(k, 1, 1).contiguous(), mask_value=n)
    else:
        lst, ptr, lsh = _tile_csr(f["nl"], f["ptr"], f["lsh"], k)
        big = dict(neighbor_list=lst, neighbor_ptr=ptr, neighbor_shifts=lsh)
    big_args = _tiled_atoms(args, k)
    one = fn(*big_args, cell, **big, **TCM.ALL[which])
    bi = torch.arange(k, device=DEV, dtype=torch.int32).repeat_interleave(n0)
    many = [(tag, fn(*big_args, cells, batch_idx=bi, **big, **TCM.ALL[which]))
            for tag, cells in (("", cell.repeat(k, 1, 1).contiguous()), (" (stride-0 cell)", cell[:1].expand(k, 3, 3)))]
    last = len(small) - 1
    _check_copies(f"cluster {which} periodic {fmt}", small, one, many, k, per_atom=tuple(range(last)), vir=last)


# ---- cluster_induced_dipoles ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("damped", [False, True], ids=["undamped", "thole"])
@pytest.mark.parametrize("fmt", ["matrix", "list"])
def test_cluster_induced_dipoles_copies_as_one_system_and_as_a_batch(fmt, damped):
    """K copies of the 150-atom cluster of tests/cluster_multipole_reference.py over its all-pairs list repeated blockwise: the operator is
    block-diagonal with identical blocks, so the exact solution is the small dense solution tiled.  The bound of the induced-dipole fold
    test above with the small block's spectrum; the iteration count is the small call's."""
    from nvalchemiops import _capi as C

    solve = TCM._api()[0]
    f, tol = TCM._solver_case("c150", damped), 1e-10
    n0, blocks = f["n"], int(C.lib().mi_induced_blocks())
    k = _copies(n0, blocks)
    n = k * n0
    assert n > 256 * blocks and n % 64 != 0
    p0, q0, a0, field = TCM._t(f["pos"]), TCM._t(f["q"]), f["polar"], f["field"]
    label = f"cluster induced {'thole' if damped else 'undamped'} {fmt}"
    common = dict(thole=f["thole"], tolerance=tol, return_info=True)
    lists = dict(neighbor_matrix=f["nm"]) if fmt == "matrix" else dict(neighbor_list=f["nl"], neighbor_ptr=f["ptr"])
    out = solve(p0, q0, a0, external_field=field, **common, **lists)
    mu_ref = TCM._check_solution(out, f["H"], f["b"], a0, f["bi"], 1, tol, f"fold sizes {label}: the small call")
    dmu = 10.0 * tol * float(f["b"].norm()) / float(torch.linalg.eigvalsh(f["H"]).min()) + 1e-14
    if fmt == "matrix":
        big = dict(neighbor_matrix=_tile_padded_matrix(f["nm"], k))
    else:
        lst, ptr, _ = _tile_csr(f["nl"], f["ptr"], None, k)
        big = dict(neighbor_list=lst, neighbor_ptr=ptr)
    P, Q, A, F = _tiled_atoms([p0, q0, a0, field], k)
    want = mu_ref.reshape(n0, 3).repeat(k, 1)
    one = solve(P, Q, A, external_field=F, **common, **big)
    err = float((one.dipoles - want).abs().max())
    print(f"[fold] {label} one system of {n} atoms: max|mu - mu_ref| {err:.3e}  bar {math.sqrt(k) * dmu:.3e}  iterations {one.iterations.tolist()} "
          f"(small call {out.iterations.tolist()})")
    assert err <= math.sqrt(k) * dmu and float(one.residual[0]) <= tol
    assert one.iterations.tolist() == out.iterations.tolist()
    bi = torch.arange(k, device=DEV, dtype=torch.int32).repeat_interleave(n0)
    many = solve(P, Q, A, external_field=F, batch_idx=bi, num_systems=k, **common, **big)
    err = (many.dipoles - want).abs().reshape(k, -1).max(1).values
    print(f"[fold] {label} batch of {k}: worst system max|mu - mu_ref| {float(err.max()):.3e}  bar {dmu:.3e}  iterations "
          f"{int(many.iterations.min())} - {int(many.iterations.max())}")
    assert bool((err <= dmu).all()) and bool((many.residual <= tol).all())
    assert many.iterations.tolist() == out.iterations.tolist() * k
    energy = many.polarization_energy
    assert bool(((energy - out.polarization_energy).abs() <= 100.0 * tol * out.polarization_energy.abs() + 1e-14).all())
