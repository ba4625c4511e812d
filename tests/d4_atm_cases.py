"""The systems tests/test_d4_atm_gpu.py compares against the restatement tests/d4_atm_reference.py: the positions, species and tables of
tests/d4_cases.py, each with a `three_body_cutoff` (rc3) and an `s9`, plus one dense cluster.  The CPU suite checks the conditions the
cases must meet (tests/test_d4_atm_reference_cpu.py); every reference is computed once and never modified.

    case(name) -> dict(pos, z, tables, cell, batch_idx, rc (list cutoff), rc3, s9, kw (model arguments of `dftd4_atm` / `reference`))
    references(name) -> (float64 restatement, the same with float32 per-pair / per-atom / per-triple arithmetic) at the case's s9
    unit_references(name) -> the same two at s9 = 1 (the term is linear in s9: `references` scales these)

The three-body term is small and the bars carry `dftd3`'s absolute 1e-6, so at s9 = 1 most small systems would be compared against
nothing.  Each parity case therefore fixes its s9 as the SMALLEST POWER OF TEN for which max|ref| >= 500 x the bar the GPU comparison
applies -- 4 x `dftd3`'s bar -- for the energy, the forces and (periodic) the virial, computed from the restatement alone (`smallest_s9`).
That reading of "500 x bar" reproduces the values the feature request lists (molecule24, molecule70, species_slots_plus_1: 1; padding: 10;
molecule7, triclinic_f32: 100; self_images: 1e3; molecule3: 1e4) with one exception: cn_cutoff, listed at 100, where the rule gives 10
(max|F| = 2.16e-3 against 2.02e-3 needed); the listed value is kept there (`ABOVE_RULE`).  The CPU suite asserts the rule, and that the
float32 deviation of the restatement scaled by the same s9 stays below `dftd3`'s bar (tests/test_d4_atm_reference_cpu.py).
"""
import functools

import numpy as np
import torch

from tests import d4_atm_reference as R3
from tests import d4_cases as K

BJ = dict(a1=0.4, a2=4.0)
EXTRA = {"energy": 0.0, "forces": 5e-6, "virial": 2e-7}  # `dftd3`'s bars: rtol = atol = 1e-6, + this x max|ref| (tests/test_d3_gpu.py)
RC3 = {
    "molecule1": 11.0, "molecule2": 11.0, "molecule3": 11.0, "molecule7": 11.0, "molecule24": 11.0, "molecule70": 20.0, "padding": 11.0,
    "no_references": 11.0, "species_slots": 10.0, "species_slots_plus_1": 10.0, "species_20": 10.0, "triclinic_f32": 7.0, "triclinic_f64": 7.0,
    "self_images": 7.0, "cn_cutoff": 7.0, "d3_limit": 7.0, "batch": 6.0, "dense": 20.0,
}
# `smallest_s9` of every case, written out (asserted by the CPU suite); 1 for the zero cases
S9 = {
    "molecule1": 1.0, "molecule2": 1.0, "molecule3": 1e4, "molecule7": 100.0, "molecule24": 1.0, "molecule70": 1.0, "padding": 10.0,
    "no_references": 100.0, "species_slots": 1.0, "species_slots_plus_1": 1.0, "species_20": 1.0, "triclinic_f32": 100.0, "triclinic_f64": 100.0,
    "self_images": 1e3, "cn_cutoff": 100.0, "d3_limit": 100.0, "batch": 100.0, "dense": 1.0,
}
ABOVE_RULE = {"cn_cutoff": 10.0}  # the feature request's value, this factor above the rule's
ZERO = ("molecule1", "molecule2")  # fewer than three atoms: every output is exactly 0
PARITY = tuple(n for n in RC3 if n not in ZERO)
NAMES = tuple(RC3)
# one row of three LDS tiles (`_shell`), judged by a test of its own; s9 by the rule above
RC3["shell"], S9["shell"] = 20.0, 1.0


def dense_atoms():
    """Atoms of the dense cluster: 24 more than one LDS tile of the triple pass holds, so that the central rows stage two tiles."""
    from nvalchemiops.interactions.dispersion.dftd4 import atm_tile

    return atm_tile() + 24


def _dense():
    """A free cluster cut from a jittered lattice (the system of tests/test_d3_atm_gpu.py::test_dense_row_needs_more_than_one_lds_tile at
    this tile size): the list holds everybody, the rows of the central atoms keep every other atom inside rc3, corner rows fewer."""
    n = dense_atoms()
    pos, _ = K.A.lattice_box((7, 7, 8), a=3.4, jitter=0.2, seed=13, triclinic=False)
    pos = pos[:n]
    z = np.random.default_rng(13).choice(np.array((1, 6, 8), np.int32), n)
    rc = 2.0 * float(np.linalg.norm(pos.max(0) - pos.min(0)))
    return dict(pos=pos, z=z, tables=K.R.d4_test_tables(17), cell=None, batch_idx=None, rc=rc, kw={})


def _shell():
    """A centre atom and a shell of 2 tiles + 8 atoms at 19 Bohr (`atm_reference.centre_and_shell`): the centre's row stages three tiles,
    every other row less than one; the list (cutoff 40) holds everybody."""
    from nvalchemiops.interactions.dispersion.dftd4 import atm_tile

    pos = K.A.centre_and_shell(2 * atm_tile() + 8)
    z = np.random.default_rng(29).choice(np.array((1, 6, 8), np.int32), len(pos))
    return dict(pos=pos, z=z, tables=K.R.d4_test_tables(17), cell=None, batch_idx=None, rc=40.0, kw={})


@functools.lru_cache(maxsize=None)
def case(name):
    c = dict(_dense() if name == "dense" else _shell() if name == "shell" else K.case(name))
    c.pop("q", None)  # the three-body term takes no charges
    c["rc3"], c["s9"] = RC3[name], S9[name]
    return c


@functools.lru_cache(maxsize=None)
def unit_references(name):
    c = case(name)
    kw = dict(three_body_cutoff=c["rc3"], s9=1.0, cell=c["cell"], batch_idx=c["batch_idx"], **c["kw"])
    r64 = R3.reference(c["pos"], c["z"], c["tables"], BJ["a1"], BJ["a2"], c["rc"], **kw)
    r32 = R3.reference(c["pos"], c["z"], c["tables"], BJ["a1"], BJ["a2"], c["rc"], work_dtype=torch.float32, **kw)
    return r64, r32


def _scaled(r, s9):
    out = {k: v for k, v in r.items() if k != "topology"}
    for k in ("energy", "forces", "virial"):
        if r[k] is not None:
            out[k] = r[k] * s9
    return out


@functools.lru_cache(maxsize=None)
def references(name):
    r64, r32 = unit_references(name)
    s9 = case(name)["s9"]
    return _scaled(r64, s9), _scaled(r32, s9)


def d3_bar(ref, key):
    """`dftd3`'s elementwise bar for a quantity with reference values `ref`."""
    return 1e-6 + 1e-6 * np.abs(ref) + EXTRA[key] * (np.abs(ref).max() if ref.size else 0.0)


def lifted(r64, s9):
    """True if at this s9 the largest component of energy, forces and (periodic) virial is at least 500 x the bar the GPU comparison
    applies to it (4 x `dftd3`'s)."""
    for k in ("energy", "forces", "virial"):
        if r64[k] is None:
            continue
        top = np.abs(r64[k]).max() * s9
        if not top >= 500.0 * 4.0 * (1e-6 + 1e-6 * top + EXTRA[k] * top):
            return False
    return True


def smallest_s9(name):
    """The rule: the smallest power of ten (from 1 upwards) that lifts the case, from the restatement at s9 = 1."""
    r64, _ = unit_references(name)
    s9 = 1.0
    while not lifted(r64, s9):
        s9 *= 10.0
        assert s9 <= 1e12, name
    return s9
