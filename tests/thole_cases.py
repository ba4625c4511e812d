"""The systems the Thole tests share beside the lattices of tests/induced_cases.py, and the dense damped problem built from them.

two_atoms: the case of `test_breakdown_is_reported` in tests/test_induced_gpu.py -- two atoms at distance d = 1.5 with a = d^3 in a cubic box of
edge 8, alpha 0.45, every image within 7, k_cutoff 3.  Its undamped H has a negative eigenvalue; damped at a_T = 0.39 it has none.

large-a lattices: the polarisabilities of an induced_cases lattice times LARGE_A[name].  The scale was chosen on the CPU from 1, 4, 6, 8, 10,
12 as the smallest at which the undamped dense H is indefinite (the damped H stays positive definite up to 12 at least);
tests/test_thole_reference_cpu.py asserts both properties and has the measured eigenvalues in its header."""
import functools

import numpy as np
import torch

from tests import induced_cases as IC
from tests import induced_reference as IR
from tests import thole_reference as TR
from tests.gaussian_reference import brute_force_entries

F64 = torch.float64
THOLE = 0.39
LARGE_A = {"l27": 4.0}


@functools.lru_cache(maxsize=None)
def two_atoms():
    d = 1.5
    cell = np.eye(3) * 8.0
    pos = np.array([[3.0, 4.0, 4.0], [3.0 + d, 4.0, 4.0]])
    return dict(n=2, pos=pos, cell=cell, q=np.zeros(2), polar=np.full(2, d**3), alpha=0.45, entries=brute_force_entries(pos, cell, 7.0, 1),
                k_cutoff=3.0)


@functools.lru_cache(maxsize=None)
def lone_atom():
    """One atom in a triclinic box of edge 6 whose list holds only its own images (cutoff 11, three shells): the third system of the batch."""
    cell = IC.triclinic(6.0)
    pos = np.array([[1.0, 2.0, 3.0]])
    return dict(n=1, pos=pos, cell=cell, q=np.array([0.7]), polar=np.array([0.8]), alpha=0.5, entries=brute_force_entries(pos, cell, 11.0, 3),
                k_cutoff=3.2)


@functools.lru_cache(maxsize=None)
def lattice(name, large=False):
    """An induced_cases lattice as a case dict; `large`: polarisabilities times LARGE_A[name]."""
    c = IC.lattice(name)
    return dict(n=c["n"], pos=c["pos"], cell=c["cell"], q=c["q"], polar=c["polar"] * (LARGE_A[name] if large else 1.0), alpha=IC.EWALD["alpha"],
                entries=IC.entries(name), k_cutoff=IC.EWALD["k_cutoff"])


FOLD_CUTOFF = 6.0


@functools.lru_cache(maxsize=None)
def fold_case(name="l27"):
    """The lattice the fold-size tests of the solvers tile (tests/test_fold_sizes_gpu.py): list cutoff `FOLD_CUTOFF` (29 - 36 entries per
    row, so that the stored operator of 911 copies stays small) and an EMPTY k set (`k_cutoff=None`): of the reciprocal term only the self
    term -(2 alpha^3 / 3 sqrt(pi)) |mu|^2 is left, which does not couple the copies.  tests/test_induced_reference_cpu.py asserts that this
    truncated H is positive definite, undamped and damped."""
    c = IC.lattice(name)
    return dict(n=c["n"], pos=c["pos"], cell=c["cell"], q=c["q"], polar=c["polar"], alpha=IC.EWALD["alpha"],
                entries=IC.entries(name, FOLD_CUTOFF, 1), k_cutoff=None)


def dense(case, thole, device="cpu", field=None):
    """dict(T, c, H, b, polar) of a case on `device`: the undamped operator for `thole=None`, E_dip + E_thole otherwise.  A case with
    `k_cutoff=None` has an empty k set [0, 3]."""
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=F64, device=device)  # noqa: E731
    pos, q, polar, cell = t(case["pos"]), t(case["q"]), t(case["polar"]), t(case["cell"])
    ent = tuple(e.to(device) for e in case["entries"])
    kv = torch.zeros((0, 3), dtype=F64, device=device) if case["k_cutoff"] is None else IC.k_vectors(case["cell"], case["k_cutoff"]).to(device)
    if thole is None:
        T, c = IR.dipole_operator(pos, q, cell, case["alpha"], ent, kv)
    else:
        T, c = TR.damped_operator(pos, q, polar, cell, case["alpha"], thole, ent, kv)
    return dict(T=T, c=c, polar=polar, H=IR.system_matrix(T, polar), b=IR.right_hand_side(c, polar, field), kv=kv, ent=ent)
