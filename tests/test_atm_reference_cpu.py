"""The float64 restatement of DFT-D3 + three-body term (tests/atm_reference.py) earns its role before it judges `dftd3_atm`.

1. Its TWO-BODY half (same coordination numbers and C6 interpolation, pair sum instead of triple sum) equals the CPU oracle `O.dftd3` on
   the small D3 cases of the suite and on a ~100-atom triclinic periodic box at the oracle-golden bar, rtol = atol = 1e-6 -- energy,
   forces, coordination numbers and virial; this also fixes the virial's sign convention for the three-body check.
2. Closed-form three-body cases with constant C6 tables: an equilateral triangle of side d (ang = 11 / (8 d^9)), a collinear equidistant
   triple (distances d, d, 2d: ang = -1 / (4 d^9)).
3. Central finite differences of the restated three-body energy against its autograd forces (free molecule and periodic box), and of
   the energy under a symmetric strain against its virial.
No GPU, no kernel: these pass with or without the feature (they validate the checker)."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import atm_reference as R
from tests import systems as S

FP = dict(a1=0.4, a2=4.0, s8=0.8, k1=16.0, k3=-4.0, s6=1.0)
BAR = dict(rtol=1e-6, atol=1e-6)


def _wide(*args, **kw):
    with O.d3_wide_sums():
        return O.dftd3(*args, **kw)


def _two_body(pos, z, t, list_cutoff, cell=None):
    return R.reference(pos, z, t, FP["a1"], FP["a2"], list_cutoff, s6=FP["s6"], s8=FP["s8"], k1=FP["k1"], k3=FP["k3"], cell=cell, term="two_body")


@pytest.mark.parametrize("pos,z", [
    ([[0, 0, 0], [1.4, 0, 0]], [1, 1]),
    ([[0, 0, 0], [5.8, 0, 0]], [10, 10]),
    ([[0, 0, 0], [2, 0, 0], [-2, 0, 0], [0, 2, 0], [0, -2, 0]], [6, 1, 1, 1, 1]),
    ([[0, 0, 0], [2.4, 0, 0], [0, 7, 0], [2.4, 7, 0]], [1, 17, 1, 17]),
    ([[0, 0, 0], [1.5, 0, 0], [3.0, 0.2, 0]], [8, 0, 1]),  # a padding atom
])
def test_two_body_half_equals_the_oracle_on_small_molecules(pos, z):
    pos = np.array(pos, np.float32)
    z = np.array(z, np.int32)
    t = O.d3_test_tables(17)
    i, j, s = R.enumerate_pairs(pos, None, 50.0)
    nm, _ = R.neighbor_matrix_of(i, j, s, len(pos))
    e, f, cn = _wide(pos, z, t, neighbor_matrix=nm, **FP)
    r = _two_body(pos, z, t, 50.0)
    np.testing.assert_allclose(r["energy"], e, **BAR)
    np.testing.assert_allclose(r["forces"], f, **BAR)
    np.testing.assert_allclose(r["cn"], cn, **BAR)


def test_two_body_half_equals_the_oracle_on_a_triclinic_periodic_box():
    # 100 atoms at condensed-phase distances (jittered lattice, nearest neighbours >= 3 Bohr) in a triclinic cell.  (Uniformly random
    # positions put atoms 0.2 Bohr apart; the oracle's fp32 pair terms then carry more rounding noise than this bar.)
    pos, cell = R.lattice_box((4, 5, 5), seed=3)
    z = np.random.default_rng(1).choice(np.array([1, 6, 8, 17], np.int32), 100)
    t = O.d3_test_tables(17)
    rc = 9.0
    nm, num, sh = O.cell_list(pos, rc, cell, [True] * 3, max_neighbors=400)
    assert int(num.max()) <= 400
    i, j, s = R.enumerate_pairs(pos, cell, rc)
    assert len(i) == int(num.sum()), "the restatement's image enumeration and the oracle's cell list must hold the same pairs"
    e, f, cn, vir = _wide(pos, z, t, neighbor_matrix=nm, neighbor_matrix_shifts=sh, cell=cell, compute_virial=True, **FP)
    r = _two_body(pos, z, t, rc, cell=cell)
    np.testing.assert_allclose(r["energy"], e, **BAR)
    np.testing.assert_allclose(r["forces"], f, **BAR)
    np.testing.assert_allclose(r["cn"], cn, **BAR)
    np.testing.assert_allclose(r["virial"], vir, **BAR)  # same sign, same convention: the three-body virial adds to dftd3's


def _constant_tables(c6=7.0, r4r2=2.5):
    """Tables whose C6 does not depend on the coordination numbers: every reference point of element 1 carries the same C6."""
    t = {k: v.copy() for k, v in O.d3_test_tables(17).items()}
    t["c6ab"][1, 1] = c6
    t["r4r2"][1] = r4r2
    return t


@pytest.mark.parametrize("alpha", [16.0, 14.0])
def test_closed_form_equilateral_and_collinear(alpha):
    c6, r4r2, a1, a2, s9, d = 7.0, 2.5, 0.4, 4.0, 0.9, 5.0
    t = _constant_tables(c6, r4r2)
    r0 = a1 * np.sqrt(3.0 * r4r2 * r4r2) + a2
    c9 = c6 ** 1.5
    z = np.array([1, 1, 1], np.int32)
    tri = np.array([[0, 0, 0], [d, 0, 0], [d / 2, d * np.sqrt(3) / 2, 0]])
    got = R.reference(tri, z, t, a1, a2, 30.0, three_body_cutoff=30.0, s9=s9, alpha=alpha)["energy"][0]
    want = s9 * c9 * 11.0 / (8.0 * d ** 9) / (1.0 + 6.0 * (r0 ** 3 / d ** 3) ** (alpha / 3.0))
    assert want > 0.0
    np.testing.assert_allclose(got, want, rtol=1e-12)
    line = np.array([[0, 0, 0], [d, 0, 0], [2 * d, 0, 0]])
    got = R.reference(line, z, t, a1, a2, 30.0, three_body_cutoff=30.0, s9=s9, alpha=alpha)["energy"][0]
    want = s9 * c9 * (-1.0 / (4.0 * d ** 9)) / (1.0 + 6.0 * (r0 ** 3 / (2.0 * d ** 3)) ** (alpha / 3.0))
    np.testing.assert_allclose(got, want, rtol=1e-12)
    # a side beyond the three-body cutoff: no triple
    assert R.reference(line, z, t, a1, a2, 30.0, three_body_cutoff=1.5 * d, s9=s9, alpha=alpha)["energy"][0] == 0.0


def _atm(pos, z, t, cell, rc3, rcl):
    return R.reference(pos, z, t, 0.4, 4.0, rcl, three_body_cutoff=rc3, cell=cell)


def test_forces_are_the_finite_difference_of_the_energy_free_molecule():
    pos, z, _ = S.molecule(12, density=0.02, min_dist=2.0, seed=5, dtype=np.float64)
    t = O.d3_test_tables(17)
    base = _atm(pos, z, t, None, 9.0, 12.0)
    assert abs(base["energy"][0]) > 0.0
    h = 1e-4
    for atom, d in ((0, 0), (3, 1), (7, 2), (11, 0)):
        p, m = pos.copy(), pos.copy()
        p[atom, d] += h
        m[atom, d] -= h
        fd = -(_atm(p, z, t, None, 9.0, 12.0)["energy"][0] - _atm(m, z, t, None, 9.0, 12.0)["energy"][0]) / (2 * h)
        np.testing.assert_allclose(base["forces"][atom, d], fd, rtol=2e-6, atol=1e-6 * np.abs(base["forces"]).max())
    np.testing.assert_allclose(base["forces"].sum(0), 0.0, atol=1e-12 * len(pos) * np.abs(base["forces"]).max() + 1e-18)


def test_forces_and_virial_are_finite_differences_periodic():
    pos, cell = S.random_box(14, 9.0, seed=11, dtype=np.float64, triclinic=True)
    z = np.random.default_rng(2).choice(np.array([1, 6, 8], np.int32), 14)
    t = O.d3_test_tables(17)
    rc3, rcl = 6.0, 7.0
    base = _atm(pos, z, t, cell, rc3, rcl)
    h = 1e-4
    scale = np.abs(base["forces"]).max()
    for atom, d in ((0, 0), (5, 1), (13, 2)):
        p, m = pos.copy(), pos.copy()
        p[atom, d] += h
        m[atom, d] -= h
        fd = -(_atm(p, z, t, cell, rc3, rcl)["energy"][0] - _atm(m, z, t, cell, rc3, rcl)["energy"][0]) / (2 * h)
        np.testing.assert_allclose(base["forces"][atom, d], fd, rtol=1e-5, atol=1e-5 * scale)
    for a, b in ((0, 0), (0, 1), (2, 2), (1, 2)):
        e = np.zeros((3, 3))
        e[a, b] += 0.5 * h
        e[b, a] += 0.5 * h
        sp, sm = np.eye(3) + e, np.eye(3) - e
        ep = _atm(pos @ sp, z, t, cell @ sp, rc3, rcl)["energy"][0]
        em = _atm(pos @ sm, z, t, cell @ sm, rc3, rcl)["energy"][0]
        want = -(ep - em) / (2 * h)  # virial = -dE/d(strain)
        got = 0.5 * (base["virial"][0][a, b] + base["virial"][0][b, a])
        np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-5 * np.abs(base["virial"]).max())


def test_float32_working_precision_is_close_to_float64():
    """The float32-per-triple evaluation (the kernels' arithmetic model) exists and differs from float64 by float32 rounding only."""
    pos, cell = S.random_box(20, 10.0, seed=4, dtype=np.float32)
    z = np.random.default_rng(3).choice(np.array([1, 6, 8], np.int32), 20)
    t = O.d3_test_tables(17)
    a = R.reference(pos, z, t, 0.4, 4.0, 8.0, three_body_cutoff=4.9, cell=cell)
    b = R.reference(pos, z, t, 0.4, 4.0, 8.0, three_body_cutoff=4.9, cell=cell, work_dtype=torch.float32)
    assert a["energy"][0] != b["energy"][0]
    np.testing.assert_allclose(b["energy"], a["energy"], rtol=1e-4)
    np.testing.assert_allclose(b["forces"], a["forces"], rtol=0, atol=1e-4 * np.abs(a["forces"]).max())
