"""The checker of `dftd3_zero` (tests/d3_zero_reference.py) checked itself, on the CPU: closed form of a dimer, autograd forces against
finite differences of the energy, the virial against finite strain, the limit in which the damping disappears against the restatement the
ATM suite already trusts, a missing pair radius, and a close contact in the float32 mode."""
import numpy as np
import pytest
import torch

from tests import atm_reference as A
from tests import d3_zero_reference as Z
from tests import systems as S

ZERO = dict(rs6=1.217, s8=0.722, rs8=1.0, alpha=14.0)


def _constant_c6_tables(nz=10, c6=37.5):
    t = {k: v.copy() for k, v in S.d3_test_tables(nz - 1).items()}
    t["c6ab"][1:, 1:] = c6  # C6 does not depend on the coordination numbers: the interpolation returns c6 whatever the weights are
    return t


@pytest.mark.parametrize("beta", [0.0, 0.3])
@pytest.mark.parametrize("alpha", [14.0, 13.5])
def test_dimer_against_the_closed_form_in_plain_floats(beta, alpha):
    t = _constant_c6_tables()
    r0ab = Z.synthetic_r0ab(10)
    za, zb, r = 6, 8, 5.3
    rs6, rs8, s6, s8 = 1.217, 0.9, 0.95, 0.722
    pos = np.array([[0.0, 0.0, 0.0], [r, 0.0, 0.0]])
    out = Z.reference(pos, [za, zb], t, r0ab, rs6, s8, 20.0, rs8=rs8, alpha=alpha, beta=beta, s6=s6)
    R0 = float(r0ab[za, zb])
    q = 3.0 * float(t["r4r2"][za]) * float(t["r4r2"][zb])
    c6 = 37.5

    def energy(d):
        f6 = 1.0 / (1.0 + 6.0 * (d / (rs6 * R0) + beta * R0) ** (-alpha))
        f8 = 1.0 / (1.0 + 6.0 * (d / (rs8 * R0) + beta * R0) ** (-(alpha + 2.0)))
        return -c6 * (s6 * f6 / d ** 6 + s8 * q * f8 / d ** 8)  # the two directed pairs, each with its half

    assert out["energy"][0] == pytest.approx(energy(r), rel=1e-13)
    # the derivative in the form the issue states: df/dr = alpha_n f (1 - f) / (r + beta rs_n R0^2)
    f6 = 1.0 / (1.0 + 6.0 * (r / (rs6 * R0) + beta * R0) ** (-alpha))
    f8 = 1.0 / (1.0 + 6.0 * (r / (rs8 * R0) + beta * R0) ** (-(alpha + 2.0)))
    d6 = alpha * f6 * (1.0 - f6) / (r + beta * rs6 * R0 * R0)
    d8 = (alpha + 2.0) * f8 * (1.0 - f8) / (r + beta * rs8 * R0 * R0)
    dEdr = -c6 * (s6 * (d6 / r ** 6 - 6.0 * f6 / r ** 7) + s8 * q * (d8 / r ** 8 - 8.0 * f8 / r ** 9))
    assert out["forces"][1, 0] == pytest.approx(-dEdr, rel=1e-11)
    assert out["forces"][0, 0] == pytest.approx(dEdr, rel=1e-11)
    assert np.abs(out["forces"][:, 1:]).max() == 0.0
    assert energy(r) < 0.0 and abs(f6 - 0.5) < 0.5


def _box12():
    pos, cell = A.lattice_box((2, 2, 3), a=4.4, jitter=0.3, seed=5, triclinic=True, dtype=np.float64)
    z = np.random.default_rng(5).choice(np.array([1, 6, 8, 17], np.int32), len(pos))
    return pos, cell, z


@pytest.mark.parametrize("beta,s5", [(0.0, None), (0.3, (5.0, 8.5))])
def test_forces_and_virial_against_finite_differences(beta, s5):
    pos, cell, z = _box12()
    assert len(pos) == 12
    t = S.d3_test_tables(17)
    r0ab = Z.synthetic_r0ab(18)
    kw = dict(beta=beta, **ZERO)
    if s5:
        kw.update(s5_on=s5[0], s5_off=s5[1])
    rc = 9.0
    out = Z.reference(pos, z, t, r0ab, list_cutoff=rc, cell=cell, **kw)
    E = lambda p, c: Z.reference(p, z, t, r0ab, list_cutoff=rc, cell=c, **kw)["energy"][0]  # noqa: E731
    h = 1e-5
    for atom, comp in ((0, 0), (5, 1), (11, 2), (7, 0)):
        p1, p2 = pos.copy(), pos.copy()
        p1[atom, comp] += h
        p2[atom, comp] -= h
        fd = -(E(p1, cell) - E(p2, cell)) / (2 * h)
        assert out["forces"][atom, comp] == pytest.approx(fd, rel=2e-6, abs=1e-10)
    # (the list changes when a pair crosses rc under the displacement; with no switch the pair energy at rc = 9 is ~1e-6 of the total and the
    #  chosen atoms have no pair within 1e-5 of the cutoff -- checked here)
    i, j, s = A.enumerate_pairs(pos, cell, rc + 1e-3)
    d = np.linalg.norm(pos[j] + s @ cell - pos[i], axis=1)
    assert np.abs(d - rc).min() > 5e-5
    for a, b in ((0, 0), (0, 1), (1, 2), (2, 2)):
        eps = np.zeros((3, 3))
        eps[a, b] += 0.5 * h
        eps[b, a] += 0.5 * h
        sp, sm = np.eye(3) + eps, np.eye(3) - eps
        fd = -(E(pos @ sp, cell @ sp) - E(pos @ sm, cell @ sm)) / (2 * h)
        assert out["virial"][0, a, b] == pytest.approx(fd, rel=2e-6, abs=1e-10)
        assert out["virial"][0, a, b] == out["virial"][0, b, a]
    assert np.abs(out["forces"].sum(0)).max() < 1e-12


def test_limit_without_damping_equals_the_trusted_restatement():
    """rs6 = rs8 = 1e-6, beta = 0: x ~ 1e6 r / R0, 6 x^-14 < 1e-70, every f_n is 1 to float64 rounding -- the undamped -C6 (s6 / r^6 +
    s8 q / r^8), which is what the BJ restatement gives with a1 = a2 = 0 (R0 = 0)."""
    pos, cell, z = _box12()
    t = S.d3_test_tables(17)
    r0ab = Z.synthetic_r0ab(18)
    got = Z.reference(pos, z, t, r0ab, 1e-6, 0.722, 9.0, rs8=1e-6, beta=0.0, s6=0.9, cell=cell)
    want = A.reference(pos, z, t, 0.0, 0.0, 9.0, s6=0.9, s8=0.722, cell=cell, term="two_body")
    for k in ("energy", "forces", "virial", "cn"):
        assert np.abs(got[k] - want[k]).max() <= 1e-13 * np.abs(want[k]).max(), k
    assert abs(want["energy"][0]) > 1e-3


def test_pair_without_radius_contributes_nothing():
    pos, _, _ = S.molecule(9, density=0.02, min_dist=2.0, seed=3)
    z = np.array([6, 8, 6, 8, 6, 8, 6, 8, 6], np.int32)
    t = _constant_c6_tables(18)  # constant C6: removing a pair's energy does not change any other pair's
    r0ab = Z.synthetic_r0ab(18)
    full = Z.reference(pos, z, t, r0ab, list_cutoff=30.0, **ZERO)
    cut = r0ab.copy()
    cut[6, 8] = cut[8, 6] = 0.0
    part = Z.reference(pos, z, t, cut, list_cutoff=30.0, **ZERO)
    only = {6: Z.reference(pos[z == 6], z[z == 6], t, r0ab, list_cutoff=30.0, **ZERO), 8: Z.reference(pos[z == 8], z[z == 8], t, r0ab, list_cutoff=30.0, **ZERO)}
    assert part["energy"][0] == pytest.approx(only[6]["energy"][0] + only[8]["energy"][0], rel=1e-13)
    assert np.allclose(part["forces"][z == 6], only[6]["forces"], rtol=1e-12, atol=1e-18)
    assert abs(full["energy"][0]) > abs(part["energy"][0]) > 0.0
    np.testing.assert_array_equal(part["cn"], full["cn"])  # the coordination numbers do not know about the radii
    neg = r0ab.copy()
    neg[6, 8] = neg[8, 6] = -1.0
    again = Z.reference(pos, z, t, neg, list_cutoff=30.0, **ZERO)
    assert again["energy"][0] == part["energy"][0] and np.array_equal(again["forces"], part["forces"])
    # a molecule of ONLY such pairs: exact zeros
    none = Z.reference(pos[:2], z[:2], t, cut, list_cutoff=30.0, **ZERO)
    assert none["energy"][0] == 0.0 and np.abs(none["forces"]).max() == 0.0


@pytest.mark.parametrize("alpha", [14.0, 13.5])
def test_close_contact_is_finite_in_the_float32_mode(alpha):
    """(R0 / 0.01)^16 overflows float32: f becomes 0, and the pair must contribute zeros, not 0 x inf."""
    pos, cell, z = _box12()
    pos = pos.copy()
    pos[3] = pos[2] + np.array([0.01, 0.0, 0.0])
    t = S.d3_test_tables(17)
    r0ab = Z.synthetic_r0ab(18)
    kw = dict(ZERO, alpha=alpha)
    r32 = Z.reference(pos, z, t, r0ab, list_cutoff=9.0, cell=cell, work_dtype=torch.float32, **kw)
    r64 = Z.reference(pos, z, t, r0ab, list_cutoff=9.0, cell=cell, **kw)
    for k in ("energy", "forces", "virial", "cn"):
        assert np.isfinite(r32[k]).all() and np.isfinite(r64[k]).all(), k
    # away from the contact the two modes agree as on any other system
    far = np.ones(len(pos), bool)
    far[[2, 3]] = False
    assert np.abs(r32["forces"][far] - r64["forces"][far]).max() <= 1e-5 * np.abs(r64["forces"][far]).max()


# ---- the three-body term with table radii ----------------------------------------------------------------------------------------------

def test_atm_trimer_against_the_closed_form_in_plain_floats():
    t = _constant_c6_tables()
    r0ab = Z.synthetic_r0ab(10)
    zs = [6, 8, 7]
    pos = np.array([[0.0, 0.0, 0.0], [4.1, 0.3, 0.0], [1.2, 3.7, 0.5]])
    rs9, s9, alpha = 4.0 / 3.0, 0.9, 16.0
    out = Z.reference(pos, zs, t, r0ab, None, None, 30.0, three_body_cutoff=30.0, rs9=rs9, s9=s9, alpha=alpha, term="atm")
    d = lambda i, j: float(np.linalg.norm(pos[i] - pos[j]))  # noqa: E731
    rab, rac, rbc = d(0, 1), d(0, 2), d(1, 2)
    a, b, c = rab ** 2, rac ** 2, rbc ** 2
    P = rab * rac * rbc
    ang = 0.375 * (a + b - c) * (a + c - b) * (b + c - a) / P ** 5 + 1.0 / P ** 3
    R = rs9 ** 3 * float(r0ab[6, 8]) * float(r0ab[6, 7]) * float(r0ab[8, 7])
    want = s9 * 37.5 ** 1.5 * ang / (1.0 + 6.0 * (R / P) ** (alpha / 3.0))
    assert out["energy"][0] == pytest.approx(want, rel=1e-13)
    assert np.abs(out["forces"].sum(0)).max() < 1e-15


def test_atm_forces_and_virial_against_finite_differences():
    pos, cell, z = _box12()
    t = S.d3_test_tables(17)
    r0ab = Z.synthetic_r0ab(18)
    kw = dict(three_body_cutoff=7.0, cell=None, term="atm")
    ref = lambda p, c: Z.reference(p, z, t, r0ab, None, None, 9.0, **dict(kw, cell=c))  # noqa: E731
    out = ref(pos, cell)
    h = 1e-5
    for atom, comp in ((0, 0), (5, 1), (11, 2)):
        p1, p2 = pos.copy(), pos.copy()
        p1[atom, comp] += h
        p2[atom, comp] -= h
        fd = -(ref(p1, cell)["energy"][0] - ref(p2, cell)["energy"][0]) / (2 * h)
        assert out["forces"][atom, comp] == pytest.approx(fd, rel=2e-6, abs=1e-11)
    for a, b in ((0, 0), (1, 2)):
        eps = np.zeros((3, 3))
        eps[a, b] += 0.5 * h
        eps[b, a] += 0.5 * h
        sp, sm = np.eye(3) + eps, np.eye(3) - eps
        fd = -(ref(pos @ sp, cell @ sp)["energy"][0] - ref(pos @ sm, cell @ sm)["energy"][0]) / (2 * h)
        assert out["virial"][0, a, b] == pytest.approx(fd, rel=2e-6, abs=1e-11)


def test_atm_with_factorising_radii_equals_the_trusted_restatement():
    """A table of the BJ form, r0ab[X, Y] = (a1 sqrt(3 r4r2_X r4r2_Y) + a2) / rs9, must give exactly what tests/atm_reference.py gives."""
    pos, cell, z = _box12()
    t = S.d3_test_tables(17)
    a1, a2, rs9 = 0.4, 4.0, 4.0 / 3.0
    r4 = t["r4r2"].astype(np.float64)
    r0ab = (a1 * np.sqrt(3.0 * r4[:, None] * r4[None, :]) + a2) / rs9
    r0ab[0, :] = r0ab[:, 0] = 0.0
    got = Z.reference(pos, z, t, r0ab, None, None, 9.0, three_body_cutoff=7.0, cell=cell, term="atm", alpha=14.0, s9=0.8)
    want = A.reference(pos, z, t, a1, a2, 9.0, three_body_cutoff=7.0, cell=cell, term="atm", alpha=14.0, s9=0.8)
    for k in ("energy", "forces", "virial", "cn"):
        assert np.abs(got[k] - want[k]).max() <= 1e-12 * np.abs(want[k]).max(), k
    assert abs(want["energy"][0]) > 0.0


def test_atm_pair_without_radius_takes_its_triples_out():
    pos, _, _ = S.molecule(8, density=0.02, min_dist=2.0, seed=3)
    z = np.array([6, 8, 6, 8, 6, 8, 6, 6], np.int32)
    t = _constant_c6_tables(18)
    r0ab = Z.synthetic_r0ab(18)
    cut = r0ab.copy()
    cut[6, 8] = cut[8, 6] = 0.0
    part = Z.reference(pos, z, t, cut, None, None, 30.0, three_body_cutoff=30.0, term="atm")
    only6 = Z.reference(pos[z == 6], z[z == 6], t, r0ab, None, None, 30.0, three_body_cutoff=30.0, term="atm")
    only8 = Z.reference(pos[z == 8], z[z == 8], t, r0ab, None, None, 30.0, three_body_cutoff=30.0, term="atm")
    # constant C6: what is left are the triples of one species only
    assert part["energy"][0] == pytest.approx(only6["energy"][0] + only8["energy"][0], rel=1e-12)
    assert abs(only6["energy"][0]) > 0.0
