"""The float64 reference of the point-dipole Ewald term (tests/dipole_reference.py) earns its role as the checker of the HIP kernels: with
converged sums the charge Ewald energy plus this term does not depend on alpha, it is the d -> 0 limit of +-|mu|/d charge pairs, its
derivative outputs match finite differences, and zero dipoles give zero.  CPU only."""
import math

import numpy as np
import torch

from tests import dipole_reference as R

F64 = torch.float64
CELL = np.array([[6.0, 0, 0], [1.2, 5.4, 0], [0.6, -0.9, 6.6]])


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=F64)


def _box(n=6, seed=1):
    """n <= 8 atoms on the jittered sites of a 2 x 2 x 2 sublattice: no pair closer than 2 A (the bond-length scale), because the d^4 term that
    Richardson extrapolation leaves behind in the finite-pair test grows as mu^2 / r_min^7."""
    g = np.random.default_rng(seed)
    sites = np.array([(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)], dtype=float)[g.permutation(8)[:n]]
    pos = (0.5 * sites + 0.25 + g.uniform(-0.06, 0.06, (n, 3))) @ CELL
    q = g.normal(size=n) + 0.2  # a charged cell
    mu = 0.3 * g.normal(size=(n, 3))
    mu[1] = 0.0
    return pos, q, mu


def _k_vectors(k_cutoff):
    from nvalchemiops.interactions.electrostatics.k_vectors import generate_k_vectors_ewald_summation

    return generate_k_vectors_ewald_summation(_t(CELL), k_cutoff)


def _converged(alpha):
    """(real-space cutoff, k cutoff) beyond which every term is below 1e-18 of the leading ones: alpha r = 6.6 and k / (2 alpha) = 6.6."""
    return 6.6 / alpha, 13.2 * alpha


def _total(pos, q, mu, alpha):
    """Charge Ewald + dipole term of one box, both with sums converged for this alpha."""
    rc, kc = _converged(alpha)
    i, j, S = R.brute_force_entries(pos, CELL, rc, int(math.ceil(rc / 5.0)) + 1)
    k = _k_vectors(kc)
    P, Q, M, C = _t(pos), _t(q), _t(mu), _t(CELL)
    cc = float(R.charge_ewald_total(P, Q, C, alpha, i, j, S, k))
    dd = float(R.energies(P, Q, M, C, alpha, (i, j, S), k).sum().detach())
    return cc, dd


def test_charge_ewald_plus_dipole_term_is_independent_of_alpha():
    pos, q, mu = _box()
    (c1, d1), (c2, d2) = _total(pos, q, mu, 0.5), _total(pos, q, mu, 0.65)
    print(f"alpha 0.50: {c1 + d1:.15e} (dipole term {d1:.6e})   alpha 0.65: {c2 + d2:.15e} (dipole term {d2:.6e})")
    assert abs((c1 + d1) - (c2 + d2)) <= 1e-12 * abs(c1 + d1)
    assert abs(d1 - d2) <= 1e-12 * abs(c1 + d1)  # ... and so is the dipole term alone: the real / reciprocal split moves, the sum does not


def test_limit_of_finite_charge_pairs_with_richardson_extrapolation():
    """mu_i -> charges +-|mu_i|/d at r_i +- (d/2) mu_i/|mu_i|.  The charge Ewald energy of that system minus the direct interaction inside each
    pair, -(|mu|/d)^2 / d, tends to charge Ewald + dipole term with an O(d^2) error: the error ratio between d and d/2 is 4."""
    pos, q, mu = _box()
    alpha = 0.55
    cc, dd = _total(pos, q, mu, alpha)
    exact = cc + dd
    norm = np.linalg.norm(mu, axis=1)
    has = norm > 0
    rc, kc = _converged(alpha)
    k = _k_vectors(kc)

    def finite(d):
        unit = mu[has] / norm[has, None]
        p = np.concatenate([pos, pos[has] + 0.5 * d * unit, pos[has] - 0.5 * d * unit])
        c = np.concatenate([q, norm[has] / d, -norm[has] / d])
        i, j, S = R.brute_force_entries(p, CELL, rc, int(math.ceil(rc / 5.0)) + 1)
        return float(R.charge_ewald_total(_t(p), _t(c), _t(CELL), alpha, i, j, S, k)) + float(np.sum((norm[has] / d) ** 2 / d))

    e1, e2 = finite(0.02), finite(0.01)
    ratio = (e1 - exact) / (e2 - exact)
    extrapolated = (4.0 * e2 - e1) / 3.0
    print(f"exact {exact:.12e}  d=0.02 err {e1 - exact:.3e}  d=0.01 err {e2 - exact:.3e}  ratio {ratio:.3f}  extrapolated rel "
          f"{abs(extrapolated - exact) / abs(exact):.2e}")
    assert 3.5 <= ratio <= 4.5
    assert abs(extrapolated - exact) <= 1e-7 * abs(exact)


def test_zero_dipoles_give_zero_energy_forces_charge_gradients_and_virial():
    """(dipole_grads is minus the electric field of the charges: it does not vanish.)"""
    pos, q, mu = _box()
    i, j, S = R.brute_force_entries(pos, CELL, 9.0, 3)
    out = R.evaluate(_t(pos), _t(q), _t(np.zeros_like(mu)), _t(CELL), 0.5, (i, j, S), _k_vectors(4.0))
    for name in ("energies", "forces", "charge_grads", "virial"):
        assert np.all(out[name] == 0.0), name
    assert np.abs(out["dipole_grads"]).max() > 1e-3


def test_per_atom_reciprocal_energies_sum_to_the_structure_factor_form():
    pos, q, mu = _box(8, seed=3)
    k = _k_vectors(5.0)
    P, Q, M, C = _t(pos), _t(q), _t(mu), _t(CELL)
    per_atom, abs_terms = R.recip_energies(P, Q, M, C, k, 0.5, return_abs=True)
    total = float(R.recip_total(P, Q, M, C, k, 0.5))
    assert abs(float(per_atom.sum()) - total) <= 1e-13 * float(abs_terms.sum())
    # no k-vectors: the self term alone
    alone = R.recip_energies(P, Q, M, C, k[:0], 0.5)
    want = -2.0 * 0.5**3 / (3.0 * math.sqrt(math.pi)) * (M * M).sum(-1)
    assert float((alone - want).abs().max()) <= 1e-16


def test_gradients_and_virial_match_finite_differences_and_the_virial_is_not_symmetric():
    pos, q, mu = _box(6, seed=5)
    i, j, S = R.brute_force_entries(pos, CELL, 8.0, 3)
    k = _k_vectors(4.0)
    P, Q, M, C = _t(pos), _t(q), _t(mu), _t(CELL)
    w = _t(np.random.default_rng(0).uniform(0.5, 1.5, 6))
    out = R.evaluate(P, Q, M, C, 0.5, (i, j, S), k, weights=w)
    plain = R.evaluate(P, Q, M, C, 0.5, (i, j, S), k)
    total = lambda p, c, m: float((R.energies(p, c, m, C, 0.5, (i, j, S), k) * w).sum().detach())  # noqa: E731
    h, g = 1e-5, np.random.default_rng(1)
    for _ in range(4):
        a_, x, y = int(g.integers(0, 6)), int(g.integers(0, 3)), int(g.integers(0, 3))
        d = torch.zeros_like(P); d[a_, x] = h
        fd = (total(P + d, Q, M) - total(P - d, Q, M)) / (2 * h)
        assert abs(-fd - out["forces"][a_, x]) < 1e-8 * max(1.0, abs(fd)), "force"
        fd = (total(P, Q, M + d) - total(P, Q, M - d)) / (2 * h)
        assert abs(fd - out["dipole_grads"][a_, x]) < 1e-8 * max(1.0, abs(fd)), "dipole gradient"
        d = torch.zeros_like(Q); d[a_] = h
        fd = (total(P, Q + d, M) - total(P, Q - d, M)) / (2 * h)
        assert abs(fd - out["charge_grads"][a_]) < 1e-8 * max(1.0, abs(fd)), "charge gradient"
        ep, em = torch.eye(3, dtype=F64), torch.eye(3, dtype=F64)
        ep[x, y] += h
        em[x, y] -= h
        e_of = lambda m: float(R.energies(P @ m.T, Q, M, C @ m.T, 0.5, (i, j, S), k @ torch.linalg.inv(m)).sum().detach())  # noqa: E731
        fd = (e_of(ep) - e_of(em)) / (2 * h)
        assert abs(-fd - plain["virial"][0, x, y]) < 1e-8 * max(1.0, abs(fd)), "virial"
    v = plain["virial"][0]
    assert np.abs(v - v.T).max() > 1e-3 * np.abs(v).max()  # dipoles fixed in the laboratory frame: nine independent components


def test_float32_distance_mode_is_close_and_differs():
    pos, q, mu = _box()
    i, j, S = R.brute_force_entries(pos, CELL, 8.0, 3)
    P, Q, M, C = _t(pos), _t(q), _t(mu), _t(CELL)
    e64 = R.real_energies(P, Q, M, C, 0.5, i, j, S)
    e32 = R.real_energies(P.float(), Q.float(), M.float(), C.float(), 0.5, i, j, S, distance_dtype=torch.float32)
    assert e32.dtype == F64 and 0 < float((e32 - e64).abs().max()) < 1e-5 * float(e64.abs().max())
