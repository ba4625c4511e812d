"""The float64 reference of the Gaussian-charge correction (tests/gaussian_reference.py) earns its role as the checker of the HIP kernel:
against an exact sum that involves no erfc at all, closed forms, and finite differences.  CPU only."""
import math

import numpy as np
import torch

from tests import gaussian_reference as R

F64 = torch.float64


def _box(n, seed, box=7.0, neutral=False):
    g = np.random.default_rng(seed)
    cell = np.array([[box, 0, 0], [0.2 * box, 0.9 * box, 0], [0.1 * box, -0.15 * box, 1.1 * box]])
    pos = g.uniform(0, 1, (n, 3)) @ cell
    q = g.normal(size=n)
    q = q - q.mean() if neutral else q + 0.3
    sigma = g.uniform(0.35, 0.9, n)
    return pos, cell, q, sigma


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=F64)


def test_point_charge_ewald_plus_correction_is_the_exact_gaussian_sum():
    pos, cell, q, sigma = _box(10, seed=1)
    assert abs(q.sum()) > 0.5  # a charged cell: the background term is on trial too
    i, j, S = R.brute_force_entries(pos, cell, 14.0, 4)  # 6 g_max = 6 sqrt(4 * 0.81) = 10.8 < 14: every pair with x < 6 is listed
    exact = R.gaussian_kspace_exact(pos, q, sigma, cell, 22)
    assert abs(R.gaussian_kspace_exact(pos, q, sigma, cell, 20) - exact) < 1e-13 * abs(exact)  # the k sum has converged
    point = R.point_charge_ewald_exact(pos, q, cell, 1.0, 2, 15)
    assert abs(R.point_charge_ewald_exact(pos, q, cell, 0.8, 3, 13) - point) < 1e-11 * abs(point)  # alpha-independent: the point sum is right
    corr = float(R.energies(_t(pos), _t(q), _t(sigma), _t(cell), i, j, S).sum())
    print(f"exact {exact:.15e}  point + correction {point + corr:.15e}  rel {abs(point + corr - exact) / abs(exact):.2e}")
    assert abs(point + corr - exact) <= 1e-10 * abs(exact)
    no_bg = float(R.energies(_t(pos), _t(q), _t(sigma), _t(cell), i, j, S, background=False).sum())
    e_bg = 2.0 * math.pi / abs(np.linalg.det(cell)) * q.sum() * (q * sigma**2).sum()
    assert abs(e_bg) > 1e-3 and abs((corr - no_bg) - e_bg) <= 1e-12 * abs(e_bg)
    assert abs(point + no_bg - exact) > 0.5 * abs(e_bg)  # ... and without it the sum is off by just that


def test_two_atoms_closed_form_energy_and_force():
    pos = _t([[0.0, 0, 0], [1.3, 0.4, -0.2]])
    q, sigma = _t([0.7, -1.1]), _t([0.5, 0.8])
    i, j, S = torch.tensor([0, 1]), torch.tensor([1, 0]), torch.zeros((2, 3), dtype=torch.long)
    r = float(torch.linalg.norm(pos[1] - pos[0]))
    gam = math.sqrt(2 * (0.25 + 0.64))
    x = r / gam
    pair = -0.7 * -1.1 * math.erfc(x) / r
    self_e = 0.49 / (2 * math.sqrt(math.pi) * 0.5) + 1.21 / (2 * math.sqrt(math.pi) * 0.8)
    out = R.evaluate(pos, q, sigma, None, i, j, S)
    assert abs(out["energies"].sum() - (pair + self_e)) < 1e-15
    assert abs(out["energies"][0] - (0.5 * pair + 0.49 / (2 * math.sqrt(math.pi) * 0.5))) < 1e-15
    # d/dr of -q1 q2 erfc(r/g)/r = q1 q2 (erfc(x)/r^2 + 2/(sqrt(pi) g) exp(-x^2)/r); the force on atom 0 is +dE/dr along (r_1 - r_0)
    dedr = 0.7 * -1.1 * (math.erfc(x) / r**2 + 2 / (math.sqrt(math.pi) * gam) * math.exp(-x * x) / r)
    want = dedr * (pos[1] - pos[0]).numpy() / r
    assert np.abs(out["forces"][0] - want).max() < 1e-15 and np.abs(out["forces"][0] + out["forces"][1]).max() < 1e-16
    assert out["virial"] is None and out["cell_grads"] is None


def test_self_term_alone():
    empty = torch.zeros(0, dtype=torch.long)
    out = R.evaluate(_t([[0.0, 0, 0]]), _t([1.7]), _t([0.6]), None, empty, empty, torch.zeros((0, 3), dtype=torch.long))
    assert abs(out["energies"][0] - 1.7**2 / (2 * math.sqrt(math.pi) * 0.6)) < 1e-16
    assert abs(out["charge_grads"][0] - 1.7 / (math.sqrt(math.pi) * 0.6)) < 1e-15
    assert abs(out["sigma_grads"][0] + 1.7**2 / (2 * math.sqrt(math.pi) * 0.36)) < 1e-15
    assert np.all(out["forces"] == 0)


def test_gradients_and_virial_match_finite_differences():
    pos, cell, q, sigma = _box(12, seed=4)
    sigma[3] = 0.0
    i, j, S = R.brute_force_entries(pos, cell, 14.0, 4)
    P, Q, Sg, Cc = _t(pos), _t(q), _t(sigma), _t(cell)
    w = _t(np.random.default_rng(0).uniform(0.5, 1.5, 12))
    out = R.evaluate(P, Q, Sg, Cc, i, j, S, weights=w)
    plain = R.evaluate(P, Q, Sg, Cc, i, j, S)
    assert out["sigma_grads"][3] == 0.0 and np.all(np.isfinite(out["sigma_grads"]))
    total = lambda p, c, s, ce: float((R.energies(p, c, s, ce, i, j, S) * w).sum())  # noqa: E731
    h, g = 1e-5, np.random.default_rng(1)
    for _ in range(4):
        k, a, b = int(g.integers(0, 12)), int(g.integers(0, 3)), int(g.integers(0, 3))
        if k == 3:
            k = 4
        d = torch.zeros_like(P); d[k, a] = h
        fd = (total(P + d, Q, Sg, Cc) - total(P - d, Q, Sg, Cc)) / (2 * h)
        assert abs(-fd - out["forces"][k, a]) < 1e-8 * max(1.0, abs(fd)), "force"
        d = torch.zeros_like(Q); d[k] = h
        fd = (total(P, Q + d, Sg, Cc) - total(P, Q - d, Sg, Cc)) / (2 * h)
        assert abs(fd - out["charge_grads"][k]) < 1e-8 * max(1.0, abs(fd)), "charge gradient"
        fd = (total(P, Q, Sg + d, Cc) - total(P, Q, Sg - d, Cc)) / (2 * h)
        assert abs(fd - out["sigma_grads"][k]) < 1e-8 * max(1.0, abs(fd)), "width gradient"
        d = torch.zeros_like(Cc); d[a, b] = h
        fd = (total(P, Q, Sg, Cc + d) - total(P, Q, Sg, Cc - d)) / (2 * h)
        assert abs(fd - out["cell_grads"][a, b]) < 1e-8 * max(1.0, abs(fd)), "cell gradient"
        eps = torch.eye(3, dtype=F64); eps[a, b] += h
        em = torch.eye(3, dtype=F64); em[a, b] -= h
        e_of = lambda m: float(R.energies(P @ m.T, Q, Sg, Cc @ m.T, i, j, S).sum())  # noqa: E731
        fd = (e_of(eps) - e_of(em)) / (2 * h)
        assert abs(-fd - plain["virial"][0, a, b]) < 1e-8 * max(1.0, abs(fd)), "virial"
    assert np.abs(plain["virial"][0] - plain["virial"][0].T).max() < 1e-12 * np.abs(plain["virial"]).max()


def test_all_point_charges_give_exactly_zero():
    pos, cell, q, _ = _box(10, seed=6)
    i, j, S = R.brute_force_entries(pos, cell, 9.0, 3)
    for sig in (np.zeros(10), -np.ones(10)):
        out = R.evaluate(_t(pos), _t(q), _t(sig), _t(cell), i, j, S)
        for name in ("energies", "forces", "charge_grads", "sigma_grads", "cell_grads", "virial"):
            assert np.all(out[name] == 0.0), name


def test_float32_distance_mode_is_close_and_entry_helpers_agree():
    pos, cell, q, sigma = _box(10, seed=7)
    i, j, S = R.brute_force_entries(pos, cell, 9.0, 3)
    e64 = R.energies(_t(pos), _t(q), _t(sigma), _t(cell), i, j, S)
    e32 = R.energies(_t(pos).float(), _t(q).float(), _t(sigma).float(), _t(cell).float(), i, j, S, distance_dtype=torch.float32)
    assert e32.dtype == F64 and 0 < float((e32 - e64).abs().max()) < 1e-5 * float(e64.abs().max())
    # the same entries as a CSR list and as a padded matrix (fill N, one row widened)
    order = torch.argsort(i, stable=True)
    i, j, S = i[order], j[order], S[order]
    counts = torch.bincount(i, minlength=10)
    ptr = torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(counts, 0)])
    ci, cj, cs = R.entries_from_csr(torch.stack([i, j]), ptr, S)
    assert torch.equal(ci, i) and torch.equal(cj, j) and torch.equal(cs, S)
    m = int(counts.max()) + 2
    nm, sh = torch.full((10, m), 10), torch.zeros((10, m, 3), dtype=torch.long)
    for a in range(10):
        nm[a, : counts[a]], sh[a, : counts[a]] = j[ptr[a]:ptr[a + 1]], S[ptr[a]:ptr[a + 1]]
    mi, mj, ms = R.entries_from_matrix(nm, sh, 10)
    assert torch.equal(mi, i) and torch.equal(mj, j) and torch.equal(ms, S)
