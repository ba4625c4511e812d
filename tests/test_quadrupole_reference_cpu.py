"""The yardstick of the point-quadrupole Ewald term (tests/quadrupole_reference.py) checked on the CPU, without the device code:

1. zero quadrupoles give exact zeros;
2. charge Ewald + dipole term + quadrupole term is independent of alpha on a small converged cell, to 1e-8 relative (the truncation of the
   sums chosen below: erfc(alpha r_c) and exp(-k_c^2 / 4 alpha^2) are both below 1e-14 at either alpha);
3. a point quadrupole Q = sym(p (x) dhat) is the d -> 0 limit of two opposite dipoles +-p/d at +-d/2 dhat evaluated with the dipole
   yardstick, with second-order convergence (the third-order moment of the pair vanishes by symmetry);
4. the expanded pair energy U and the self term, written out plainly, agree with the nested-autograd definition to 1e-12 relative.
"""
import math

import numpy as np
import torch

from tests import dipole_reference as D
from tests import quadrupole_reference as R

F64 = torch.float64


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=F64)


def _half_space(cell, k_cutoff):
    """Every reciprocal vector of `cell` with 0 < |k| <= k_cutoff in the half space (h > 0) or (h = 0, k > 0) or (h = k = 0, l > 0)."""
    rec = 2.0 * np.pi * np.linalg.inv(cell).T
    m = int(np.ceil(k_cutoff * np.linalg.norm(cell, axis=1).max() / (2.0 * np.pi))) + 1  # |index_a| = |k . cell_a| / 2 pi
    rng = np.arange(-m, m + 1)
    idx = np.stack(np.meshgrid(rng, rng, rng, indexing="ij"), axis=-1).reshape(-1, 3)
    half = (idx[:, 0] > 0) | ((idx[:, 0] == 0) & (idx[:, 1] > 0)) | ((idx[:, 0] == 0) & (idx[:, 1] == 0) & (idx[:, 2] > 0))
    k = idx[half] @ rec
    return _t(k[np.linalg.norm(k, axis=1) <= k_cutoff])


def _system(n, seed, box, traceless=False):
    g = np.random.default_rng(seed)
    cell = np.eye(3) * box
    pos = g.uniform(0.1, 0.9, (n, 3)) * box
    q = g.normal(size=n) + 0.3  # charged
    mu = 0.4 * g.normal(size=(n, 3))
    Q = 0.3 * g.normal(size=(n, 3, 3))
    Q = 0.5 * (Q + Q.transpose(0, 2, 1))
    if traceless:
        Q -= np.eye(3) * (np.trace(Q, axis1=1, axis2=2) / 3.0)[:, None, None]
    return pos, cell, q, mu, Q


def _total(pos, q, mu, Q, cell, alpha, entries, kv):
    """Charge Ewald + dipole term + quadrupole term of one system, all from the yardsticks."""
    P, Qc, M, QQ, C = _t(pos), _t(q), _t(mu), _t(Q), _t(cell)
    e = float(D.charge_ewald_total(P, Qc, C, alpha, *entries, kv)) + float(D.energies(P, Qc, M, C, alpha, entries, kv).sum().detach())
    return e + float(R.energies(P, Qc, M, QQ, C, alpha, entries, kv).sum().detach())


def test_zero_quadrupoles_give_exact_zeros():
    pos, cell, q, mu, Q = _system(6, seed=1, box=5.0)
    entries = R.brute_force_entries(pos, cell, 6.0, 2)
    kv = _half_space(cell, 4.0)
    for part in (dict(entries=entries), dict(k_vectors=kv), dict(entries=entries, k_vectors=kv)):
        out = R.evaluate(_t(pos), _t(q), _t(mu), _t(0.0 * Q), _t(cell), 0.6, **part)
        for name in ("energies", "forces", "charge_grads", "dipole_grads", "virial"):
            assert np.abs(out[name]).max() == 0.0, (sorted(part), name)
    # the field gradient of charges and dipoles at the atoms is there all the same
    assert np.abs(out["quadrupole_grads"]).max() > 1e-3
    assert float(R.self_energies(_t(q), _t(mu), _t(0.0 * Q), _t(np.full(6, 0.6))).detach().abs().max()) == 0.0


def test_total_is_independent_of_alpha_with_traced_quadrupoles():
    pos, cell, q, mu, Q = _system(4, seed=2, box=4.0)
    assert abs(q.sum()) > 0.3 and np.abs(np.trace(Q, axis1=1, axis2=2)).min() > 1e-3
    entries = R.brute_force_entries(pos, cell, 7.5, 3)  # erfc(0.9 * 7.5) = 1e-21, times the r^-5 and (2 alpha^2)^4 factors of B4: below 1e-14
    kv = _half_space(cell, 16.0)                        # exp(-16^2 / (4 * 1.2^2)) k^2 = 5e-20 * 256
    totals = [_total(pos, q, mu, Q, cell, alpha, entries, kv) for alpha in (0.9, 1.2)]
    print(f"alpha = 0.9: {totals[0]:.12f}   alpha = 1.2: {totals[1]:.12f}   difference {abs(totals[0] - totals[1]):.3e}")
    assert abs(totals[0] - totals[1]) <= 1e-8 * abs(totals[0])
    # the quadrupole term alone is NOT independent of alpha term by term: real and reciprocal halves each move by far more than the bar
    P, Qc, M, QQ, C = _t(pos), _t(q), _t(mu), _t(Q), _t(cell)
    halves = [float(R.energies(P, Qc, M, QQ, C, alpha, entries, None).sum().detach()) for alpha in (0.9, 1.2)]
    assert abs(halves[0] - halves[1]) > 1e-3 * abs(totals[0])


def test_quadrupole_is_the_limit_of_two_opposite_dipoles():
    pos, cell, q, mu, Q = _system(4, seed=3, box=6.0)
    g = np.random.default_rng(4)
    alpha, a = 0.7, 0  # atom `a` is replaced by itself without quadrupole plus two dipoles
    p = 0.5 * g.normal(size=3)
    dhat = g.normal(size=3)
    dhat /= np.linalg.norm(dhat)
    Q[a] = 0.5 * (np.outer(p, dhat) + np.outer(dhat, p))
    kv = _half_space(cell, 9.0)

    def total(pos_, q_, mu_, Q_):
        return _total(pos_, q_, mu_, Q_, cell, alpha, R.brute_force_entries(pos_, cell, 9.0, 2), kv)

    # the interaction of atom a with the rest: E(all) - E(a alone) - E(rest alone); the last is the same in both models and drops out, and the
    # intra-atomic terms of the split atom, which diverge with d -> 0, are in E(all) and E(a alone) alike
    point = total(pos, q, mu, Q) - total(pos[[a]], q[[a]], mu[[a]], Q[[a]])
    ei, ej, eS = R.brute_force_entries(pos, cell, 3.0, 1)
    assert float(torch.linalg.norm(_t(pos)[ej] - _t(pos)[ei] + eS.to(F64) @ _t(cell), dim=-1).min()) > 1.0  # r_min, for the last assertion
    errs, splits, ds = [], [], (0.2, 0.1, 0.05)
    for d in ds:
        Q0 = Q.copy()
        Q0[a] = 0.0
        pos_s = np.concatenate([pos, [pos[a] + 0.5 * d * dhat, pos[a] - 0.5 * d * dhat]])
        q_s, mu_s, Q_s = np.concatenate([q, [0.0, 0.0]]), np.concatenate([mu, [p / d, -p / d]]), np.concatenate([Q0, np.zeros((2, 3, 3))])
        own = [a, 4, 5]
        split = total(pos_s, q_s, mu_s, Q_s) - total(pos_s[own], q_s[own], mu_s[own], Q_s[own])
        splits.append(split)
        errs.append(abs(split - point))
        print(f"d = {d}: split {split:.12f} point {point:.12f} error {errs[-1]:.3e}")
    for k in (0, 1):
        assert 3.5 <= errs[k] / errs[k + 1] <= 4.5, errs  # second order: halving d quarters the error
    # with error(d) = c2 d^2 + c4 d^4 the Richardson value of the last two is off by c4 d^4 / 4 (d = 0.1), i.e. by (c4 / c2) d^2 of the last
    # error; c4 / c2 is of the order 1 / r_min^2 < 1 here, so 5 % of the last error leaves a factor of ten for the coefficients
    assert abs((4.0 * splits[2] - splits[1]) / 3.0 - point) <= 0.05 * errs[2], (splits, point)


def _closed_form_pair(R_, qi, mi, Qi, qj, mj, Qj, alpha):
    """U of the issue text, with B_n by the recursion of the kernel's header."""
    r2 = (R_ * R_).sum(-1)
    r = torch.sqrt(r2)
    pre = torch.exp(-alpha * alpha * r2) / (alpha * math.sqrt(math.pi))
    B = [torch.erfc(alpha * r) / r]
    for n in range(1, 5):
        B.append(((2 * n - 1) * B[-1] + (2.0 * alpha * alpha) ** n * pre) / r2)
    ci, cj = (mi * R_).sum(-1), (mj * R_).sum(-1)
    ti, tj = Qi.diagonal(dim1=-2, dim2=-1).sum(-1), Qj.diagonal(dim1=-2, dim2=-1).sum(-1)
    ai, aj = torch.einsum("eab,eb->ea", Qi, R_), torch.einsum("eab,eb->ea", Qj, R_)
    si, sj = (R_ * ai).sum(-1), (R_ * aj).sum(-1)
    return (qi * (B[2] * sj - B[1] * tj) + qj * (B[2] * si - B[1] * ti)
            + B[3] * ci * sj - B[2] * (2.0 * (mi * aj).sum(-1) + tj * ci) - B[3] * cj * si + B[2] * (2.0 * (mj * ai).sum(-1) + ti * cj)
            + B[4] * si * sj - B[3] * (ti * sj + tj * si + 4.0 * (ai * aj).sum(-1)) + B[2] * (ti * tj + 2.0 * (Qi * Qj).sum((-1, -2))))


def test_closed_form_pair_energy_and_self_term_agree_with_the_definition():
    pos, cell, q, mu, Q = _system(12, seed=5, box=6.0)
    alpha = 0.55
    i, j, S = R.brute_force_entries(pos, cell, 5.5, 1)
    P, Qc, M, QQ, C = _t(pos), _t(q), _t(mu), _t(Q), _t(cell)
    want = R.real_energies(P, Qc, M, QQ, C, alpha, i, j, S).detach()
    Rv = P[j] - P[i] + S.to(F64) @ C
    u = _closed_form_pair(Rv, Qc[i], M[i], QQ[i], Qc[j], M[j], QQ[j], alpha)
    got = torch.zeros(12, dtype=F64).index_add(0, i, 0.5 * u)
    err = float((got - want).abs().max() / want.abs().max())
    print(f"closed-form U vs nested autograd: {err:.2e} of the largest |E_i|")
    assert err <= 1e-12
    sp = math.sqrt(math.pi)
    t = QQ.diagonal(dim1=-2, dim2=-1).sum(-1)
    self_closed = 4.0 * alpha**3 / (3.0 * sp) * Qc * t - 4.0 * alpha**5 / (5.0 * sp) * (2.0 * (QQ * QQ).sum((-1, -2)) + t * t)
    self_ref = R.self_energies(Qc, M, QQ, _t(np.full(12, alpha))).detach()
    err = float((self_closed - self_ref).abs().max() / self_ref.abs().max())
    print(f"closed-form self term vs nested autograd: {err:.2e}")
    assert err <= 1e-12
    # L_i L_j - l_i l_j formed as a difference of the two products is the same numbers
    sub = R.real_energies(P, Qc, M, QQ, C, alpha, i, j, S, subtract=True).detach()
    assert float((sub - want).abs().max()) <= 1e-13 * float(want.abs().max())
    sub = R.self_energies(Qc, M, QQ, _t(np.full(12, alpha)), subtract=True).detach()
    assert float((sub - self_ref).abs().max()) <= 1e-13 * float(self_ref.abs().max())
    # an unsymmetric input is used as 1/2 (Q + Q^T)
    skew = torch.as_tensor(np.random.default_rng(6).normal(size=(12, 3, 3)))
    skew = skew - skew.transpose(-1, -2)
    again = R.real_energies(P, Qc, M, QQ + skew, C, alpha, i, j, S).detach()
    assert float((again - want).abs().max()) <= 1e-14 * float(want.abs().max())  # the rounding of (Q + skew) + (Q + skew)^T
