"""The dense reference of the induced-dipole problem (tests/induced_reference.py) checked against itself on the CPU, and the condition the
shared systems (tests/induced_cases.py) have to meet: H positive definite with a margin.

Measured with this reference for the cases l27, l64, l27dense:
    d_min                                             2.02, 1.97, 1.80
    smallest eigenvalue of D^1/2 H D^1/2, D = diag(a) 0.65, 0.72, 0.65       (largest 1.34, 1.35, 1.44)
    dense PCG iterations from mu0 = a b to 1e-10      11, 12, 13
    alpha independence (l27, l27dense)                max |dT| 7.2e-9, 1.5e-9 on max |T| 0.25, 0.32; max |db| 2.1e-9, 3.6e-10: the truncation
                                                      of the two parameter sets (0.45, cutoff 11, k_cutoff 3.2) and (0.6, 9, 4.2)
"""
import functools

import pytest
import torch

from tests import induced_cases as IC
from tests import induced_reference as R

F64 = torch.float64
NAMES = tuple(IC.CASES)


def _t(a):
    return torch.as_tensor(a, dtype=F64)


@functools.lru_cache(maxsize=None)
def _problem(name, alpha=IC.EWALD["alpha"], cutoff=IC.EWALD["cutoff"], k_cutoff=IC.EWALD["k_cutoff"]):
    c = IC.lattice(name)
    T, lin = R.dipole_operator(_t(c["pos"]), _t(c["q"]), _t(c["cell"]), alpha, IC.entries(name, cutoff), IC.k_vectors(c["cell"], k_cutoff))
    polar = _t(c["polar"])
    return dict(T=T, c=lin, polar=polar, H=R.system_matrix(T, polar), b=R.right_hand_side(lin, polar))


@pytest.mark.parametrize("name", NAMES)
def test_operator_is_symmetric_and_the_inputs_are_positive_definite_with_a_margin(name):
    f = _problem(name)
    assert float((f["T"] - f["T"].T).abs().max()) <= 1e-15
    ev = R.scaled_spectrum(f["H"], f["polar"])
    print(f"{name}: d_min {IC.lattice(name)['d_min']:.3f}, spectrum of D^1/2 H D^1/2 in [{float(ev.min()):.3f}, {float(ev.max()):.3f}]")
    assert float(ev.min()) > 0.5  # a condition on the inputs, not a measurement


@pytest.mark.parametrize("name", ["l27", "l27dense"])
def test_operator_and_right_hand_side_do_not_depend_on_alpha(name):
    f, g = _problem(name), _problem(name, 0.6, 9.0, 4.2)
    dT, db = float((f["T"] - g["T"]).abs().max()), float((f["b"] - g["b"]).abs().max())
    print(f"{name}: max |dT| {dT:.2e} on max |T| {float(f['T'].abs().max()):.3f}, max |db| {db:.2e} on max |b| {float(f['b'].abs().max()):.3f}")
    assert dT <= 1e-5 and db <= 1e-5


@pytest.mark.parametrize("name", NAMES)
def test_solution_minimises_the_energy_and_pcg_agrees_with_the_dense_solve(name):
    f = _problem(name)
    H, b = f["H"], f["b"]
    mu = R.solve(H, b)
    u = float(R.energy(H, b, mu))
    assert abs(-0.5 * float(mu.reshape(-1) @ b) - u) <= 1e-13 * abs(u)
    g = torch.Generator().manual_seed(7)
    for _ in range(5):
        delta = 1e-3 * torch.randn(mu.shape, dtype=F64, generator=g)
        assert float(R.energy(H, b, mu + delta)) > u
    x, its = R.pcg(H, b, R.preconditioner(f["polar"]), 1e-10)
    print(f"{name}: dense PCG from mu0 = a b to 1e-10 in {its} iterations")
    lam = float(torch.linalg.eigvalsh(H).min())
    assert 0 < its < 40 and float((x - mu).abs().max()) <= 10 * 1e-10 * float(b.norm()) / lam


@pytest.mark.parametrize("thole", [None, 0.39], ids=["undamped", "thole"])
def test_fold_case_truncated_operator_with_the_self_term_alone_is_positive_definite(thole):
    """The problem tests/test_fold_sizes_gpu.py tiles: the real-space sum cut at 6 and an empty k set.  Measured: spectrum of D^1/2 H D^1/2 in
    [0.631, 1.215] undamped, [0.698, 1.150] damped; rows of 29 - 36 entries; dense PCG to 1e-10 in 10 iterations both."""
    from tests import thole_cases as TC

    case = TC.fold_case()
    d = TC.dense(case, thole)
    assert d["kv"].shape == (0, 3)
    ev = R.scaled_spectrum(d["H"], d["polar"])
    _, its = R.pcg(d["H"], d["b"], R.preconditioner(d["polar"]), 1e-10)
    rows = torch.bincount(case["entries"][0], minlength=case["n"])
    print(f"fold case {'undamped' if thole is None else 'thole'}: spectrum of D^1/2 H D^1/2 in [{float(ev.min()):.3f}, {float(ev.max()):.3f}], "
          f"rows of {int(rows.min())} - {int(rows.max())} entries (mean {float(rows.double().mean()):.1f}), dense PCG to 1e-10 in {its} iterations")
    assert float((d["H"] - d["H"].T).abs().max()) <= 1e-15
    assert float(ev.min()) > 0.5 and float(torch.linalg.eigvalsh(d["H"]).min()) > 0  # a condition on the inputs, not a measurement
    assert float(d["b"].abs().max()) > 0 and 0 < its < 40
    # the self term is all that the empty k set leaves: H differs from the real-space operator by -(4 alpha^3 / 3 sqrt(pi)) on the diagonal
    pos, q, cell = _t(case["pos"]), _t(case["q"]), _t(case["cell"])
    if thole is None:
        t_real, _ = R.dipole_operator(pos, q, cell, case["alpha"], case["entries"])
    else:
        t_real, _ = TC.TR.damped_operator(pos, q, d["polar"], cell, case["alpha"], thole, case["entries"])
    self_term = 4.0 * case["alpha"] ** 3 / (3.0 * torch.pi ** 0.5)
    assert float((d["T"] - t_real + self_term * torch.eye(3 * case["n"], dtype=F64)).abs().max()) <= 1e-14


def test_non_polarisable_atoms_are_inert():
    c = IC.lattice("l27")
    f = _problem("l27")
    polar = f["polar"].clone()
    polar[[2, 11]] = 0.0
    polar[20] = float("nan")
    H, b = R.system_matrix(f["T"], polar), R.right_hand_side(f["c"], polar, field=torch.ones((c["n"], 3), dtype=F64))
    mu = R.solve(H, b)
    assert bool((mu[[2, 11, 20]] == 0).all()) and float(mu.abs().max()) > 0
    assert float((H - H.T).abs().max()) <= 1e-15 and float(torch.linalg.eigvalsh(H).min()) > 0
    x, its = R.pcg(H, b, R.preconditioner(polar), 1e-10)
    assert bool((x[[2, 11, 20]] == 0).all()) and float((x - mu).abs().max()) <= 1e-8 * float(mu.abs().max())
