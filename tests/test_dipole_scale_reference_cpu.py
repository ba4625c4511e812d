"""The yardstick tests/dipole_scale_reference.py against things that already exist, and the conditions on the inputs of the scaled solves
(tests/dipole_scale_cases.py).  CPU only."""
import numpy as np
import pytest
import torch

from tests import cluster_multipole_reference as CR
from tests import dipole_scale_cases as SC
from tests import dipole_scale_reference as SR
from tests import induced_reference as IR
from tests import pair_scale_reference as PR
from tests import thole_reference as TR

F64 = torch.float64


def _arrays(p):
    return [torch.as_tensor(p[k], dtype=F64) for k in ("pos", "q", "mu", "polar")]


@pytest.mark.parametrize("kind", ["ladder70", "periodic", "molecules"])
def test_equal_scales_without_thole_are_the_pair_scale_yardstick_without_its_charge_term(kind):
    p = SC.problem(kind)
    pos, q, mu, polar = _arrays(p)
    s = torch.as_tensor(p["scales"])
    cell = None if p["cell"] is None else torch.as_tensor(p["cell"])
    bi = None if p["batch_idx"] is None else torch.as_tensor(p["batch_idx"])
    zero_q = torch.zeros((p["n"], 3, 3), dtype=F64)
    got = SR.evaluate(pos, q, mu, polar, s, s, p["entries"], cell=cell, batch_idx=bi)
    full = PR.evaluate(pos, q, mu, zero_q, s, p["entries"], cell=cell, batch_idx=bi)
    charges = PR.evaluate(pos, q, None, None, s, p["entries"], cell=cell, batch_idx=bi)
    for name in ("energies", "forces", "charge_grads", "dipole_grads") + (("virial",) if cell is not None else ()):
        ref = full[name] if name == "dipole_grads" else full[name] - charges[name]  # (the second term does not depend on mu)
        assert np.abs(got[name] - ref).max() <= 1e-12 * np.abs(ref).max(), name
    assert not got["polar_grads"].any()


@pytest.mark.parametrize("thole", [None, SC.A_T])
def test_unit_scales_are_identically_zero_and_both_sides_of_the_exit_occur(thole):
    p = SC.problem("ladder70")
    pos, q, mu, polar = _arrays(p)
    one = torch.ones(p["sd"].shape[0], dtype=F64)
    out = SR.evaluate(pos, q, mu, polar, one, one, p["entries"], thole=thole)
    assert all(not v.any() for v in out.values())
    i, j, _ = p["entries"]
    ok = (polar[i] > 0) & (polar[j] > 0)
    E = SC.A_T * (pos[j] - pos[i]).norm(dim=1)[ok] ** 3 / torch.sqrt(polar[i][ok] * polar[j][ok])
    assert bool((E < 50).any()) and bool((E >= 50).any()) and bool((~ok).any())
    assert {SC.CLASS[float(s)] for s in p["scales"]} == set(SC.CLASS.values())


@pytest.mark.parametrize("thole", [None, SC.A_T])
def test_zero_scales_cancel_the_dipole_dependent_interaction_of_the_pair(thole):
    g = np.random.default_rng(3)
    pos = torch.as_tensor([[0.0, 0.0, 0.0], [1.1, 0.9, -0.4]], dtype=F64)
    q, mu, polar = (torch.as_tensor(a) for a in (g.normal(size=2), g.normal(size=(2, 3)), g.uniform(0.5, 1.5, 2)))
    ent, zero = CR.all_pairs([2]), torch.zeros(2, dtype=F64)
    total = CR.dipole_energies(pos, q, mu, ent) + SR.pair_energies(pos, q, mu, polar, zero, zero, *ent, thole=thole)
    if thole is not None:
        total = total + TR.energies(pos, q, mu, polar, None, thole, *ent)
    assert float(CR.dipole_energies(pos, q, mu, ent).detach().abs().max()) > 0.1 and float(total.detach().abs().max()) <= 1e-15


@pytest.mark.parametrize("kind,thole", [("bent", None), ("bent", SC.A_T), ("chains", None), ("chains", SC.A_T)])
def test_the_scaled_solve_cases_are_well_conditioned(kind, thole):
    c = SC.solve_case(kind)
    H, _ = SC.dense(c, thole)
    ev = IR.scaled_spectrum(H, c["polar"])
    print(f"{kind} thole {thole}: spectrum of D^1/2 H D^1/2 in [{float(ev.min()):.3f}, {float(ev.max()):.3f}]")
    assert float(ev.min()) > 0.5 and float((H - H.T).abs().max()) <= 1e-12 * float(H.abs().max())
