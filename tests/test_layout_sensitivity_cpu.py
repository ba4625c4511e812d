"""What makes the layout sweeps of tests/test_arg_layouts_gpu.py worth running, checked without a GPU on the fixtures those sweeps use
(tests/layout_cases.py): an entry point that hands a kernel a misread argument -- modelled as the argument ROLLED BY ONE along its first
axis -- must move at least one output of the float64 restatement by 100 x the bar the sweep applies to that output.  Otherwise a variant
read with the wrong stride could pass.  A fixture that fails this is changed; the bars are those of the ops' own parity modules.

`en` is the argument that decides the D4 fixtures: it enters through the electronegativity factor of the coordination numbers of unlike
pairs only.  With the 70 + 60 atoms of the batch taken as the FIRST sites of the lattice (slabs with few contacts) rolled `en` moved the
`dftd4` restatement by 0.45 bars and `dftd4_atm`'s by 0.05 (rolled `rcov`: 54): the batch is therefore built of compact blocks.  On the
130-atom single system `en` moves `dftd4` by 881 bars but the three-body term by 66 only, so the table sweeps of `dftd4_atm` run on a
compact 130-atom block as well, where every table is asserted; on the single system itself the figures of `dftd4_atm` are printed
and its `s9` rule is asserted.  Every test prints its table (`pytest -s`)."""
import numpy as np
import pytest
import torch

from tests import d4_atm_cases as K3
from tests import layout_cases as L

FACTOR = 100.0


def _roll(a):
    return np.roll(np.asarray(a), 1, axis=0)


def _ratio(moved, ref, bar):
    return float((np.abs(moved - ref) / bar).max())


@pytest.mark.parametrize("batch", [False, True], ids=["single", "batch"])
def test_dftd4_fixture_rolled_charges_and_tables_move_the_restatement(batch):
    c = L.d4(batch)
    r64, r32 = L.d4_references(batch)
    keys = [k for k in L.D4_KEYS if r64[k] is not None]
    bars = {k: L.d4_bar(r64, r32, k) for k in keys}
    assert float(r64["cn"].max()) < 3.0, "the coordination numbers must stay near the range [0, 1] of the reference values"
    worst = {}
    for arg in ("q",) + L.R.TABLE_KEYS:
        moved = L.d4_reference(batch, **{arg: _roll(c["q"] if arg == "q" else c["tables"][arg])})
        worst[arg] = max(_ratio(moved[k], r64[k], bars[k]) for k in keys)
    print(f"[sensitivity dftd4 {'batch' if batch else 'single'}] largest |moved - ref| / bar: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert all(v >= FACTOR for v in worst.values()), worst


def _atm_table_ratios(batch, compact):
    s9 = L.d4_atm_s9(batch, compact)
    r64u = L.d4_atm_unit_references(batch, compact)[0]
    assert K3.lifted(r64u, s9) and (s9 == 1.0 or not K3.lifted(r64u, s9 / 10.0))
    c = L.d4(batch, compact)
    r64, r32 = L.d4_atm_references(batch, compact)
    keys = [k for k in L.ATM_KEYS if r64[k] is not None]
    bars = {k: L.d4_bar(r64, r32, k, K3.EXTRA) for k in keys}
    worst = {}
    for arg in L.R.TABLE_KEYS:
        moved = L.d4_atm_reference(batch, compact, **{arg: _roll(c["tables"][arg])})
        worst[arg] = max(_ratio(moved[k] * s9, r64[k], bars[k]) for k in keys)
    print(f"[sensitivity dftd4_atm {'batch' if batch else 'compact' if compact else 'single'}] s9 {s9:g}; largest |moved - ref| / bar: "
          + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    return s9, worst


@pytest.mark.parametrize("batch,compact", [(False, True), (True, False)], ids=["compact", "batch"])
def test_dftd4_atm_table_fixtures_rolled_tables_move_the_restatement(batch, compact):
    """The two fixtures on which the table sweeps of `dftd4_atm` are judged."""
    _, worst = _atm_table_ratios(batch, compact)
    assert all(v >= FACTOR for v in worst.values()), worst


def test_dftd4_atm_single_system_s9_rule():
    """The prescribed single system: s9 by the rule of tests/d4_atm_cases.py is 10.  Its table figures are printed; the tables of
    `dftd4_atm` are judged on the compact block above (`en`: 66 bars here)."""
    s9, _ = _atm_table_ratios(False, False)
    assert s9 == 10.0


@pytest.mark.parametrize("batch", [False, True], ids=["single", "batch"])
def test_gaussian_fixture_rolled_charges_and_widths(batch):
    """The float32 sweep's bar is 1e-6 max|ref| (+ 1e-14), the float64 sweep's 1e-11 max|ref|: the wider one is used here."""
    c = L.gaussian(batch)
    ref = L.gaussian_reference(batch)
    assert abs(float(c["q"].sum())) > 1.0 and int((c["sigma"] == 0).sum()) == (4 if batch else 2)
    worst = {}
    for arg in ("q", "sigma"):
        moved = L.gaussian_reference(batch, **{arg: _roll(c[arg])})
        worst[arg] = max(_ratio(moved[k], ref[k], 1e-6 * np.abs(ref[k]).max() + 1e-14) for k in L.GC_NAMES)
    print(f"[sensitivity gaussian {'batch' if batch else 'single'}] largest |moved - ref| / bar: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert all(v >= FACTOR for v in worst.values()), worst


@pytest.mark.parametrize("case", ["cluster", "periodic"])
def test_qeq_fixtures_rolled_electronegativity_hardness_and_widths(case):
    """The periodic sweep compares charges at twice `_check_solution`'s bound; the cluster sweep demands equal bits, so any movement counts
    there -- it is held to the same bound all the same."""
    c = L.qeq_cluster() if case == "cluster" else L.qeq_periodic()
    h, chi, total, bi = L.qeq_dense(c)
    bound = torch.tensor(L.qeq_charge_bound(h, chi, total, bi, c["nsys"]))[bi.long()]
    q_ref, _ = L.QR.solve(h, chi, total, bi, c["nsys"])
    assert all(float(torch.linalg.eigvalsh(h[bi == s][:, bi == s]).min()) > 0 for s in range(c["nsys"]))
    worst = {}
    for arg in ("chi", "hard", "sigma"):
        hm, chim, _, _ = L.qeq_dense(c, **{arg: _roll(c[arg])})
        q, _ = L.QR.solve(hm, chim, total, bi, c["nsys"])
        worst[arg] = float(((q - q_ref).abs() / (2.0 * bound)).max())
    print(f"[sensitivity qeq {case}] largest |moved - ref| / (2 x bound): " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert all(v >= FACTOR for v in worst.values()), worst


@pytest.mark.parametrize("op", ["ewald", "pme"])
@pytest.mark.parametrize("batch", [False, True], ids=["single", "batch"])
def test_dipole_fixture_rolled_dipoles_charges_and_alpha(batch, op):
    """The widest bar the sweep applies to the canonical call is used: 1e-6 max|ref| (+ 1e-14) for the explicit sums (their float32 bar) and
    4 x the restatement's own float32-against-float64 deviation for the mesh term (at most 4e-5 of max|ref|).  `alpha` holds one value per
    system: on the single system rolling it changes nothing, so it is judged on the batch (0.4 and 0.375) only."""
    c = L.dipole(batch)
    ref = L.dipole_reference(batch, op)
    assert abs(float(c["q"].sum())) > 1.0 and int((~c["mu"].any(axis=1)).sum()) == (4 if batch else 2)
    if op == "ewald":
        bars = {k: 1e-6 * np.abs(ref[k]).max() + 1e-14 for k in L.DP_NAMES}
    else:
        r32 = L.dipole_reference(batch, op, dtype=torch.float32)
        bars = {k: 4.0 * np.abs(r32[k] - ref[k]).max() for k in L.DP_NAMES}
        assert all(bars[k] <= 4e-5 * np.abs(ref[k]).max() for k in L.DP_NAMES)
    worst = {}
    for arg in ("mu", "q") + (("alpha",) if batch else ()):
        moved = L.dipole_reference(batch, op, **{arg: _roll(c[arg])})
        worst[arg] = max(_ratio(moved[k], ref[k], bars[k]) for k in L.DP_NAMES)
    print(f"[sensitivity {op} dipole {'batch' if batch else 'single'}] largest |moved - ref| / bar: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert all(v >= FACTOR for v in worst.values()), worst
