"""What makes the layout sweeps of tests/test_arg_layouts_gpu.py worth running, checked without a GPU on the fixtures those sweeps use
(tests/layout_cases.py): an entry point that hands a kernel a misread argument -- modelled as the argument ROLLED BY ONE along its first
axis -- must move at least one output of the float64 restatement by 100 x the bar the sweep applies to that output.  Otherwise a variant
read with the wrong stride could pass.  A fixture that fails this is changed; the bars are those of the ops' own parity modules.

`en` is the argument that decides the D4 fixtures: it enters through the electronegativity factor of the coordination numbers of unlike
pairs only.  With the 70 + 60 atoms of the batch taken as the FIRST sites of the lattice (slabs with few contacts) rolled `en` moved the
`dftd4` restatement by 0.45 bars and `dftd4_atm`'s by 0.05 (rolled `rcov`: 54): the batch is therefore built of compact blocks.  On the
130-atom single system `en` moves `dftd4` by 881 bars but the three-body term by 66 only, so the table sweeps of `dftd4_atm` run on a
compact 130-atom block as well, where every table is asserted; on the single system itself the figures of `dftd4_atm` are printed
and its `s9` rule is asserted.  Every test prints its table (`pytest -s`).

Quadrupole, Thole and induced-dipole fixtures, measured here (largest |moved - ref| / bar, single / batch): quadrupole restatement --
quadrupoles 2.3e6 / 1.7e6, dipoles 1.1e6 / 9.5e5, charges 9.7e5 / 1.1e6, alpha (batch) 738; Thole restatement -- polarisabilities 8.3e5 /
6.0e5, dipoles 1.9e6 / 2.8e6, charges 1.5e6 / 1.6e6, E between 0.27 and 60; dense induced-dipole solution against 2 x `_check_solution`'s
bound -- polarisabilities, charges and external field 1e7 - 1e8 in all four fixtures, alpha (batch) 3.5e3 undamped and 1.9e4 damped.  The
alpha of the induced batch is why its 27-atom lattice runs at alpha 0.625 with a truncated k sum: with two converged parameter sets the
operator does not depend on alpha and a rolled `alpha` moved the solution by 1.25 x (2 x bound).  Smallest eigenvalue of D^1/2 H D^1/2:
0.717 (single) and 0.653, 0.717 (batch) undamped; 0.475 and 0.481, 0.472 damped at polarisabilities in [2, 8], where the undamped H is
indefinite (asserted).

Pair-scale and local-frame fixtures, measured here (single / batch): rolled `pair_scales` 4.5e5 / 9.8e5 bars; rolled `frame_atoms` 1.8e6 /
2.0e6, `local_quadrupoles` 1.4e6 / 1.3e6, `quadrupole_grads` 1.7e6 / 1.9e6.  Geometry of the frame fixture: bonds 0.957 - 1.446, angles
42.0 - 131.1 degrees, Z_ONLY axes 0.053 from the switch, chiral triple products >= 0.47, fractional components of frame vectors <= 0.145."""
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


@pytest.mark.parametrize("batch", [False, True], ids=["single", "batch"])
def test_quadrupole_fixture_rolled_quadrupoles_dipoles_charges_and_alpha(batch):
    """The widest bar the sweep applies to the canonical call: 1e-6 max|ref| (+ 1e-14), the float32 bar of tests/test_quadrupole_gpu.py.
    `alpha` is judged on the batch (0.4 and 0.375) only.  Also the properties the fixture promises: two zero rows and four unsymmetric rows
    per system, and that reading Q transposed changes nothing in the restatement (1/2 (Q + Q^T) is what counts) while Q itself is not
    symmetric -- so a T variant whose storage was read untransposed agrees, and one read with a wrong stride does not."""
    c = L.quadrupole(batch)
    ref = L.quadrupole_reference(batch)
    nsys = 2 if batch else 1
    assert int((~c["qd"].any(axis=(1, 2))).sum()) == 2 * nsys
    assert int((np.abs(c["qd"] - c["qd"].transpose(0, 2, 1)).max(axis=(1, 2)) > 1e-3).sum()) == 4 * nsys
    bars = {k: 1e-6 * np.abs(ref[k]).max() + 1e-14 for k in L.QD_NAMES}
    flipped = L.quadrupole_reference(batch, qd=np.ascontiguousarray(c["qd"].transpose(0, 2, 1)))
    assert all(_ratio(flipped[k], ref[k], bars[k]) <= 1e-3 for k in L.QD_NAMES)
    worst = {}
    for arg in ("qd", "mu", "q") + (("alpha",) if batch else ()):
        moved = L.quadrupole_reference(batch, **{arg: _roll(c[arg])})
        worst[arg] = max(_ratio(moved[k], ref[k], bars[k]) for k in L.QD_NAMES)
    print(f"[sensitivity quadrupole {'batch' if batch else 'single'}] largest |moved - ref| / bar: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert all(v >= FACTOR for v in worst.values()), worst


@pytest.mark.parametrize("batch", [False, True], ids=["single", "batch"])
def test_thole_fixture_rolled_polarisabilities_dipoles_and_charges(batch):
    """The widest bar of the sweep: 1e-6 max|ref| (+ 1e-14), the float32 bar of tests/test_thole_gpu.py.  The correction does not depend on
    alpha.  Both sides of the kernel's exit at E = 50 are present among the stored entries."""
    c = L.thole(batch)
    ref = L.thole_reference(batch)
    assert int((c["polar"] == 0).sum()) == (4 if batch else 2) and float(c["polar"][c["polar"] > 0].min()) >= 2.0 and float(c["polar"].max()) <= 8.0
    i, j, S = L._entries(c["pos"], c["cell"], c["batch_idx"], L.GC_RC)
    bi = np.zeros(len(c["pos"]), np.int64) if c["batch_idx"] is None else c["batch_idx"]
    r = np.linalg.norm(c["pos"][j] - c["pos"][i] + np.einsum("ea,eab->eb", S.numpy().astype(np.float64), c["cell"][bi[i]].astype(np.float64)), axis=1)
    ok = (c["polar"][i] > 0) & (c["polar"][j] > 0)
    E = L.THOLE * r[ok] ** 3 / np.sqrt(c["polar"][i][ok].astype(np.float64) * c["polar"][j][ok])
    assert (E < 1.0).any() and (E >= 50.0).any()
    bars = {k: 1e-6 * np.abs(ref[k]).max() + 1e-14 for k in L.TH_NAMES}
    worst = {}
    for arg in ("polar", "mu", "q"):
        moved = L.thole_reference(batch, **{arg: _roll(c[arg])})
        worst[arg] = max(_ratio(moved[k], ref[k], bars[k]) for k in L.TH_NAMES)
    print(f"[sensitivity thole {'batch' if batch else 'single'}] E in [{E.min():.3g}, {E.max():.3g}]; largest |moved - ref| / bar: "
          + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert all(v >= FACTOR for v in worst.values()), worst


@pytest.mark.parametrize("damped", [False, True], ids=["undamped", "thole"])
@pytest.mark.parametrize("batch", [False, True], ids=["single", "batch"])
def test_induced_fixtures_are_positive_definite_and_rolled_arguments_move_the_dipoles(batch, damped):
    """The sweep of the solves compares the canonical call with the dense solution at `_check_solution`'s bound and variants by their bits;
    the one `reciprocal="pme"` pass is held to twice that bound, which is the widest bar: a rolled `polarizability`, `charges`,
    `external_field` or (batch) `alpha` must move the dense solution by 100 x (2 x bound).  The smallest eigenvalue of D^1/2 H D^1/2 is
    positive for every system: undamped at the cases' polarisabilities, damped at polarisabilities drawn as the Thole fixture's (uniform in
    [2, 8], where the undamped operator is NOT positive definite, which is asserted too: the damping is what the damped fixture tests)."""
    thole = L.THOLE if damped else None
    c = L.induced(batch)
    d = L.induced_dense(c, thole)
    nsys = c["nsys"]
    sys_of = (torch.zeros(c["n"], dtype=torch.long) if d["bi"] is None else d["bi"].long()).repeat_interleave(3)
    low = []
    for s in range(nsys):
        m = torch.nonzero(sys_of == s).flatten()
        ev = L.IR.scaled_spectrum(d["H"][m][:, m], d["polar"][m[::3] // 3])
        low.append(float(ev.min()))
    assert min(low) > 0, low
    if damped:
        assert int((c["polar_thole"] == 0).sum()) == 2 * nsys
        plain = L.induced_dense(c, None, polar=c["polar_thole"])
        assert float(torch.linalg.eigvalsh(plain["H"]).min()) < 0, "without damping these polarisabilities must be beyond the polarisation catastrophe"
    bound = torch.tensor(L.induced_bound(d, nsys))[sys_of].reshape(-1, 3)
    mu_ref = L.IR.solve(d["H"], d["b"], d["bi"], nsys)
    worst = {}
    for arg in ("polar", "q", "field") + (("alpha",) if batch else ()):
        m = L.induced_dense(c, thole, **{arg: _roll(c["polar_thole" if damped and arg == "polar" else arg])})
        worst[arg] = float(((L.IR.solve(m["H"], m["b"], m["bi"], nsys) - mu_ref).abs() / (2.0 * bound)).max())
    print(f"[sensitivity induced {'batch' if batch else 'single'} {'thole' if damped else 'undamped'}] smallest eigenvalue of D^1/2 H D^1/2 per system "
          f"{[round(v, 3) for v in low]}; largest |moved - ref| / (2 x bound): " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert all(v >= FACTOR for v in worst.values()), worst


@pytest.mark.parametrize("batch", [False, True], ids=["single", "batch"])
def test_pme_quadrupole_fixture_rolled_arguments_and_a_transposed_cell(batch):
    """The widest bar the sweep applies to the canonical call of `pme_quadrupole_reciprocal_space`: 4 x the restatement's own
    float32-against-float64 deviation (at most 1e-4 of max |ref|), mesh (12, 10, 14), order 6.  A rolled `positions`, `charges`, `dipoles`,
    `quadrupoles`, (batch) `alpha` or `batch_idx`, or a transposed cell, must move the restatement by 100 bars.  A transposed `quadrupoles`
    must NOT move it: 1/2 (Q + Q^T) is what counts, so a variant that hands the kernel Q^T agrees by construction (the `F` variant of the
    sweep), and only one read with a wrong stride differs.  Measured (single / batch): positions 3.2e5 / 3.9e5, charges 2.3e5 / 2.5e5,
    dipoles 1.8e5 / 2.4e5, quadrupoles 3.0e5 / 3.2e5, cell 2.3e5 / 2.4e5, alpha (batch) 6.0e4, batch_idx (batch) 1.3e5."""
    c = L.pme_quadrupole(batch)
    ref, r32 = L.pme_quadrupole_references(batch)
    bars = {k: 4.0 * np.abs(r32[k] - ref[k]).max() for k in L.QD_NAMES}
    assert all(0.0 < bars[k] <= 1e-4 * np.abs(ref[k]).max() for k in L.QD_NAMES), {k: bars[k] / np.abs(ref[k]).max() for k in L.QD_NAMES}
    assert np.abs(c["qd"] - c["qd"].transpose(0, 2, 1)).max() > 1e-3 and np.abs(c["cell"] - c["cell"].transpose(0, 2, 1)).max() > 1.0
    flipped = L.pme_quadrupole_reference(batch, qd=np.ascontiguousarray(c["qd"].transpose(0, 2, 1)))
    assert all(_ratio(flipped[k], ref[k], bars[k]) <= 1e-3 for k in L.QD_NAMES), "Q transposed: the same symmetric part"
    worst = {}
    for arg in ("pos", "q", "mu", "qd") + (("alpha", "batch_idx") if batch else ()):
        moved = L.pme_quadrupole_reference(batch, **{arg: _roll(c[arg])})
        worst[arg] = max(_ratio(moved[k], ref[k], bars[k]) for k in L.QD_NAMES)
    moved = L.pme_quadrupole_reference(batch, cell=np.ascontiguousarray(c["cell"].transpose(0, 2, 1)))
    worst["cell transposed"] = max(_ratio(moved[k], ref[k], bars[k]) for k in L.QD_NAMES)
    print(f"[sensitivity pme_quadrupole {'batch' if batch else 'single'}] largest |moved - ref| / bar: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert all(v >= FACTOR for v in worst.values()), worst


@pytest.mark.parametrize("batch", [False, True], ids=["single", "batch"])
def test_pair_scale_fixture_rolled_scales(batch):
    """`pair_scales` is the one argument class `pair_scale_correction` adds: one value per stored entry.  Rolled by one entry it must move the
    restatement by 100 x the widest bar of the sweep, 1e-6 max|ref| (+ 1e-14), the float32 bar of tests/test_pair_scale_gpu.py.  Also what the
    fixture promises: the four classes are present, the scales are symmetric, every listed distance is at least the 1.3 the bars assume,
    and the sub-list of the `minimum_image` calls is full, holds shifted entries and is not the whole list."""
    from tests.cluster_multipole_reference import D_MIN

    c = L.pair_scale(batch)
    i, j, S = c["ent"]
    t = torch.as_tensor
    bi = None if c["batch_idx"] is None else t(c["batch_idx"])
    d, _ = L.pair_vectors(t(c["pos"]), t(c["cell"]), bi, i, j, S)
    assert float(d.norm(dim=1).min()) >= D_MIN and sorted(set(c["scales"].tolist())) == sorted(L.PS_SCALES)
    by_pair = {(a, b, tuple(s)): v for a, b, s, v in zip(i.tolist(), j.tolist(), S.tolist(), c["scales"].tolist())}
    assert all(by_pair[(b, a, tuple(-x for x in s))] == v for (a, b, s), v in by_pair.items()), "s_ij = s_ji"
    keep = L.minimum_image_entries(t(c["pos"]), t(c["cell"]), bi, i, j, S)
    kept = {(a, b) for a, b in zip(i[keep].tolist(), j[keep].tolist())}
    assert 0 < len(kept) == int(keep.sum()) < keep.shape[0] and all((b, a) in kept for a, b in kept) and bool((S[keep] != 0).any())
    ref = L.pair_scale_reference(batch)
    bars = {k: 1e-6 * np.abs(ref[k]).max() + 1e-14 for k in L.QD_NAMES}
    moved = L.pair_scale_reference(batch, scales=_roll(c["scales"]))
    worst = max(_ratio(moved[k], ref[k], bars[k]) for k in L.QD_NAMES)
    print(f"[sensitivity pair_scale {'batch' if batch else 'single'}] largest |moved - ref| / bar: pair_scales {worst:.3g}; minimum-image sub-list "
          f"{int(keep.sum())} of {keep.shape[0]} entries")
    assert worst >= FACTOR


@pytest.mark.parametrize("batch", [False, True], ids=["single", "batch"])
def test_frames_fixture_geometry_and_rolled_tables_multipoles_and_gradients(batch):
    """The geometry conditions behind the bars of tests/test_local_frames_gpu.py on the float32 numbers of the fixture: bond lengths in
    [0.9, 1.6], angles between frame vectors in [40, 140] degrees, Z_ONLY axes at least 0.05 from the switch, chiral triple products above 0.2,
    every fractional component of a frame vector at least 0.05 away from +-0.5.  Then `frame_atoms`, `local_quadrupoles` and
    `quadrupole_grads` rolled by one row: each must move the restatement by 100 x the widest bar of the sweep, 1e-6 max|ref| (+ 1e-14).
    A rolled `frame_atoms` makes some atoms name themselves (non-finite values there): the figure is taken over the finite entries and
    the number of non-finite ones is printed."""
    c = L.frames(batch)
    t = torch.as_tensor
    cond = L.frame_conditions(t(c["pos"]), t(c["atoms"]), t(c["kinds"]), t(c["cell"]), None if c["batch_idx"] is None else t(c["batch_idx"]))
    assert 0.9 <= cond["bond"][0] and cond["bond"][1] <= 1.6 and 40.0 <= cond["angle"][0] and cond["angle"][1] <= 140.0, cond
    assert cond["z_only"] > 0.05 and cond["chiral"] > 0.2 and cond["image"] <= 0.45, cond
    assert sorted(set(c["kinds"].tolist())) == list(range(6))
    chiral = (c["kinds"] == 2) & (c["atoms"][:, 2] >= 0)
    assert chiral.any() and ((c["kinds"] == 2) & ~chiral).any(), "Z_THEN_X with and without a y atom"
    ref = L.frames_reference(batch)
    bars = {k: 1e-6 * np.abs(ref[k]).max() + 1e-14 for k in L.FR_NAMES}
    worst, lost = {}, 0
    for arg in ("atoms", "quad", "w_q"):
        moved = L.frames_reference(batch, **{arg: _roll(c[arg])})
        finite = {k: np.isfinite(moved[k]) for k in L.FR_NAMES}
        lost = max(lost, sum(int((~m).sum()) for m in finite.values()))
        worst[arg] = max(_ratio(moved[k][finite[k]], ref[k][finite[k]], bars[k]) for k in L.FR_NAMES if finite[k].any())
    print(f"[sensitivity frames {'batch' if batch else 'single'}] {cond}; largest |moved - ref| / bar: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items())
          + f"; non-finite entries under rolled frame_atoms: {lost}")
    assert all(v >= FACTOR for v in worst.values()), worst
