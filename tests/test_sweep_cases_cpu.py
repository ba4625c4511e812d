"""The conditions every case of tests/sweep_cases.py must meet before it is worth a GPU run, checked without a GPU from the float64
restatements alone: the margin of every cutoff, the lifting rule and the float32 model of the three-body cases, the counts that make a rung
sit on its boundary, the separation of every variant from its default, the coverage of the twelve seeds of each op, a bound on the cost,
and the sensitivity of the reference-side numbers to four faults a kernel could have (DESIGN.md section 3.18 has the table).  Last section:
the conditions of the cluster, pair-scale and local-frame sweeps of tests/test_sweep_cluster_frames_gpu.py."""
import os
import re
import time

import numpy as np
import pytest
import torch

from tests import atm_reference as A
from tests import d4_atm_cases as K3
from tests import d4_atm_reference as R3
from tests import dipole_reference as DR
from tests import quadrupole_reference as XR
from tests import sweep_cases as W
from tests import thole_reference as TR

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nvalchemi-toolkit-ops_amd", "csrc")


def _define(header, name):
    with open(os.path.join(CSRC, header)) as f:
        return int(re.search(rf"^#define {name}\s+(\d+)", f.read(), re.M).group(1))


def _visible_species(c):
    """Distinct species the kernels treat as real: inside the tables and, for the D4 ops, with references."""
    z = c["z"]
    ok = (z > 0) & (z <= W.Z_MAX)
    if c["op"] in W.D4_OPS:
        ok &= W.R.valid_atoms(z, c["tables"])
    return len(np.unique(z[ok]))


def _float32_model(op, r64, r32, what):
    """The restatement's float32 deviation at the case's s9 stays below `dftd3`'s bar (tests/test_d4_atm_reference_cpu.py's check)."""
    for k in ("energy", "forces", "virial"):
        if r64[k] is None:
            continue
        dev = np.abs(r32[k] - r64[k])
        bar = W.d3_bar(r64[k], k)
        print(f"{what:32s} {k:7s} max|ref| {np.abs(r64[k]).max():.3e}  scaled fp32 deviation {dev.max():.3e}  worst dev/bar {(dev / bar).max():.3f}")
        assert (dev <= bar).all(), (what, k)


def _lifting(kind, op, key):
    unit, _ = W.unit_references(kind, op, key)
    s9 = W.s9_of(kind, op, key)
    assert np.log10(s9) == round(np.log10(s9)) and K3.lifted(unit, s9), "a power of ten that lifts energy, forces and virial to 500 bars"
    assert s9 == 1.0 or not K3.lifted(unit, s9 / 10.0), "and the smallest one"


# ---- the constants the cases are built around ----------------------------------------------------------------------------------------------

def test_tile_sizes_and_species_thresholds_are_the_kernels():
    assert W.TILES == {"dftd4_atm": _define("d4_atm.h", "D4_ATM_TILE"), "dftd3_atm": _define("d3_atm.h", "D3_ATM_TILE"),
                       "dftd3_zero_atm": _define("d3_atm.h", "D3_ATM_TILE")} and (W.TILES["dftd4_atm"], W.TILES["dftd3_atm"]) == (288, 320)
    lds_s, slots = _define("d3_atm.h", "D3_ATM_LDS_S"), _define("d4.hip", "D4_SLOTS")
    assert {lds_s, lds_s + 1, slots, slots + 1} <= set(W.SPECIES_COUNTS)
    assert W.tile_rungs("dftd4_atm") == (255, 256, 257, 288, 289, 576) and W.tile_rungs("dftd3_atm") == (255, 256, 257, 320, 321, 640)
    assert W.tile_rungs("dftd3_zero_atm") == (320, 321)


# ---- sweep seeds ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", W.SEEDS)
@pytest.mark.parametrize("op", W.OPS)
def test_sweep_seed_meets_its_conditions(op, seed):
    c = W.case(op, seed)
    r64, r32 = W.references("sweep", op, seed)
    n = len(c["pos"])
    print(f"{op} {seed}: sizes {c['sizes']}, {'periodic' if c['cell'] is not None else 'free'}, {c['pos'].dtype}, species {_visible_species(c)}, "
          f"padding {c['padding']}, rc {c['rc']:.4f}, margins {({k: f'{v:.1e}' for k, v in c['margins'].items()})}, widest row {c['widest']}, s9 {c.get('s9')}")
    assert all(v >= W.MARGIN for v in c["margins"].values()), c["margins"]
    assert n == sum(c["sizes"]) <= 70 and 1 <= len(c["sizes"]) <= 3 and set(c["sizes"]) <= set(W.SIZES)
    assert _visible_species(c) == W.SPECIES_BY_SEED[seed]
    assert c["widest"] == c["counts"].max() > 0 and c["lists"]["pad"] % 2 == 1 and 1 <= c["lists"]["pad"] <= 9
    if c["cell"] is not None:
        bi = np.zeros(n, np.int64) if c["batch_idx"] is None else c["batch_idx"]
        for s, cell in enumerate(c["cell"]):
            short = W.heights(cell).min() < c["rc"]
            assert short == (s == c["short_system"]), "one cell shorter than the list cutoff where the seed says so, no other"
            if short:
                i, j, sh = A.enumerate_pairs(c["pos"][bi == s], cell, c["rc"])
                assert ((i == j) & (np.abs(sh).sum(1) > 0)).any(), "rows of a short cell hold the atom's own images"
    if op in W.THREE_BODY:
        assert c["rc3"] < c["rc"] and r64["triples"] > 0
        _lifting("sweep", op, seed)
        _float32_model(op, r64, r32, f"{op} {seed}")
    assert r64.get("triples", 0) <= 100_000, "cost: the restatement of a sweep case stays far below a second"
    # what the GPU module requires to be exactly zero is exactly zero in the restatement
    if c["padding"] in ("z0", "beyond") or (c["padding"] == "dead" and op in W.D4_OPS):
        assert not r64["forces"][c["padding_atom"]].any() and np.abs(r64["forces"]).max() > 0


@pytest.mark.parametrize("op", W.OPS)
def test_twelve_seeds_cover_what_they_are_meant_to(op):
    cases = [W.case(op, s) for s in W.SEEDS]
    for k in W.DRAWN[op]:
        values = {c["model"][k] for c in cases}
        assert len(values) >= (2 if k in W.TWO_VALUED else 3), (k, values)  # (beta is drawn from {0, 0.05})
        assert not all(c["model"][k] == W.DEFAULTS[op][k] for c in cases)
    assert all(any(c["model"][k] != W.DEFAULTS[op][k] for k in W.DRAWN[op]) for c in cases), "never all at their defaults"
    if "s8" in W.DRAWN[op]:
        assert sum(c["model"]["s8"] == 0.0 for c in cases) == 1
    if "alpha" in W.DRAWN[op]:
        assert {c["model"]["alpha"] for c in cases} == set(W.ALPHAS)
    if "beta" in W.DRAWN[op]:
        assert {c["model"]["beta"] for c in cases} == {0.0, 0.05}
    if op == "dftd3_zero":
        assert any(c["model"]["s5_off"] < 1e9 for c in cases) and any(c["model"]["s5_off"] > 1e9 for c in cases)
    if op in W.D4_OPS:
        assert any(c["model"]["cn_cutoff"] is not None for c in cases) and any(c["model"]["cn_cutoff"] is None for c in cases)
    assert {_visible_species(c) for c in cases} == set(W.SPECIES_COUNTS)
    assert {c["pos"].dtype for c in cases} == {np.dtype(np.float32), np.dtype(np.float64)}
    assert {c["padding"] for c in cases} == {None, "z0", "beyond", "dead"}
    periodic = [c for c in cases if c["cell"] is not None]
    assert len(periodic) == 8 and sum(c["short_system"] is not None for c in periodic) == 3
    assert any(c["cell"] is not None and len(c["sizes"]) > 1 and c["short_system"] is not None for c in cases), "a short cell next to ordinary ones"
    assert any(1 in c["sizes"] for c in cases) and any(2 in c["sizes"] for c in cases) and any(len(c["sizes"]) == 1 for c in cases)
    for key in ("int64", "foreign_fill", "permuted"):
        assert {c["lists"][key] for c in cases} == {False, True}, key
    assert len({c["lists"]["pad"] for c in cases}) >= 3


# ---- ladders --------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", W.LANE_RUNGS)
@pytest.mark.parametrize("op", W.LANE_OPS)
def test_lane_rung_rows_sit_on_the_trip_boundary(op, name):
    c = W.ladder_case(op, name)
    n = len(c["pos"])
    kept, _, _, margin = A.kept_and_triples(c["pos"], c["rc"])
    assert n == int(name[1:]) and (kept == n - 1).all() and (c["counts"] == n - 1).all() and margin > W.MARGIN
    assert n - 1 in (63, 64, 65, 128)
    r64, _ = W.references("ladder", op, name)
    assert r64["energy"][0] < 0.0


@pytest.mark.parametrize("op,m", [(op, m) for op in W.TILES for m in W.tile_rungs(op)])
def test_tile_rung_counts_reach_the_boundary(op, m):
    c = W.ladder_case(op, f"m{m}")
    tile = W.TILES[op]
    kept, pairs0, triples, margin = A.kept_and_triples(c["pos"], c["rc3"])
    r64, r32 = W.references("ladder", op, f"m{m}")
    print(f"{op} m{m}: rc3 {c['rc3']:.4f}, margin {margin:.2e}, centre keeps {kept[0]}, the others at most {kept[1:].max()}, pairs at the centre {pairs0}, "
          f"triples {triples}, s9 {c['s9']}")
    assert kept[0] == m and kept[1:].max() < tile and margin > W.MARGIN and c["margins"]["three_body"] == pytest.approx(margin)
    assert (c["counts"] == m).all() and r64["triples"] == triples and pairs0 > 0
    assert triples <= 2_200_000, "cost: the two-tile rungs are the most expensive restatements of the suite"
    _lifting("ladder", op, f"m{m}")
    _float32_model(op, r64, r32, f"{op} m{m}")


# ---- variants -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("op", tuple(W.VARIANTS))
def test_variant_base_meets_the_conditions(op):
    c = W.variant_case(op, "default")
    assert all(v >= W.MARGIN for v in c["margins"].values()), c["margins"]
    assert c["model"] == W.DEFAULTS[op]
    if op in W.THREE_BODY:
        _lifting("variant", op, "default")


@pytest.mark.parametrize("op,name", [(op, name) for op in W.VARIANTS for name in W.variant_names(op)])
def test_variant_separates_from_its_default(op, name):
    c = W.variant_case(op, name)
    moved = [k for k in c["model"] if c["model"][k] != W.DEFAULTS[op][k]]
    assert len(moved) == 1 and name.startswith(moved[0] + "=")
    sep = W.separation(op, name)
    print(f"{op} {name}: float64 references apart by (bars) {({k: round(v, 1) for k, v in sep.items()})}")
    assert max(sep.values()) > W.SEPARATION
    if op in W.THREE_BODY:
        assert c["s9"] == W.variant_case(op, "default")["s9"]
        _float32_model(op, *W.references("variant", op, name), f"{op} {name}")


# ---- what a faulty kernel would do to the numbers the GPU tests compare ----------------------------------------------------------------------------

def _bars_apart(c, r64, r32, wrong, keys):
    return {k: float((np.abs(wrong[k] - r64[k]) / W.bar(r64, r32, k)).max()) for k in keys if r64[k] is not None}


def _scaled(c, **override):
    return K3._scaled(W.evaluate(c, **override), c.get("s9", 1.0))


def test_fault_sensitivity_of_the_reference_side_numbers():
    """Each fault is put into the RESTATEMENT (never into the product) and the distance to the correct reference is measured in the bars
    of the test that would see it: at least 100 in the named variant; the sweep figures are printed next to it."""
    out = {}
    # alpha fixed at 16 (the copy of the per-triple arithmetic in csrc/d4_atm.h): dftd4_atm alpha = 14 and 13.5, and the sweep seeds off 16
    for name in ("alpha=14", "alpha=13.5"):
        out[f"alpha fixed at 16: variant dftd4_atm {name}"] = max(W.separation("dftd4_atm", name).values())
    # wf fixed at 6
    for op in W.D4_OPS:
        out[f"wf fixed at 6: variant {op} wf=4.5"] = max(W.separation(op, "wf=4.5").values())
    for what, op, override in (("alpha fixed at 16", "dftd4_atm", dict(alpha=16.0)), ("alpha fixed at 16", "dftd3_atm", dict(alpha=16.0)),
                               ("wf fixed at 6", "dftd4", dict(wf=6.0)), ("wf fixed at 6", "dftd4_atm", dict(wf=6.0))):
        seen = []
        for seed in W.SEEDS:
            c = W.case(op, seed)
            if all(c["model"][k] == v for k, v in override.items()):
                continue
            r64, r32 = W.references("sweep", op, seed)
            seen.append(max(_bars_apart(c, r64, r32, _scaled(c, **override), W.OUTPUTS[op]).values()))
        out[f"{what}: sweep {op}, {sum(v >= 100 for v in seen)} of {len(seen)} seeds above 100 bars, smallest / median"] = (min(seen), float(np.median(seen)))
        assert sum(v >= 100 for v in seen) >= len(seen) // 2
    # s6 used in the energy and dropped from the force: the forces are those of s6 = 1
    c = W.variant_case("dftd4", "s6=0.8")
    r64, r32 = W.references("variant", "dftd4", "s6=0.8")
    out["s6 dropped from the force: variant dftd4 s6=0.8 (forces, virial)"] = min(_bars_apart(c, r64, r32, _scaled(c, s6=1.0), ("forces", "virial")).values())
    seen = []
    for seed in W.SEEDS:
        c = W.case("dftd4", seed)
        r64, r32 = W.references("sweep", "dftd4", seed)
        seen.append(_bars_apart(c, r64, r32, _scaled(c, s6=1.0), ("forces",))["forces"])
    out[f"s6 dropped from the force: sweep dftd4 forces, {sum(v >= 100 for v in seen)} of 12 seeds above 100 bars, smallest / median"] = (min(seen), float(np.median(seen)))
    # record TILE - 1 of a full tile not paired: on the rung m = tile the centre's last kept entry is atom m; without the triples (0, j, m)
    op, tile = "dftd4_atm", W.TILES["dftd4_atm"]
    c = W.ladder_case(op, f"m{tile}")
    r64, r32 = W.references("ladder", op, f"m{tile}")
    mo = c["model"]
    kw = dict(three_body_cutoff=c["rc3"], s9=c["s9"], alpha=mo["alpha"], wf=mo["wf"], ga=mo["ga"], gc=mo["gc"], k_cn=mo["k_cn"])
    full = R3.reference(c["pos"], c["z"], c["tables"], mo["a1"], mo["a2"], c["rc"], **kw)
    li, lj, ls, inside, vp, vq = full["topology"]
    ti, tj = li[inside], lj[inside]
    dropped = (ti[vp] == 0) & (tj[vq] == tile)  # (free system: centre < j < k, so atom m can only be k)
    less = R3.reference(c["pos"], c["z"], c["tables"], mo["a1"], mo["a2"], c["rc"], topology=(li, lj, ls, inside, vp[~dropped], vq[~dropped]), **kw)
    assert np.array_equal(full["energy"], r64["energy"]) or np.allclose(full["energy"], r64["energy"], rtol=1e-12)
    out[f"record TILE - 1 not paired: rung dftd4_atm m{tile}, {int(dropped.sum())} of {full['triples']} triples (and as many visits at the centre)"] = \
        max(_bars_apart(c, r64, r32, less, ("energy", "forces")).values())
    assert dropped.sum() > 0
    for k, v in out.items():
        print(f"{k}: {v if isinstance(v, tuple) else round(v, 1)}")
    for k, v in out.items():
        if not isinstance(v, tuple):
            assert v >= 100.0, (k, v)


# ---- Gaussian charges and charge equilibration ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("op", W.CHARGE_OPS)
def test_charge_seeds_cover_what_they_are_meant_to(op):
    cases = [W.case(op, s) for s in W.SEEDS]
    assert {c["dtype"] for c in cases} == {"float32", "float64"}
    assert {n for c in cases for n in c["sizes"]} == set(W.CHARGE_SIZES) and {len(c["sizes"]) for c in cases} == {1, 2, 3}
    assert any(c["self_images"] for c in cases) and any(not c["self_images"] for c in cases)
    assert any((c["sigma"] == 0).any() for c in cases) and all(((c["sigma"] == 0) | ((c["sigma"] >= 0.3) & (c["sigma"] <= 0.8))).all() for c in cases)
    assert any(c["neutral"] for c in cases) and any(not c["neutral"] for c in cases)
    assert any(c["emptied_row"] is not None for c in cases)
    assert {c["pad"] % 2 for c in cases} == {1}
    if op == "gaussian_charge_correction":
        flags = [tuple(sorted(k for k, v in c["flags"].items() if v)) for c in cases]
        assert len(set(flags)) >= 6 and {c["self_energy"] for c in cases} == {False, True} and {c["background"] for c in cases} == {False, True}
    for c in cases:
        bi = c["batch_idx"]
        for s, cell in enumerate(c["cells"]):
            i, j, S = W.charge_entries(c, s)
            own = bool(((i == j) & (np.abs(S).sum(1) > 0)).any())
            assert own == (s in c["self_images"]), "self-image entries where the seed says so"
        assert len(c["pos"]) == len(bi) == sum(c["sizes"])


@pytest.mark.parametrize("name", W.LANE_RUNGS)
def test_charge_lane_rungs(name):
    c = W.ladder_case("charge_equilibration", name)
    n = len(c["pos"])
    d = np.linalg.norm(c["pos"][:, None] - c["pos"][None], axis=2)
    assert n == int(name[1:]) and d[~np.eye(n, dtype=bool)].min() > 0.5 and n - 1 in (63, 64, 65, 128)


def test_qeq_unrolled_product_rung_rows():
    """`box150` at cutoff 9.5: every row fits in 335 columns, some row exceeds 256 (more than one pass of the four unrolled trips of 64), and
    one image per direction is enough."""
    c = W.unrolled_case()
    i, j, S = W.charge_entries(c, 0)
    counts = np.bincount(i, minlength=150)
    print(f"box150 at 9.5: rows of {counts.min()} - {counts.max()} entries")
    assert counts.max() <= 335 and counts.max() > 256 and np.abs(S).max() == 1
    i2, _, _ = W.charge_entries(c, 0, images=2)
    assert len(i2) == len(i)
    assert W.UNROLLED_WIDTHS == (255, 256, 257, 335)


# ---- point dipoles --------------------------------------------------------------------------------------------------------------------------------
# The conditions of the cases of tests/test_sweep_dipoles_gpu.py.  COST: the restatement of a case is to stay below about a second; that is
# asserted through what decides it (entries, atoms x k-vectors, atoms x mesh) and the time itself is only printed, so that a loaded machine
# cannot fail the suite.  MEASURED here: 0.01 - 0.05 s per sweep seed for the explicit sum (up to 19 338 entries, 3 x 364 k-vectors), 0.03 -
# 0.3 s for one evaluation of the mesh term; the float32 mode of the mesh restatement leaves its float64 mode by at most 2.6e-6 of
# max |ref| over the twelve seeds, 3.3e-7 to 4.3e-6 on the spread / gather ladder and 2.8e-6 on the mesh of the two solve paths: all below
# half of the 1e-5 asserted.

FLOAT32_CAP = 1e-5  # of max |ref| per output: caps the float32 bar of the mesh term on the device at 4e-5


def _tt(a):
    return torch.as_tensor(np.ascontiguousarray(a))


def _antisymmetric(v):
    return float(np.linalg.norm(0.5 * (v - v.T)) / np.linalg.norm(v))


def _nontrivial(c, ref, what):
    """max |energies| > 0 (zero-dipole seeds: exactly 0 everywhere but dipole_grads, which exceed 1e-3), and a virial whose antisymmetric
    part is above 1e-6 of its norm in every system with dipoles on two atoms or more (one dipole among its own images in a cubic cell has a
    symmetric virial: there it must only be non-zero)."""
    if c["zero_dipoles"]:
        assert all(not ref[k].any() for k in ("energies", "forces", "charge_grads", "virial") if k in ref), what
        assert np.abs(ref["dipole_grads"]).max() > 1e-3, what
        return
    assert np.abs(ref["energies"]).max() > 0.0, what
    for s, v in enumerate(ref.get("virial", ())):
        dipoles = int(c["mu"][c["batch_idx"] == s].any(axis=1).sum())
        if dipoles >= 2:
            assert _antisymmetric(v) > 1e-6, (what, s)
        elif dipoles == 1:
            assert v.any(), (what, s)
        else:
            assert not v.any(), (what, s, "a system without a dipole (or without atoms) has an exactly zero virial row")


def _geometry_of_a_dipole_seed(c, seed):
    n = len(c["pos"])
    assert n == sum(c["sizes"]) == len(c["q"]) == len(c["mu"]) == len(c["batch_idx"]) == len(c["weights"])
    assert 1 <= len(c["sizes"]) <= 3 and set(c["sizes"]) <= set(W.CHARGE_SIZES) | {0} and max(c["sizes"]) >= 9
    assert c["min_dist"] >= W.MIN_CONTACT == 1.0 and c["min_dist"] == W.entry_distances(c).min()
    assert 6.0 <= c["cutoff"] <= 7.0 and ((c["alpha"] >= 0.3) & (c["alpha"] <= 0.45)).all() and len(c["alpha"]) == len(c["sizes"]) == len(c["cells"])
    assert c["dtype"] == ("float64", "float32")[seed % 2] and c["pad"] % 2 == 1 and 3 <= c["pad"] <= 9
    for s, cell in enumerate(c["cells"]):
        small = c["sizes"][s] in (0, 1, 9)
        box = float(cell[0, 0])
        assert box == (W._BOX[c["sizes"][s]] if not small else (5.0 if seed % 3 == 0 else 14.0))
        i, j, S = W.charge_entries(c, s)
        assert bool(((i == j) & (np.abs(S).sum(1) > 0)).any()) == (s in c["self_images"]) == (small and seed % 3 == 0 and c["sizes"][s] > 0)
    i, j, S = W.stored_entries(c)
    row = c["emptied_row"]
    assert not (i == row).any() and not (j == row).any() and len(i) < len(c["entries"][0]), "one row emptied from both ends: the list stays full"
    pairs = set(zip(i.tolist(), j.tolist(), map(tuple, S.tolist())))
    assert all((b, a, (-s[0], -s[1], -s[2])) in pairs for a, b, s in list(pairs)[:2000]), "a full (symmetric) list"
    assert c["zero_dipoles"] == (seed in W.ZERO_DIPOLE_SEEDS) == (not c["mu"].any())
    zero_rows = int((~c["mu"].any(axis=1)).sum())
    assert c["zero_dipoles"] or 1 <= zero_rows <= 3, "a few exact-zero rows"
    if seed in W.INTERLEAVED_SEEDS:
        p = W.interleaved(c)
        assert len(c["sizes"]) >= 2 and (np.diff(p["batch_idx"]) < 0).any() and sorted(c["perm"].tolist()) == list(range(n))
        assert np.array_equal(p["pos"], c["pos"][c["perm"]]) and np.isclose(W.entry_distances(p).min(), c["min_dist"], rtol=1e-12, atol=0.0)
        assert np.array_equal(np.sort(W.entry_distances(p)), np.sort(W.entry_distances(c)))
    else:
        assert c["perm"] is None
    if seed in W.EMPTY_SYSTEM_SEEDS:
        assert len(c["sizes"]) == 3 and c["sizes"][1] == 0 and set(c["batch_idx"].tolist()) == {0, 2} and c["cells"].shape == (3, 3, 3) and c["empty_system"] == 1
    else:
        assert 0 not in c["sizes"] and c["empty_system"] is None


def test_dipole_constants_are_the_kernels():
    with open(os.path.join(CSRC, "pme.hip")) as f:
        lanes = int(re.search(r"^#define PG_LANES\s+(\d+)", f.read(), re.M).group(1))
    assert W.PG_ATOMS == 256 // lanes == 32
    assert [W.spread_atoms_per_block(o) for o in W.PME_ORDERS] == [16, 10, 7]
    assert W.spread_rungs(4) == (15, 16, 17, 31, 32, 33) and W.spread_rungs(5) == (9, 10, 11, 20, 31, 32, 33) and W.spread_rungs(6) == (6, 7, 8, 14, 31, 32, 33)
    assert W.LANE_RUNGS == ("n64", "n65", "n66", "n129") and W.K_RUNGS == (63, 64, 65, 255, 256, 257, 513) and W.ATOM_RUNGS == (255, 256, 257, 1)
    assert W.SPREAD_MESH == (9, 10, 11) and W.BIG_MESH == (40, 36, 96) and 40 * 36 * (96 // 2 + 1) > 256 * 256


@pytest.mark.parametrize("seed", W.SEEDS)
def test_ewald_dipole_seed_meets_its_conditions(seed):
    c = W.dipole_case("sweep", ("ewald_dipole", seed))
    _geometry_of_a_dipole_seed(c, seed)
    pos, q, mu, cells, alpha, bi = W.dipole_tensors(c)
    kv = W.dipole_k_vectors(c)
    ent = tuple(_tt(e) for e in W.stored_entries(c))
    assert len(ent[0]) <= 40_000 and len(pos) * kv.shape[-2] <= 200_000, "cost: the restatement of a sweep case stays far below a second"
    t0 = time.perf_counter()
    ref = DR.evaluate(pos, q, mu, cells, alpha, ent, kv, batch_idx=bi)
    took = time.perf_counter() - t0
    print(f"ewald_dipole {seed}: sizes {c['sizes']} {c['dtype']}, {len(ent[0])} entries, widest row {c['widest']}, K {kv.shape[-2]}, closest contact {c['min_dist']:.4f}, "
          f"own images in {sorted(c['self_images'])}, max |E| {np.abs(ref['energies']).max():.3e}, restatement {took:.2f} s")
    _nontrivial(c, ref, f"ewald_dipole {seed}")
    if seed in W.INTERLEAVED_SEEDS:  # the real-space half on the interleaved batch is the sorted one's, atom by atom
        p = W.interleaved(c)
        a = DR.evaluate(*W.dipole_tensors(p)[:5], tuple(_tt(e) for e in W.stored_entries(p)), None, batch_idx=_tt(p["batch_idx"]))
        b = DR.evaluate(pos, q, mu, cells, alpha, ent, None, batch_idx=bi)
        assert np.abs(a["energies"] - b["energies"][c["perm"]]).max() <= 1e-12 * np.abs(b["energies"]).max()
        assert np.abs(a["virial"] - b["virial"]).max() <= 1e-12 * np.abs(b["virial"]).max()


@pytest.mark.parametrize("seed", W.SEEDS)
def test_pme_dipole_seed_meets_its_conditions(seed):
    c = W.dipole_case("sweep", ("pme_dipole", seed))
    _geometry_of_a_dipole_seed(c, seed)
    order, mesh = c["order"], c["mesh"]
    assert order == W.PME_ORDERS[seed % 3] and set(mesh) <= set(W.mesh_choices(order)) and min(mesh) >= order
    assert len(c["pos"]) * max(mesh) <= 10_000 and mesh[0] * mesh[1] * mesh[2] <= 4096, "cost: dense weights and one small mesh per system"
    t0 = time.perf_counter()
    ref = W.pme_dipole_reference("sweep", ("pme_dipole", seed))
    took = time.perf_counter() - t0
    _nontrivial(c, ref, f"pme_dipole {seed}")
    dev = {**W.pme_float32_deviation("sweep", ("pme_dipole", seed)),
           **{"weighted " + k: v for k, v in W.pme_float32_deviation("sweep", ("pme_dipole", seed), weighted=True).items() if k != "energies"}}
    print(f"pme_dipole {seed}: sizes {c['sizes']} {c['dtype']}, order {order} mesh {mesh}, restatement {took:.2f} s, float32 mode against float64 mode: "
          + ", ".join(f"{k} {v:.1e}" for k, v in dev.items()))
    assert max(dev.values()) <= FLOAT32_CAP, dev
    if mesh[2] % 2 == 1 and not c["zero_dipoles"]:
        # the plane k = (nz - 1) / 2 has Hermitian weight 2 on an odd axis; a kernel that gives it 1 must be seen by the virial comparison
        plane = np.abs(W.hermitian_plane_virial("sweep", ("pme_dipole", seed))).max() / np.abs(ref["virial"]).max()
        bar = 1e-10 if c["dtype"] == "float64" else 4.0 * dev["virial"]
        print(f"pme_dipole {seed}: the last plane of the odd axis holds {plane:.2e} of max |virial|: {plane / bar:.3g} bars")
        assert plane >= 100.0 * bar, (plane, bar)
    if seed in W.INTERLEAVED_SEEDS:  # the restatement needs no contiguous systems
        p = W.interleaved(c)
        pp, pq, pm, pc, pa, _ = W.dipole_tensors(p)
        a = W.PR.evaluate(pp, pq, pm, pc, pa, mesh, order, batch_idx=_tt(p["batch_idx"]))
        assert np.abs(a["energies"] - ref["energies"][c["perm"]]).max() <= 1e-12 * np.abs(ref["energies"]).max()
        assert np.abs(a["virial"] - ref["virial"]).max() <= 1e-12 * np.abs(ref["virial"]).max()


@pytest.mark.parametrize("op", W.DIPOLE_OPS)
def test_dipole_seeds_cover_what_they_are_meant_to(op):
    cases = [W.dipole_case("sweep", (op, s)) for s in W.SEEDS]
    assert {c["dtype"] for c in cases} == {"float32", "float64"}
    assert {n for c in cases for n in c["sizes"]} == set(W.CHARGE_SIZES) | {0} and {len(c["sizes"]) for c in cases} == {1, 2, 3}
    assert any(c["self_images"] for c in cases) and any(not c["self_images"] for c in cases)
    assert any(c["neutral"] for c in cases) and any(not c["neutral"] for c in cases)
    assert sum(c["zero_dipoles"] for c in cases) == 3 == len(W.SEEDS) // 4 and {c["dtype"] for c in cases if c["zero_dipoles"]} == {"float32", "float64"}
    assert sum(c["perm"] is not None for c in cases) == 2 and sum(c["empty_system"] is not None for c in cases) == 2
    assert all(c["dtype"] == "float64" for c in cases if c["perm"] is not None)
    assert not set(W.ZERO_DIPOLE_SEEDS) & set(W.INTERLEAVED_SEEDS + W.EMPTY_SYSTEM_SEEDS) and not set(W.INTERLEAVED_SEEDS) & set(W.EMPTY_SYSTEM_SEEDS)
    assert any(np.allclose(c["cells"][s], np.diag(np.diag(c["cells"][s]))) for c in cases for s in range(len(c["sizes"])))
    assert any(c["cells"][s][1, 0] != 0 for c in cases for s in range(len(c["sizes"])))
    assert len({c["pad"] for c in cases}) >= 3
    if op == "ewald_dipole":
        flags = [tuple(sorted(k for k, v in c["flags"].items() if v)) for c in cases]
        assert len(set(flags)) >= 6 and {c["autograd"] for c in cases} == {False, True}
        assert all(any(c["flags"][k] for c in cases if not c["zero_dipoles"]) for k in W.DIPOLE_FLAGS)
    else:
        assert [c["order"] for c in cases] == [4, 5, 6] * 4
        odd = [c["seed"] for c in cases if c["mesh"][2] % 2 == 1]
        equal = [c["seed"] for c in cases if c["order"] in c["mesh"]]
        print(f"pme_dipole: odd nz in seeds {odd}, a dimension equal to the order in seeds {equal}, meshes {[c['mesh'] for c in cases]}")
        assert len(odd) >= 4 and len(equal) >= 2
        assert any(not c["zero_dipoles"] for c in cases if c["seed"] in odd) and any(c["mesh"][2] % 2 == 0 and not c["zero_dipoles"] for c in cases)


@pytest.mark.parametrize("name", W.LANE_RUNGS)
def test_dipole_row_rung(name):
    c = W.dipole_case("row", name)
    n = len(c["pos"])
    i, j, S = c["entries"]
    d = np.linalg.norm(c["pos"][:, None] - c["pos"][None], axis=2)
    off = d[~np.eye(n, dtype=bool)]
    assert n == int(name[1:]) and n - 1 in (63, 64, 65, 128) and (np.bincount(i, minlength=n) == n - 1).all() and not S.any() and c["widest"] == n - 1
    assert off.min() >= W.MIN_CONTACT and c["min_dist"] == pytest.approx(off.min()) and c["diameter"] == pytest.approx(off.max())
    assert np.array_equal(c["cells"][0], np.eye(3) * 4.0 * c["diameter"]), "a cubic cell four cluster diameters wide: no image inside any cutoff"
    pos, q, mu, cells, alpha, _ = W.dipole_tensors(c)
    ref = DR.evaluate(pos, q, mu, cells, alpha, tuple(_tt(e) for e in c["entries"]), None)
    _nontrivial(c, ref, name)


def test_dipole_k_ladder_set_and_atom_ladder_batch():
    c = W.dipole_case("k", None)
    kv = W.dipole_k_vectors(c)
    assert c["sizes"] == (60,) and c["cells"][0][0, 0] == 9.0 and kv.dim() == 2 and kv.shape[0] >= max(W.K_RUNGS) == 513
    g = W.green_weights(c, kv[:513].numpy())
    print(f"K ladder: smallest / largest Green weight of the first 513 vectors {g.min() / g.max():.1e}")
    assert g.min() >= 1e-7 * g.max(), "every vector of every rung weighs: one skipped vector moves the sums by 1e4 bars or more"
    pos, q, mu, cells, alpha, _ = W.dipole_tensors(c)
    for k in W.K_RUNGS:
        _nontrivial(c, DR.evaluate(pos, q, mu, cells, alpha, None, kv[:k]), f"K = {k}")
    a = W.dipole_case("atoms", None)
    ka = W.dipole_k_vectors(a)
    print(f"K ladder: the set holds {kv.shape[0]} vectors; atom ladder: {ka.shape[1]} vectors per system")
    assert a["sizes"] == (255, 256, 257, 1) and min(float(cl[0, 0]) for cl in a["cells"]) >= 14.0 and ka.shape[0] == 4 and 60 <= ka.shape[1] <= 70
    assert np.array_equal(a["batch_idx"], np.repeat(np.arange(4), a["sizes"]))
    pos, q, mu, cells, alpha, bi = W.dipole_tensors(a)
    _nontrivial(a, DR.evaluate(pos, q, mu, cells, alpha, None, ka, batch_idx=bi), "atom ladder")


@pytest.mark.parametrize("order", W.PME_ORDERS)
def test_pme_dipole_ladders_float32_mode(order):
    """The spread / gather ladder of this order, the mesh of tests/test_sweep_dipoles_gpu.py::test_both_solve_paths (the system of
    tests/test_pme_dipole_gpu.py) and, at order 5, the big mesh: non-trivial, and the float32 mode within the cap."""
    from tests import test_pme_dipole_gpu as TP

    worst, lowest = 0.0, 1.0
    for n in W.spread_rungs(order):
        c = W.dipole_case("spread", (order, n))
        assert len(c["pos"]) == n and c["mesh"] == W.SPREAD_MESH and c["order"] == order
        frac = c["pos"] @ np.linalg.inv(c["cells"][0])
        assert n < 9 or ((frac < 0).any() and (frac > 1).any()), "atoms outside the cell: stencils cross the faces"
        _nontrivial(c, W.pme_dipole_reference("spread", (order, n)), f"order {order} N {n}")
        dev = {**W.pme_float32_deviation("spread", (order, n)), **{"w " + k: v for k, v in W.pme_float32_deviation("spread", (order, n), weighted=True).items()}}
        worst, lowest = max(worst, max(dev.values())), min(lowest, min(dev.values()))
        assert max(dev.values()) <= FLOAT32_CAP, (n, dev)
    r64, r32 = TP._reference(order, TP.MESH), TP._reference(order, TP.MESH, torch.float32)
    solve = max(float(np.abs(r32[k] - r64[k]).max() / np.abs(r64[k]).max()) for k in r64)
    print(f"order {order}: float32 mode against float64 mode, spread / gather ladder {lowest:.1e} to {worst:.1e}, mesh {TP.MESH} of the two solve paths {solve:.1e}")
    assert solve <= FLOAT32_CAP
    if order == 5:
        c = W.dipole_case("big", None)
        assert c["mesh"] == W.BIG_MESH and len(c["pos"]) == 12 and c["order"] == 5
        _nontrivial(c, W.pme_dipole_reference("big", None), "big mesh")


# ---- point quadrupoles and Thole damping ----------------------------------------------------------------------------------------------------------
# The conditions of the cases of tests/test_sweep_multipoles_gpu.py.  A seed is the dipole recipe under the operator's own BASE, so its
# geometry is held to `_geometry_of_a_dipole_seed`; what the multipole section adds is asserted here.  MEASURED here: the restatement of a
# quadrupole seed (nested autograd over up to 33 000 entries) takes 0.05 - 2 s -- the interleaved seed 4 evaluates three and takes 5 - 7 s
# in all --, that of a Thole seed below 0.1 s.


def _multipole_reference(c, entries, kv=None):
    pos, q, mu, cells, alpha, bi = W.dipole_tensors(c)
    ent = tuple(_tt(e) for e in entries)
    if "qd" in c:
        return XR.evaluate(pos, q, mu, _tt(c["qd"]), cells, alpha, ent, kv, batch_idx=bi)
    return TR.evaluate(pos, q, mu, _tt(c["polar"]), cells, W.THOLE, ent, batch_idx=bi)


@pytest.mark.parametrize("seed", W.SEEDS)
@pytest.mark.parametrize("op", W.MULTIPOLE_OPS)
def test_multipole_seed_meets_its_conditions(op, seed):
    base, c = W._dipole_sweep(op, seed), W.multipole_case("sweep", (op, seed))
    _geometry_of_a_dipole_seed(base, seed)
    n = len(c["pos"])
    for k in ("pos", "q", "batch_idx", "weights", "cells", "alpha"):
        assert np.array_equal(c[k], base[k]), k
    assert c["entries"] is base["entries"] and c["emptied_row"] == base["emptied_row"] and c["min_dist"] >= W.MIN_CONTACT
    assert W.entry_distances(c).min() >= W.MIN_CONTACT, "no contact below 1: one close pair must not decide a float32 comparison"
    assert not c["zero_dipoles"] and c["mu"].any() and 1 <= int((~c["mu"].any(axis=1)).sum()) <= 3, "dipoles on every seed"
    assert c["zero"] == (seed in W.ZERO_MULTIPOLE_SEEDS) and set(c["flags"]) == set(W.MULTIPOLE_FLAGS[op])
    if seed in W.SINGLE_FLAG_SEEDS:
        assert [k for k, v in c["flags"].items() if v] == [W.MULTIPOLE_FLAGS[op][W.SINGLE_FLAG_SEEDS.index(seed)]]
    ent = W.stored_entries(c)
    kv = W.dipole_k_vectors(c) if op == "ewald_quadrupole" else None
    assert len(ent[0]) <= 40_000 and (kv is None or n * kv.shape[-2] <= 200_000), "cost"
    t0 = time.perf_counter()
    ref = _multipole_reference(c, ent, kv)
    took = time.perf_counter() - t0
    if op == "ewald_quadrupole":
        assert c["qd"].shape == (n, 3, 3) and (not c["qd"].any()) == c["zero"]
        if c["zero"]:  # what the parity module asserts as exact zeros is exactly zero in the restatement, and the field gradient is not
            assert all(not ref[k].any() for k in ("energies", "forces", "charge_grads", "dipole_grads", "virial")) and np.abs(ref["quadrupole_grads"]).max() > 1e-3
        else:
            zero_rows = int((~c["qd"].any(axis=(1, 2))).sum())
            assert 1 <= zero_rows <= 3 and np.abs(ref["energies"]).max() > 0
            if n > 6:
                assert np.abs(c["qd"] - c["qd"].transpose(0, 2, 1)).max() > 1e-3, "a few unsymmetric rows"
    else:
        assert c["polar"].shape == (n,) and (not c["polar"].any()) == c["zero"] and c["polar"].min() >= 0.0 and c["polar"].max() <= 4.0
        if c["zero"]:
            assert all(not v.any() for v in ref.values()), "every atom non-polarisable: every output exactly 0"
        else:
            E, _ = W.thole_exponents(c, ent)
            assert (n <= 3 or (c["polar"] == 0).any()) and np.abs(ref["energies"]).max() > 0
            if max(c["sizes"]) >= 60:
                assert (E < 1.0).any() and (E >= W.THOLE_EXIT).any(), "both sides of the exit at E = 50"
    if seed in W.INTERLEAVED_SEEDS:  # the real-space sums on the interleaved batch are the sorted ones, atom by atom
        p = W.multipole_interleaved(c)
        a = _multipole_reference(p, W.stored_entries(p))
        b = _multipole_reference(c, ent)
        assert np.abs(a["energies"] - b["energies"][c["perm"]]).max() <= 1e-12 * np.abs(b["energies"]).max()
        assert np.abs(a["virial"] - b["virial"]).max() <= 1e-12 * np.abs(b["virial"]).max()
    print(f"{op} {seed}: sizes {c['sizes']} {c['dtype']}, {len(ent[0])} entries, widest row {c['widest']}, flags {[k[8:] for k, v in c['flags'].items() if v]}, "
          f"max |E| {np.abs(ref['energies']).max():.3e}, restatement {took:.2f} s")


@pytest.mark.parametrize("op", W.MULTIPOLE_OPS)
def test_multipole_seeds_cover_what_they_are_meant_to(op):
    cases = [W.multipole_case("sweep", (op, s)) for s in W.SEEDS]
    assert {c["dtype"] for c in cases} == {"float32", "float64"} and all(c["dtype"] == ("float64", "float32")[c["seed"] % 2] for c in cases)
    assert {n for c in cases for n in c["sizes"]} == set(W.CHARGE_SIZES) | {0} and {len(c["sizes"]) for c in cases} == {1, 2, 3}
    assert any(c["self_images"] for c in cases) and any(not c["self_images"] for c in cases)
    assert any(np.allclose(c["cells"][s], np.diag(np.diag(c["cells"][s]))) for c in cases for s in range(len(c["sizes"])))
    assert any(c["cells"][s][1, 0] != 0 for c in cases for s in range(len(c["sizes"])))
    assert sum(c["zero"] for c in cases) == 3 and {c["dtype"] for c in cases if c["zero"]} == {"float32", "float64"}
    assert sum(c["perm"] is not None for c in cases) == 2 and sum(c["empty_system"] is not None for c in cases) == 2
    assert all(c["dtype"] == "float64" for c in cases if c["perm"] is not None)
    designated = set(W.ZERO_MULTIPOLE_SEEDS) | set(W.INTERLEAVED_SEEDS) | set(W.EMPTY_SYSTEM_SEEDS)
    assert len(designated) == 7 and set(W.SINGLE_FLAG_SEEDS) == set(W.SEEDS) - designated
    alone = [tuple(k for k, v in c["flags"].items() if v) for c in cases if not c["zero"]]
    assert all((k,) in alone for k in W.MULTIPOLE_FLAGS[op]), "every flag alone at least once, on a seed with quadrupoles / polarisabilities"
    assert len(set(alone)) >= 7 and {c["autograd"] for c in cases} == {False, True}
    assert max(c["widest"] for c in cases) > 64 and sum(c["widest"] > 64 for c in cases) >= 6, "rows longer than one trip of the wave"


def test_multipole_ladders():
    a = W.multipole_case("atoms")
    assert a["sizes"] == W.ATOM_RUNGS == (255, 256, 257, 1) and a["qd"].shape == (769, 3, 3) and np.array_equal(a["pos"], W.dipole_atom_case()["pos"])
    ka = W.dipole_k_vectors(a)
    assert ka.shape[0] == 4 and 60 <= ka.shape[1] <= 70
    pos, q, mu, cells, alpha, bi = W.dipole_tensors(a)
    ref = XR.evaluate(pos, q, mu, _tt(a["qd"]), cells, alpha, None, ka, batch_idx=bi)
    assert all(np.abs(ref["energies"][bi.numpy() == s]).max() > 0 for s in range(4)) and all(_antisymmetric(v) > 1e-6 for v in ref["virial"][:3])
    c = W.multipole_case("no_shifts")
    i, j, S = c["entries"]
    assert len(c["pos"]) == 65 and (np.bincount(i, minlength=65) == 64).all() and not S.any() and c["min_dist"] >= W.MIN_CONTACT
    assert np.array_equal(c["cells"][0], np.eye(3) * 4.0 * c["diameter"]), "no image inside any cutoff: zero shifts are the whole list"
    s = W.multipole_case("shared_k")
    assert s["sizes"] == (60, 9) and np.array_equal(s["cells"][0], s["cells"][1]) and s["alpha"][0] == s["alpha"][1]
    ks = W.dipole_k_vectors(s)
    assert ks.shape[0] == 2 and torch.equal(ks[0], ks[1]) and ks.shape[1] > 64, "one k set serves both systems"
    for k in (0, 1):
        p = s["pos"][s["batch_idx"] == k]
        assert (np.linalg.norm(p[:, None] - p[None], axis=-1) + 9.0 * np.eye(len(p))).min() >= W.MIN_CONTACT


@pytest.mark.parametrize("periodic", [True, False], ids=["periodic", "cluster"])
def test_thole_row_ladder_rows_straddle_the_exit(periodic):
    c = W.multipole_case("thole_rows", periodic)
    i, j, S = c["entries"]
    n = len(c["pos"])
    counts = np.bincount(i, minlength=n)
    assert tuple(counts[:len(W.THOLE_ROWS)]) == W.THOLE_ROWS == (0, 1, 63, 64, 65, 128, 129) and n == 7 + (40 if periodic else 130)
    assert (c["cells"] is None) == (not periodic) and (periodic or not S.any()) and c["min_dist"] >= W.MIN_CONTACT
    pairs = set(zip(i.tolist(), j.tolist(), map(tuple, S.tolist())))
    assert len(pairs) == len(i) and all((b, a, (-s[0], -s[1], -s[2])) in pairs for a, b, s in pairs), "distinct entries, a full (symmetric) list"
    assert (c["polar"][:7] > 0).all() and int((c["polar"] == 0).sum()) == 2
    E, rows = W.thole_exponents(c)
    inside = [int((E[rows == t] < W.THOLE_EXIT).sum()) for t in range(7)]
    beyond = [int((E[rows == t] >= W.THOLE_EXIT).sum()) for t in range(7)]
    print(f"thole row ladder ({'periodic' if periodic else 'cluster'}): entries inside / beyond the exit per ladder row {list(zip(inside, beyond))}")
    assert inside[1] == 1, "the row of one entry lies inside the exit: it contributes"
    assert all(inside[t] >= 3 and beyond[t] >= 3 for t in range(2, 7)), "every longer row has entries on both sides of E = 50"
    ref = TR.evaluate(_tt(c["pos"]), _tt(c["q"]), _tt(c["mu"]), _tt(c["polar"]), _tt(c["cells"]) if periodic else None, W.THOLE,
                      tuple(_tt(e) for e in c["entries"]))
    assert not ref["energies"][0] and all(abs(ref["energies"][t]) > 0 for t in range(1, 7))


def test_induced_idle_systems_case():
    from tests import thole_cases as TC

    c = W.induced_idle_systems_case()
    assert c["sizes"] == (27, 0, 9) and set(c["batch_idx"].tolist()) == {0, 2} and c["cells"].shape == (3, 3, 3)
    assert (c["polar"][:27] > 0).all() and not c["polar"][27:].any() and np.abs(c["q"][27:]).min() > 0
    i, j, S = c["entries"]
    assert ((i < 27) == (j < 27)).all() and (np.bincount(i, minlength=36)[27:] > 0).all(), "no entry joins two systems; the idle atoms do have neighbours"
    d = TC.dense(TC.lattice("l27"), None)
    assert float(torch.linalg.eigvalsh(d["H"]).min()) > 0 and float(d["b"].abs().max()) > 0, "system 0 has a solve to do"


# ---- point quadrupoles on the mesh -------------------------------------------------------------------------------------------------------------
# The conditions of the cases of tests/test_sweep_pme_quadrupole_gpu.py.  A seed is the dipole recipe under the operator's own BASE, so its
# geometry is held to `_geometry_of_a_dipole_seed`.  MEASURED here: one evaluation of the restatement takes 0.3 - 1.6 s on a seed (the
# seeds with 150-atom systems are the slow ones), below 0.2 s on a rung or a knot case, 1 s on the big mesh.

PMEQ_FLOAT32_CAP = 2.5e-5  # of max |ref| per output: caps the float32 bar of the quadrupole mesh term on the device at 1e-4
PMEQ_ZERO = ("energies", "forces", "charge_grads", "dipole_grads", "virial")


def _pmeq_nontrivial(c, ref, what):
    """Every compared output is non-trivial: max |.| > 0 for each, and in every system with quadrupoles on two atoms or more a virial whose
    antisymmetric part is above 1e-6 of its norm (the mesh virial is NOT symmetric; a symmetrised one must fail); zero-quadrupole seeds:
    exactly 0 everywhere but quadrupole_grads, which exceed 1e-3; a system without atoms has an exactly zero virial row."""
    if c["zero"]:
        assert all(not ref[k].any() for k in PMEQ_ZERO if k in ref), what
        assert np.abs(ref["quadrupole_grads"]).max() > 1e-3, what
        return
    for k, v in ref.items():
        assert np.abs(v).max() > 0.0, (what, k)
    for s, v in enumerate(ref.get("virial", ())):
        quadrupoles = int(c["qd"][c["batch_idx"] == s].any(axis=(1, 2)).sum())
        if quadrupoles >= 2:
            assert _antisymmetric(v) > 1e-6, (what, s)
        elif quadrupoles == 0:
            assert not v.any(), (what, s)


def _pmeq_deviation(kind, key):
    """The float32 mode against the float64 mode, forward and weighted backward, every output."""
    return {**W.pmeq_float32_deviation(kind, key), **{"weighted " + k: v for k, v in W.pmeq_float32_deviation(kind, key, weighted=True).items() if k != "energies"}}


@pytest.mark.parametrize("seed", W.SEEDS)
def test_pme_quadrupole_seed_meets_its_conditions(seed):
    base, c = W._dipole_sweep("pme_quadrupole", seed), W.pmeq_case("sweep", seed)
    _geometry_of_a_dipole_seed(base, seed)
    n = len(c["pos"])
    for k in ("pos", "q", "batch_idx", "weights", "cells", "alpha"):
        assert np.array_equal(c[k], base[k]), k
    assert c["entries"] is base["entries"] and c["emptied_row"] == base["emptied_row"]
    order, mesh = c["order"], c["mesh"]
    assert order == W.PMEQ_ORDERS[(seed // 2) % 2] and set(mesh) <= set(W.mesh_choices(order)) and min(mesh) >= order
    assert n * max(mesh) <= 10_000 and mesh[0] * mesh[1] * mesh[2] <= 4096, "cost: dense weights and one small mesh per system"
    assert c["no_dipoles"] == (seed == W.NO_DIPOLE_SEED) == (not c["mu"].any())
    if c["no_dipoles"]:
        assert sum(s > 0 for s in c["sizes"]) >= 2, "dipoles=None in a batch of at least two systems with atoms"
    else:
        assert 1 <= int((~c["mu"].any(axis=1)).sum()) <= 3, "dipoles on every other seed, a few zero rows"
    assert c["zero"] == (seed in W.ZERO_MULTIPOLE_SEEDS) == (not c["qd"].any()) and c["qd"].shape == (n, 3, 3) and set(c["flags"]) == set(W.QUADRUPOLE_FLAGS)
    if seed in W.SINGLE_FLAG_SEEDS:
        assert [k for k, v in c["flags"].items() if v] == [W.QUADRUPOLE_FLAGS[W.SINGLE_FLAG_SEEDS.index(seed)]]
    if not c["zero"]:
        assert 1 <= int((~c["qd"].any(axis=(1, 2))).sum()) <= 3, "a few atoms without a quadrupole"
        assert n <= 6 or np.abs(c["qd"] - c["qd"].transpose(0, 2, 1)).max() > 1e-3, "a few unsymmetric rows"
    t0 = time.perf_counter()
    ref = W.pme_quadrupole_reference("sweep", seed)
    took = time.perf_counter() - t0
    _pmeq_nontrivial(c, ref, f"pme_quadrupole {seed}")
    _pmeq_nontrivial(c, W.pme_quadrupole_reference("sweep", seed, "float64", True), f"pme_quadrupole {seed} weighted")
    dev = _pmeq_deviation("sweep", seed)
    print(f"pme_quadrupole {seed}: sizes {c['sizes']} {c['dtype']}, order {order} mesh {mesh}, flags {[k[8:] for k, v in c['flags'].items() if v]}, "
          f"restatement {took:.2f} s, float32 mode against float64 mode: " + ", ".join(f"{k} {v:.1e}" for k, v in dev.items()))
    if c["dtype"] == "float32" or seed == W.pmeq_batch_seed():
        assert max(dev.values()) <= PMEQ_FLOAT32_CAP, dev
    if mesh[2] % 2 == 1 and not c["zero"]:
        # the plane k = (nz - 1) / 2 has Hermitian weight 2 on an odd axis; a kernel that gives it 1 must be seen by the virial comparison
        plane = np.abs(W.pmeq_plane_virial("sweep", seed)).max() / np.abs(ref["virial"]).max()
        print(f"pme_quadrupole {seed}: the last plane of the odd axis holds {plane:.2e} of max |virial|: {plane / 1e-10:.3g} float64 bars")
        assert plane >= 100.0 * 1e-10, plane
    if seed in W.INTERLEAVED_SEEDS:  # the restatement needs no contiguous systems
        p = W.multipole_interleaved(c)
        a = W.pmeq_evaluate(p)
        assert np.abs(a["energies"] - ref["energies"][c["perm"]]).max() <= 1e-12 * np.abs(ref["energies"]).max()
        assert np.abs(a["virial"] - ref["virial"]).max() <= 1e-12 * np.abs(ref["virial"]).max()


def test_pme_quadrupole_seeds_cover_what_they_are_meant_to():
    cases = [W.pmeq_case("sweep", s) for s in W.SEEDS]
    assert all(c["dtype"] == ("float64", "float32")[c["seed"] % 2] for c in cases) and {len(c["sizes"]) for c in cases} == {1, 2, 3}
    assert [c["order"] for c in cases] == [5, 5, 6, 6] * 3 and {(c["order"], c["dtype"]) for c in cases} == {(o, d) for o in (5, 6) for d in ("float32", "float64")}
    assert sum(c["zero"] for c in cases) == 3 and {c["dtype"] for c in cases if c["zero"]} == {"float32", "float64"}
    assert sum(c["perm"] is not None for c in cases) == 2 and sum(c["empty_system"] is not None for c in cases) == 2
    assert all(c["dtype"] == "float64" and len(c["sizes"]) >= 2 for c in cases if c["perm"] is not None)
    assert W.NO_DIPOLE_SEED in W.EMPTY_SYSTEM_SEEDS and sum(c["no_dipoles"] for c in cases) == 1
    assert any(c["dtype"] == "float32" and sum(s > 0 for s in c["sizes"]) >= 2 for c in cases), "a float32 batch"
    designated = set(W.ZERO_MULTIPOLE_SEEDS) | set(W.INTERLEAVED_SEEDS) | set(W.EMPTY_SYSTEM_SEEDS)
    assert len(designated) == 7 and set(W.SINGLE_FLAG_SEEDS) == set(W.SEEDS) - designated
    alone = [tuple(k for k, v in c["flags"].items() if v) for c in cases if not c["zero"]]
    assert all((k,) in alone for k in W.QUADRUPOLE_FLAGS), "every flag alone at least once, on a seed with quadrupoles"
    assert any(np.allclose(c["cells"][s], np.diag(np.diag(c["cells"][s]))) for c in cases for s in range(len(c["sizes"])))
    assert any(c["cells"][s][1, 0] != 0 for c in cases for s in range(len(c["sizes"])))
    odd = [c["seed"] for c in cases if c["mesh"][2] % 2 == 1]
    equal = {o: [c["seed"] for c in cases if c["order"] == o and o in c["mesh"]] for o in W.PMEQ_ORDERS}
    print(f"pme_quadrupole: odd nz in seeds {odd}, an axis equal to the order in seeds {equal}, meshes {[c['mesh'] for c in cases]}, batch seed {W.pmeq_batch_seed()}")
    assert len(odd) >= 2 and sum(not cases[s]["zero"] for s in odd) >= 2, "odd nz on at least two seeds with quadrupoles (the Hermitian weight of the last plane)"
    assert all(any(not cases[s]["zero"] for s in equal[o]) for o in W.PMEQ_ORDERS), "an axis equal to the order, for each order, on a seed with quadrupoles"
    b = cases[W.pmeq_batch_seed()]
    assert len(b["sizes"]) == 3 and min(b["sizes"]) > 0 and not b["zero"] and not b["no_dipoles"] and b["perm"] is None


def test_pme_quadrupole_constants_are_the_kernels():
    with open(os.path.join(CSRC, "pme.hip")) as f:
        src = f.read()
    assert re.search(r"pme_quadrupole_spread_kernel.*?constexpr int tpa = ORDER \* ORDER, apb = 256 / tpa;", src, re.S)
    assert [W.spread_atoms_per_block(o) for o in W.PMEQ_ORDERS] == [10, 7]
    assert W.pmeq_spread_rungs(5) == (1, 9, 10, 11, 20, 31, 32, 33) and W.pmeq_spread_rungs(6) == (1, 6, 7, 8, 14, 31, 32, 33)


@pytest.mark.parametrize("order", W.PMEQ_ORDERS)
def test_pme_quadrupole_ladder_and_big_mesh(order):
    """The spread / gather ladder of this order and, at order 5, the big mesh: non-trivial, every rung within the float32 cap in every
    output.  Rung 1 (`sweep_cases.pmeq_spread_case`): within the cap in energies, charge_grads, quadrupole_grads, virial and the weighted
    charge and quadrupole gradients; forces and dipole_grads, forward and weighted, are the two exempt outputs, and each must really be over
    the cap -- an exemption that the figures do not call for fails here."""
    worst, lowest = 0.0, 1.0
    for n in W.pmeq_spread_rungs(order):
        c = W.pmeq_case("spread", (order, n))
        assert len(c["pos"]) == n and c["mesh"] == W.SPREAD_MESH and c["order"] == order and c["qd"].shape == (n, 3, 3)
        frac = c["pos"] @ np.linalg.inv(c["cells"][0])
        assert frac.min() >= -0.2 and frac.max() <= 1.2 and (n < 9 or ((frac < 0).any() and (frac > 1).any())), "atoms outside the cell: stencils cross the faces"
        t0 = time.perf_counter()
        ref = W.pme_quadrupole_reference("spread", (order, n))
        took = time.perf_counter() - t0
        assert all(np.abs(v).max() > 0 for v in ref.values()) and (n == 1 or _antisymmetric(ref["virial"][0]) > 1e-6), n
        dev = _pmeq_deviation("spread", (order, n))
        print(f"order {order} N {n}: restatement {took:.2f} s, float32 mode against float64 mode " + ", ".join(f"{k} {v:.1e}" for k, v in dev.items()))
        if n == 1:
            exempt = {k: v for k, v in dev.items() if k.replace("weighted ", "") in W.PMEQ_LONE_ATOM_EXEMPT}
            held = {k: v for k, v in dev.items() if k not in exempt}
            assert c["qd"].any() and c["mu"].any() and len(exempt) == 4 and len(held) == 6
            assert max(held.values()) <= PMEQ_FLOAT32_CAP, ("one atom alone: four outputs and their weighted gradients are within the cap", held)
            assert min(exempt.values()) > PMEQ_FLOAT32_CAP, ("one atom alone: forces and dipole_grads are exempt because they are over the cap", exempt)
            continue
        worst, lowest = max(worst, max(dev.values())), min(lowest, min(dev.values()))
        assert max(dev.values()) <= PMEQ_FLOAT32_CAP, (n, dev)
    print(f"order {order}: float32 mode against float64 mode on the spread / gather ladder from 6 atoms on {lowest:.1e} to {worst:.1e}")
    if order == 5:
        c = W.pmeq_case("big")
        assert c["mesh"] == W.BIG_MESH and len(c["pos"]) == 12 and c["order"] == 5 and np.array_equal(c["pos"], W.dipole_big_mesh_case()["pos"])
        t0 = time.perf_counter()
        ref = W.pme_quadrupole_reference("big", None)
        print(f"big mesh {W.BIG_MESH}: restatement {time.perf_counter() - t0:.2f} s")
        assert all(np.abs(v).max() > 0 for v in ref.values()) and _antisymmetric(ref["virial"][0]) > 1e-6


@pytest.mark.parametrize("order,mesh", W.PMEQ_KNOT_CASES)
def test_pme_quadrupole_knot_case(order, mesh):
    """The construction (which atoms sit on which knots), the float32 cap, and that the restatement is CONTINUOUS across the knots: moving
    every atom by +1e-7 or by -1e-7 along (1, 1, 1) moves every output by a small amount (measured: at most 5.3e-8 of its maximum) that
    shrinks tenfold with the displacement, and is the same for both signs wherever the output is differentiable at the knot (a jump at a knot
    would show as a move that does not shrink)."""
    c = W.pmeq_case("knots", (order, mesh))
    u, dims = c["mesh_coordinates"], np.array(mesh)
    assert np.array_equal(c["cells"][0], np.eye(3) * 8.0) and len(c["pos"]) == 12 and np.array_equal(c["pos"], c["pos"].astype(np.float32).astype(np.float64))
    assert u.min() >= -3.0 and (u <= dims + 3).all()
    assert np.array_equal(u[0], np.zeros(3)) and np.array_equal(u[1], dims) and np.array_equal(u[2], (-1.0, mesh[1], 0.5))
    generic = {(3, 0), (6, 1), (7, 2)}
    for i in range(12):
        for d in range(3):
            if (i, d) in generic:
                assert abs(2.0 * u[i, d] - round(2.0 * u[i, d])) > 1e-3, "a generic axis"
            elif (i, d) != (2, 2):
                assert (u[i, d] == np.floor(u[i, d])) if i < 6 else (u[i, d] - 0.5 == np.floor(u[i, d])), (i, d)
    on_mesh = c["pos"] / 8.0 * dims  # what the kernels form, in float64
    knots = np.array([[(i, d) not in generic for d in range(3)] for i in range(12)])
    assert np.abs(on_mesh - u)[knots].max() <= 4e-7
    for d in range(3):
        if mesh[d] in (8, 16):
            exact = [i for i in range(12) if (i, d) not in generic]
            assert np.array_equal(on_mesh[exact, d], u[exact, d]), "on axes of 8 and 16 points the float32 position IS the knot"
    moved = W.pmeq_translated(c)
    assert np.array_equal(moved["pos"], moved["pos"].astype(np.float32).astype(np.float64)) and np.abs(moved["pos"] - c["pos"]).max() == 24.0
    ref = W.pme_quadrupole_reference("knots", (order, mesh))
    assert all(np.abs(v).max() > 0 and np.isfinite(v).all() for v in ref.values())
    dev = _pmeq_deviation("knots", (order, mesh))
    print(f"knots order {order} mesh {mesh}: float32 mode against float64 mode " + ", ".join(f"{k} {v:.1e}" for k, v in dev.items()))
    assert max(dev.values()) <= PMEQ_FLOAT32_CAP, dev
    moves = {h: [W.pmeq_evaluate(dict(c, pos=c["pos"] + s * h)) for s in (1.0, -1.0)] for h in (1e-7, 1e-8)}
    for k, v in ref.items():
        (a, b), (a8, b8) = ([np.abs(m[k] - v).max() / np.abs(v).max() for m in moves[h]] for h in (1e-7, 1e-8))
        print(f"knots order {order} mesh {mesh}: {k:16s} moves by {a:.2e} (+1e-7) and {b:.2e} (-1e-7), by {a8:.2e} and {b8:.2e} (+-1e-8) of its maximum")
        assert max(a, b) <= 1e-6 and max(a8, b8) <= 0.2 * max(a, b) + 1e-12, (k, "a jump at a knot does not shrink with the displacement")
        if order == 6 or k not in ("forces", "virial"):  # (order 5: the fourth derivative of M_5 jumps at a knot, so the third derivatives have a kink there: continuous, two slopes)
            assert abs(a - b) <= 0.05 * max(a, b) + 1e-12, (k, "the same move for both signs")


def test_pme_quadrupole_convergence_bars():
    """The per-output differences between the mesh restatement at order 6 on 32^3 and the explicit restatement on the converged k set, on
    the 37-atom system: ten times these are the bars of test_mesh_term_converges_to_the_explicit_sum_in_every_output."""
    d = W.pmeq_convergence()
    print("pme_quadrupole, order 6 on 32^3 against the explicit sum: " + ", ".join(f"{k} {v:.2e}" for k, v in d.items()))
    assert set(d) == set(W.QUADRUPOLE_NAMES) and all(0.0 < v < 1e-3 for v in d.values())


# ---- cluster multipoles, scaled pairs, local frames ----------------------------------------------------------------------------------------------

def _mirrored(i, j, S):
    keys = {(int(a), int(b)) + tuple(int(x) for x in s) for a, b, s in zip(i, j, S)}
    return all((b, a, -x, -y, -z) in keys for a, b, x, y, z in keys)


@pytest.mark.parametrize("seed", W.SEEDS)
@pytest.mark.parametrize("op", W.CLUSTER_OPS)
def test_cluster_seed_meets_its_conditions(op, seed):
    """Every stored distance at or above the 1.3 of tests/cluster_multipole_reference.py (but for the one coincident pair, at exactly 0), a
    full list, symmetric scales of the four classes, minimum-image pairs at least 0.05 from a flip, and a matrix that holds all three kinds
    of padding, a padding slot between live entries, and the entries in their order."""
    from tests.cluster_multipole_reference import D_MIN

    c = W.cluster_case("sweep", (op, seed))
    i, j, S = c["entries"]
    n = len(c["pos"])
    assert W.CLUSTER_D_MIN == D_MIN and c["dtype"] == ("float64" if seed % 2 == 0 else "float32")
    assert 1 <= len(c["sizes"]) <= 4 and set(c["sizes"]) <= set(W.CLUSTER_SIZES) | {0} and (0 in c["sizes"]) == (seed in W.EMPTY_SYSTEM_SEEDS)
    assert c["periodic"] == (seed in W.CLUSTER_PERIODIC_SEEDS) and (c["cells"] is None) == (not c["periodic"])
    r = W.entry_distances(c) if not c["minimum_image"] else np.linalg.norm(
        np.einsum("ea,eab->eb", (lambda f: f - np.rint(f))(W.fractional_pair_vectors(c)), c["cells"][c["batch_idx"][i]]), axis=1)
    live = np.ones(len(i), bool)
    if c["coincident"] is not None:
        a, b = c["coincident"]
        live = ~(((i == a) & (j == b)) | ((i == b) & (j == a)))
        assert int((~live).sum()) == 2 and float(r[~live].max()) == 0.0 and not c["periodic"]
    assert float(r[live].min()) >= D_MIN and _mirrored(i, j, S)
    if not c["periodic"]:
        assert not S.any() and len(i) == sum(k * (k - 1) for k in c["sizes"]) and not c["flags"]["compute_virial"]
    if c["minimum_image"]:
        f = W.fractional_pair_vectors(c)
        assert c["periodic"] and float(np.abs(f).max()) <= W.PS_IMAGE_MARGIN and bool(S.any()) and bool((np.rint(f) == 0).all())
    if op == "pair_scale":
        s = c["scales"]
        by = {(int(a), int(b)) + tuple(int(x) for x in sh): v for a, b, sh, v in zip(i, j, S, s)}
        assert all(by[(b, a, -x, -y, -z)] == v for (a, b, x, y, z), v in by.items())
        assert (set(s.tolist()) == {1.0}) if c["zero"] else (set(s.tolist()) == {0.0, 0.4, 0.8, 1.0})
        assert c["scale_dtype"] == ("float32" if seed in W.PS_F32_SCALE_SEEDS else "float64") and c["minimum_image"] == (seed in W.PS_MIN_IMAGE_SEEDS)
    else:
        zero = c["mu"] if op == "coulomb_dipole" else c["qd"]
        assert (not zero.any()) == c["zero"]
    nm, sh, val = W.padded_matrix(c["entries"], n, c.get("scales"))
    ok = (nm >= 0) & (nm < n)
    assert (nm == n).any() and (nm == -1).any() and (nm == n + 7).any()
    assert np.array_equal(np.nonzero(ok)[0], i) and np.array_equal(nm[ok], j) and np.array_equal(sh[ok], S)
    assert bool((~ok[:, :-1] & ok[:, 1:]).any()), "a padding slot between live entries"
    if val is not None:
        assert np.array_equal(val[ok], c["scales"]) and np.isnan(val[~ok]).all()
    if c["perm"] is not None:
        ci = W.cluster_interleaved(c)
        assert len(c["sizes"]) >= 2 and bool((np.diff(ci["batch_idx"]) < 0).any()) and np.array_equal(ci["pos"], c["pos"][c["perm"]])


@pytest.mark.parametrize("op", W.CLUSTER_OPS)
def test_cluster_seeds_cover_what_they_are_meant_to(op):
    cases = [W.cluster_case("sweep", (op, s)) for s in W.SEEDS]
    alone = {k for c in cases if sum(c["flags"].values()) == 1 for k, v in c["flags"].items() if v}
    assert alone == set(W.CLUSTER_FLAGS[op]), "each compute flag alone"
    assert any(c["dtype"] == "float32" and sum(c["flags"].values()) == 1 and not (c["flags"]["compute_forces"] or c["flags"]["compute_virial"]) for c in cases)
    assert {c["periodic"] for c in cases} == {True, False} and {n for c in cases for n in c["sizes"]} >= set(W.CLUSTER_SIZES)
    assert all(cases[s]["periodic"] and cases[s]["perm"] is not None for s in W.INTERLEAVED_SEEDS) and any(cases[s]["periodic"] for s in W.EMPTY_SYSTEM_SEEDS)
    if op == "pair_scale":
        assert cases[W.PS_NO_DIPOLE_SEED]["no_dipoles"] and cases[W.PS_NO_QUADRUPOLE_SEED]["no_quadrupoles"] and cases[W.PS_COINCIDENT_SEED]["coincident"]
        assert any(len(cases[s]["sizes"]) > 1 for s in W.PS_MIN_IMAGE_SEEDS)


def test_pair_scale_ladder_case():
    c = W.cluster_case("ps_ladder")
    i, j, S = c["entries"]
    f = W.fractional_pair_vectors(c)
    red = f - np.rint(f)
    r = np.linalg.norm(np.einsum("ea,eab->eb", red, c["cells"][c["batch_idx"][i]]), axis=1)
    counts = np.bincount(i, minlength=len(c["pos"]))
    assert c["sizes"] == (255, 256, 257, 1) and not S.any() and _mirrored(i, j, S) and bool((c["batch_idx"][i] == c["batch_idx"][j]).all())
    assert float(r.min()) >= W.CLUSTER_D_MIN and float(np.abs(red).max()) <= W.PS_IMAGE_MARGIN and bool((np.rint(f) != 0).any())
    assert counts.min() == 0 and counts.max() >= 9 and counts[-1] == 0
    assert set(c["scales"].tolist()) == {0.0, 0.4, 0.8, 1.0}


@pytest.mark.parametrize("seed", W.SEEDS)
def test_frame_seed_meets_its_conditions(seed):
    """Bond lengths in [0.9, 1.6], angles between frame vectors in [40, 140] degrees, Z_ONLY axes more than 0.06 from the switch, chiral triple
    products above 0.2, under a cell every fractional component of a frame vector at least 0.05 from +-0.5, and the restatement's own change
    under float32 rounding of its inputs at most 1e-7 of max|ref| per output (the figure tests/test_local_frames_gpu.py states)."""
    from tests import layout_cases as LC
    from tests import local_frames_reference as LR

    c = W.cluster_case("frames", seed)
    n = c["n"]
    assert n == W.FRAME_TOTAL_BY_SEED[seed] and sum(c["sizes"]) == n and (0 in c["sizes"]) == (seed in W.FRAME_EMPTY_SEEDS)
    cond = LC.frame_conditions(c["pos"], c["atoms"], c["kinds"], c["cells"], None if c["batch_idx"] is None else c["batch_idx"].long())
    named = c["atoms"] >= 0
    if bool(named.any()):
        assert 0.9 <= cond["bond"][0] and cond["bond"][1] <= 1.6 and cond["z_only"] > W.FRAME_SWITCH_MARGIN and cond["chiral"] > 0.2 and cond["image"] <= 0.45, cond
        if bool((named.sum(1) >= 2).any()):
            assert 40.0 <= cond["angle"][0] and cond["angle"][1] <= 140.0, cond
    if n >= 63:
        owner = torch.arange(n)[:, None].expand(n, 3)
        assert sorted(set(c["kinds"].tolist())) == list(range(6))
        assert bool((c["atoms"][named] > owner[named]).any()) and bool((c["atoms"][named] < owner[named]).any()), "frame atoms above and below their owner"
        chiral = (c["kinds"] == LR.Z_THEN_X) & (c["atoms"][:, 2] >= 0)
        assert bool(chiral.any()) and bool(((c["kinds"] == LR.Z_THEN_X) & ~chiral).any())
    if n >= 257:
        assert bool(((c["atoms"][named].long() // 256) != (owner[named] // 256)).any()), "a frame atom in another block of 256"
    if c["batch_idx"] is not None:
        used = torch.where(named, c["atoms"].long(), torch.arange(n)[:, None].expand(n, 3))
        assert bool((c["batch_idx"][used] == c["batch_idx"][:, None]).all())
        assert (seed in W.FRAME_INTERLEAVED_SEEDS) == bool((torch.diff(c["batch_idx"]) < 0).any())
    rnd = lambda x: None if x is None else x.float().double()  # noqa: E731
    args = lambda f: (f(c["pos"]), f(c["mu"]), f(c["quad"]), c["atoms"], c["kinds"], f(c["w_mu"]), f(c["w_q"]))  # noqa: E731
    kw = lambda f: dict(cell=f(c["cells"]), batch_idx=c["batch_idx"])  # noqa: E731
    ref, low = LR.evaluate(*args(lambda x: x), **kw(lambda x: x)), LR.evaluate(*args(rnd), **kw(rnd))
    for k, v in ref.items():
        if v is not None and v.numel() and float(v.abs().max()) > 0:
            assert float((low[k] - v).abs().max()) <= 1e-7 * float(v.abs().max()), (k, float((low[k] - v).abs().max()) / float(v.abs().max()))


def test_frame_seeds_cover_what_they_are_meant_to():
    cases = [W.cluster_case("frames", s) for s in W.SEEDS]
    assert {c["n"] for c in cases} == set(W.FRAME_TOTALS) and {c["form"] for c in cases} == set(W.FRAME_FORMS)
    assert cases[W.FRAME_NO_DIPOLE_SEED]["mu"] is None and cases[W.FRAME_NO_QUADRUPOLE_SEED]["quad"] is None
    assert all(cases[s]["form"] == "batch" for s in W.FRAME_INTERLEAVED_SEEDS + W.FRAME_EMPTY_SEEDS)
    assert {c["dtype"] for c in cases if c["form"] == "batch"} == {"float64", "float32"}
