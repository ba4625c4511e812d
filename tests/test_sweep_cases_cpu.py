"""The conditions every case of tests/sweep_cases.py must meet before it is worth a GPU run, checked without a GPU from the float64
restatements alone: the margin of every cutoff, the lifting rule and the float32 model of the three-body cases, the counts that make a rung
sit on its boundary, the separation of every variant from its default, the coverage of the twelve seeds of each op, a bound on the cost,
and the sensitivity of the reference-side numbers to four faults a kernel could have (DESIGN.md section 3.18 has the table)."""
import os
import re

import numpy as np
import pytest

from tests import atm_reference as A
from tests import d4_atm_cases as K3
from tests import d4_atm_reference as R3
from tests import sweep_cases as W

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
