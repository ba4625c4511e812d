"""The restatement tests/d4_atm_reference.py checked on its own, without a GPU -- closed forms, its autograd derivatives against central
differences, its one-reference / ga = 0 limit against the DFT-D3 three-body restatement -- and the conditions the cases of
tests/d4_atm_cases.py must meet so that the GPU comparison is not vacuous.

The figures these conditions were measured at (s9 = 1 magnitudes, the s9 of every case, scaled float32 deviation, the share of the path
through the coordination numbers) are kept in one place: DESIGN.md section 3.15.  No case had to be dropped from the parity set."""
import numpy as np
import pytest
import torch

from tests import atm_reference as A
from tests import d4_atm_cases as K3
from tests import d4_atm_reference as R3
from tests import d4_reference as R
from tests import systems as S

H = 1e-4
FD_RTOL, FD_ATOL = 1e-6, 1e-9  # tests/test_d4_reference_cpu.py's step and bars: the same kind of smooth energy, the same reasoning


def _one_reference_tables():
    t = R.d4_test_tables(17)
    t["n_ref"][1:] = 1
    return R.blank_unused(t)


def test_closed_forms_equilateral_and_collinear():
    """Constant C6 (one reference per element, ga = 0) and fdamp -> 1 (a2 = 0, a1 -> 0): E = 11 C9 / (8 d^9) for an equilateral triangle
    of side d, -C9 / (4 d^9) for three atoms in a line at spacing d, C9 = sqrt(C6_AB C6_AC C6_BC)."""
    t = _one_reference_tables()
    z = np.array([1, 6, 8], np.int32)
    c6 = t["c6_ref"].astype(np.float64)[:, :, 0, 0]
    c9 = np.sqrt(c6[1, 6] * c6[1, 8] * c6[6, 8])
    d = 3.7
    kw = dict(a1=1e-9, a2=0.0, list_cutoff=20.0, three_body_cutoff=20.0, ga=0.0)
    tri = np.array([[0, 0, 0], [d, 0, 0], [0.5 * d, 0.5 * np.sqrt(3.0) * d, 0]])
    line = np.array([[0, 0, 0], [d, 0, 0], [2 * d, 0, 0]])
    for s9 in (1.0, 0.3):
        e = R3.reference(tri, z, t, s9=s9, **kw)["energy"][0]
        assert abs(e - s9 * 11.0 * c9 / (8.0 * d ** 9)) <= 1e-13 * abs(e)
        e = R3.reference(line, z, t, s9=s9, **kw)["energy"][0]
        assert e < 0 and abs(e + s9 * c9 / (4.0 * d ** 9)) <= 1e-13 * abs(e)
    out = R3.reference(tri, z, t, **kw)
    # net force: zero to the rounding of three float64 terms of this size
    assert out["triples"] == 1 and out["kept"] == 2 and np.abs(out["forces"].sum(0)).max() <= 8 * np.finfo(np.float64).eps * np.abs(out["forces"]).max()


def test_forces_and_virial_equal_central_differences():
    c = K3.case("triclinic_f32")
    pos, cell = c["pos"].astype(np.float64), c["cell"].astype(np.float64)
    kw = dict(three_body_cutoff=c["rc3"], cell=None, **c["kw"])
    base = R3.reference(pos, c["z"], c["tables"], K3.BJ["a1"], K3.BJ["a2"], c["rc"], **dict(kw, cell=cell))
    topo = base["topology"]
    energy = lambda p, h: R3.reference(p, c["z"], c["tables"], K3.BJ["a1"], K3.BJ["a2"], c["rc"], topology=topo, **dict(kw, cell=h))["energy"][0]  # noqa: E731
    n = len(pos)
    assert n == 18 and base["energy"][0] > 0 and base["triples"] > 1000
    fd = np.zeros((n, 3))
    for i in range(n):
        for k in range(3):
            d = np.zeros_like(pos); d[i, k] = H
            fd[i, k] = -(energy(pos + d, cell) - energy(pos - d, cell)) / (2 * H)
    worst_f = np.abs(fd - base["forces"]).max()
    fv = np.zeros((3, 3))
    for a in range(3):
        for b in range(a, 3):
            e = np.zeros((3, 3)); e[a, b] = e[b, a] = 0.5 * H if a != b else H
            up, dn = np.eye(3) + e, np.eye(3) - e
            fv[a, b] = fv[b, a] = -(energy(pos @ up, cell @ up) - energy(pos @ dn, cell @ dn)) / (2 * H)
    worst_v = np.abs(fv - base["virial"][0]).max()
    print(f"central differences vs autograd: forces {worst_f:.2e} on {np.abs(base['forces']).max():.2e}, virial {worst_v:.2e} on "
          f"{np.abs(base['virial']).max():.2e}")
    assert worst_f <= FD_ATOL + FD_RTOL * np.abs(base["forces"]).max()
    assert worst_v <= FD_ATOL + FD_RTOL * np.abs(base["virial"]).max()
    # without the path through the coordination numbers the forces are NOT the derivative of the energy
    fixed = R3.reference(pos, c["z"], c["tables"], K3.BJ["a1"], K3.BJ["a2"], c["rc"], cn_path=False, **dict(kw, cell=cell))
    assert np.abs(fd - fixed["forces"]).max() > 100 * (FD_ATOL + FD_RTOL * np.abs(base["forces"]).max())


def test_one_reference_limit_is_the_dftd3_three_body_term():
    """Both float64, C6 constant: the two restatements differ in summation order only."""
    c = K3.case("d3_limit")
    t4 = c["tables"]
    d3 = {k: v.copy() for k, v in S.d3_test_tables(17, seed=1000).items()}
    np.testing.assert_array_equal(d3["rcov"], t4["rcov"])
    np.testing.assert_array_equal(d3["r4r2"], t4["r4r2"])
    d3["c6ab"] = np.broadcast_to(t4["c6_ref"][:, :, 0, 0][:, :, None, None], d3["c6ab"].shape).copy()
    got = R3.reference(c["pos"], c["z"], t4, K3.BJ["a1"], K3.BJ["a2"], c["rc"], three_body_cutoff=c["rc3"], s9=0.7, alpha=14.0, cell=c["cell"],
                       **c["kw"])
    want = A.reference(c["pos"], c["z"], d3, K3.BJ["a1"], K3.BJ["a2"], c["rc"], three_body_cutoff=c["rc3"], s9=0.7, alpha=14.0, cell=c["cell"],
                       term="atm")
    for k in ("energy", "forces", "virial"):
        scale = np.abs(want[k]).max()
        err = np.abs(got[k] - want[k]).max()
        print(f"D3 limit {k}: {err:.2e} on {scale:.2e}")
        assert scale > 0 and err <= 1e-12 * scale, k


@pytest.mark.parametrize("name", K3.PARITY)
def test_every_parity_case_is_lifted_and_its_float32_deviation_stays_below_the_bar(name):
    c = K3.case(name)
    r64, r32 = K3.unit_references(name)
    s9 = c["s9"]
    smallest = K3.smallest_s9(name)
    assert np.log10(s9) == round(np.log10(s9)), "a power of ten"
    assert K3.lifted(r64, s9), "max|ref| >= 500 of the bars the GPU comparison applies, for energy, forces and virial"
    assert s9 == smallest * K3.ABOVE_RULE.get(name, 1.0), "the smallest such power of ten (cn_cutoff: the feature request's value, a decade above)"
    s64, s32 = K3.references(name)
    for k in ("energy", "forces", "virial"):
        if s64[k] is None:
            continue
        dev = np.abs(s32[k] - s64[k])
        bar = K3.d3_bar(s64[k], k)
        print(f"{name:22s} {k:7s} s9 {s9:g}  max|ref| {np.abs(s64[k]).max():.3e}  scaled fp32 deviation {dev.max():.3e}  worst dev/bar {(dev / bar).max():.3f}")
        assert (dev <= bar).all(), k


@pytest.mark.parametrize("name", K3.ZERO)
def test_fewer_than_three_atoms_give_exactly_zero(name):
    r64, r32 = K3.unit_references(name)
    for r in (r64, r32):
        assert r["triples"] == 0 and not r["energy"].any() and not r["forces"].any()


def _cn_path_in_force_bars(name):
    c = K3.case(name)
    s64, _ = K3.references(name)
    fixed = R3.reference(c["pos"], c["z"], c["tables"], K3.BJ["a1"], K3.BJ["a2"], c["rc"], three_body_cutoff=c["rc3"], s9=c["s9"], cell=c["cell"],
                         batch_idx=c["batch_idx"], cn_path=False, **c["kw"])
    return float((np.abs(s64["forces"] - fixed["forces"]) / K3.d3_bar(s64["forces"], "forces")).max())


def test_the_path_through_the_coordination_numbers_is_visible_and_vanishes_in_the_d3_limit():
    """A missing chain-rule pass must not go unseen: the path moves the forces by >= 100 force bars in at least three parity cases (here in
    every one but no_references, batch and d3_limit), and by exactly nothing where C6 does not depend on CN (one reference per element:
    the restatement takes W = g / g as the constant 1 it is)."""
    moved = {name: _cn_path_in_force_bars(name) for name in K3.PARITY if name != "dense"}
    print({k: round(v, 1) for k, v in moved.items()})
    assert sum(v >= 100.0 for v in moved.values()) >= 3
    # exactly nothing: both evaluations on one thread, so that the two float64 sums run in the same order (with several threads two
    # evaluations of the SAME graph already differ in the last bits, which is all `moved["d3_limit"]` holds)
    assert moved["d3_limit"] <= 1e-9
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        c = K3.case("d3_limit")
        kw = dict(three_body_cutoff=c["rc3"], s9=c["s9"], cell=c["cell"], **c["kw"])
        both = [R3.reference(c["pos"], c["z"], c["tables"], K3.BJ["a1"], K3.BJ["a2"], c["rc"], cn_path=on, **kw) for on in (True, False)]
    finally:
        torch.set_num_threads(threads)
    assert np.array_equal(both[0]["forces"], both[1]["forces"]) and np.array_equal(both[0]["virial"], both[1]["virial"])
    assert np.abs(both[0]["forces"]).max() > 0.0
    c = K3.case("d3_limit")
    z = torch.as_tensor(c["z"], dtype=torch.long)
    for cn in (0.0, 0.37, 2.5, 40.0):
        W, mask = R.gaussian_weights(torch.full((len(z),), cn, dtype=torch.float64), z, c["tables"])
        assert bool((W[:, 0] == 1.0).all()) and bool((W[:, 1:] == 0.0).all()) and c["kw"]["ga"] == 0.0


def test_cases_hold_one_and_seven_reference_elements_and_a_row_longer_than_a_tile():
    from nvalchemiops.interactions.dispersion.dftd4 import atm_tile

    c = K3.case("molecule24")
    assert (c["z"] == R.ONE_REF_Z).any() and (c["z"] == R.SEVEN_REF_Z).any()
    assert c["tables"]["n_ref"][R.ONE_REF_Z] == 1 and c["tables"]["n_ref"][R.SEVEN_REF_Z] == 7
    d = K3.case("dense")
    r64, _ = K3.unit_references("dense")
    tile = atm_tile()
    dist = np.linalg.norm(d["pos"][:, None, :].astype(np.float64) - d["pos"][None, :, :], axis=2)
    kept = ((dist < d["rc3"]) & (dist > 0)).sum(1)
    assert len(d["pos"]) == tile + 24 and kept.max() == r64["kept"] > tile, (kept.max(), tile)
    assert kept.min() < tile, "rows of one tile and rows of two tiles in the same call"
    assert (d["z"] == R.ONE_REF_Z).any() and (d["z"] == R.SEVEN_REF_Z).any()


def test_shell_case_holds_one_row_of_three_tiles_and_its_s9_follows_the_rule():
    """`shell` is judged by a GPU test of its own (it is not in PARITY); its conditions, as for `dense`.  The restatement of this system
    (585 atoms at a tile of 288, 1.6e6 triples) takes 5.6 s for float64 + float32 together on 16 CPU threads, so both are used."""
    from nvalchemiops.interactions.dispersion.dftd4 import atm_tile

    d = K3.case("shell")
    r64, r32 = K3.unit_references("shell")
    tile = atm_tile()
    kept, pairs0, triples, margin = A.kept_and_triples(d["pos"], d["rc3"])
    assert len(d["pos"]) == 2 * tile + 9 and kept[0] == r64["kept"] > 2 * tile and kept[1:].max() < tile, (kept[0], kept[1:].max(), tile)
    assert r64["triples"] == triples and pairs0 > 0
    assert margin > 2e-5, "no pair within float32 rounding of the cutoff (ulp(20) = 1.9e-6, a few per distance)"
    assert d["s9"] == K3.smallest_s9("shell") and K3.lifted(r64, d["s9"])
    for k in ("energy", "forces"):
        assert (np.abs(r32[k] - r64[k]) <= K3.d3_bar(r64[k], k)).all(), k
    assert (d["z"] == R.ONE_REF_Z).any() and (d["z"] == R.SEVEN_REF_Z).any()
