"""`dftd3_atm` (three-body Axilrod-Teller-Muto term, HIP triple pass) against the float64 restatement tests/atm_reference.py.

Lists are built by this package's `neighbor_list` / `cell_list`.  Bars: the restatement is evaluated once in float64 and once with every
per-pair / per-triple quantity in float32 (float64 sums: the kernels' arithmetic model); a quantity's bar is 4 x the larger of that
float32-vs-float64 deviation on the same system and `dftd3`'s existing bar (tests/test_d3_gpu.py:49-54: energy rtol = atol = 1e-6; forces
rtol 1e-6, atol 1e-6 + 5e-6 max|F|; virial rtol 1e-6, atol 1e-6 + 2e-7 max|V|).  4 x is the factor the suite allows between two summation
orders (tests/test_oracle_golden.py).  Every atom and every system of every input is compared; each figure is printed before it is asserted.

MEASURED on one MI355X (max over components; restatement float32 vs float64 | kernel vs float64 restatement | worst err / bar; matrix and
CSR agree to the digits shown; the full table with max|ref| is in DESIGN.md section 3.10, every test prints its figures under `pytest -s`):
  molecule 60 atoms           E 5.6e-8 | 1.4e-9 | 0.000    F 6.4e-9 | 5.4e-9 | 0.001
  non-factorising tables      E 1.2e-8 | 4.1e-9 | 0.001    F 4.4e-9 | 2.5e-9 | 0.001
  20 species                  E 8.6e-9 | 4.3e-8 | 0.008    F 4.7e-8 | 1.2e-8 | 0.003
  10 species                  E 7.5e-9 | 4.7e-9 | 0.001    F 1.5e-8 | 3.6e-9 | 0.001
  cubic 125, fp32             E 5.9e-9 | 1.1e-9 | 0.000    F 5.2e-10 | 1.0e-9 | 0.000   V 2.4e-8 | 1.4e-8 | 0.003
  triclinic 150, fp32         E 2.6e-8 | 1.3e-8 | 0.003    F 8.0e-10 | 2.1e-9 | 0.001   V 6.2e-8 | 3.1e-8 | 0.006
  triclinic 150, fp64         E 2.4e-8 | 3.6e-10 | 0.000   F 7.7e-10 | 2.0e-9 | 0.000   V 6.6e-8 | 3.0e-8 | 0.005
  small cell (own images)     E 1.3e-8 | 3.4e-9 | 0.001    F 3.8e-9 | 8.7e-9 | 0.002    V 8.6e-9 | 2.4e-8 | 0.006
  batch of three              E 3.6e-10 | 7.5e-10 | 0.000  F 2.3e-10 | 1.1e-10 | 0.000  V 1.5e-9 | 1.5e-9 | 0.000
  dense row, 343 staged       E 1.5e-7 | 1.4e-8 | 0.001    F 1.5e-8 | 2.1e-8 | 0.004
  renumbered 80-atom box      E 1.5e-10 | 2.8e-9 | 0.001   F 4.7e-10 | 2.5e-10 | 0.000  V 5.0e-9 | 3.3e-9 | 0.001
  three-tile row, 648 staged  E 1.5e-7 | 3.0e-7 | 0.035    F 7.2e-9 | 5.1e-9 | 0.001
The float32 deviation never exceeds `dftd3`'s bar on these systems, so every bar is 4 x `dftd3`'s."""
import numpy as np
import pytest
import torch

from tests import atm_reference as R
from tests import systems as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BJ = dict(a1=0.4, a2=4.0)


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def _params(t):
    from nvalchemiops.interactions.dispersion import D3Parameters

    return D3Parameters(rcov=_t(t["rcov"]), r4r2=_t(t["r4r2"]), c6ab=_t(t["c6ab"]), cn_ref=_t(t["cn_ref"]))


def _lists(pos, cell, rc, batch_idx=None, max_neighbors=None):
    """(matrix kwargs, CSR kwargs) of the full list with cutoff rc, built on the device by the package."""
    from nvalchemiops.neighborlist import neighbor_list

    tp = _t(pos)
    kw = {}
    if cell is not None:
        c = _t(np.asarray(cell).reshape(-1, 3, 3))
        kw = dict(cell=c, pbc=torch.ones((c.shape[0], 3), dtype=torch.bool, device=DEV))
        method = "cell_list" if batch_idx is None else "batch_cell_list"
        if batch_idx is None:
            kw = dict(cell=c[0], pbc=kw["pbc"][0])
    else:
        method = "naive" if batch_idx is None else "batch_naive"
    if batch_idx is not None:
        kw["batch_idx"] = _t(np.asarray(batch_idx, np.int32))
    mn = max_neighbors or len(pos) + 8
    out = neighbor_list(tp, rc, method=method, max_neighbors=mn, **kw)
    nm, num = out[0], out[1]
    assert int(num.max()) <= nm.shape[1], "neighbour matrix too narrow for this test system"
    lst = neighbor_list(tp, rc, method=method, max_neighbors=mn, return_neighbor_list=True, **kw)
    m = dict(neighbor_matrix=nm)
    l = dict(neighbor_list=lst[0], neighbor_ptr=lst[1])
    if cell is not None:
        m["neighbor_matrix_shifts"] = out[2]
        l["unit_shifts"] = lst[2]
    return m, l, int(num.max())


def _references(pos, z, t, rc_list, rc3, cell=None, batch_idx=None, s9=1.0, alpha=16.0):
    kw = dict(three_body_cutoff=rc3, s9=s9, alpha=alpha, cell=cell, batch_idx=batch_idx)
    r64 = R.reference(pos, z, t, BJ["a1"], BJ["a2"], rc_list, **kw)
    r32 = R.reference(pos, z, t, BJ["a1"], BJ["a2"], rc_list, work_dtype=torch.float32, **kw)
    return r64, r32


def _judge(name, out, r64, r32):
    """Asserts out = (energy, forces[, virial]) against the float64 restatement at the module's bars; prints the figures first."""
    got = [o.detach().cpu().numpy().astype(np.float64) for o in out]
    keys = ["energy", "forces"] + (["virial"] if len(got) == 3 else [])
    extra = {"energy": 0.0, "forces": 5e-6, "virial": 2e-7}
    fails = []
    for g, k in zip(got, keys):
        ref, low = r64[k], r32[k]
        assert g.shape == ref.shape, (k, g.shape, ref.shape)
        dev32 = np.abs(low - ref).max() if ref.size else 0.0
        scale = np.abs(ref).max() if ref.size else 0.0
        bar = 4.0 * np.maximum(dev32, 1e-6 + 1e-6 * np.abs(ref) + extra[k] * scale)
        err = np.abs(g - ref)
        worst = (err / bar).max() if ref.size else 0.0
        print(f"[atm] {name:34s} {k:7s} max|ref| {scale:.3e}  fp32-vs-fp64 {dev32:.3e}  kernel-vs-fp64 {err.max() if ref.size else 0.0:.3e}  "
              f"worst err/bar {worst:.3f}")
        if not (err <= bar).all():
            fails.append(f"{k}: max err {err.max():.3e}, bar {bar.flat[(err / bar).argmax()]:.3e}")
    assert not fails, f"{name}: " + "; ".join(fails)


def _zs(n, seed, choices=(1, 6, 8, 17)):
    return np.random.default_rng(seed).choice(np.array(choices, np.int32), n)


# ---- molecules -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,seed", [(3, 1), (7, 2), (24, 3), (60, 4)])
def test_molecules_matrix_and_csr(n, seed):
    from nvalchemiops.interactions.dispersion import dftd3_atm

    pos, z, _ = S.molecule(n, density=0.02, min_dist=2.0, seed=seed)
    z = _zs(n, seed)
    t = S.d3_test_tables(17)
    p = _params(t)
    rc_list, rc3 = 14.0, 11.0
    m, l, _ = _lists(pos, None, rc_list)
    r64, r32 = _references(pos, z, t, rc_list, rc3)
    assert n < 7 or abs(r64["energy"][0]) > 0.0
    a = dftd3_atm(_t(pos), _t(z), three_body_cutoff=rc3, d3_params=p, **BJ, **m)
    b = dftd3_atm(_t(pos), _t(z), three_body_cutoff=rc3, d3_params=p, **BJ, **l)
    assert len(a) == 2 and a[0].dtype == torch.float32 and a[1].shape == (n, 3)
    _judge(f"molecule{n} matrix", a, r64, r32)
    _judge(f"molecule{n} csr", b, r64, r32)


def test_padding_atom_single_atom_pair_and_s9_zero():
    from nvalchemiops.interactions.dispersion import dftd3_atm

    t = S.d3_test_tables(17)
    p = _params(t)
    # a padding atom (Z = 0) inside a molecule: it is part of no triple and of no coordination number
    pos, _, _ = S.molecule(9, density=0.02, min_dist=2.0, seed=8)
    z = _zs(9, 8)
    z[4] = 0
    m, l, _ = _lists(pos, None, 14.0)
    r64, r32 = _references(pos, z, t, 14.0, 12.0)
    out = dftd3_atm(_t(pos), _t(z), three_body_cutoff=12.0, d3_params=p, **BJ, **m)
    _judge("padding atom", out, r64, r32)
    assert torch.equal(out[1][4], torch.zeros(3, device=DEV))
    # a single atom and a pair: exactly zero
    for k in (1, 2):
        pk = np.array([[0, 0, 0], [3.0, 0, 0]], np.float32)[:k]
        nm = np.full((k, 4), k, np.int32)
        if k == 2:
            nm[0, 0], nm[1, 0] = 1, 0
        e, f = dftd3_atm(_t(pk), _t(np.full(k, 6, np.int32)), three_body_cutoff=10.0, d3_params=p, neighbor_matrix=_t(nm), **BJ)
        assert float(e.abs().max()) == 0.0 and float(f.abs().max()) == 0.0
    # s9 = 0: exactly zero
    z = _zs(9, 8)
    e, f = dftd3_atm(_t(pos), _t(z), three_body_cutoff=12.0, s9=0.0, d3_params=p, **BJ, **m)
    assert float(e.abs().max()) == 0.0 and float(f.abs().max()) == 0.0


def test_alpha_14_and_16_differ_and_both_match():
    from nvalchemiops.interactions.dispersion import dftd3_atm

    t = S.d3_test_tables(17)
    p = _params(t)
    pos, _, _ = S.molecule(20, density=0.03, min_dist=2.0, seed=12)
    z = _zs(20, 12)
    m, _, _ = _lists(pos, None, 13.0)
    outs = {}
    for alpha in (14.0, 16.0):
        r64, r32 = _references(pos, z, t, 13.0, 10.0, alpha=alpha, s9=0.8)
        outs[alpha] = dftd3_atm(_t(pos), _t(z), three_body_cutoff=10.0, alpha=alpha, s9=0.8, d3_params=p, **BJ, **m)
        _judge(f"alpha {alpha:g}", outs[alpha], r64, r32)
    assert float(outs[14.0][0]) != float(outs[16.0][0])


def test_general_tables_and_more_than_16_species():
    """The other C6 table paths: tables whose reference CN depends on the partner (no factorised weights: the 25-term form from the
    compact table), more than 16 species present (the global table), and factorised weights with 7 - 16 species (c6 rows not in LDS)."""
    from nvalchemiops.interactions.dispersion import dftd3_atm

    pos, _, _ = S.molecule(30, density=0.03, min_dist=2.0, seed=21)
    t = {k: v.copy() for k, v in S.d3_test_tables(17).items()}
    zi = np.arange(18, dtype=np.float32)
    t["cn_ref"] *= (1.0 + 0.01 * zi[None, :, None, None])  # partner-dependent reference CN, still cn_ref[a,b][p,q] <-> cn_ref[b,a][q,p] consistent per side
    z = _zs(30, 21)
    m, l, _ = _lists(pos, None, 13.0)
    r64, r32 = _references(pos, z, t, 13.0, 10.0)
    _judge("general tables", dftd3_atm(_t(pos), _t(z), three_body_cutoff=10.0, d3_params=_params(t), **BJ, **m), r64, r32)
    t = S.d3_test_tables(30, seed=5)
    z = (np.arange(30) % 20 + 1).astype(np.int32)  # 20 species
    r64, r32 = _references(pos, z, t, 13.0, 10.0)
    _judge("20 species", dftd3_atm(_t(pos), _t(z), three_body_cutoff=10.0, d3_params=_params(t), **BJ, **l), r64, r32)
    # factorised weights with more species than the triple pass keeps in LDS (7 - 16): the c6 rows of the j-k pair come from global memory
    t = S.d3_test_tables(17)
    z = (np.arange(30) % 10 + 1).astype(np.int32)
    r64, r32 = _references(pos, z, t, 13.0, 10.0)
    _judge("10 species", dftd3_atm(_t(pos), _t(z), three_body_cutoff=10.0, d3_params=_params(t), **BJ, **m), r64, r32)


# ---- periodic ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("triclinic,dtype", [(False, np.float32), (True, np.float32), (True, np.float64)])
def test_periodic_boxes_energy_forces_virial(triclinic, dtype):
    """100-200 atoms, three-body cutoff below half the shortest cell height, list cutoff above it (CN over the long list, triples over the
    short range)."""
    from nvalchemiops.interactions.dispersion import dftd3_atm

    shape = (5, 5, 6) if triclinic else (5, 5, 5)
    pos, cell = R.lattice_box(shape, seed=7, triclinic=triclinic, dtype=dtype)
    n = len(pos)
    z = _zs(n, 7)
    t = S.d3_test_tables(17)
    p = _params(t)
    rc_list, rc3 = 10.0, 8.5
    heights = 1.0 / np.linalg.norm(np.linalg.inv(cell.astype(np.float64)), axis=0)
    assert rc3 < 0.5 * heights.min()
    m, l, widest = _lists(pos, cell, rc_list, max_neighbors=160)
    r64, r32 = _references(pos, z, t, rc_list, rc3, cell=cell)
    tc = _t(cell.reshape(1, 3, 3))
    a = dftd3_atm(_t(pos), _t(z), three_body_cutoff=rc3, d3_params=p, cell=tc, compute_virial=True, **BJ, **m)
    b = dftd3_atm(_t(pos), _t(z), three_body_cutoff=rc3, d3_params=p, cell=tc, compute_virial=True, **BJ, **l)
    assert a[2].shape == (1, 3, 3) and a[2].dtype == torch.float32
    assert r64["energy"][0] > 0.0, "the three-body term of a condensed phase is repulsive"
    tag = f"{'triclinic' if triclinic else 'cubic'} {n} {np.dtype(dtype).name}"
    _judge(tag + " matrix", a, r64, r32)
    _judge(tag + " csr", b, r64, r32)
    # net force per system: zero to rounding
    assert float(a[1].double().sum(0).abs().max()) <= 1e-5 * float(a[1].abs().max()) * np.sqrt(n)


def test_small_cell_own_images_and_repeated_neighbours():
    """L < three_body_cutoff: rows hold an atom's own images and several images of one neighbour -- distinct vertices."""
    from nvalchemiops.interactions.dispersion import dftd3_atm

    pos, cell = R.lattice_box((2, 2, 2), a=3.6, jitter=0.2, seed=9, triclinic=True)
    z = _zs(8, 9, (6, 8))
    t = S.d3_test_tables(17)
    rc_list, rc3 = 9.5, 8.0
    assert np.linalg.norm(cell, axis=1).min() < rc3
    m, l, widest = _lists(pos, cell, rc_list, max_neighbors=400)
    nm, sh = m["neighbor_matrix"].cpu().numpy(), m["neighbor_matrix_shifts"].cpu().numpy()
    assert ((nm[0] == 0) & (np.abs(sh[0]).sum(1) > 0)).any(), "the test needs rows with the atom's own images"
    r64, r32 = _references(pos, z, t, rc_list, rc3, cell=cell)
    tc = _t(cell.reshape(1, 3, 3))
    for tag, lk in (("matrix", m), ("csr", l)):
        out = dftd3_atm(_t(pos), _t(z), three_body_cutoff=rc3, d3_params=_params(t), cell=tc, compute_virial=True, **BJ, **lk)
        _judge("small cell " + tag, out, r64, r32)


def test_batch_of_three_systems():
    from nvalchemiops.interactions.dispersion import dftd3_atm

    boxes = [R.lattice_box((3, 3, 3), seed=1, triclinic=False), R.lattice_box((4, 3, 3), seed=2, triclinic=True), R.lattice_box((2, 3, 2), a=4.6, seed=3, triclinic=True)]
    pos = np.concatenate([b[0] for b in boxes])
    cell = np.stack([b[1] for b in boxes])
    bi = np.concatenate([np.full(len(b[0]), k, np.int32) for k, b in enumerate(boxes)])
    n = len(pos)
    z = _zs(n, 5)
    t = S.d3_test_tables(17)
    rc_list, rc3 = 8.0, 6.5
    m, l, _ = _lists(pos, cell, rc_list, batch_idx=bi, max_neighbors=200)
    r64, r32 = _references(pos, z, t, rc_list, rc3, cell=cell, batch_idx=bi)
    for tag, lk in (("matrix", m), ("csr", l)):
        out = dftd3_atm(_t(pos), _t(z), three_body_cutoff=rc3, d3_params=_params(t), cell=_t(cell), batch_idx=_t(bi), compute_virial=True, **BJ, **lk)
        assert out[0].shape == (3,) and out[2].shape == (3, 3, 3)
        _judge("batch of three " + tag, out, r64, r32)
        f = out[1].double()
        for s in range(3):
            sel = torch.as_tensor(bi == s, device=DEV)
            assert float(f[sel].sum(0).abs().max()) <= 1e-5 * float(f.abs().max()) * np.sqrt(n)


def test_dense_row_needs_more_than_one_lds_tile():
    """A free cluster in which every atom has more neighbours inside the three-body cutoff than one LDS tile of the triple pass holds
    (tile = `atm_tile()` = 320 staged neighbours when this was written): 344 atoms, every row stages 343 neighbours, i.e. two tiles --
    within-tile pairs of both tiles and the cross-tile pairs."""
    from nvalchemiops.interactions.dispersion import dftd3_atm
    from nvalchemiops.interactions.dispersion.dftd3 import atm_tile

    tile = atm_tile()
    n = tile + 24
    pos, cell = R.lattice_box((7, 7, 8), a=3.4, jitter=0.2, seed=13, triclinic=False)
    pos = pos[:n]
    z = _zs(n, 13, (1, 6, 8))
    t = S.d3_test_tables(17)
    rc = 2.0 * float(np.linalg.norm(pos.max(0) - pos.min(0)))  # everything is everybody's neighbour
    m, l, widest = _lists(pos, None, rc)
    assert widest == n - 1 and widest > tile, (widest, tile)
    r64, r32 = _references(pos, z, t, rc, rc)
    _judge(f"dense row ({widest} staged) matrix", dftd3_atm(_t(pos), _t(z), three_body_cutoff=rc, d3_params=_params(t), **BJ, **m), r64, r32)
    _judge(f"dense row ({widest} staged) csr", dftd3_atm(_t(pos), _t(z), three_body_cutoff=rc, d3_params=_params(t), **BJ, **l), r64, r32)


def _visits(pos, z, t, lists, rc3, scalars, zero=None):
    """Per-centre triangle-visit counters of one triple pass on the matrix list (`want_visits`)."""
    import importlib

    from nvalchemiops import _capi as C

    D3 = importlib.import_module("nvalchemiops.interactions.dispersion.dftd3")  # (the package re-exports a function of the same name)
    n = len(pos)
    nm = C.i32(lists["neighbor_matrix"])
    f32 = dict(dtype=torch.float32, device=DEV)
    tables = tuple(_t(t[k]) for k in ("rcov", "r4r2", "c6ab", "cn_ref"))
    return D3._launch_atm(positions=_t(pos), numbers=_t(z), idx=nm, shifts=None, nptr=None, max_neighbors=nm.shape[1], fill_value=n, cell=None,
                          batch_idx=None, num_systems=1, tables=tables, scalars=scalars, s9=1.0, alpha=16.0, three_body_cutoff=rc3,
                          compute_virial=False, energy=torch.empty(1, **f32), forces=torch.empty((n, 3), **f32),
                          virial=torch.zeros((0, 3, 3), **f32), want_visits=True, zero=zero).cpu().numpy()


def shell_system():
    """A centre atom whose row stages THREE tiles (`atm_reference.centre_and_shell` with 2 tiles + 8 shell atoms, three-body cutoff 20, list
    cutoff 40: everybody is listed) while every other row stages less than one: all six tile pairs of the long row, (1, 2) among them.
    Returns (pos, z, tile, pairs among the centre's kept entries, triples), the last two counted from numpy distances."""
    from nvalchemiops.interactions.dispersion.dftd3 import atm_tile

    tile = atm_tile()
    pos = R.centre_and_shell(2 * tile + 8)
    kept, pairs0, triples, margin = R.kept_and_triples(pos, 20.0)
    assert kept[0] > 2 * tile and kept[1:].max() < tile, (kept[0], kept[1:].max(), tile)
    assert margin > 2e-5, "no pair within float32 rounding (ulp(20) = 1.9e-6, a few per distance) of the cutoff: the counts below are exact"
    return pos, _zs(len(pos), 29, (1, 6, 8)), tile, pairs0, triples


def test_row_of_three_lds_tiles_runs_every_tile_pair_once():
    from nvalchemiops.interactions.dispersion import dftd3_atm
    from nvalchemiops.interactions.dispersion.dftd3 import atm_scalars

    pos, z, tile, pairs0, triples = shell_system()
    t = S.d3_test_tables(17)
    m, l, widest = _lists(pos, None, 40.0)
    assert widest == len(pos) - 1
    r64, r32 = _references(pos, z, t, 40.0, 20.0)
    assert r64["triples"] == triples
    _judge("three-tile row matrix", dftd3_atm(_t(pos), _t(z), three_body_cutoff=20.0, d3_params=_params(t), **BJ, **m), r64, r32)
    _judge("three-tile row csr", dftd3_atm(_t(pos), _t(z), three_body_cutoff=20.0, d3_params=_params(t), **BJ, **l), r64, r32)
    visits = _visits(pos, z, t, m, 20.0, atm_scalars(BJ["a1"], BJ["a2"], 16.0, -4.0))
    assert visits[0] == pairs0 and int(visits.sum()) == 3 * r64["triples"], (visits[0], pairs0, int(visits.sum()), 3 * r64["triples"])


# ---- invariances ---------------------------------------------------------------------------------------------------------------------

def test_renumbering_net_force_and_dftd3_untouched():
    from nvalchemiops.interactions.dispersion import dftd3, dftd3_atm

    pos, cell = R.lattice_box((5, 4, 4), seed=17, triclinic=True)
    n = len(pos)
    z = _zs(n, 17)
    t = S.d3_test_tables(17)
    p = _params(t)
    tc = _t(cell.reshape(1, 3, 3))
    rc_list, rc3 = 10.0, 7.5
    m, _, _ = _lists(pos, cell, rc_list, max_neighbors=200)
    tp, tz = _t(pos), _t(z)
    two_body = dict(a1=0.4, a2=4.0, s8=0.8, d3_params=p, cell=tc, compute_virial=True, **m)
    before = dftd3(tp, tz, **two_body)
    e, f, v = dftd3_atm(tp, tz, three_body_cutoff=rc3, d3_params=p, cell=tc, compute_virial=True, **BJ, **m)
    after = dftd3(tp, tz, **two_body)
    assert all(torch.equal(a, b) for a, b in zip(before, after)), "dftd3 must not see that dftd3_atm ran on the same tensors"
    assert float(f.double().sum(0).abs().max()) <= 1e-5 * float(f.abs().max()) * np.sqrt(n)
    # a random renumbering of the atoms: energy and virial unchanged, forces permuted -- each run against the (permuted) restatement,
    # and against each other within the two bars added (the renumbering changes which neighbour plays which role in a triple)
    r64, r32 = _references(pos, z, t, rc_list, rc3, cell=cell)
    _judge("original numbering", (e, f, v), r64, r32)
    perm = np.random.default_rng(0).permutation(n)
    m2, _, _ = _lists(pos[perm], cell, rc_list, max_neighbors=200)
    out2 = dftd3_atm(_t(pos[perm]), _t(z[perm]), three_body_cutoff=rc3, d3_params=p, cell=tc, compute_virial=True, **BJ, **m2)
    p64 = dict(r64, forces=r64["forces"][perm])
    p32 = dict(r32, forces=r32["forces"][perm])
    _judge("renumbered", out2, p64, p32)


def test_fullgraph_compile_of_dftd3_plus_atm_equals_eager():
    from nvalchemiops.interactions.dispersion import dftd3, dftd3_atm
    from nvalchemiops.neighborlist import neighbor_list

    pos, cell = R.lattice_box((5, 4, 4), seed=19, triclinic=True)
    n = len(pos)
    z = _t(_zs(n, 19))
    p = _params(S.d3_test_tables(17))
    tc = _t(cell.reshape(1, 3, 3))
    m, l, _ = _lists(pos, cell, 10.0, max_neighbors=200)
    tables = {"rcov": p.rcov, "r4r2": p.r4r2, "c6ab": p.c6ab, "cn_ref": p.cn_ref}

    def total_matrix(x):
        e2, f2, cn, v2 = dftd3(x, z, a1=0.4, a2=4.0, s8=0.8, d3_params=p, cell=tc, compute_virial=True, **m)
        e3, f3, v3 = dftd3_atm(x, z, three_body_cutoff=7.5, d3_params=p, cell=tc, compute_virial=True, **BJ, **m)
        return e2 + e3, f2 + f3, v2 + v3, e3

    def total_csr(x):
        e2, f2, cn = dftd3(x, z, a1=0.4, a2=4.0, s8=0.8, d3_params=tables, cell=tc, **l)
        e3, f3 = dftd3_atm(x, z, three_body_cutoff=7.5, alpha=14.0, d3_params=tables, cell=tc, **BJ, **l)
        return e2 + e3, f2 + f3, e3

    for fn in (total_matrix, total_csr):
        torch._dynamo.reset()
        got = torch.compile(fn, mode="default", fullgraph=True)(_t(pos))
        want = fn(_t(pos))
        assert float(want[-1].abs()) > 0.0
        assert len(got) == len(want) and all(torch.equal(a, b) for a, b in zip(got, want))
