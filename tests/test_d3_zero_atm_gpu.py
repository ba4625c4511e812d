"""`dftd3_zero_atm` (the three-body Axilrod-Teller-Muto term with the radii of the zero damping, R0_XY = rs9 r0ab[Z_X, Z_Y]: the
zero-damping instantiation of the HIP triple pass) against the float64 restatement tests/d3_zero_reference.py (`term="atm"`).

Lists, bars and reporting are those of tests/test_d3_atm_gpu.py: the restatement once in float64 and once with every per-pair / per-triple
quantity in float32; bar per quantity = 4 x the larger of that float32-vs-float64 deviation and `dftd3`'s existing bar (energy rtol = atol =
1e-6; forces + 5e-6 max|F|; virial + 2e-7 max|V|); every atom and every system compared; figures printed before they are asserted.

MEASURED on one MI355X (max over components; restatement float32 vs float64 | kernel vs float64 restatement | worst err / bar; matrix and
CSR agree to the digits shown -- the larger of the two is listed; every test prints its figures under `pytest -s`; the table with max|ref|
is in DESIGN.md section 3.11):
  molecule3                                E 1.3e-13 | 4.6e-14 | 0.000   F 1.1e-13 | 3.4e-14 | 0.000
  molecule7                                E 2.5e-11 | 1.4e-11 | 0.000   F 1.8e-11 | 2.1e-11 | 0.000
  molecule24                               E 4.5e-09 | 4.4e-09 | 0.001   F 5.2e-10 | 4.1e-10 | 0.000
  molecule60                               E 1.2e-07 | 1.5e-07 | 0.029   F 8.8e-09 | 8.7e-09 | 0.002
  {'rs9': 1.0}                             E 1.1e-08 | 2.7e-08 | 0.005   F 5.9e-08 | 1.4e-08 | 0.003
  {'alpha': 14.0}                          E 6.2e-09 | 8.1e-09 | 0.002   F 2.5e-09 | 1.4e-09 | 0.000
  {'s9': 0.5}                              E 3.2e-09 | 3.3e-09 | 0.001   F 9.1e-10 | 5.7e-10 | 0.000
  general                                  E 3.4e-08 | 3.8e-08 | 0.009   F 2.7e-09 | 3.8e-09 | 0.001
  20 species                               E 1.5e-08 | 1.5e-08 | 0.004   F 1.4e-08 | 1.7e-09 | 0.000
  10 species                               E 6.8e-09 | 8.5e-09 | 0.002   F 9.6e-09 | 1.7e-09 | 0.000
  factorised                               E 3.4e-08 | 4.1e-08 | 0.010   F 1.8e-08 | 4.1e-09 | 0.001
  cubic 125 float32                        E 4.4e-08 | 4.5e-08 | 0.011   F 1.7e-09 | 2.3e-09 | 0.001   V 4.7e-08 | 5.0e-08 | 0.011
  triclinic 150 float32                    E 8.4e-08 | 8.0e-08 | 0.018   F 5.3e-09 | 5.4e-09 | 0.001   V 1.0e-07 | 1.2e-07 | 0.025
  triclinic 150 float64                    E 8.4e-08 | 8.2e-08 | 0.018   F 4.4e-09 | 4.0e-09 | 0.001   V 1.1e-07 | 1.3e-07 | 0.026
  batch of three                           E 2.9e-09 | 2.8e-09 | 0.001   F 7.5e-10 | 9.5e-10 | 0.000   V 6.5e-09 | 7.1e-09 | 0.002
  dense row (327 staged)                   E 4.3e-07 | 4.5e-07 | 0.033   F 1.1e-08 | 1.6e-08 | 0.004
  original numbering                       E 7.6e-09 | 7.3e-09 | 0.002   F 5.9e-10 | 5.9e-10 | 0.000   V 1.7e-08 | 1.7e-08 | 0.004
  renumbered                               E 7.6e-09 | 7.3e-09 | 0.002   F 5.9e-10 | 5.9e-10 | 0.000   V 1.7e-08 | 1.7e-08 | 0.004
Worst err / bar of any figure: 0.033.
"""
import numpy as np
import pytest
import torch

from tests import atm_reference as A
from tests import d3_zero_reference as Z
from tests import systems as S
from tests.test_d3_zero_gpu import DEV, ZERO, _lists, _params, _t, _tables, _z20, _zs

pytestmark = pytest.mark.gpu
_EXTRA = {"energy": 0.0, "forces": 5e-6, "virial": 2e-7}


def _references(pos, z, t, r0ab, rc_list, rc3, cell=None, batch_idx=None, **kw):
    kw = dict(three_body_cutoff=rc3, cell=cell, batch_idx=batch_idx, term="atm", **kw)
    return Z.reference(pos, z, t, r0ab, None, None, rc_list, **kw), Z.reference(pos, z, t, r0ab, None, None, rc_list, work_dtype=torch.float32, **kw)


def _judge(name, out, r64, r32):
    got = [o.detach().cpu().numpy().astype(np.float64) for o in out]
    keys = ["energy", "forces"] + (["virial"] if len(got) == 3 else [])
    fails = []
    for g, k in zip(got, keys):
        ref, low = r64[k], r32[k]
        assert g.shape == ref.shape, (k, g.shape, ref.shape)
        dev32 = np.abs(low - ref).max() if ref.size else 0.0
        scale = np.abs(ref).max() if ref.size else 0.0
        bar = 4.0 * np.maximum(dev32, 1e-6 + 1e-6 * np.abs(ref) + _EXTRA[k] * scale)
        err = np.abs(g - ref)
        worst = (err / bar).max() if ref.size else 0.0
        print(f"[d3zero-atm] {name:34s} {k:7s} max|ref| {scale:.3e}  fp32-vs-fp64 {dev32:.3e}  kernel-vs-fp64 {err.max() if ref.size else 0.0:.3e}  "
              f"worst err/bar {worst:.3f}")
        if not (err <= bar).all():
            fails.append(f"{k}: max err {err.max():.3e}, bar {bar.flat[(err / bar).argmax()]:.3e}")
    assert not fails, f"{name}: " + "; ".join(fails)


@pytest.mark.parametrize("n,seed", [(3, 1), (7, 2), (24, 3), (60, 4)])
def test_molecules_matrix_and_csr(n, seed):
    from nvalchemiops.interactions.dispersion import dftd3_zero_atm

    pos, _, _ = S.molecule(n, density=0.02, min_dist=2.0, seed=seed)
    z = _zs(n, seed)
    t, r0ab = _tables()
    p = _params(t, r0ab)
    rc_list, rc3 = 14.0, 11.0
    m, l = _lists(pos, None, rc_list)
    r64, r32 = _references(pos, z, t, r0ab, rc_list, rc3)
    assert n < 7 or abs(r64["energy"][0]) > 0.0
    a = dftd3_zero_atm(_t(pos), _t(z), rc3, d3_params=p, **m)
    b = dftd3_zero_atm(_t(pos), _t(z), rc3, d3_params=p, **l)
    assert len(a) == 2 and a[0].dtype == torch.float32 and a[1].shape == (n, 3)
    _judge(f"molecule{n} matrix", a, r64, r32)
    _judge(f"molecule{n} csr", b, r64, r32)


def test_table_radii_are_what_is_used():
    """A table of the BJ form, r0ab = (a1 sqrt(3 r4r2 r4r2) + a2) / rs9, reproduces `dftd3_atm`; another table, rs9, alpha or s9 does not."""
    from nvalchemiops.interactions.dispersion import dftd3_atm, dftd3_zero_atm

    pos, _, _ = S.molecule(24, density=0.03, min_dist=2.0, seed=12)
    z = _zs(24, 12)
    t, r0ab = _tables()
    m, _ = _lists(pos, None, 13.0)
    rs9 = 4.0 / 3.0
    r4 = t["r4r2"].astype(np.float64)
    bj = (0.4 * np.sqrt(3.0 * r4[:, None] * r4[None, :]) + 4.0) / rs9
    bj[0, :] = bj[:, 0] = 0.0
    e1, f1 = dftd3_atm(_t(pos), _t(z), a1=0.4, a2=4.0, three_body_cutoff=10.0, d3_params=_params(t, r0ab), **m)
    e2, f2 = dftd3_zero_atm(_t(pos), _t(z), 10.0, cutoff_radii=_t(bj), d3_params=_params(t, r0ab), **m)
    assert abs(float(e1) - float(e2)) <= 4e-6 * (1.0 + abs(float(e1))) and float((f1 - f2).abs().max()) <= 4 * (1e-6 + 5e-6 * float(f1.abs().max()))
    base = float(dftd3_zero_atm(_t(pos), _t(z), 10.0, d3_params=_params(t, r0ab), **m)[0])
    for kw in (dict(rs9=1.0), dict(alpha=14.0), dict(s9=0.5)):
        r64, r32 = _references(pos, z, t, r0ab, 13.0, 10.0, **kw)
        out = dftd3_zero_atm(_t(pos), _t(z), 10.0, d3_params=_params(t, r0ab), **kw, **m)
        _judge(f"{kw}", out, r64, r32)
        assert float(out[0]) != base and base != float(e1)


def test_general_tables_more_than_16_species_and_missing_radii():
    """The other table paths of the triple pass (25-term form from the compact table; global table above 16 species; factorised with 7 - 16
    species: radii and c6 rows through L1 instead of LDS), a padding atom, and species pairs without a radius."""
    from nvalchemiops.interactions.dispersion import dftd3_zero_atm

    pos, _, _ = S.molecule(30, density=0.03, min_dist=2.0, seed=21)
    for kind in ("general", "20 species", "10 species", "factorised"):
        t, r0ab = _tables("factorised" if kind == "10 species" else kind)
        z = _z20(30) if kind == "20 species" else ((np.arange(30) % 10 + 1).astype(np.int32) if kind == "10 species" else _zs(30, 21))
        z = z.copy()
        z[7] = 0
        r0ab = r0ab.copy()
        r0ab[6, 8] = r0ab[8, 6] = 0.0
        r0ab[1, 1] = -1.0
        m, l = _lists(pos, None, 13.0)
        r64, r32 = _references(pos, z, t, r0ab, 13.0, 10.0)
        assert abs(r64["energy"][0]) > 0.0
        for tag, lk in (("matrix", m), ("csr", l)):
            out = dftd3_zero_atm(_t(pos), _t(z), 10.0, d3_params=_params(t, r0ab), **lk)
            _judge(f"{kind} {tag}", out, r64, r32)
            assert torch.equal(out[1][7], torch.zeros(3, device=DEV))


@pytest.mark.parametrize("triclinic,dtype", [(False, np.float32), (True, np.float32), (True, np.float64)])
def test_periodic_boxes_energy_forces_virial(triclinic, dtype):
    from nvalchemiops.interactions.dispersion import dftd3_zero_atm

    shape = (5, 5, 6) if triclinic else (5, 5, 5)
    pos, cell = A.lattice_box(shape, seed=7, triclinic=triclinic, dtype=dtype)
    n = len(pos)
    z = _zs(n, 7)
    t, r0ab = _tables()
    p = _params(t, r0ab)
    rc_list, rc3 = 10.0, 8.5
    m, l = _lists(pos, cell, rc_list, max_neighbors=160)
    r64, r32 = _references(pos, z, t, r0ab, rc_list, rc3, cell=cell)
    tc = _t(cell.reshape(1, 3, 3))
    a = dftd3_zero_atm(_t(pos), _t(z), rc3, d3_params=p, cell=tc, compute_virial=True, **m)
    b = dftd3_zero_atm(_t(pos), _t(z), rc3, d3_params=p, cell=tc, compute_virial=True, **l)
    assert a[2].shape == (1, 3, 3) and a[2].dtype == torch.float32
    tag = f"{'triclinic' if triclinic else 'cubic'} {n} {np.dtype(dtype).name}"
    _judge(tag + " matrix", a, r64, r32)
    _judge(tag + " csr", b, r64, r32)
    assert float(a[1].double().sum(0).abs().max()) <= 1e-5 * float(a[1].abs().max()) * np.sqrt(n)


def test_batch_of_three_systems():
    from nvalchemiops.interactions.dispersion import dftd3_zero_atm

    boxes = [A.lattice_box((3, 3, 3), seed=1, triclinic=False), A.lattice_box((4, 3, 3), seed=2, triclinic=True), A.lattice_box((2, 3, 2), a=4.6, seed=3, triclinic=True)]
    pos = np.concatenate([b[0] for b in boxes])
    cell = np.stack([b[1] for b in boxes])
    bi = np.concatenate([np.full(len(b[0]), k, np.int32) for k, b in enumerate(boxes)])
    z = _zs(len(pos), 5)
    t, r0ab = _tables()
    rc_list, rc3 = 8.0, 6.5
    m, l = _lists(pos, cell, rc_list, batch_idx=bi, max_neighbors=200)
    r64, r32 = _references(pos, z, t, r0ab, rc_list, rc3, cell=cell, batch_idx=bi)
    for tag, lk in (("matrix", m), ("csr", l)):
        out = dftd3_zero_atm(_t(pos), _t(z), rc3, d3_params=_params(t, r0ab), cell=_t(cell), batch_idx=_t(bi), compute_virial=True, **lk)
        assert out[0].shape == (3,) and out[2].shape == (3, 3, 3)
        _judge("batch of three " + tag, out, r64, r32)


def test_dense_row_needs_more_than_one_lds_tile():
    from nvalchemiops.interactions.dispersion import dftd3_zero_atm
    from nvalchemiops.interactions.dispersion.dftd3 import atm_tile

    tile = atm_tile()
    n = tile + 8
    pos, _ = A.lattice_box((7, 7, 8), a=3.4, jitter=0.2, seed=13, triclinic=False)
    pos = pos[:n]
    z = _zs(n, 13, (1, 6, 8))
    t, r0ab = _tables()
    rc = 2.0 * float(np.linalg.norm(pos.max(0) - pos.min(0)))  # everything is everybody's neighbour
    m, l = _lists(pos, None, rc)
    assert int((m["neighbor_matrix"] < n).sum(1).max()) == n - 1 > tile
    r64, r32 = _references(pos, z, t, r0ab, rc, rc)
    _judge(f"dense row ({n - 1} staged) matrix", dftd3_zero_atm(_t(pos), _t(z), rc, d3_params=_params(t, r0ab), **m), r64, r32)
    _judge(f"dense row ({n - 1} staged) csr", dftd3_zero_atm(_t(pos), _t(z), rc, d3_params=_params(t, r0ab), **l), r64, r32)


def test_row_of_three_lds_tiles_runs_every_tile_pair_once():
    """The system of tests/test_d3_atm_gpu.py's test of the same name with the table radii of this file's dense test."""
    from nvalchemiops.interactions.dispersion import dftd3_zero_atm
    from nvalchemiops.interactions.dispersion.dftd3 import atm_scalars
    from tests.test_d3_atm_gpu import _visits, shell_system

    pos, z, tile, pairs0, triples = shell_system()
    t, r0ab = _tables()
    m, l = _lists(pos, None, 40.0)
    assert int((m["neighbor_matrix"] < len(pos)).sum(1).min()) == len(pos) - 1
    r64, r32 = _references(pos, z, t, r0ab, 40.0, 20.0)
    _judge("three-tile row matrix", dftd3_zero_atm(_t(pos), _t(z), 20.0, d3_params=_params(t, r0ab), **m), r64, r32)
    _judge("three-tile row csr", dftd3_zero_atm(_t(pos), _t(z), 20.0, d3_params=_params(t, r0ab), **l), r64, r32)
    visits = _visits(pos, z, t, m, 20.0, atm_scalars(0.0, 0.0, 16.0, -4.0), zero=(4.0 / 3.0, _t(r0ab)))
    assert r64["triples"] == triples
    assert visits[0] == pairs0 and int(visits.sum()) == 3 * r64["triples"], (visits[0], pairs0, int(visits.sum()), 3 * r64["triples"])


def test_renumbering_and_dftd3_atm_untouched():
    from nvalchemiops.interactions.dispersion import dftd3_atm, dftd3_zero_atm

    pos, cell = A.lattice_box((5, 4, 4), seed=17, triclinic=True)
    n = len(pos)
    z = _zs(n, 17)
    t, r0ab = _tables()
    p = _params(t, r0ab)
    tc = _t(cell.reshape(1, 3, 3))
    rc_list, rc3 = 10.0, 7.5
    m, _ = _lists(pos, cell, rc_list, max_neighbors=200)
    tp, tz = _t(pos), _t(z)
    bj = dict(a1=0.4, a2=4.0, three_body_cutoff=rc3, d3_params=p, cell=tc, compute_virial=True, **m)
    before = dftd3_atm(tp, tz, **bj)
    out = dftd3_zero_atm(tp, tz, rc3, d3_params=p, cell=tc, compute_virial=True, **m)
    after = dftd3_atm(tp, tz, **bj)
    assert all(torch.equal(a, b) for a, b in zip(before, after)), "dftd3_atm must not see that dftd3_zero_atm ran on the same tensors"
    r64, r32 = _references(pos, z, t, r0ab, rc_list, rc3, cell=cell)
    _judge("original numbering", out, r64, r32)
    perm = np.random.default_rng(0).permutation(n)
    m2, _ = _lists(pos[perm], cell, rc_list, max_neighbors=200)
    out2 = dftd3_zero_atm(_t(pos[perm]), _t(z[perm]), rc3, d3_params=p, cell=tc, compute_virial=True, **m2)
    _judge("renumbered", out2, dict(r64, forces=r64["forces"][perm]), dict(r32, forces=r32["forces"][perm]))


def test_fullgraph_compile_of_dftd3_zero_plus_atm_equals_eager():
    from nvalchemiops.interactions.dispersion import dftd3_zero, dftd3_zero_atm

    pos, cell = A.lattice_box((5, 4, 4), seed=19, triclinic=True)
    z = _t(_zs(len(pos), 19))
    t, r0ab = _tables()
    p = _params(t, r0ab)
    tc = _t(cell.reshape(1, 3, 3))
    m, l = _lists(pos, cell, 10.0, max_neighbors=200)
    # copies carry no companion of the search: the eager call then walks the arrays like the op does (with a companion whose search-side
    # coordination numbers it adopts, eager differs from the op by the documented CN tolerance -- that path has its own test)
    m = {k: v.clone() for k, v in m.items()}

    def total_matrix(x):
        e2, f2, cn, v2 = dftd3_zero(x, z, d3_params=p, cell=tc, compute_virial=True, **ZERO, **m)
        e3, f3, v3 = dftd3_zero_atm(x, z, 7.5, d3_params=p, cell=tc, compute_virial=True, **m)
        return e2 + e3, f2 + f3, v2 + v3, e3

    def total_csr(x):
        e2, f2, cn = dftd3_zero(x, z, d3_params=p, cell=tc, beta=0.05, **ZERO, **l)
        e3, f3 = dftd3_zero_atm(x, z, 7.5, alpha=14.0, rs9=1.2, d3_params=p, cell=tc, **l)
        return e2 + e3, f2 + f3, e3

    for fn in (total_matrix, total_csr):
        torch._dynamo.reset()
        got = torch.compile(fn, mode="default", fullgraph=True)(_t(pos))
        want = fn(_t(pos))
        assert float(want[-1].abs()) > 0.0
        assert len(got) == len(want) and all(torch.equal(a, b) for a, b in zip(got, want))
