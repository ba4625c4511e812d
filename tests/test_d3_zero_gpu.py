"""`dftd3_zero` (DFT-D3 with zero damping, D3(0) / D3M(0): the zero-damping instantiations of the HIP energy kernels) against the float64
restatement tests/d3_zero_reference.py.

Lists are built by this package's `neighbor_list` / `cell_list`.  Bars (the ATM suite's rule): the restatement is evaluated once in float64
and once with every per-pair quantity in float32 (float64 sums: the kernels' arithmetic model); a quantity's bar is 4 x the larger of that
float32-vs-float64 deviation on the same system and `dftd3`'s existing bar (tests/test_d3_gpu.py: energy and coordination numbers
rtol = atol = 1e-6; forces rtol 1e-6, atol 1e-6 + 5e-6 max|F|; virial rtol 1e-6, atol 1e-6 + 2e-7 max|V|).  Every atom and every system of
every input is compared; each figure is printed before it is asserted (`pytest -s`).

The three-body term with table radii (`dftd3_zero_atm`) has its own module, tests/test_d3_zero_atm_gpu.py.

MEASURED on one MI355X (max over components; restatement float32 vs float64 | kernel vs float64 restatement | worst err / bar; matrix and
CSR agree to the digits shown -- the larger of the two is listed; every test prints its figures under `pytest -s`; the table with max|ref|
is in DESIGN.md section 3.11):
  molecule3                                E 2.8e-10 | 1.1e-09 | 0.000   F 7.7e-10 | 1.4e-09 | 0.000
  molecule7                                E 5.8e-08 | 3.6e-08 | 0.008   F 9.1e-09 | 2.2e-08 | 0.004
  molecule24                               E 2.9e-08 | 5.6e-11 | 0.000   F 6.4e-08 | 1.0e-07 | 0.015
  molecule60                               E 4.6e-07 | 1.3e-06 | 0.038   F 1.9e-07 | 4.9e-07 | 0.038
  general beta 0                           E 2.1e-06 | 2.7e-06 | 0.078   F 3.6e-06 | 1.0e-06 | 0.061
  general beta 0.05                        E 2.0e-05 | 2.9e-05 | 0.116   F 9.8e-06 | 6.6e-06 | 0.043
  20 species beta 0                        E 2.3e-07 | 9.3e-07 | 0.052   F 1.1e-06 | 5.0e-07 | 0.044
  20 species beta 0.05                     E 2.3e-06 | 1.2e-05 | 0.105   F 1.5e-05 | 2.7e-06 | 0.047
  alpha 14                                 E 1.2e-07 | 6.3e-07 | 0.045   F 3.8e-07 | 2.3e-07 | 0.022
  alpha 13.5                               E 9.1e-08 | 6.0e-07 | 0.043   F 1.9e-07 | 2.4e-07 | 0.023
  beta 0.05                                E 1.7e-07 | 3.3e-06 | 0.064   F 1.7e-06 | 6.2e-07 | 0.024
  beta 0.05 alpha 13.5                     E 1.5e-06 | 6.0e-07 | 0.007   F 6.1e-06 | 1.5e-06 | 0.023
  s8 0                                     E 1.8e-08 | 3.5e-08 | 0.006   F 3.0e-08 | 6.5e-09 | 0.001
  s6 0.8 rs8 0.85                          E 1.0e-06 | 1.7e-06 | 0.061   F 6.1e-07 | 5.9e-07 | 0.028
  s5 switch                                E 1.4e-07 | 4.6e-07 | 0.039   F 3.1e-07 | 2.4e-07 | 0.023
  padding atom, missing radii factorised   E 4.8e-09 | 1.5e-08 | 0.003   F 4.1e-09 | 4.6e-09 | 0.001
  padding atom, missing radii general      E 7.9e-09 | 1.3e-08 | 0.003   F 5.8e-09 | 5.8e-09 | 0.001
  cubic 125 float32                        E 1.7e-07 | 2.8e-06 | 0.044   F 1.5e-07 | 3.3e-07 | 0.035   V 1.1e-06 | 6.6e-06 | 0.091
  cubic 125 float32 D3M                    E 2.3e-06 | 5.7e-06 | 0.032   F 4.2e-07 | 8.7e-07 | 0.039   V 3.0e-06 | 9.2e-06 | 0.037
  triclinic 150 float32                    E 9.2e-07 | 3.6e-06 | 0.049   F 2.6e-07 | 4.1e-07 | 0.036   V 2.3e-06 | 5.9e-06 | 0.067
  triclinic 150 float32 D3M                E 9.6e-07 | 9.9e-06 | 0.044   F 6.5e-07 | 8.9e-07 | 0.036   V 8.6e-06 | 1.5e-05 | 0.080
  triclinic 150 float64                    E 4.4e-07 | 3.0e-06 | 0.040   F 2.1e-07 | 3.6e-07 | 0.029   V 2.1e-06 | 8.0e-06 | 0.102
  triclinic 150 float64 D3M                E 2.2e-06 | 6.5e-06 | 0.029   F 4.4e-07 | 8.2e-07 | 0.033   V 3.6e-06 | 1.8e-05 | 0.062
  periodic general                         E 3.9e-06 | 1.1e-05 | 0.066   F 6.5e-07 | 1.4e-06 | 0.046   V 5.9e-06 | 1.3e-05 | 0.065
  periodic 20 species                      E 3.9e-06 | 2.8e-06 | 0.013   F 2.1e-06 | 4.2e-06 | 0.086   V 8.5e-06 | 1.5e-05 | 0.069
  small cell                               E 1.3e-08 | 2.2e-08 | 0.004   F 3.5e-08 | 8.7e-08 | 0.016   V 1.9e-07 | 3.2e-07 | 0.052
  batch of three                           E 1.7e-07 | 1.4e-06 | 0.054   F 1.7e-07 | 2.8e-07 | 0.022   V 8.6e-07 | 2.9e-06 | 0.116
  close contact alpha 14                   E 3.3e-07 | 3.0e-07 | 0.017   F 1.7e-07 | 1.4e-07 | 0.016   V 7.9e-07 | 1.6e-06 | 0.147
  close contact alpha 13.5                 E 3.5e-07 | 5.0e-07 | 0.029   F 1.5e-07 | 2.4e-07 | 0.029   V 6.6e-07 | 2.0e-06 | 0.132
Coordination numbers (not listed: they are `dftd3`'s pass): worst err / bar 0.099.  The adopted-CN comparison against the array path sits at
0.44 of `dftd3`'s own bar (coordination numbers: 1.9e-6 on 4.8).  Worst err / bar of any listed figure: 0.147.
"""

import numpy as np
import pytest
import torch

from tests import atm_reference as A
from tests import d3_zero_reference as Z
from tests import systems as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ZERO = dict(rs6=1.217, s8=0.722)  # (the size of a published D3(0) parameter set; rs8 = 1, alpha = 14, beta = 0 are the defaults)


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def _params(t, r0ab):
    """The tables as the dict form of `d3_params`, radii under the key "r0ab"."""
    return {"rcov": _t(t["rcov"]), "r4r2": _t(t["r4r2"]), "c6ab": _t(t["c6ab"]), "cn_ref": _t(t["cn_ref"]), "r0ab": _t(r0ab)}


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
    return m, l


_REF_NAMES = dict(s5_smoothing_on="s5_on", s5_smoothing_off="s5_off")


def _references(pos, z, t, r0ab, rc, cell=None, batch_idx=None, **zero):
    kw = {_REF_NAMES.get(k, k): v for k, v in dict(ZERO, **zero).items()}
    kw.update(list_cutoff=rc, cell=cell, batch_idx=batch_idx)
    return Z.reference(pos, z, t, r0ab, **kw), Z.reference(pos, z, t, r0ab, work_dtype=torch.float32, **kw)


_EXTRA = {"energy": 0.0, "forces": 5e-6, "cn": 0.0, "virial": 2e-7}


def _judge(name, out, r64, r32, atoms=None):
    """Asserts out = (energy, forces, coord_num[, virial]) against the float64 restatement at the module's bars; prints the figures first.
    `atoms`: boolean mask of the atoms whose forces / coordination numbers are compared here (default: all)."""
    got = [o.detach().cpu().numpy().astype(np.float64) for o in out]
    keys = ["energy", "forces", "cn"] + (["virial"] if len(got) == 4 else [])
    fails = []
    for g, k in zip(got, keys):
        ref, low = r64[k], r32[k]
        assert g.shape == ref.shape, (k, g.shape, ref.shape)
        assert np.isfinite(g).all(), k
        if atoms is not None and k in ("forces", "cn"):
            g, ref, low = g[atoms], ref[atoms], low[atoms]
        dev32 = np.abs(low - ref).max() if ref.size else 0.0
        scale = np.abs(ref).max() if ref.size else 0.0
        bar = 4.0 * np.maximum(dev32, 1e-6 + 1e-6 * np.abs(ref) + _EXTRA[k] * scale)
        err = np.abs(g - ref)
        worst = (err / bar).max() if ref.size else 0.0
        print(f"[d3zero] {name:36s} {k:7s} max|ref| {scale:.3e}  fp32-vs-fp64 {dev32:.3e}  kernel-vs-fp64 {err.max() if ref.size else 0.0:.3e}  "
              f"worst err/bar {worst:.3f}")
        if not (err <= bar).all():
            fails.append(f"{k}: max err {err.max():.3e}, bar {bar.flat[(err / bar).argmax()]:.3e}")
    assert not fails, f"{name}: " + "; ".join(fails)


def _zs(n, seed, choices=(1, 6, 8, 17)):
    return np.random.default_rng(seed).choice(np.array(choices, np.int32), n)


def _tables(kind="factorised"):
    """(tables, r0ab) for the three C6 paths of the energy pass: factorised weights (MODE 2), tables whose reference CN depends on the
    partner (the 25-term form from the compact table, MODE 1), and -- with the 20-species numbering of `_z20` -- the global table (MODE 0)."""
    if kind == "factorised":
        return S.d3_test_tables(17), Z.synthetic_r0ab(18)
    if kind == "general":
        t = {k: v.copy() for k, v in S.d3_test_tables(17).items()}
        t["cn_ref"] *= (1.0 + 0.01 * np.arange(18, dtype=np.float32)[None, :, None, None])
        return t, Z.synthetic_r0ab(18)
    return S.d3_test_tables(30, seed=5), Z.synthetic_r0ab(31)


def _z20(n):
    return (np.arange(n) % 20 + 1).astype(np.int32)


# ---- molecules -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,seed", [(3, 1), (7, 2), (24, 3), (60, 4)])
def test_molecules_matrix_and_csr(n, seed):
    from nvalchemiops.interactions.dispersion import dftd3_zero

    pos, _, _ = S.molecule(n, density=0.02, min_dist=2.0, seed=seed)
    z = _zs(n, seed)
    t, r0ab = _tables()
    p = _params(t, r0ab)
    m, l = _lists(pos, None, 14.0)
    r64, r32 = _references(pos, z, t, r0ab, 14.0)
    assert r64["energy"][0] < 0.0
    a = dftd3_zero(_t(pos), _t(z), d3_params=p, **ZERO, **m)
    b = dftd3_zero(_t(pos), _t(z), d3_params=p, **ZERO, **l)
    assert len(a) == 3 and all(o.dtype == torch.float32 for o in a) and a[0].shape == (1,) and a[1].shape == (n, 3) and a[2].shape == (n,)
    _judge(f"molecule{n} matrix", a, r64, r32)
    _judge(f"molecule{n} csr", b, r64, r32)


def test_explicit_radii_next_to_d3parameters_equal_the_dict_form():
    from nvalchemiops.interactions.dispersion import D3Parameters, dftd3_zero

    pos, _, _ = S.molecule(24, density=0.02, min_dist=2.0, seed=3)
    z = _zs(24, 3)
    t, r0ab = _tables()
    p = _params(t, r0ab)
    m, _ = _lists(pos, None, 14.0)
    a = dftd3_zero(_t(pos), _t(z), d3_params=p, **ZERO, **m)
    dp = D3Parameters(rcov=p["rcov"], r4r2=p["r4r2"], c6ab=p["c6ab"], cn_ref=p["cn_ref"])
    b = dftd3_zero(_t(pos), _t(z), d3_params=dp, cutoff_radii=_t(r0ab.astype(np.float64)), **ZERO, **m)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("kind", ["general", "20 species"])
def test_tables_that_do_not_factorise_and_more_than_16_species(kind):
    """MODE 1 (pair constants in the spare word of the LDS-staged compact table) and MODE 0 (in the global table), plain lists."""
    from nvalchemiops.interactions.dispersion import dftd3_zero

    pos, _, _ = S.molecule(30, density=0.03, min_dist=2.0, seed=21)
    t, r0ab = _tables(kind)
    z = _z20(30) if kind == "20 species" else _zs(30, 21)
    m, l = _lists(pos, None, 13.0)
    for beta in (0.0, 0.05):
        r64, r32 = _references(pos, z, t, r0ab, 13.0, beta=beta, rs8=0.9)
        for tag, lk in (("matrix", m), ("csr", l)):
            out = dftd3_zero(_t(pos), _t(z), d3_params=_params(t, r0ab), beta=beta, rs8=0.9, **ZERO, **lk)
            _judge(f"{kind} beta {beta:g} {tag}", out, r64, r32)


def test_beta_alpha_s8_and_switch_variants():
    """beta = 0 and beta != 0; alpha = 14 (powers by squaring) and 13.5 (log2 / exp2) both match and differ from each other; s8 = 0;
    the S5 switch on."""
    from nvalchemiops.interactions.dispersion import dftd3_zero

    pos, _, _ = S.molecule(40, density=0.03, min_dist=2.0, seed=12)
    z = _zs(40, 12)
    t, r0ab = _tables()
    p = _params(t, r0ab)
    m, l = _lists(pos, None, 13.0)
    outs = {}
    variants = {"alpha 14": dict(alpha=14.0), "alpha 13.5": dict(alpha=13.5), "beta 0.05": dict(beta=0.05, rs8=1.1), "beta 0.05 alpha 13.5": dict(beta=0.05, alpha=13.5),
                "s8 0": dict(s8=0.0), "s6 0.8 rs8 0.85": dict(s6=0.8, rs8=0.85), "s5 switch": dict(s5_smoothing_on=6.0, s5_smoothing_off=11.0)}
    for name, kw in variants.items():
        r64, r32 = _references(pos, z, t, r0ab, 13.0, **kw)
        call = dict(ZERO, **kw)
        outs[name] = dftd3_zero(_t(pos), _t(z), d3_params=p, **call, **m)
        _judge(name + " matrix", outs[name], r64, r32)
        _judge(name + " csr", dftd3_zero(_t(pos), _t(z), d3_params=p, **call, **l), r64, r32)
    e = {k: float(v[0]) for k, v in outs.items()}
    assert e["alpha 14"] != e["alpha 13.5"] and e["alpha 14"] != e["beta 0.05"] and e["alpha 14"] != e["s8 0"] and e["alpha 14"] != e["s5 switch"]
    assert all(torch.equal(outs["alpha 14"][2], v[2]) for v in outs.values()), "the coordination numbers do not know about the damping"


def test_padding_atom_and_species_pair_without_radius():
    from nvalchemiops.interactions.dispersion import dftd3_zero

    pos, _, _ = S.molecule(12, density=0.02, min_dist=2.0, seed=8)
    z = _zs(12, 8, (6, 8, 17))
    z[4] = 0
    for kind in ("factorised", "general"):
        t, r0ab = _tables(kind)
        r0ab = r0ab.copy()
        r0ab[6, 8] = r0ab[8, 6] = 0.0
        r0ab[17, 17] = -2.0
        m, l = _lists(pos, None, 14.0)
        r64, r32 = _references(pos, z, t, r0ab, 14.0)
        for tag, lk in (("matrix", m), ("csr", l)):
            out = dftd3_zero(_t(pos), _t(z), d3_params=_params(t, r0ab), **ZERO, **lk)
            _judge(f"padding atom, missing radii {kind} {tag}", out, r64, r32)
            assert torch.equal(out[1][4], torch.zeros(3, device=DEV)) and float(out[2][4]) == 0.0
    # only pairs without a radius: exact zeros (the coordination numbers are still there)
    t, r0ab = _tables()
    r0ab = r0ab.copy()
    r0ab[6, 8] = r0ab[8, 6] = 0.0
    pk = np.array([[0, 0, 0], [3.0, 0, 0]], np.float32)
    nm = np.array([[1, 2], [0, 2]], np.int32)
    e, f, cn = dftd3_zero(_t(pk), _t(np.array([6, 8], np.int32)), d3_params=_params(t, r0ab), neighbor_matrix=_t(nm), **ZERO)
    assert float(e.abs().max()) == 0.0 and float(f.abs().max()) == 0.0 and float(cn.min()) > 0.0


# ---- periodic ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("triclinic,dtype", [(False, np.float32), (True, np.float32), (True, np.float64)])
def test_periodic_boxes_energy_forces_virial(triclinic, dtype):
    """100-150 atoms; the matrix runs the packed-list kernels, the CSR list the plain ones; fp64 positions the uncapped wrappers."""
    from nvalchemiops.interactions.dispersion import dftd3_zero

    shape = (5, 5, 6) if triclinic else (5, 5, 5)
    pos, cell = A.lattice_box(shape, seed=7, triclinic=triclinic, dtype=dtype)
    n = len(pos)
    z = _zs(n, 7)
    t, r0ab = _tables()
    p = _params(t, r0ab)
    rc = 10.0
    m, l = _lists(pos, cell, rc, max_neighbors=160)
    tc = _t(cell.reshape(1, 3, 3))
    for name, kw in (("", {}), (" D3M", dict(beta=0.04, rs8=1.05, alpha=13.5))):
        r64, r32 = _references(pos, z, t, r0ab, rc, cell=cell, **kw)
        call = dict(ZERO, **kw)
        a = dftd3_zero(_t(pos), _t(z), d3_params=p, cell=tc, compute_virial=True, **call, **m)
        b = dftd3_zero(_t(pos), _t(z), d3_params=p, cell=tc, compute_virial=True, **call, **l)
        assert len(a) == 4 and a[3].shape == (1, 3, 3) and a[3].dtype == torch.float32
        tag = f"{'triclinic' if triclinic else 'cubic'} {n} {np.dtype(dtype).name}{name}"
        _judge(tag + " matrix", a, r64, r32)
        _judge(tag + " csr", b, r64, r32)
        assert float(a[1].double().sum(0).abs().max()) <= 1e-5 * float(a[1].abs().max()) * np.sqrt(n)
        c = dftd3_zero(_t(pos), _t(z), d3_params=p, cell=tc, **call, **m)  # without the virial: the same numbers
        assert len(c) == 3 and all(torch.equal(x, y) for x, y in zip(a[:3], c))


@pytest.mark.parametrize("kind", ["general", "20 species"])
def test_periodic_matrix_with_the_other_table_paths(kind):
    """Packed list x MODE 1 / MODE 0: the bodies of the fallback launch."""
    from nvalchemiops.interactions.dispersion import dftd3_zero

    pos, cell = A.lattice_box((4, 4, 5), seed=11, triclinic=True)
    n = len(pos)
    t, r0ab = _tables(kind)
    z = _z20(n) if kind == "20 species" else _zs(n, 11)
    rc = 9.0
    m, l = _lists(pos, cell, rc, max_neighbors=140)
    tc = _t(cell.reshape(1, 3, 3))
    r64, r32 = _references(pos, z, t, r0ab, rc, cell=cell, beta=0.03)
    for tag, lk in (("matrix", m), ("csr", l)):
        out = dftd3_zero(_t(pos), _t(z), d3_params=_params(t, r0ab), cell=tc, compute_virial=True, beta=0.03, **ZERO, **lk)
        _judge(f"periodic {kind} {tag}", out, r64, r32)


def test_small_cell_own_images():
    from nvalchemiops.interactions.dispersion import dftd3_zero

    pos, cell = A.lattice_box((2, 2, 2), a=3.6, jitter=0.2, seed=9, triclinic=True)
    z = _zs(8, 9, (6, 8))
    t, r0ab = _tables()
    rc = 9.5
    m, l = _lists(pos, cell, rc, max_neighbors=400)
    nm, sh = m["neighbor_matrix"].cpu().numpy(), m["neighbor_matrix_shifts"].cpu().numpy()
    assert ((nm[0] == 0) & (np.abs(sh[0]).sum(1) > 0)).any(), "the test needs rows with the atom's own images"
    r64, r32 = _references(pos, z, t, r0ab, rc, cell=cell)
    tc = _t(cell.reshape(1, 3, 3))
    for tag, lk in (("matrix", m), ("csr", l)):
        out = dftd3_zero(_t(pos), _t(z), d3_params=_params(t, r0ab), cell=tc, compute_virial=True, **ZERO, **lk)
        _judge("small cell " + tag, out, r64, r32)


def test_batch_of_three_systems():
    from nvalchemiops.interactions.dispersion import dftd3_zero

    boxes = [A.lattice_box((3, 3, 3), seed=1, triclinic=False), A.lattice_box((4, 3, 3), seed=2, triclinic=True), A.lattice_box((2, 3, 2), a=4.6, seed=3, triclinic=True)]
    pos = np.concatenate([b[0] for b in boxes])
    cell = np.stack([b[1] for b in boxes])
    bi = np.concatenate([np.full(len(b[0]), k, np.int32) for k, b in enumerate(boxes)])
    n = len(pos)
    z = _zs(n, 5)
    t, r0ab = _tables()
    rc = 8.0
    m, l = _lists(pos, cell, rc, batch_idx=bi, max_neighbors=200)
    r64, r32 = _references(pos, z, t, r0ab, rc, cell=cell, batch_idx=bi)
    for tag, lk in (("matrix", m), ("csr", l)):
        out = dftd3_zero(_t(pos), _t(z), d3_params=_params(t, r0ab), cell=_t(cell), batch_idx=_t(bi), compute_virial=True, **ZERO, **lk)
        assert out[0].shape == (3,) and out[3].shape == (3, 3, 3)
        _judge("batch of three " + tag, out, r64, r32)


@pytest.mark.parametrize("alpha", [14.0, 13.5])
def test_close_contact_stays_finite(alpha):
    """One pair at 0.01 Bohr: (R0 / r)^alpha overflows float32.  Everything is finite; every other atom is within the bars of the float64
    restatement; the two atoms of the contact are compared with the float32 mode of the restatement only (its arithmetic model is the
    kernels'; in float64 nothing overflows), at 4 x `dftd3`'s bar."""
    from nvalchemiops.interactions.dispersion import dftd3_zero

    pos, cell = A.lattice_box((4, 4, 4), seed=23, triclinic=True)
    pos = pos.copy()
    pos[11] = pos[10] + np.array([0.006, 0.008, 0.0], np.float32)
    n = len(pos)
    z = _zs(n, 23)
    t, r0ab = _tables()
    rc = 9.0
    m, l = _lists(pos, cell, rc, max_neighbors=150)
    r64, r32 = _references(pos, z, t, r0ab, rc, cell=cell, alpha=alpha)
    assert np.isfinite(r32["forces"]).all()
    far = np.ones(n, bool)
    far[[10, 11]] = False
    tc = _t(cell.reshape(1, 3, 3))
    for tag, lk in (("matrix", m), ("csr", l)):
        out = dftd3_zero(_t(pos), _t(z), d3_params=_params(t, r0ab), cell=tc, compute_virial=True, alpha=alpha, **ZERO, **lk)
        assert all(bool(torch.isfinite(o).all()) for o in out)
        _judge(f"close contact alpha {alpha:g} {tag}", out, r64, r32, atoms=far)
        f = out[1].cpu().numpy().astype(np.float64)[~far]
        ref = r32["forces"][~far]
        bar = 4.0 * (1e-6 + 1e-6 * np.abs(ref) + 5e-6 * np.abs(r32["forces"]).max())
        err = np.abs(f - ref)
        print(f"[d3zero] contact pair {tag} alpha {alpha:g}: max|F| {np.abs(ref).max():.3e}  kernel-vs-fp32-restatement {err.max():.3e}  worst err/bar {(err / bar).max():.3f}")
        assert (err <= bar).all()


# ---- the companion of the neighbour search -------------------------------------------------------------------------------------------

def test_packed_companion_and_search_side_coordination_numbers(monkeypatch):
    """search -> dftd3_zero -> search -> dftd3_zero, the headline-style sequence: the second call finds the companion and the coordination
    numbers the search summed, and adopts them (CN output = the search's block bit for bit, as tests/test_search_cn_gpu.py observes it).
    Against the array path (copies of matrix and shifts, which carry no companion): with the search's coordination numbers switched off the
    companion path is bit-identical; with them adopted the coordination numbers differ by the documented <= 1e-6 relative
    (include/nvalchemiops_hip.h, mi_d3_packed_cn) and energy / forces / virial stay inside `dftd3`'s own bars of the array path."""
    from nvalchemiops.interactions.dispersion import dftd3_zero
    from nvalchemiops.neighborlist import _engine as E
    from nvalchemiops.neighborlist import cell_list

    monkeypatch.setattr(E, "_PACKED_POLICY", "auto")
    monkeypatch.setattr(E, "_PACKED_WANTED", set())
    monkeypatch.setattr(E, "_D3CTX_BY_SHAPE", {})
    t, r0ab = _tables()
    p = _params(t, r0ab)
    pos, cell, _, numbers = S.fcc_box(2048, seed=9, dtype=np.float32)
    tp, tz, tc = _t(pos), _t(numbers), _t(cell)
    pbc = torch.tensor([True] * 3, device=DEV)
    n, width = 2048, 256
    nm = torch.empty((n, width), dtype=torch.int32, device=DEV)
    sh = torch.empty((n, width, 3), dtype=torch.int32, device=DEV)
    num = torch.empty(n, dtype=torch.int32, device=DEV)
    call = dict(d3_params=p, cell=tc[None], compute_virial=True, beta=0.02, **ZERO)
    cell_list(tp, 9.0, tc, pbc, neighbor_matrix=nm, neighbor_matrix_shifts=sh, num_neighbors=num)
    assert not hasattr(nm, E._PACKED_ATTR)
    array_path = dftd3_zero(tp, tz, neighbor_matrix=nm.clone(), neighbor_matrix_shifts=sh.clone(), **call)
    first = dftd3_zero(tp, tz, neighbor_matrix=nm, neighbor_matrix_shifts=sh, **call)  # no companion yet; learns shape + species
    assert all(torch.equal(a, b) for a, b in zip(first, array_path))
    cell_list(tp, 9.0, tc, pbc, neighbor_matrix=nm, neighbor_matrix_shifts=sh, num_neighbors=num)
    rec = getattr(nm, E._PACKED_ATTR)
    assert rec.cn is not None and rec.words is not None
    second = dftd3_zero(tp, tz, neighbor_matrix=nm, neighbor_matrix_shifts=sh, **call)
    assert torch.equal(second[2], rec.cn[1024:].view(torch.float32)), "the search's coordination numbers were not adopted"
    monkeypatch.setenv("NVALCHEMIOPS_D3_SEARCH_CN", "0")
    companion_only = dftd3_zero(tp, tz, neighbor_matrix=nm, neighbor_matrix_shifts=sh, **call)
    monkeypatch.delenv("NVALCHEMIOPS_D3_SEARCH_CN")
    assert all(torch.equal(a, b) for a, b in zip(companion_only, array_path)), "companion path without adopted CN: bit-identical"
    extra = [0.0, 5e-6, 0.0, 2e-7]
    for k, (a, b) in enumerate(zip(second, array_path)):
        a, b = a.double(), b.double()
        bar = 1e-6 + 1e-6 * b.abs() + extra[k] * b.abs().max()
        print(f"[d3zero] adopted CN vs array path, output {k}: max|ref| {float(b.abs().max()):.3e} max err {float((a - b).abs().max()):.3e} "
              f"worst err/bar {float(((a - b).abs() / bar).max()):.3f}")
        assert bool(((a - b).abs() <= bar).all())
    assert float(array_path[0].abs()) > 0.0


# ---- invariances ---------------------------------------------------------------------------------------------------------------------

def test_dftd3_is_untouched_by_a_dftd3_zero_call():
    from nvalchemiops.interactions.dispersion import D3Parameters, dftd3, dftd3_zero

    pos, cell = A.lattice_box((5, 4, 4), seed=17, triclinic=True)
    z = _zs(len(pos), 17)
    t, r0ab = _tables()
    p = _params(t, r0ab)
    dp = D3Parameters(rcov=p["rcov"], r4r2=p["r4r2"], c6ab=p["c6ab"], cn_ref=p["cn_ref"])
    tc = _t(cell.reshape(1, 3, 3))
    m, l = _lists(pos, cell, 10.0, max_neighbors=200)
    tp, tz = _t(pos), _t(z)
    for lk in (m, l):
        two_body = dict(a1=0.4, a2=4.0, s8=0.8, d3_params=dp, cell=tc, compute_virial=True, **lk)
        before = dftd3(tp, tz, **two_body)
        zero = dftd3_zero(tp, tz, d3_params=p, cell=tc, compute_virial=True, **ZERO, **lk)
        after = dftd3(tp, tz, **two_body)
        assert all(torch.equal(a, b) for a, b in zip(before, after)), "dftd3 must not see that dftd3_zero ran on the same tensors"
        assert torch.equal(before[2], zero[2]) and not torch.equal(before[1], zero[1])


def test_fullgraph_compile_equals_eager():
    from nvalchemiops.interactions.dispersion import dftd3_zero

    pos, cell = A.lattice_box((5, 4, 4), seed=19, triclinic=True)
    z = _t(_zs(len(pos), 19))
    t, r0ab = _tables()
    p = _params(t, r0ab)
    tc = _t(cell.reshape(1, 3, 3))
    m, l = _lists(pos, cell, 10.0, max_neighbors=200)
    # copies carry no companion of the search: the eager call then walks the arrays like the op does (with a companion whose search-side
    # coordination numbers it adopts, eager differs from the op by the documented CN tolerance -- that path has its own test)
    m = {k: v.clone() for k, v in m.items()}

    def matrix(x):
        return dftd3_zero(x, z, d3_params=p, cell=tc, compute_virial=True, beta=0.05, **ZERO, **m)

    def csr(x):
        e, f, cn = dftd3_zero(x, z, rs6=1.1, s8=0.9, alpha=13.5, d3_params=p, cell=tc, **l)
        return e, f, cn

    for fn in (matrix, csr):
        torch._dynamo.reset()
        got = torch.compile(fn, mode="default", fullgraph=True)(_t(pos))
        want = fn(_t(pos))
        assert float(want[0].abs()) > 0.0
        assert len(got) == len(want) and all(torch.equal(a, b) for a, b in zip(got, want))
