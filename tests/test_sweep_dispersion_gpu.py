"""Seeded sweeps, boundary ladders and one-scalar variants of `dftd3_atm`, `dftd3_zero`, `dftd3_zero_atm`, `dftd4` and `dftd4_atm` against
their float64 restatements.  The cases, and what each of them has to satisfy before it is worth a GPU run, are in tests/sweep_cases.py and
tests/test_sweep_cases_cpu.py; this module builds the lists on the device (`neighbor_list`), stores them the way the case says (matrix width
= widest row + an odd pad, int64, a foreign fill value, rows permuted with the padding kept at the end) and judges every output with the
`_judge` of the op's own module: bar = 4 x max(float32-vs-float64 deviation of the restatement on this very case, `dftd3`'s bar), both
layouts, matrix against CSR within one bar, every atom and every system, figures printed before they are asserted (`pytest -s`).  Exact
zeros are required of padding atoms, of one-atom systems and, for the three-body ops, of two-atom systems.  No tolerance is new.

A tile rung also reads the visit counters of the triple pass: the centre's equal the pairs among its kept entries and their sum is 3 x the
triples the restatement enumerates, so a dropped or doubled tile pair, or a record staged at the wrong ordinal, fails exactly.

MEASURED on one MI355X (worst err / bar of any output over both layouts; every test prints its figures, DESIGN.md section 3.18 has them):
  sweep, 12 seeds   dftd3_atm 0.033   dftd3_zero 0.294   dftd3_zero_atm 0.042   dftd4 0.125   dftd4_atm 0.079
  lane ladder       dftd4 0.123 (n129, CN)   dftd3_zero 0.106 (n129, CN)
  tile ladder       dftd4_atm 0.030   dftd3_atm 0.025   dftd3_zero_atm 0.039; the visit counters equal the restatement's counts on every rung
                    (m640: 53421 at the centre, 5675142 = 3 x 1891714 in all)
  variants          dftd4 0.074   dftd4_atm 0.027   dftd3_atm 0.036   dftd3_zero_atm 0.065
The first run of these sweeps met atoms with Z >= nz as row owners of the D3 passes (csrc/d3.hip tested Z != 0): an illegal memory access in
`dftd3_zero`, a force on a padding atom in `dftd3_atm` (10.6 bars on seed 2).  Fixed there; DESIGN.md section 3.18.
"""
import importlib

import numpy as np
import pytest
import torch

from tests import sweep_cases as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_JUDGES = {"dftd3_atm": "tests.test_d3_atm_gpu", "dftd3_zero": "tests.test_d3_zero_gpu", "dftd3_zero_atm": "tests.test_d3_zero_atm_gpu",
           "dftd4": "tests.test_d4_gpu", "dftd4_atm": "tests.test_d4_atm_gpu"}


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def _judge(op, name, out, r64, r32):
    importlib.import_module(_JUDGES[op])._judge(name, out, r64, r32)


def _search(c):
    """The full list with cutoff c["rc"] from the package's search: (matrix, counts, shifts or None, list [2,P], ptr, list shifts or None),
    the matrix exactly as wide as the case asks.  The float64 enumeration and the float32 search hold the same rows."""
    from nvalchemiops.neighborlist import neighbor_list

    tp = _t(c["pos"])
    width = c["widest"] + c["lists"]["pad"]
    kw = {}
    if c["cell"] is not None:
        cells = _t(c["cell"])
        pbc = torch.ones((cells.shape[0], 3), dtype=torch.bool, device=DEV)
        kw = dict(cell=cells, pbc=pbc) if c["batch_idx"] is not None else dict(cell=cells[0], pbc=pbc[0])
        method = "cell_list" if c["batch_idx"] is None else "batch_cell_list"
    else:
        method = "naive" if c["batch_idx"] is None else "batch_naive"
    if c["batch_idx"] is not None:
        kw["batch_idx"] = _t(np.asarray(c["batch_idx"], np.int32))
    out = neighbor_list(tp, c["rc"], method=method, max_neighbors=width, **kw)
    lst = neighbor_list(tp, c["rc"], method=method, max_neighbors=width, return_neighbor_list=True, **kw)
    nm, num = out[0], out[1]
    assert nm.shape[1] == width and np.array_equal(num.cpu().numpy(), c["counts"]), "the search and the float64 enumeration disagree on a row"
    periodic = c["cell"] is not None
    return nm, num, (out[2] if periodic else None), lst[0], lst[1], (lst[2] if periodic else None)


def _stored(c):
    """(matrix kwargs, CSR kwargs) as the case's `lists` entry wants them stored."""
    nm, num, sh, nl, ptr, lsh = _search(c)
    n, opt = len(c["pos"]), c["lists"]
    if opt["permuted"]:  # the stored entries of every row in another order, padding kept at the end: only the order of fp64 additions changes
        g = np.random.default_rng(len(c["pos"]) + c["widest"])
        a, k = nm.cpu().numpy().copy(), num.cpu().numpy()
        s = None if sh is None else sh.cpu().numpy().copy()
        b, p = nl.cpu().numpy().copy(), ptr.cpu().numpy()
        ls = None if lsh is None else lsh.cpu().numpy().copy()
        for i in range(n):
            o = g.permutation(k[i])
            a[i, :k[i]] = a[i, :k[i]][o]
            o2 = g.permutation(k[i]) + p[i]
            b[:, p[i]:p[i + 1]] = b[:, o2]
            if s is not None:
                s[i, :k[i]] = s[i, :k[i]][o]
                ls[p[i]:p[i + 1]] = ls[o2]
        nm, nl = _t(a), _t(b)
        sh, lsh = (None, None) if s is None else (_t(s), _t(ls))
    m = dict(neighbor_matrix=nm)
    if opt["foreign_fill"]:
        nm = nm.clone()
        nm[nm == n] = n + 5
        m = dict(neighbor_matrix=nm, fill_value=n + 5)
    l = dict(neighbor_list=nl, neighbor_ptr=ptr)
    if opt["int64"]:
        m["neighbor_matrix"] = m["neighbor_matrix"].long()
        l = dict(neighbor_list=nl.long(), neighbor_ptr=ptr.long())
    if sh is not None:
        m["neighbor_matrix_shifts"], l["unit_shifts"] = sh, lsh
    return m, l


def _d3_params(c, radii):
    p = {k: _t(c["tables"][k]) for k in ("rcov", "r4r2", "c6ab", "cn_ref")}
    if radii:
        p["r0ab"] = _t(c["r0ab"])
    return p


def _call(c, lists):
    """The op on case c with its model scalars, on `lists`."""
    from nvalchemiops.interactions import dispersion as D

    op, m = c["op"], c["model"]
    z = _t(c["z"]).long() if c["lists"]["int64"] else _t(c["z"])
    kw = dict(lists)
    if c["cell"] is not None:
        kw.update(cell=_t(c["cell"]), compute_virial=True)
    if c["batch_idx"] is not None:
        kw["batch_idx"] = _t(np.asarray(c["batch_idx"], np.int32))
    pos = _t(c["pos"])
    if op == "dftd3_atm":
        return D.dftd3_atm(pos, z, a1=m["a1"], a2=m["a2"], three_body_cutoff=c["rc3"], s9=c["s9"], alpha=m["alpha"], k1=m["k1"], k3=m["k3"],
                           d3_params=_d3_params(c, False), **kw)
    if op == "dftd3_zero":
        return D.dftd3_zero(pos, z, rs6=m["rs6"], s8=m["s8"], rs8=m["rs8"], alpha=m["alpha"], beta=m["beta"], k1=m["k1"], k3=m["k3"], s6=m["s6"],
                            s5_smoothing_on=m["s5_on"], s5_smoothing_off=m["s5_off"], d3_params=_d3_params(c, True), **kw)
    if op == "dftd3_zero_atm":
        return D.dftd3_zero_atm(pos, z, c["rc3"], rs9=m["rs9"], s9=c["s9"], alpha=m["alpha"], k1=m["k1"], k3=m["k3"], d3_params=_d3_params(c, True), **kw)
    d4 = D.D4Parameters(**{k: _t(c["tables"][k]) for k in W.R.TABLE_KEYS})
    common = dict(d4_params=d4, cn_cutoff=m["cn_cutoff"], wf=m["wf"], ga=m["ga"], gc=m["gc"], k_cn=m["k_cn"])
    if op == "dftd4":
        return D.dftd4(pos, z, _t(c["q"]), m["a1"], m["a2"], m["s8"], m["s6"], **common, **kw)
    return D.dftd4_atm(pos, z, m["a1"], m["a2"], c["rc3"], c["s9"], m["alpha"], **common, **kw)


def _np(out):
    return [o.detach().cpu().numpy().astype(np.float64) for o in out]


def _both_layouts(c, kind, key, tag):
    """Both layouts at the module bars and within one bar of each other; returns (outputs per layout, references, matrix kwargs)."""
    op = c["op"]
    r64, r32 = W.references(kind, op, key)
    m, l = _stored(c)
    keys = [k for k in W.OUTPUTS[op] if r64[k] is not None]
    outs = {}
    for layout, lk in (("matrix", m), ("csr", l)):
        outs[layout] = _call(c, lk)
        assert len(outs[layout]) == len(keys) and all(o.dtype == torch.float32 for o in outs[layout])
        _judge(op, f"{tag} {layout}", outs[layout], r64, r32)
    for a, b, k in zip(_np(outs["matrix"]), _np(outs["csr"]), keys):
        assert (np.abs(a - b) <= W.bar(r64, r32, k)).all(), f"matrix and CSR further apart than one bar: {k}"
    return outs, (r64, r32), m


def _exact_zeros(c, outs):
    op = c["op"]
    keys = [k for k in W.OUTPUTS[op] if k != "virial" or c["cell"] is not None]
    n = len(c["pos"])
    bi = np.zeros(n, np.int64) if c["batch_idx"] is None else np.asarray(c["batch_idx"])
    sizes = np.bincount(bi)
    small = 2 if op in W.THREE_BODY else 1  # a pair has a two-body energy
    padding = c.get("padding") in ("z0", "beyond") or (c.get("padding") == "dead" and op in W.D4_OPS)
    for out in outs.values():
        got = dict(zip(keys, _np(out)))
        if padding:
            at = c["padding_atom"]
            assert all(not got[k][at].any() for k in ("forces", "cn", "charge_grad") if k in got), "a padding atom's outputs are exactly zero"
        for s in np.nonzero(sizes <= small)[0]:
            atoms = bi == s
            assert got["energy"][s] == 0.0 and not got["forces"][atoms].any(), f"system {s} of {sizes[s]} atom(s) is exactly zero"
            assert "virial" not in got or not got["virial"][s].any()
            if sizes[s] == 1:
                assert all(not got[k][atoms].any() for k in ("cn", "charge_grad") if k in got)


# ---- sweeps ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", W.SEEDS)
@pytest.mark.parametrize("op", W.OPS)
def test_sweep(op, seed):
    c = W.case(op, seed)
    assert min(c["margins"].values()) >= W.MARGIN
    outs, _, _ = _both_layouts(c, "sweep", seed, f"sweep {op} {seed}")
    _exact_zeros(c, outs)


# ---- lane trips -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", W.LANE_RUNGS)
@pytest.mark.parametrize("op", W.LANE_OPS)
def test_lane_trip_ladder(op, name):
    """Free clusters of 64, 65, 66 and 129 atoms, everybody in everybody's row: rows of 63 (one lane trip short by one), 64 (exactly one),
    65 (one plus one entry) and 128 (exactly two) entries, as CSR and as a matrix exactly that wide -- no padding column at all."""
    c = W.ladder_case(op, name)
    n = len(c["pos"])
    outs, _, m = _both_layouts(c, "ladder", name, f"lane {op} {name}")
    nm = m["neighbor_matrix"]
    assert nm.shape == (n, n - 1) and int(nm.max()) == n - 1 and n == int(name[1:])


# ---- block trips and LDS tiles --------------------------------------------------------------------------------------------------------------

def _visits(c, m):
    """Per-centre triangle-visit counters of one triple pass on the matrix list."""
    n = len(c["pos"])
    if c["op"] != "dftd4_atm":
        from nvalchemiops.interactions.dispersion.dftd3 import atm_scalars
        from tests.test_d3_atm_gpu import _visits as d3_visits

        mo = c["model"]
        if c["op"] == "dftd3_atm":
            return d3_visits(c["pos"], c["z"], c["tables"], m, c["rc3"], atm_scalars(mo["a1"], mo["a2"], mo["k1"], mo["k3"]))
        return d3_visits(c["pos"], c["z"], c["tables"], m, c["rc3"], atm_scalars(0.0, 0.0, mo["k1"], mo["k3"]), zero=(mo["rs9"], _t(c["r0ab"])))
    from nvalchemiops import _capi as C

    D4 = importlib.import_module("nvalchemiops.interactions.dispersion.dftd4")  # (the package re-exports a function of the same name)
    mo = c["model"]
    tables = tuple(_t(c["tables"][k]) for k in W.R.TABLE_KEYS)
    scalars = D4.d4_scalars(mo["a1"], mo["a2"], 0.0, 0.0, mo["k_cn"], mo["wf"], mo["ga"], mo["gc"], None)
    f32 = dict(dtype=torch.float32, device=DEV)
    nm = C.i32(m["neighbor_matrix"])
    return D4._launch_atm(positions=_t(c["pos"]), numbers=_t(c["z"]), idx=nm, shifts=None, nptr=None, max_neighbors=nm.shape[1], fill_value=n, cell=None,
                          batch_idx=None, num_systems=1, tables=tables, scalars=scalars, s9=c["s9"], alpha=mo["alpha"], three_body_cutoff=c["rc3"],
                          compute_virial=False, energy=torch.empty(1, **f32), forces=torch.empty((n, 3), **f32),
                          virial=torch.zeros((0, 3, 3), **f32), want_visits=True).cpu().numpy()


def _tile_rungs():
    return [(op, rung) for op in W.TILES for rung in range(len(W.tile_rungs(op)))]


@pytest.mark.parametrize("op,rung", _tile_rungs())
def test_block_trip_and_tile_ladder(op, rung):
    """`centre_and_shell(m)`: the centre's row keeps all m, every other row less than one tile.  m = 255, 256, 257: the 256-entry stream
    trips of the triple pass; m = tile, tile + 1, 2 tile: `min(TILE, n - tq * TILE)`, `ntiles = (n + TILE - 1) / TILE` and the ordinal slot
    at the values where they are exact or degenerate."""
    tile = W.tile_of(op)
    assert tile == W.TILES[op], "tests/sweep_cases.py's tile sizes are the library's"
    m_atoms = W.tile_rungs(op, tile)[rung]
    name = f"m{m_atoms}"
    c = W.ladder_case(op, name)
    kept, pairs0, triples, margin = W.A.kept_and_triples(c["pos"], c["rc3"])
    assert kept[0] == m_atoms and kept[1:].max() < tile and margin > W.MARGIN, (kept[0], kept[1:].max(), margin)
    outs, (r64, _), m = _both_layouts(c, "ladder", name, f"tile {op} {name}")
    assert r64["triples"] == triples and m["neighbor_matrix"].shape[1] == m_atoms
    visits = _visits(c, m)
    print(f"[sweep] tile {op} {name}: centre visits {visits[0]} (pairs among its kept entries {pairs0}), all visits {int(visits.sum())} (3 x {triples} triples)")
    assert visits[0] == pairs0 and int(visits.sum()) == 3 * triples, (visits[0], pairs0, int(visits.sum()), 3 * triples)


# ---- one scalar at a time ---------------------------------------------------------------------------------------------------------------------

def _variants():
    return [(op, name) for op in W.VARIANTS for name in W.variant_names(op)]


@pytest.mark.parametrize("op,name", _variants())
def test_one_scalar_off_its_default(op, name):
    """The variant matches its own restatement in both layouts, and leaves the kernel's result at the defaults by more than 100 bars in at
    least one output (the CPU suite has shown from the two float64 references that it must)."""
    c = W.variant_case(op, name)
    outs, (r64, r32), m = _both_layouts(c, "variant", name, f"variant {op} {name}")
    base = _call(W.variant_case(op, "default"), m)
    keys = [k for k in W.OUTPUTS[op] if r64[k] is not None]
    moved = {k: float((np.abs(a - b) / W.bar(r64, r32, k)).max()) for k, a, b in zip(keys, _np(outs["matrix"]), _np(base))}
    print(f"[sweep] variant {op} {name}: kernel(variant) - kernel(default) in bars {({k: round(v, 1) for k, v in moved.items()})}")
    assert max(moved.values()) > 100.0
