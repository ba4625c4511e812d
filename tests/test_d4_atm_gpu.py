"""`dftd4_atm` (three-body Axilrod-Teller-Muto term of DFT-D4, csrc/d4_atm.h) against the float64 restatement tests/d4_atm_reference.py.

Lists are built by this package's `neighbor_list`.  The systems are those of tests/d4_atm_cases.py: the positions, species and tables of the
`dftd4` cases, each with a three-body cutoff and an s9 that lifts energy, forces and virial to at least 500 of the bars applied here (the CPU
suite checks that, and that the float32 deviation of the restatement scaled by the same s9 stays below the bar:
tests/test_d4_atm_reference_cpu.py).  Bars, as in tests/test_d3_atm_gpu.py: the restatement is evaluated once in float64 and once with
every per-pair / per-atom / per-triple quantity in float32 (float64 sums: the kernels' arithmetic model); a quantity's bar is 4 x the larger
of that float32-vs-float64 deviation on the same system and `dftd3`'s bar (energy rtol = atol = 1e-6; forces rtol 1e-6, atol 1e-6 + 5e-6
max|F|; virial rtol 1e-6, atol 1e-6 + 2e-7 max|V|).  Every atom and every system of every input is compared; each figure is printed before
it is asserted (`pytest -s`).  The measured figures of every case are kept in one place: DESIGN.md section 3.15.
"""
import numpy as np
import pytest
import torch

from tests import d4_atm_cases as K3
from tests import systems as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BJ = K3.BJ
KEYS = ("energy", "forces", "virial")
EXTRA = K3.EXTRA


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def _params(t):
    from nvalchemiops.interactions.dispersion import D4Parameters

    return D4Parameters(**{k: _t(t[k]) for k in K3.K.R.TABLE_KEYS})


def _lists(pos, cell, rc, batch_idx=None, max_neighbors=None):
    """(matrix kwargs, CSR kwargs, widest row) of the full list with cutoff rc, built on the device by the package."""
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
    mn = max_neighbors or (len(pos) + 8 if cell is None else 160)
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


def _bars(r64, r32):
    """Per quantity: (the elementwise bar of this module, the float32-vs-float64 deviation of the restatement, max|ref|)."""
    bars = {}
    for k in KEYS:
        ref, low = r64[k], r32[k]
        if ref is None:
            continue
        dev32 = np.abs(low - ref).max() if ref.size else 0.0
        scale = np.abs(ref).max() if ref.size else 0.0
        bars[k] = (4.0 * np.maximum(dev32, 1e-6 + 1e-6 * np.abs(ref) + EXTRA[k] * scale), dev32, scale)
    return bars


def _judge(name, out, r64, r32):
    """Asserts out = (energy, forces[, virial]) against the float64 restatement; prints the figures first."""
    got = [o.detach().cpu().numpy().astype(np.float64) for o in out]
    bars = _bars(r64, r32)
    fails = []
    for g, k in zip(got, KEYS):
        ref = r64[k]
        bar, dev32, scale = bars[k]
        assert g.shape == ref.shape, (k, g.shape, ref.shape)
        err = np.abs(g - ref)
        worst = (err / bar).max() if ref.size else 0.0
        print(f"[d4_atm] {name:30s} {k:7s} max|ref| {scale:.3e}  fp32-vs-fp64 {dev32:.3e}  kernel-vs-fp64 {err.max() if ref.size else 0.0:.3e}  "
              f"worst err/bar {worst:.3f}")
        if not (err <= bar).all():
            fails.append(f"{k}: max err {err.max():.3e}, bar {bar.flat[(err / bar).argmax()]:.3e}")
    assert not fails, f"{name}: " + "; ".join(fails)


def _inputs(name, max_neighbors=None):
    c = K3.case(name)
    m, l, widest = _lists(c["pos"], c["cell"], c["rc"], c["batch_idx"], max_neighbors)
    kw = dict(d4_params=_params(c["tables"]), three_body_cutoff=c["rc3"], s9=c["s9"], **BJ, **c["kw"])
    if c["cell"] is not None:
        kw.update(cell=_t(np.asarray(c["cell"]).reshape(-1, 3, 3)), compute_virial=True)
    if c["batch_idx"] is not None:
        kw["batch_idx"] = _t(c["batch_idx"])
    return c, (_t(c["pos"]), _t(c["z"])), kw, m, l, widest


def _both_layouts(name, max_neighbors=None):
    from nvalchemiops.interactions.dispersion import dftd4_atm

    c, args, kw, m, l, widest = _inputs(name, max_neighbors)
    r64, r32 = K3.references(name)
    outs = {}
    for tag, lk in (("matrix", m), ("csr", l)):
        outs[tag] = dftd4_atm(*args, **kw, **lk)
        assert all(o.dtype == torch.float32 for o in outs[tag]) and len(outs[tag]) == (3 if c["cell"] is not None else 2)
        _judge(f"{name} {tag}", outs[tag], r64, r32)
    bars = _bars(r64, r32)
    for a, b, k in zip(outs["matrix"], outs["csr"], KEYS):  # the two layouts within one bar of each other
        assert (np.abs(a.cpu().numpy().astype(np.float64) - b.cpu().numpy().astype(np.float64)) <= bars[k][0]).all(), k
    return c, outs, r64, bars, widest


# ---- parity: every case, both layouts -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", K3.PARITY)
def test_every_case_matrix_and_csr_against_the_restatement(name):
    c, outs, r64, bars, widest = _both_layouts(name)
    n = len(c["pos"])
    assert np.abs(r64["energy"]).max() > 0.0
    f = outs["matrix"][1]
    if c["cell"] is None:  # the net force of a molecule: zero to the force bar x sqrt(N)
        assert float(f.double().sum(0).abs().max()) <= float(bars["forces"][0].min()) * np.sqrt(n)
    if name == "padding":
        for out in outs.values():
            assert float(out[1][4].abs().max()) == 0.0 and float(out[1][7].abs().max()) == 0.0  # Z = 0 and Z >= nz
    if name == "no_references":
        sel = torch.as_tensor(c["z"] == 8, device=DEV)
        assert int(sel.sum()) >= 3 and all(float(out[1][sel].abs().max()) == 0.0 for out in outs.values())
    if name.startswith("species"):
        from nvalchemiops.interactions.dispersion.dftd4 import species_slots

        count = {"species_slots": 16, "species_slots_plus_1": 17, "species_20": 20}[name]
        assert species_slots() == 16 and len(np.unique(c["z"])) == count
    if name == "triclinic_f64":
        assert c["pos"].dtype == np.float64
    if name == "self_images":
        _, _, _, m, _, _ = _inputs(name)
        nm, sh = m["neighbor_matrix"].cpu().numpy(), m["neighbor_matrix_shifts"].cpu().numpy()
        assert ((nm[0] == 0) & (np.abs(sh[0]).sum(1) > 0)).any(), "the test needs rows with the atom's own images"
    if name == "batch":  # three systems, the last a single atom: its energy and virial are written, as zeros
        for out in outs.values():
            assert out[0].shape == (3,) and out[2].shape == (3, 3, 3)
            assert float(out[0][2]) == 0.0 and float(out[2][2].abs().max()) == 0.0 and float(out[1][-1].abs().max()) == 0.0
    if name == "dense":
        from nvalchemiops.interactions.dispersion.dftd4 import atm_tile

        assert widest == n - 1 and r64["kept"] > atm_tile(), "a row must stage more than one LDS tile"


# ---- list dtypes, wide matrices, fill values ----------------------------------------------------------------------------------------------

def test_int64_lists_and_a_wider_matrix_with_another_fill_value():
    from nvalchemiops.interactions.dispersion import dftd4_atm

    c, args, kw, m, l, _ = _inputs("padding")
    n = len(c["pos"])
    base_m = dftd4_atm(*args, **kw, **m)
    base_l = dftd4_atm(*args, **kw, **l)
    got = dftd4_atm(args[0], args[1].long(), **kw, neighbor_matrix=m["neighbor_matrix"].long())
    assert all(torch.equal(a, b) for a, b in zip(got, base_m))
    got = dftd4_atm(args[0], args[1].long(), **kw, neighbor_list=l["neighbor_list"].long(), neighbor_ptr=l["neighbor_ptr"].long())
    assert all(torch.equal(a, b) for a, b in zip(got, base_l))
    _, _, _, wide, _, _ = _inputs("padding", max_neighbors=2 * n + 8)
    nm = wide["neighbor_matrix"].clone()
    assert nm.shape[1] == 2 * n + 8
    nm[nm == n] = n + 5
    got = dftd4_atm(*args, **kw, neighbor_matrix=nm, fill_value=n + 5)
    assert all(torch.equal(a, b) for a, b in zip(got, base_m))


# ---- exact zeros --------------------------------------------------------------------------------------------------------------------------

def test_one_atom_two_atoms_and_s9_zero_give_exactly_zero():
    from nvalchemiops.interactions.dispersion import dftd4_atm

    for name in K3.ZERO:
        c, args, kw, m, l, _ = _inputs(name)
        for lk in (m, l):
            e, f = dftd4_atm(*args, **kw, **lk)
            assert e.shape == (1,) and f.shape == (len(c["pos"]), 3) and float(e.abs().max()) == 0.0 and float(f.abs().max()) == 0.0
    c, args, kw, m, l, _ = _inputs("triclinic_f32")
    kw = dict(kw, s9=0.0)
    for lk in (m, l):
        out = dftd4_atm(*args, **kw, **lk)
        assert len(out) == 3 and all(float(o.abs().max()) == 0.0 for o in out)


# ---- the D3 limit against the dftd3_atm kernel ---------------------------------------------------------------------------------------------

def test_one_reference_limit_equals_the_dftd3_atm_kernel():
    """One reference per element and ga = 0: C6 is the constant c6_ref[Z_i, Z_j, 0, 0], whatever the coordination numbers (D4's differ from
    D3's) -- the term is `dftd3_atm`'s with constant c6ab tables on the same list.  Bar: the two kernels' bars added."""
    from nvalchemiops.interactions.dispersion import D3Parameters, dftd3_atm

    c, outs, r64, bars, _ = _both_layouts("d3_limit")
    _, args, kw, m, _, _ = _inputs("d3_limit")
    d3 = S.d3_test_tables(17, seed=1000)
    c6ab = np.broadcast_to(c["tables"]["c6_ref"][:, :, 0, 0][:, :, None, None], d3["c6ab"].shape).copy()
    p3 = D3Parameters(rcov=_t(d3["rcov"]), r4r2=_t(d3["r4r2"]), c6ab=_t(c6ab), cn_ref=_t(d3["cn_ref"]))
    e3, f3, v3 = dftd3_atm(args[0], args[1], three_body_cutoff=c["rc3"], s9=c["s9"], d3_params=p3, cell=kw["cell"], compute_virial=True, **BJ, **m)
    for k, a, b in zip(KEYS, outs["matrix"], (e3, f3, v3)):
        d3_bar = K3.d3_bar(r64[k], k)
        err = np.abs(a.cpu().numpy().astype(np.float64) - b.cpu().numpy().astype(np.float64))
        print(f"[d4_atm] D3 limit vs dftd3_atm kernel   {k:7s} max |d4 - d3| {err.max():.3e}  worst / (bar_d4 + bar_d3) {(err / (bars[k][0] + d3_bar)).max():.3f}")
        assert (err <= bars[k][0] + d3_bar).all(), k


# ---- determinism, streams, cross-talk -------------------------------------------------------------------------------------------------------

def test_two_calls_and_a_side_stream_are_bit_identical():
    from nvalchemiops.interactions.dispersion import dftd4_atm

    c, args, kw, m, l, _ = _inputs("triclinic_f32")
    for lk in (m, l):
        a = dftd4_atm(*args, **kw, **lk)
        b = dftd4_atm(*args, **kw, **lk)
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    base = dftd4_atm(*args, **kw, **m)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        other = dftd4_atm(*args, **kw, **m)
    stream.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(base, other))


def test_dftd4_is_bit_identical_before_and_after_a_dftd4_atm_call():
    from nvalchemiops.interactions.dispersion import dftd4, dftd4_atm

    c, args, kw, m, l, _ = _inputs("triclinic_f32")
    q = _t(K3.K.case("triclinic_f32")["q"])
    two = dict(d4_params=kw["d4_params"], cell=kw["cell"], compute_virial=True, **K3.K.BJ)
    for lk in (m, l):
        before = dftd4(args[0], args[1], q, **two, **lk)
        e3 = dftd4_atm(*args, **kw, **lk)[0]
        after = dftd4(args[0], args[1], q, **two, **lk)
        assert float(e3.abs().max()) > 0.0 and all(torch.equal(a, b) for a, b in zip(before, after))


def test_renumbering_the_atoms_permutes_the_forces():
    from nvalchemiops.interactions.dispersion import dftd4_atm

    c, args, kw, m, _, _ = _inputs("triclinic_f32")
    r64, r32 = K3.references("triclinic_f32")
    n = len(c["pos"])
    out = dftd4_atm(*args, **kw, **m)
    perm = np.random.default_rng(0).permutation(n)
    m2, _, _ = _lists(c["pos"][perm], c["cell"], c["rc"])
    out2 = dftd4_atm(_t(c["pos"][perm]), _t(c["z"][perm]), **kw, **m2)
    _judge("renumbered", out2, dict(r64, forces=r64["forces"][perm]), dict(r32, forces=r32["forces"][perm]))
    bars = _bars(r64, r32)
    tperm = torch.as_tensor(perm, device=DEV)
    for a, b, k in zip((out[0], out[1][tperm], out[2]), out2, KEYS):  # within one bar of the original numbering
        ref_bar = bars[k][0][perm] if k == "forces" else bars[k][0]
        assert (np.abs(a.cpu().numpy().astype(np.float64) - b.cpu().numpy().astype(np.float64)) <= ref_bar).all(), k


def test_visit_counters_of_a_molecule_count_every_triple_three_times():
    from nvalchemiops import _capi as C
    import importlib

    D4 = importlib.import_module("nvalchemiops.interactions.dispersion.dftd4")  # (the package re-exports a function of the same name)
    c, args, kw, m, l, _ = _inputs("molecule24")
    r64, _ = K3.references("molecule24")
    n = len(c["pos"])
    p = kw["d4_params"]
    tables = tuple(getattr(p, k) for k in K3.K.R.TABLE_KEYS)
    scalars = D4.d4_scalars(BJ["a1"], BJ["a2"], 0.0, 0.0, 7.5, 6.0, 3.0, 2.0, None)
    f32 = dict(dtype=torch.float32, device=DEV)
    for idx, nptr, width, fill in ((C.i32(m["neighbor_matrix"]), None, m["neighbor_matrix"].shape[1], n),
                                   (C.i32(l["neighbor_list"][1]), C.i32(l["neighbor_ptr"]), 0, 0)):
        e, f = torch.empty(1, **f32), torch.empty((n, 3), **f32)
        visits = D4._launch_atm(args[0], args[1], idx, None, nptr, width, fill, None, None, 1, tables, scalars, c["s9"], 16.0, c["rc3"], False, e, f,
                                torch.zeros((0, 3, 3), **f32), want_visits=True)
        assert visits.shape == (n,) and int(visits.sum()) == 3 * r64["triples"] > 0


def test_row_of_three_lds_tiles_runs_every_tile_pair_once():
    """`shell` (tests/d4_atm_cases.py): the centre's row stages three tiles -- all six tile pairs, (1, 2) among them -- every other row less
    than one.  Both layouts at the module's bars, and the visit counters: the centre's equal the pairs among its kept entries, their sum is
    3 x the triples the restatement enumerates, so no tile pair is dropped or run twice."""
    from nvalchemiops import _capi as C
    from nvalchemiops.interactions.dispersion.dftd4 import atm_tile
    import importlib

    D4 = importlib.import_module("nvalchemiops.interactions.dispersion.dftd4")
    c, outs, r64, bars, widest = _both_layouts("shell", max_neighbors=len(K3.case("shell")["pos"]) + 8)
    n, tile = len(c["pos"]), atm_tile()
    kept, pairs0, triples, margin = K3.K.A.kept_and_triples(c["pos"], c["rc3"])
    assert widest == n - 1 and kept[0] > 2 * tile and kept[1:].max() < tile, (widest, kept[0], kept[1:].max(), tile)
    assert margin > 2e-5, "no pair within float32 rounding (ulp(20) = 1.9e-6, a few per distance) of the cutoff: the counts below are exact"
    assert r64["triples"] == triples and r64["kept"] == kept[0]
    _, args, kw, m, _, _ = _inputs("shell", max_neighbors=n + 8)
    p = kw["d4_params"]
    tables = tuple(getattr(p, k) for k in K3.K.R.TABLE_KEYS)
    scalars = D4.d4_scalars(BJ["a1"], BJ["a2"], 0.0, 0.0, 7.5, 6.0, 3.0, 2.0, None)
    f32 = dict(dtype=torch.float32, device=DEV)
    nm = C.i32(m["neighbor_matrix"])
    visits = D4._launch_atm(positions=args[0], numbers=args[1], idx=nm, shifts=None, nptr=None, max_neighbors=nm.shape[1], fill_value=n, cell=None,
                            batch_idx=None, num_systems=1, tables=tables, scalars=scalars, s9=c["s9"], alpha=16.0, three_body_cutoff=c["rc3"],
                            compute_virial=False, energy=torch.empty(1, **f32), forces=torch.empty((n, 3), **f32),
                            virial=torch.zeros((0, 3, 3), **f32), want_visits=True).cpu().numpy()
    assert visits[0] == pairs0 and int(visits.sum()) == 3 * r64["triples"], (visits[0], pairs0, int(visits.sum()), 3 * r64["triples"])


# ---- autograd -------------------------------------------------------------------------------------------------------------------------------

def test_backward_gives_minus_forces_and_differentiating_twice_raises():
    from nvalchemiops.interactions.dispersion import dftd4_atm

    c, args, kw, m, l, _ = _inputs("batch")
    for dt in (torch.float32, torch.float64):
        pos = args[0].detach().clone().to(dt).requires_grad_()
        e, f, v = dftd4_atm(pos, args[1], **kw, **l)
        assert e.requires_grad and not f.requires_grad and not v.requires_grad
        w = torch.tensor([1.0, -2.0, 0.5], device=DEV)
        (e * w).sum().backward()
        wa = w[kw["batch_idx"].long()]
        assert pos.grad.dtype == dt and torch.equal(pos.grad, (-wa[:, None] * f).to(dt))
    c, args, kw, m, l, _ = _inputs("molecule24")
    pos = args[0].clone().requires_grad_()
    e, f = dftd4_atm(pos, args[1], **kw, **m)
    e.sum().backward()
    assert torch.equal(pos.grad, -f)
    pos = args[0].clone().requires_grad_()
    e = dftd4_atm(pos, args[1], **kw, **m)[0]
    (g,) = torch.autograd.grad(e.sum(), pos, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()
    assert not dftd4_atm(*args, **kw, **m)[0].requires_grad


# ---- torch.compile ---------------------------------------------------------------------------------------------------------------------------

def test_fullgraph_compile_of_dftd4_plus_atm_equals_eager():
    from nvalchemiops.interactions.dispersion import dftd4, dftd4_atm

    c, args, kw, m, l, _ = _inputs("triclinic_f32")
    q = _t(K3.K.case("triclinic_f32")["q"])
    p = kw["d4_params"]
    tables = {k: getattr(p, k) for k in K3.K.R.TABLE_KEYS}
    z, tc = args[1], kw["cell"]

    def total_matrix(x):
        e2, f2, cn, dq, v2 = dftd4(x, z, q, d4_params=p, cell=tc, compute_virial=True, **K3.K.BJ, **m)
        e3, f3, v3 = dftd4_atm(x, z, three_body_cutoff=c["rc3"], s9=c["s9"], d4_params=p, cell=tc, compute_virial=True, **BJ, **m)
        return e2 + e3, f2 + f3, v2 + v3, e3

    def total_csr(x):
        e2, f2, cn, dq = dftd4(x, z, q, d4_params=tables, cell=tc, **K3.K.BJ, **l)
        e3, f3 = dftd4_atm(x, z, three_body_cutoff=c["rc3"], s9=c["s9"], alpha=14.0, cn_cutoff=8.0, d4_params=tables, cell=tc, **BJ, **l)
        return e2 + e3, f2 + f3, e3

    for fn in (total_matrix, total_csr):
        torch._dynamo.reset()
        got = torch.compile(fn, mode="default", fullgraph=True)(args[0])
        want = fn(args[0])
        assert float(want[-1].abs()) > 0.0
        assert len(got) == len(want) and all(torch.equal(a, b) for a, b in zip(got, want))
