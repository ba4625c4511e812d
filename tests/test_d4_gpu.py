"""`dftd4` (two-body DFT-D4 with charge-dependent C6, csrc/d4.hip) against the float64 restatement tests/d4_reference.py.

Lists are built by this package's `neighbor_list`.  The systems are those of tests/d4_cases.py (the CPU suite checks on the same systems
that the synthetic tables exercise the weight derivatives).  Bars, as in tests/test_d3_atm_gpu.py: the restatement is evaluated once in
float64 and once with every per-pair / per-atom quantity in float32 (float64 sums: the kernels' arithmetic model); a quantity's bar is
4 x the larger of that float32-vs-float64 deviation on the same system and `dftd3`'s existing bar (tests/test_d3_gpu.py:49-54: energy and
coordination numbers rtol = atol = 1e-6; forces rtol 1e-6, atol 1e-6 + 5e-6 max|F|; virial rtol 1e-6, atol 1e-6 + 2e-7 max|V|).  dE/dq takes
the force bar: the same kind of per-atom owner sum of float32 pair terms.  4 x is the factor the suite allows between two summation orders
(tests/test_oracle_golden.py).  Every atom and every system of every input is compared; each figure is printed before it is asserted.

MEASURED on one MI355X (max over components; restatement float32 vs float64 | kernel vs float64 restatement | worst err / bar; matrix and
CSR agree to the digits shown; the table with max|ref| is in DESIGN.md section 3.14, every test prints its figures under `pytest -s`):
  molecule2             E 3.8e-09 | 2.9e-09 | 0.001   F 3.8e-09 | 1.3e-08 | 0.003   CN 2.9e-08 | 2.1e-07 | 0.028   dE/dq 2.2e-09 | 1.2e-09 | 0.000
  molecule3             E 3.6e-09 | 5.7e-10 | 0.000   F 3.1e-09 | 1.1e-08 | 0.003   CN 3.9e-07 | 4.2e-07 | 0.090   dE/dq 2.4e-09 | 2.7e-09 | 0.001
  molecule7             E 3.0e-08 | 1.9e-08 | 0.004   F 5.2e-08 | 1.5e-08 | 0.003   CN 1.7e-07 | 4.1e-07 | 0.044   dE/dq 1.7e-08 | 2.4e-09 | 0.000
  molecule24            E 1.9e-08 | 6.1e-08 | 0.006   F 3.3e-07 | 6.3e-08 | 0.008   CN 7.2e-07 | 5.9e-07 | 0.073   dE/dq 4.9e-08 | 2.2e-08 | 0.002
  molecule70            E 6.9e-07 | 7.3e-07 | 0.018   F 1.8e-06 | 5.4e-07 | 0.045   CN 7.2e-07 | 8.9e-07 | 0.094   dE/dq 1.4e-07 | 5.3e-08 | 0.004
  padding               E 3.7e-08 | 2.0e-08 | 0.004   F 4.1e-08 | 1.2e-08 | 0.002   CN 2.6e-07 | 3.2e-08 | 0.007   dE/dq 1.9e-08 | 1.1e-08 | 0.002
  no_references         E 1.9e-08 | 1.4e-08 | 0.003   F 1.9e-09 | 8.4e-10 | 0.000   CN 1.8e-08 | 1.4e-08 | 0.003   dE/dq 7.3e-09 | 3.5e-09 | 0.001
  species_slots (16)    E 2.8e-07 | 1.8e-07 | 0.009   F 1.2e-06 | 1.1e-07 | 0.018   CN 6.0e-07 | 5.6e-07 | 0.059   dE/dq 1.5e-07 | 2.0e-08 | 0.002
  species_slots_plus_1  E 2.7e-07 | 4.2e-08 | 0.002   F 3.6e-06 | 5.6e-08 | 0.004   CN 8.7e-07 | 8.4e-07 | 0.098   dE/dq 7.8e-08 | 1.5e-08 | 0.002
  species_20            E 7.0e-08 | 4.5e-08 | 0.002   F 3.8e-06 | 2.4e-07 | 0.016   CN 6.1e-07 | 6.7e-07 | 0.077   dE/dq 5.4e-08 | 1.6e-08 | 0.002
  triclinic_f32         E 1.7e-07 | 1.4e-07 | 0.010   F 9.7e-08 | 2.8e-08 | 0.006   CN 3.7e-07 | 4.2e-07 | 0.071   dE/dq 9.0e-08 | 3.0e-08 | 0.002   V 1.8e-07 | 2.2e-08 | 0.004
  triclinic_f64         E 1.2e-07 | 1.1e-07 | 0.008   F 1.5e-07 | 3.0e-08 | 0.006   CN 2.3e-07 | 1.9e-07 | 0.040   dE/dq 8.3e-08 | 5.3e-08 | 0.004   V 3.9e-07 | 2.7e-07 | 0.023
  self_images           E 1.5e-07 | 5.2e-08 | 0.010   F 3.9e-09 | 5.4e-09 | 0.001   CN 4.8e-08 | 8.1e-08 | 0.015   dE/dq 6.1e-08 | 1.6e-08 | 0.002   V 1.5e-07 | 3.0e-08 | 0.006
  batch                 E 6.0e-08 | 5.4e-08 | 0.006   F 1.8e-08 | 2.3e-08 | 0.006   CN 1.3e-07 | 2.5e-07 | 0.050   dE/dq 7.8e-08 | 3.9e-08 | 0.003   V 1.6e-07 | 6.5e-08 | 0.010
  zero_charges          E 5.2e-08 | 3.6e-08 | 0.004   F 2.9e-07 | 5.8e-08 | 0.007   CN 7.2e-07 | 5.9e-07 | 0.073   dE/dq 2.5e-08 | 1.4e-08 | 0.002
  zeff_negative         E 7.7e-09 | 9.3e-09 | 0.001   F 1.2e-08 | 1.0e-08 | 0.002   CN 3.3e-08 | 9.3e-08 | 0.012   dE/dq 3.4e-08 | 1.1e-08 | 0.002
  cn_cutoff             E 2.6e-07 | 4.7e-08 | 0.004   F 7.4e-08 | 6.3e-08 | 0.013   CN 1.3e-07 | 2.2e-07 | 0.051   dE/dq 7.3e-08 | 2.0e-08 | 0.001   V 2.5e-07 | 2.9e-07 | 0.027
  d3_limit              E 2.7e-07 | 5.4e-08 | 0.005   F 5.8e-09 | 6.1e-09 | 0.001   CN 3.7e-07 | 4.2e-07 | 0.071   dE/dq 0 | 0 | 0                 V 2.6e-07 | 1.1e-07 | 0.012
molecule1 is zero throughout.  The D3 limit against the `dftd3` kernel: energy equal to the bit, forces 5.1e-9, virial 6.0e-8 (0.006 of the two
bars added).  QEq -> dftd4: largest relative deviation of the assembled gradient 1.2e-15 to 3.0e-15 in two runs.  The float32 deviation
exceeds `dftd3`'s bar only in the forces of the 17- and 20-species molecules (3.6e-6 / 3.8e-6 against 1.4e-6 / 1.5e-6: those bars are 4 x the
deviation); every other bar is 4 x `dftd3`'s.  The coordination numbers come closest to theirs (0.1): it has no term relative to the largest
value."""
import numpy as np
import pytest
import torch

from tests import d4_cases as K
from tests import systems as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BJ = K.BJ
KEYS = ("energy", "forces", "cn", "charge_grad", "virial")
EXTRA = {"energy": 0.0, "forces": 5e-6, "cn": 0.0, "charge_grad": 5e-6, "virial": 2e-7}


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def _params(t):
    from nvalchemiops.interactions.dispersion import D4Parameters

    return D4Parameters(**{k: _t(t[k]) for k in K.R.TABLE_KEYS})


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
    """Per quantity: the elementwise bar of this module."""
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
    """Asserts out = (energy, forces, coord_num, charge_gradients[, virial]) against the float64 restatement; prints the figures first."""
    got = [o.detach().cpu().numpy().astype(np.float64) for o in out]
    bars = _bars(r64, r32)
    fails = []
    for g, k in zip(got, KEYS):
        ref = r64[k]
        bar, dev32, scale = bars[k]
        assert g.shape == ref.shape, (k, g.shape, ref.shape)
        err = np.abs(g - ref)
        worst = (err / bar).max() if ref.size else 0.0
        print(f"[d4] {name:30s} {k:11s} max|ref| {scale:.3e}  fp32-vs-fp64 {dev32:.3e}  kernel-vs-fp64 {err.max() if ref.size else 0.0:.3e}  "
              f"worst err/bar {worst:.3f}")
        if not (err <= bar).all():
            fails.append(f"{k}: max err {err.max():.3e}, bar {bar.flat[(err / bar).argmax()]:.3e}")
    assert not fails, f"{name}: " + "; ".join(fails)


def _inputs(name, max_neighbors=None):
    c = K.case(name)
    m, l, widest = _lists(c["pos"], c["cell"], c["rc"], c["batch_idx"], max_neighbors)
    kw = dict(d4_params=_params(c["tables"]), **BJ, **c["kw"])
    if c["cell"] is not None:
        kw.update(cell=_t(np.asarray(c["cell"]).reshape(-1, 3, 3)), compute_virial=True)
    if c["batch_idx"] is not None:
        kw["batch_idx"] = _t(c["batch_idx"])
    return c, (_t(c["pos"]), _t(c["z"]), _t(c["q"])), kw, m, l, widest


def _both_layouts(name, max_neighbors=None):
    from nvalchemiops.interactions.dispersion import dftd4

    c, args, kw, m, l, widest = _inputs(name, max_neighbors)
    r64, r32 = K.references(name)
    outs = {}
    for tag, lk in (("matrix", m), ("csr", l)):
        outs[tag] = dftd4(*args, **kw, **lk)
        assert all(o.dtype == torch.float32 for o in outs[tag]) and len(outs[tag]) == (5 if c["cell"] is not None else 4)
        _judge(f"{name} {tag}", outs[tag], r64, r32)
    return c, outs, r64, widest


# ---- molecules -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["molecule1", "molecule2", "molecule3", "molecule7", "molecule24", "molecule70"])
def test_molecules_matrix_and_csr(name):
    c, outs, r64, widest = _both_layouts(name)
    n = len(c["pos"])
    if n == 1:
        assert all(float(o.abs().max()) == 0.0 for o in outs["matrix"] + outs["csr"])
    else:
        assert r64["energy"][0] < 0.0 and np.abs(r64["charge_grad"]).max() > 0.0
    if name == "molecule70":
        assert widest == 69 > 64, "every row must need a second lane trip"
    f = outs["matrix"][1].double()
    assert float(f.sum(0).abs().max()) <= 1e-5 * max(float(f.abs().max()), 1e-30) * np.sqrt(n)


# ---- padding and fill ------------------------------------------------------------------------------------------------------------------

def test_padding_atoms_fill_values_and_wide_matrix():
    from nvalchemiops.interactions.dispersion import dftd4

    c, outs, r64, _ = _both_layouts("padding")  # fill_value = N (the default), matrix 8 columns wider than any row
    n = len(c["pos"])
    for out in outs.values():
        for i in (4, 7):  # Z = 0 and Z >= nz: force, coordination number and charge gradient are exactly 0
            assert float(out[1][i].abs().max()) == 0.0 and float(out[2][i]) == 0.0 and float(out[3][i]) == 0.0
    # fill_value > N, in a matrix twice as wide
    _, args, kw, m, _, _ = _inputs("padding", max_neighbors=2 * n + 8)
    nm = m["neighbor_matrix"].clone()
    nm[nm == n] = n + 5
    other = dftd4(*args, **kw, neighbor_matrix=nm, fill_value=n + 5)
    assert all(torch.equal(a, b) for a, b in zip(other, outs["matrix"]))
    # explicit fill_value = N
    same = dftd4(*args, **kw, neighbor_matrix=m["neighbor_matrix"], fill_value=n)
    assert all(torch.equal(a, b) for a, b in zip(same, outs["matrix"]))


def test_element_without_references_is_padding():
    c, outs, r64, _ = _both_layouts("no_references")
    sel = torch.as_tensor(c["z"] == 8, device=DEV)
    assert int(sel.sum()) >= 3
    for out in outs.values():
        assert float(out[1][sel].abs().max()) == 0.0 and float(out[2][sel].abs().max()) == 0.0 and float(out[3][sel].abs().max()) == 0.0


# ---- references and species --------------------------------------------------------------------------------------------------------------

def test_one_and_seven_reference_elements_are_present_in_the_molecules():
    """The molecule cases hold atoms of the 1-reference and of the 7-reference element, references with ngw = 3, and NaN beyond n_ref."""
    c = K.case("molecule24")
    t = c["tables"]
    assert (c["z"] == K.R.ONE_REF_Z).any() and (c["z"] == K.R.SEVEN_REF_Z).any()
    assert (t["ngw"][K.R.SEVEN_REF_Z] == 3).any() and np.isnan(t["c6_ref"]).any() and np.isnan(t["cn_ref"][K.R.ONE_REF_Z, 1:]).all()
    _both_layouts("molecule24")


@pytest.mark.parametrize("name,count", [("species_slots", 16), ("species_slots_plus_1", 17), ("species_20", 20)])
def test_species_count_at_and_beyond_the_lds_slots(name, count):
    from nvalchemiops.interactions.dispersion.dftd4 import species_slots

    assert species_slots() == 16, "the species cases of tests/d4_cases.py are built around 16 slots"
    c, _, _, _ = _both_layouts(name)
    assert len(np.unique(c["z"])) == count


# ---- periodic ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["triclinic_f32", "triclinic_f64"])
def test_triclinic_box_with_virial(name):
    c, outs, r64, _ = _both_layouts(name)
    assert outs["matrix"][4].shape == (1, 3, 3) and r64["energy"][0] < 0.0
    assert c["pos"].dtype == (np.float64 if name.endswith("f64") else np.float32)


def test_cell_shorter_than_the_cutoff_self_images():
    _, _, _, m, _, _ = _inputs("self_images")
    nm, sh = m["neighbor_matrix"].cpu().numpy(), m["neighbor_matrix_shifts"].cpu().numpy()
    assert ((nm[0] == 0) & (np.abs(sh[0]).sum(1) > 0)).any(), "the test needs rows with the atom's own images"
    _both_layouts("self_images")


def test_batch_of_three_systems_one_of_them_a_single_atom():
    c, outs, r64, _ = _both_layouts("batch")
    assert outs["matrix"][0].shape == (3,) and outs["matrix"][4].shape == (3, 3, 3)
    assert float(outs["matrix"][0][2]) == 0.0 and float(outs["matrix"][4][2].abs().max()) == 0.0  # the single atom


# ---- charges and cn_cutoff -----------------------------------------------------------------------------------------------------------------

def test_zero_float64_and_strongly_negative_charges():
    from nvalchemiops.interactions.dispersion import dftd4

    _both_layouts("zero_charges")
    _both_layouts("zeff_negative")
    c, args, kw, m, _, _ = _inputs("molecule24")
    a = dftd4(args[0], args[1], args[2].double(), **kw, **m)  # float64 charges holding float32 values: the same numbers
    b = dftd4(*args, **kw, **m)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    z = K.references("zero_charges")[0]["energy"][0]
    assert z != K.references("molecule24")[0]["energy"][0]


def test_cn_cutoff_below_the_list_cutoff():
    from nvalchemiops.interactions.dispersion import dftd4

    c, outs, r64, _ = _both_layouts("cn_cutoff")
    _, args, kw, m, _, _ = _inputs("cn_cutoff")
    kw_all = dict(kw)
    kw_all.pop("cn_cutoff")
    every = dftd4(*args, **kw_all, **m)
    assert float((every[2] - outs["matrix"][2]).abs().max()) > 0.0, "pairs between cn_cutoff and the list cutoff must exist and count"


# ---- the D3 limit against the dftd3 kernel -----------------------------------------------------------------------------------------------

def test_one_reference_limit_equals_the_dftd3_kernel():
    from nvalchemiops.interactions.dispersion import D3Parameters, dftd3

    c, outs, r64, _ = _both_layouts("d3_limit")
    _, args, kw, m, _, _ = _inputs("d3_limit")
    d3 = S.d3_test_tables(17, seed=1000)
    c6ab = np.broadcast_to(c["tables"]["c6_ref"][:, :, 0, 0][:, :, None, None], d3["c6ab"].shape).copy()
    p3 = D3Parameters(rcov=_t(d3["rcov"]), r4r2=_t(d3["r4r2"]), c6ab=_t(c6ab), cn_ref=_t(d3["cn_ref"]))
    e3, f3, _, v3 = dftd3(args[0], args[1], d3_params=p3, cell=kw["cell"], compute_virial=True, **BJ, **m)
    bars = _bars(*K.references("d3_limit"))
    for k, a, b in (("energy", outs["matrix"][0], e3), ("forces", outs["matrix"][1], f3), ("virial", outs["matrix"][4], v3)):
        ref = r64[k]
        d3_bar = 1e-6 + 1e-6 * np.abs(ref) + EXTRA[k] * np.abs(ref).max()
        err = np.abs(a.cpu().numpy().astype(np.float64) - b.cpu().numpy().astype(np.float64))
        print(f"[d4] D3 limit vs dftd3 kernel   {k:11s} max |d4 - d3| {err.max():.3e}  worst / (bar_d4 + bar_d3) {(err / (bars[k][0] + d3_bar)).max():.3f}")
        assert (err <= bars[k][0] + d3_bar).all(), k
    assert float(outs["matrix"][3].abs().max()) == 0.0  # ga = 0: dE/dq = 0 exactly


# ---- determinism, layout, streams ------------------------------------------------------------------------------------------------------

def test_two_calls_are_bit_identical_and_layout_or_stream_do_not_matter():
    from nvalchemiops.interactions.dispersion import dftd4

    c, args, kw, m, l, _ = _inputs("triclinic_f32")
    for lk in (m, l):
        a = dftd4(*args, **kw, **lk)
        b = dftd4(*args, **kw, **lk)
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    wide = torch.zeros((args[0].shape[0], 6), dtype=args[0].dtype, device=DEV)
    wide[:, ::2] = args[0]
    strided = wide[:, ::2]
    assert not strided.is_contiguous()
    base = dftd4(*args, **kw, **m)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        other = dftd4(strided, args[1], args[2], **kw, **m)
    stream.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(base, other))


# ---- autograd ----------------------------------------------------------------------------------------------------------------------------

def test_backward_gives_minus_forces_and_charge_gradients():
    from nvalchemiops.interactions.dispersion import dftd4

    c, args, kw, m, l, _ = _inputs("batch")
    for dt in (torch.float32, torch.float64):
        pos = args[0].detach().clone().to(dt).requires_grad_()
        q = args[2].detach().clone().to(dt).requires_grad_()
        e, f, cn, cg, v = dftd4(pos, args[1], q, **kw, **l)
        assert e.requires_grad and not f.requires_grad and not cg.requires_grad and not cn.requires_grad
        w = torch.tensor([1.0, -2.0, 0.5], device=DEV)
        (e * w).sum().backward()
        wa = w[kw["batch_idx"].long()]
        assert pos.grad.dtype == dt and q.grad.dtype == dt
        assert torch.equal(pos.grad, (-wa[:, None] * f).to(dt)) and torch.equal(q.grad, (wa * cg).to(dt))
    pos = args[0].clone().requires_grad_()
    e = dftd4(pos, args[1], args[2], **kw, **m)[0]
    (g,) = torch.autograd.grad(e.sum(), pos, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()
    plain = dftd4(*args, **kw, **m)
    assert not plain[0].requires_grad


def test_charge_equilibration_into_dftd4_total_gradient():
    """q(positions) from `charge_equilibration`, then `dftd4`: backward assembles -forces + (dq/dr)^T dE/dq from the same kernels."""
    from nvalchemiops.interactions.dispersion import dftd4
    from nvalchemiops.interactions.electrostatics import charge_equilibration

    c = K.case("molecule24")
    n = len(c["pos"])
    g = np.random.default_rng(3)
    m, _, widest = _lists(c["pos"].astype(np.float64), None, 100.0)
    assert widest == n - 1
    pos = _t(c["pos"].astype(np.float64)).requires_grad_()
    chi, hard, sigma = _t(g.normal(size=n)), _t(g.uniform(1.0, 2.0, n)), _t(g.uniform(0.8, 1.5, n))
    q = charge_equilibration(pos, chi, hard, sigma, total_charge=0.0, tolerance=1e-10, **m)
    assert q.dtype == torch.float64 and q.requires_grad
    e, f, cn, cg = dftd4(pos, _t(c["z"]), q, d4_params=_params(c["tables"]), **BJ, **m)
    e.sum().backward(retain_graph=True)
    (chain,) = torch.autograd.grad(q, pos, grad_outputs=cg.double())
    want = -f.double() + chain
    err = (pos.grad - want).abs()
    rel = float((err / want.abs().clamp(min=1e-300)).max())
    print(f"[d4] QEq -> dftd4: max|grad| {float(want.abs().max()):.3e}, max|chain part| {float(chain.abs().max()):.3e}, max rel deviation {rel:.3e}")
    assert float(chain.abs().max()) > 0.0
    assert bool((err <= 1e-12 * want.abs()).all())


# ---- torch.compile -----------------------------------------------------------------------------------------------------------------------

def test_fullgraph_compile_equals_eager():
    from nvalchemiops.interactions.dispersion import dftd4

    c, args, kw, m, l, _ = _inputs("triclinic_f32")

    def matrix(x, q):
        return dftd4(x, args[1], q, **kw, **m)

    def csr(x, q):
        return dftd4(x, args[1], q, **kw, **l)

    for fn in (matrix, csr):
        torch._dynamo.reset()
        got = torch.compile(fn, mode="default", fullgraph=True)(args[0], args[2])
        want = fn(args[0], args[2])
        assert len(got) == len(want) == 5 and all(torch.equal(a, b) for a, b in zip(got, want))
