"""The eager path of the six dispersion operators against their custom ops, bit for bit.

A public function called eagerly and `torch.ops.nvalchemiops.<name>_nm` / `_nl` called directly on caller-owned outputs both end in one
launch function with the list arguments of `interactions/dispersion/_call.py::list_args`; given the same inputs the two launches get the
same arguments, so any difference between their outputs is a wiring error (a swapped width / fill value, a lost shift tensor, a scalar in
the wrong slot), not rounding: every output is compared with `==` on its bit pattern.

The input is the smallest on which those arguments can go wrong: a batch of two periodic systems with different triclinic cells (10 + 14
atoms, three species; the first cell is shorter than the cutoff along c, so the list holds the atoms' own images and the shifts matter;
the second has a vacuum gap with one atom alone in it: its row is empty), a padded matrix 44 wide (not a multiple of 64, wider than every
row), the default fill value and an explicit one above n, a three-body cutoff below the list cutoff, virials, positions in float32 and
float64.  Matrix and shifts are copies of what the search wrote: the copy is not the search's own tensor, so `dftd3` / `dftd3_zero` do not
take the packed-companion route, which the ops never take, and both paths are the same launch.
"""
import functools

import numpy as np
import pytest
import torch

from tests import atm_reference as A
from tests import d3_zero_reference as Z
from tests import d4_reference as R
from tests import systems as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RC, RC3, WIDTH = 7.0, 5.5, 44
D4_KEYS = R.TABLE_KEYS


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def two_boxes(dtype):
    """(positions [24,3], cells [2,3,3], batch_idx, numbers, charges) of the batch described in the module docstring."""
    pa, ca = A.lattice_box((2, 5, 1), a=4.2, seed=1, triclinic=True, dtype=np.float64)
    pb, cb = A.lattice_box((2, 3, 2), a=4.4, seed=2, triclinic=True, dtype=np.float64)
    inside = np.array([[0.5, 0.5, 0.5]]) @ cb          # an interstitial site of the slab
    cb[2] *= 3.0                                       # vacuum above the slab ...
    alone = np.array([[0.5, 0.5, 0.65]]) @ cb          # ... and one atom in the middle of it, farther than RC from every atom and image
    pos = np.concatenate([pa, pb, inside, alone])
    bi = np.concatenate([np.zeros(len(pa), np.int32), np.ones(len(pb) + 2, np.int32)])
    g = np.random.default_rng(4)
    z = g.choice(np.array([1, 6, 8], np.int32), len(pos))
    z[:3] = (1, 6, 8)
    q = g.uniform(-0.3, 0.3, len(pos)).astype(np.float32)
    return pos.astype(dtype), np.stack([ca, cb]).astype(dtype), bi, z, q


@functools.lru_cache(maxsize=None)
def inputs(dtype):
    """Device tensors of the batch and its three lists: ("matrix", "matrix_fill", "csr") -> the list keywords of a public function."""
    from nvalchemiops.neighborlist import neighbor_list

    pos, cell, bi, z, q = two_boxes(dtype)
    n = len(pos)
    tp, tc, tb = _t(pos), _t(cell), _t(bi)
    kw = dict(cell=tc, pbc=torch.ones((2, 3), dtype=torch.bool, device=DEV), batch_idx=tb, method="batch_cell_list", max_neighbors=WIDTH)
    lists = {}
    for tag, fill in (("matrix", None), ("matrix_fill", n + 7)):
        nm, num, sh = neighbor_list(tp, RC, fill_value=fill, **kw)
        assert nm.shape[1] == WIDTH and int(num.max()) < WIDTH and int(num.min()) == 0 and len(set(num.tolist())) > 3, num.tolist()
        assert int(nm.max()) == (n if fill is None else fill)
        lists[tag] = dict(neighbor_matrix=nm.clone(), neighbor_matrix_shifts=sh.clone(), fill_value=fill)
    nl, nptr, ush = neighbor_list(tp, RC, return_neighbor_list=True, **kw)
    assert int((nptr[1:] == nptr[:-1]).sum()) == 1  # the atom in the vacuum
    lists["csr"] = dict(neighbor_list=nl, neighbor_ptr=nptr, unit_shifts=ush)
    d3 = {k: _t(v) for k, v in S.d3_test_tables(17).items()}
    d4 = {k: _t(v) for k, v in R.d4_test_tables(17).items()}
    return dict(pos=tp, cell=tc, bi=tb, z=_t(z), q=_t(q), lists=lists, d3=d3, d4=d4, r0ab=_t(Z.synthetic_r0ab(18)))


def operator(name, x):
    """(public function, leading tensors after numbers, the tables in the op's order, the tables as public keywords, required scalars by
    name in the op's order, optional scalars by name, per-atom outputs) of one operator.  The optional scalars differ from the defaults."""
    from nvalchemiops.interactions import dispersion as D

    d3t = [x["d3"][k] for k in ("rcov", "r4r2", "c6ab", "cn_ref")]
    d3kw = dict(covalent_radii=d3t[0], r4r2=d3t[1], c6_reference=d3t[2], coord_num_ref=d3t[3])
    d4t = [x["d4"][k] for k in D4_KEYS]
    d4kw = dict(d4_params=D.D4Parameters(**{k: x["d4"][k] for k in D4_KEYS}))
    bj = dict(a1=0.4289, a2=4.4407)
    s5 = dict(s6=0.9, k1=15.0, k3=-3.5, s5_smoothing_on=5.0, s5_smoothing_off=6.5)
    d4s = dict(cn_cutoff=6.0, wf=5.5, ga=2.8, gc=1.9, k_cn=7.0)
    return {
        "dftd3": (D.dftd3, (), d3t, d3kw, dict(bj, s8=0.7875), s5, 1),
        "dftd3_zero": (D.dftd3_zero, (), d3t + [x["r0ab"]], dict(d3kw, cutoff_radii=x["r0ab"]), dict(rs6=1.217, s8=0.722),
                       dict(s5, rs8=0.95, alpha=13.5, beta=0.05), 1),
        "dftd3_atm": (D.dftd3_atm, (), d3t, d3kw, dict(bj, three_body_cutoff=RC3), dict(s9=0.9, alpha=14.0, k1=15.0, k3=-3.5), 0),
        "dftd3_zero_atm": (D.dftd3_zero_atm, (), d3t + [x["r0ab"]], dict(d3kw, cutoff_radii=x["r0ab"]), dict(three_body_cutoff=RC3),
                           dict(rs9=1.3, s9=0.9, alpha=14.0, k1=15.0, k3=-3.5), 0),
        "dftd4": (D.dftd4, (x["q"],), d4t, d4kw, dict(a1=0.4, a2=4.0, s8=0.8), dict(d4s, s6=0.9), 2),
        "dftd4_atm": (D.dftd4_atm, (), d4t, d4kw, dict(a1=0.4, a2=4.0, three_body_cutoff=RC3), dict(d4s, s9=0.9, alpha=14.0), 0),
    }[name]


def eager_and_op(name, layout, dtype):
    """The outputs of the public function called eagerly, and the caller-owned outputs `torch.ops.nvalchemiops.<name>_nm/_nl` wrote."""
    x = inputs(dtype)
    fn, lead, tables, table_kw, required, optional, k = operator(name, x)
    lst = x["lists"][layout]
    eager = fn(x["pos"], x["z"], *lead, **required, **optional, **table_kw, batch_idx=x["bi"], cell=x["cell"], compute_virial=True, **lst)
    n = x["pos"].shape[0]
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)  # noqa: E731
    outs = [nan(2), nan(n, 3)] + [nan(n) for _ in range(k)] + [nan(2, 3, 3)]
    common = dict(optional, batch_idx=x["bi"], cell=x["cell"], compute_virial=True)
    if layout == "csr":
        op = getattr(torch.ops.nvalchemiops, name + "_nl")
        op(x["pos"], x["z"], *lead, lst["neighbor_list"][1], lst["neighbor_ptr"], *tables, *required.values(), *outs,
           unit_shifts=lst["unit_shifts"], **common)
    else:
        op = getattr(torch.ops.nvalchemiops, name + "_nm")
        op(x["pos"], x["z"], *lead, lst["neighbor_matrix"], *tables, *required.values(), *outs, fill_value=lst["fill_value"],
           neighbor_matrix_shifts=lst["neighbor_matrix_shifts"], **common)
    return eager, outs


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("layout", ["matrix", "matrix_fill", "csr"])
@pytest.mark.parametrize("name", ["dftd3", "dftd3_zero", "dftd3_atm", "dftd3_zero_atm", "dftd4", "dftd4_atm"])
def test_eager_call_and_custom_op_are_bit_identical(name, layout, dtype):
    eager, outs = eager_and_op(name, layout, dtype)
    assert len(eager) == len(outs)
    for i, (a, b) in enumerate(zip(eager, outs)):
        assert a.shape == b.shape and a.dtype == b.dtype == torch.float32, (i, a.shape, b.shape)
        assert torch.isfinite(a).all(), f"output {i} of the eager call is not finite"
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"output {i}: eager call and custom op differ by {(a - b).abs().max().item():.3e}"
    assert float(eager[0].abs().min()) > 0 and float(eager[-1].abs().max()) > 0  # both systems have an energy, and there is a virial


# ---- the energy op pairs of _eops.py outside tests/test_multipole_call_gpu.py: van der Waals pairs, the dispersion Ewald sum and its mesh half,
# ---- Gaussian charges, scaled dipole pairs, the five valence kinds -----------------------------------------------------------------------------
# Every pair is a row of one table built by one maker (one forward / backward pair, outputs not asked for as empty [0] tensors), so they are
# compared here: the eager `_forward` against the op, bit for bit, and the op's backward against the adjoint function.  The inputs are the
# batch fixtures of tests/layout_cases.py (cells of their own, reduced sites, scales, per-system alpha and k-vectors, an (8, 10, 12) mesh) and
# the "batch" case of tests/test_valence_gpu.py (three cells, the middle system empty): tens of atoms in 2 - 3 systems, the smallest input
# that tells an argument in the wrong slot, a scalar taken for a saved tensor, a dropped flag and a per-system mix-up apart.
VALENCE_KINDS = ("bond_stretch", "angle_bend", "stretch_bend", "out_of_plane_bend", "torsion")
MESH_DIMS, MESH_ORDER = (8, 10, 12), 5
# family: (the op's outputs after the energies, the inputs whose gradient the op refuses)
FAMILIES = {
    "buffered_14_7": (("forces", "radius_gradients", "epsilon_gradients", "virial"), ()),
    "lennard_jones": (("forces", "radius_gradients", "epsilon_gradients", "virial"), ()),
    "ewald_dispersion_real_space": (("forces", "coefficient_gradients", "virial"), ("cell", "alpha")),
    "ewald_dispersion_reciprocal_space": (("forces", "coefficient_gradients", "virial"), ("cell", "k_vectors", "alpha")),
    "pme_dispersion_reciprocal_space": (("forces", "coefficient_gradients", "virial"), ("cell", "alpha")),
    "gaussian_charge_correction": (("forces", "charge_gradients", "sigma_gradients", "virial"), ()),
    "dipole_pair_scale_correction": (("forces", "charge_gradients", "dipole_gradients", "polarizability_gradients", "virial"), ("cell",)),
    **{k: (("forces", "parameter_gradients", "virial"), ()) for k in VALENCE_KINDS},
}
CASES = ([(f, m) for f in ("buffered_14_7", "lennard_jones", "ewald_dispersion_real_space", "gaussian_charge_correction") for m in ("matrix", "csr")]
         + [("dipole_pair_scale_correction", "csr")]
         + [(f, "none") for f in ("ewald_dispersion_reciprocal_space", "pme_dispersion_reciprocal_space") + VALENCE_KINDS])


def _stored(entries, n, fmt, values=None):
    """(the five list arguments, mask value, `values` per slot | None) of row-sorted entries (i, j, S) as a padded matrix or as CSR."""
    from tests import sweep_cases as W

    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=DEV, dtype=torch.int32)  # noqa: E731
    i, j, S = (np.asarray(e) for e in entries)
    assert (np.diff(i) >= 0).all()
    if fmt == "matrix":
        nm, sh, val = W.padded_matrix((i, j, S), n, values)
        return (None, None, None, t(nm), t(sh)), n, val
    ptr = np.zeros(n + 1, np.int32)
    ptr[1:] = np.cumsum(np.bincount(i, minlength=n))
    return (t(np.stack([i, j])), t(ptr), t(S), None, None), -1, values


def _family_args(family, dtype, fmt):
    """(op, forward, adjoint, number of differentiable inputs, the op's arguments before the flags by name) of one family."""
    import importlib

    from nvalchemiops import _eops
    from nvalchemiops import interactions as IA
    from tests import layout_cases as LC
    from tests import sweep_cases as W

    t = lambda a, dt=None: torch.as_tensor(np.ascontiguousarray(a), device=DEV, dtype=dt)  # noqa: E731
    lists = ("neighbor_list", "neighbor_ptr", "neighbor_shifts", "neighbor_matrix", "neighbor_matrix_shifts")
    named = lambda names, values: dict(zip(names, values, strict=True))  # noqa: E731
    if family in VALENCE_KINDS:
        from nvalchemiops.interactions import valence as V
        from tests import test_valence_gpu as TV

        kind = VALENCE_KINDS.index(family)
        fn = importlib.import_module("nvalchemiops.interactions.valence.functions")
        c = TV._case(family, "batch")
        bi = c["batch"].to(DEV)
        terms = V.ValenceTerms(c["atoms"].to(DEV), c["pos"].shape[0], batch_idx=bi)
        args = named(("positions", "parameters", "cell", "batch_idx", "atoms", "slot_ptr", "slot_idx", "cubic", "quartic", "pentic", "sextic", "plane"),
                     (c["pos"].to(DEV, dtype), c["par"].to(DEV, dtype), c["cell"].to(DEV, dtype), bi, terms.atoms, terms.slot_ptr, terms.slot_idx,
                      *TV._model(family)[0]["consts"], fn.PLANES["wdc"]))
        return _eops.VALENCE_OPS[kind], functools.partial(fn._forward, kind), functools.partial(fn._adjoint, kind), 2, args
    if family == "gaussian_charge_correction":
        ga = importlib.import_module("nvalchemiops.interactions.electrostatics.gaussian")
        c = LC.gaussian(True)
        i, j, S = (e.numpy() for e in LC._entries(c["pos"], c["cell"], c["batch_idx"], LC.GC_RC))
        order = np.argsort(i, kind="stable")
        stored, mask, _ = _stored((i[order], j[order], S[order]), len(c["pos"]), fmt)
        args = named(("positions", "charges", "sigma", "cell", "batch_idx") + lists + ("mask_value", "self_energy", "neutralizing_background"),
                     (t(c["pos"], dtype), t(c["q"], dtype), t(c["sigma"], dtype), t(c["cell"], dtype), t(c["batch_idx"], torch.int32), *stored, mask,
                      True, True))
        return _eops.gaussian_charge_correction_op, ga._forward, ga._adjoint, 4, args
    if family == "dipole_pair_scale_correction":
        from tests import dipole_scale_cases as SC

        ds = importlib.import_module("nvalchemiops.interactions.electrostatics.dipole_scale")
        p = LC.dipole_scale(True)
        stored, mask, _ = _stored(p["entries"], p["n"], fmt)
        polar = np.where(np.isnan(p["polar"]), 0.0, p["polar"])  # (a NaN polarisability has a NaN gradient slot, which equals nothing)
        args = named(("positions", "charges", "dipoles", "polarizability", "direct_scales", "mutual_scales", "cell", "batch_idx") + lists
                     + ("mask_value", "minimum_image", "thole"),
                     (t(p["pos"], dtype), t(p["q"], dtype), t(p["mu"], dtype), t(polar, dtype), t(p["sd"], torch.float64), t(p["sm"], torch.float64),
                      t(p["cell"], dtype), t(p["batch_idx"], torch.int32), *stored, mask, False, SC.A_T))
        return _eops.dipole_pair_scale_correction_op, ds._forward, ds._adjoint, 4, args
    vdw = family in W.VDW_KINDS
    c = LC.vdw(True, family) if vdw else LC.dispersion_ewald(True)
    n = len(c["pos"])
    bi = t(c["batch_idx"], torch.int32)
    if vdw:
        stored, mask, scales = _stored(c["entries"], n, fmt, c["scales"])
        kind = W.VDW_KINDS.index(family)
        pair = importlib.import_module("nvalchemiops.interactions.vdw.pair")
        sites = IA.ReducedSites(t(c["parent"], torch.int32), t(c["kappa"], dtype), batch_idx=bi)
        m = W.vdw_model(c, family)
        args = named(("positions", "radii", "epsilons", "cell", "batch_idx", "parent", "reduction", "child_ptr", "child_idx", "pair_scales") + lists
                     + ("mask_value", "cutoff", "taper", "delta", "gamma", "radius_rule", "epsilon_rule"),
                     (t(c["pos"], dtype), t(c["radii"], dtype), t(c["eps"], dtype), t(c["cells"], dtype), bi, sites.parent, sites.reduction,
                      sites.child_ptr, sites.child_idx, t(scales, torch.float64), *stored, mask, float(m["cutoff"]), float(m["taper"]),
                      float(m.get("delta", 1.0)), float(m.get("gamma", 1.0)), pair.RADIUS_RULES[m["radius_rule"]], pair.EPSILON_RULES[m["epsilon_rule"]]))
        return _eops.VDW_OPS[kind], functools.partial(pair._forward, kind), functools.partial(pair._adjoint, kind), 3, args
    ew = importlib.import_module("nvalchemiops.interactions.vdw.ewald")
    head = dict(positions=t(c["pos"], dtype), coefficients=t(c["c"], dtype), cell=t(c["cells"], dtype))
    alpha = t(c["alpha"], dtype)
    if family == "ewald_dispersion_real_space":
        stored, mask, _ = _stored(c["entries"], n, fmt)
        args = dict(head, alpha=alpha, batch_idx=bi, **named(lists, stored), mask_value=mask, counted_cutoff=float(c["counted"][0]),
                    counted_taper=-1.0 if c["counted"][1] is None else float(c["counted"][1]))
        return _eops.ewald_dispersion_real_space_op, ew._real_forward, ew._real_adjoint, 2, args
    if family == "pme_dispersion_reciprocal_space":
        pme = importlib.import_module("nvalchemiops.interactions.vdw.pme")
        args = dict(head, alpha=alpha, batch_idx=bi, nx=MESH_DIMS[0], ny=MESH_DIMS[1], nz=MESH_DIMS[2], order=MESH_ORDER)
        return _eops.pme_dispersion_reciprocal_space_op, pme._recip_forward, pme._recip_adjoint, 2, args
    args = dict(head, k_vectors=c["k_vectors"].to(DEV).to(dtype), alpha=alpha, batch_idx=bi)
    return _eops.ewald_dispersion_reciprocal_space_op, ew._recip_forward, ew._recip_adjoint, 2, args


def _same(got, ref, exact, what):
    """Bit for bit, but for the float64 outputs of the mesh half: its float64 spread adds in arrival order, and they get the relative 1e-12
    tests/test_multipole_call_gpu.py grants float64 mesh outputs."""
    assert got.shape == ref.shape and got.dtype == ref.dtype, what
    if exact:
        assert torch.equal(got, ref), f"{what}: max difference {(got - ref).abs().max().item():.3e}"
    else:
        scale, err = ref.abs().max().item(), (got - ref).abs().max().item()
        assert err <= 1e-12 * scale, f"{what}: max err {err:.3e} > 1e-12 x {scale:.3e}"


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("family,fmt", CASES)
def test_vdw_and_dispersion_ewald_ops_match_the_eager_path_and_the_adjoint(family, fmt, dtype):
    op, forward, adjoint, n_diff, named = _family_args(family, dtype, fmt)
    args, n_flags = tuple(named.values()), len(FAMILIES[family][0])
    exact = not (family == "pme_dispersion_reciprocal_space" and dtype == torch.float64)
    for flags in ((True,) * n_flags, (False,) * n_flags, (False,) * (n_flags - 1) + (True,)):
        eager, direct = forward(*args, *flags), op(*args, *flags)
        assert len(eager) == len(direct) == n_flags + 1
        for k, (e, d, want) in enumerate(zip(eager, direct, (True,) + flags)):
            if not want:
                assert e is None and tuple(d.shape) == (0,), f"{family} output {k}: not asked for"
                continue
            assert e.dtype == dtype and float(e.abs().max()) > 0, f"{family} {fmt} flags {flags}: output {k}"
            _same(d, e, exact, f"{family} {fmt} flags {flags}: output {k}")
    leaves = [a.clone().requires_grad_(True) for a in args[:n_diff]]  # (for the Gaussian op the fourth is the cell)
    g = torch.as_tensor(np.random.default_rng(5).normal(size=leaves[0].shape[0]), device=DEV).to(dtype)
    grads = torch.autograd.grad(op(*leaves, *args[n_diff:], *(False,) * n_flags)[0], leaves, grad_outputs=g)
    ref = adjoint(*args, g)
    assert len(grads) == len(ref) == n_diff
    for k, (got, r) in enumerate(zip(grads, ref)):
        assert r.dtype == torch.float64 and float(r.abs().max()) > 0, f"{family} {fmt}: gradient {k}"
        _same(got, r.reshape(got.shape).to(dtype), exact, f"{family} {fmt}: gradient {k} against the adjoint's")


@pytest.mark.parametrize("family,fmt", [(f, m) for f, m in CASES if m != "matrix"])
def test_refusals_and_silent_nones_of_the_energy_ops(family, fmt):
    """A gradient of an explicit output raises the second-order text with the op's name; an input without an adjoint that requires a gradient
    raises its refusal where the family has one (dispersion sums: cell, alpha, k-vectors; scaled dipole pairs: cell).  The van der Waals and
    valence ops have none: their cell gets no gradient (None), silently, while the other gradients arrive."""
    op, _, _, n_diff, named = _family_args(family, torch.float64, fmt)
    outputs, refused = FAMILIES[family]
    name = f"alchemiops::_{family}"
    for what in refused:
        a = dict(named, positions=named["positions"].clone().requires_grad_(True))
        a[what] = named[what].clone().requires_grad_(True)
        with pytest.raises(NotImplementedError) as err:
            op(*a.values(), *[False] * len(outputs))[0].sum().backward()
        assert f"{name}: gradients w.r.t. {what} are not provided by the " in str(err.value)
        if family != "dipole_pair_scale_correction":
            assert "not provided by the dispersion Ewald sum (out of scope); use compute_virial for the strain derivative." in str(err.value)
    positions = named["positions"].clone().requires_grad_(True)
    out = op(positions, *list(named.values())[1:], *[True] * len(outputs))
    for what, o in zip(outputs, out[1:]):
        with pytest.raises(NotImplementedError) as err:
            torch.autograd.grad(o.sum(), positions, retain_graph=True)
        assert f"{name}: derivatives of the '{what}' output are second derivatives of the pair kernels" in str(err.value)
    if family in VALENCE_KINDS or family in ("buffered_14_7", "lennard_jones"):
        a = dict(named, positions=named["positions"].clone().requires_grad_(True), cell=named["cell"].clone().requires_grad_(True))
        op(*a.values(), *[False] * len(outputs))[0].sum().backward()
        assert a["cell"].grad is None and float(a["positions"].grad.abs().max()) > 0
