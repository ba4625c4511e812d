"""The call layer of the ten point-multipole operator halves (interactions/electrostatics/_multipoles.py and the op table of _eops.py) and of
`rotate_multipoles`, whose op is written out beside that table: the eager path against the custom op, and the op's backward against the
operator's adjoint function.

Both sides of every comparison reach the same launches, so everything but the float64 mesh outputs must agree bit for bit (the float64
spread adds in arrival order; those agree to the relative 1e-12 of tests/test_pme_quadrupole_gpu.py).  What can differ is the wiring: an
argument in the wrong slot of the generated forward / setup_context / backward, a saved tensor taken for a scalar, a flag dropped.  The input
is the batch of tests/test_dispersion_call_gpu.py (two triclinic cells of 10 + 14 atoms, self-images in the first, an empty row in the
second) on a full list as a matrix 44 wide with an explicit mask value above N and as CSR with shifts, two different alphas, a (8, 10, 12)
mesh, and for the operators that take `cell=None` the first system alone as a cluster.  `pair_scales` is a symmetric hash of the two atom
indices (the classes 0, 0.4, 0.8 and 1 of tests/pair_scale_cases.py, whatever the image) on every slot of that list.  `rotate_multipoles`
runs on the batch of three cells of tests/test_local_frames_gpu.py.
"""
import functools

import numpy as np
import pytest
import torch

from tests.test_dispersion_call_gpu import RC, WIDTH, two_boxes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MESH_DIMS = (8, 10, 12)
DTYPES = {"f32": torch.float32, "f64": torch.float64}
PER_ATOM = {"positions": (3,), "charges": (), "dipoles": (3,), "quadrupoles": (3, 3), "polarizability": ()}
DP, QD, TH = ("positions", "charges", "dipoles"), ("positions", "charges", "dipoles", "quadrupoles"), ("positions", "charges", "dipoles",
                                                                                                         "polarizability")
LISTS = ("batch_idx", "neighbor_list", "neighbor_ptr", "neighbor_shifts", "neighbor_matrix", "neighbor_matrix_shifts", "mask_value")
MESH = ("cell", "alpha", "batch_idx", "nx", "ny", "nz", "spline_order")
KSUM = ("cell", "k_vectors", "alpha", "batch_idx")
# operator: (module, adjoint function, differentiable inputs, the op's arguments after them, extra output | None, inputs without an adjoint,
#            may the cell be None, spline orders | None)
OPERATORS = {
    "ewald_dipole_real_space": ("dipole", "_real_adjoint", DP, ("cell", "alpha") + LISTS, None, ("cell", "alpha"), False, None),
    "ewald_dipole_reciprocal_space": ("dipole", "_recip_adjoint", DP, KSUM, None, ("cell", "k_vectors", "alpha"), False, None),
    "pme_dipole_reciprocal_space": ("pme_dipole", "_recip_adjoint", DP, MESH, None, ("cell", "alpha"), False, (4, 5)),
    "thole_dipole_correction": ("thole", "_adjoint", TH, ("cell",) + LISTS + ("thole",), "polarizability_gradients", ("cell",), True, None),
    "ewald_quadrupole_real_space": ("quadrupole", "_real_adjoint", QD, ("cell", "alpha") + LISTS, "quadrupole_gradients", ("cell", "alpha"),
                                    False, None),
    "ewald_quadrupole_reciprocal_space": ("quadrupole", "_recip_adjoint", QD, KSUM, "quadrupole_gradients", ("cell", "k_vectors", "alpha"),
                                          False, None),
    "pme_quadrupole_reciprocal_space": ("pme_quadrupole", "_recip_adjoint", QD, MESH, "quadrupole_gradients", ("cell", "alpha"), False, (5, 6)),
    "coulomb_dipole_correction": ("cluster", "_dipole_adjoint", DP, ("cell",) + LISTS, None, ("cell",), True, None),
    "coulomb_quadrupole_correction": ("cluster", "_quadrupole_adjoint", QD, ("cell",) + LISTS, "quadrupole_gradients", ("cell",), True, None),
    "pair_scale_correction": ("pair_scale", "_adjoint", QD, ("pair_scales", "cell") + LISTS + ("minimum_image",), "quadrupole_gradients", ("cell",),
                              True, None),
}


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def _pair_scales(i, j, dtype):
    """One scale per slot, symmetric in (i, j) whatever the image; a padding slot gets a value that is not looked at."""
    table = torch.tensor([0.0, 0.4, 0.8, 1.0, 0.4], dtype=dtype, device=DEV)
    i, j = i.long(), j.long()
    return table[(i * j + i + j) % 5].contiguous()


def _row_of(nm):
    return torch.arange(nm.shape[0], device=nm.device)[:, None].expand_as(nm)


@functools.lru_cache(maxsize=None)
def inputs(tag):
    """Everything an operator can be given, by argument name: "batch" (both boxes, with the matrix and the CSR form of the full list) and
    "cluster" (the first box's atoms without a cell, all pairs inside RC as a matrix without shifts)."""
    from nvalchemiops.interactions.electrostatics import generate_k_vectors_ewald_summation
    from nvalchemiops.neighborlist import neighbor_list

    dtype = DTYPES[tag]
    npdt = np.float32 if tag == "f32" else np.float64
    pos, cell, bi, _, q = two_boxes(npdt)
    n = len(pos)
    g = np.random.default_rng(11)
    atoms = dict(positions=_t(pos), charges=_t(q.astype(npdt)), dipoles=_t(g.normal(0.0, 0.2, (n, 3)).astype(npdt)),
                 quadrupoles=_t(g.normal(0.0, 0.3, (n, 3, 3)).astype(npdt)), polarizability=_t(g.uniform(0.8, 1.6, n).astype(npdt)))
    tc, tb = _t(cell), _t(bi)
    kw = dict(cell=tc, pbc=torch.ones((2, 3), dtype=torch.bool, device=DEV), batch_idx=tb, method="batch_cell_list", max_neighbors=WIDTH)
    nm, num, sh = neighbor_list(atoms["positions"], RC, fill_value=n + 7, **kw)
    assert nm.shape[1] == WIDTH and int(num.min()) == 0 and int(nm.max()) == n + 7
    nl, nptr, ush = neighbor_list(atoms["positions"], RC, return_neighbor_list=True, **kw)
    none = dict(neighbor_list=None, neighbor_ptr=None, neighbor_shifts=None, neighbor_matrix=None, neighbor_matrix_shifts=None)
    common = dict(cell=tc, alpha=torch.tensor([0.30, 0.36], dtype=dtype, device=DEV), batch_idx=tb, thole=0.39,
                  k_vectors=generate_k_vectors_ewald_summation(tc, 1.1), nx=MESH_DIMS[0], ny=MESH_DIMS[1], nz=MESH_DIMS[2])
    assert common["k_vectors"].shape[0] == 2 and 8 <= common["k_vectors"].shape[1] <= 400
    common["minimum_image"] = False
    batch = {"matrix": dict(atoms, **common, **dict(none, neighbor_matrix=nm.clone(), neighbor_matrix_shifts=sh.clone()), mask_value=n + 7,
                            pair_scales=_pair_scales(_row_of(nm), nm, dtype)),
             "csr": dict(atoms, **common, **dict(none, neighbor_list=nl, neighbor_ptr=nptr, neighbor_shifts=ush), mask_value=-1,
                         pair_scales=_pair_scales(nl[0], nl[1], dtype))}
    assert {0.0, 0.4, 0.8, 1.0} == {round(float(v), 6) for v in batch["csr"]["pair_scales"].unique()}
    first = np.flatnonzero(bi == 0)
    d = np.linalg.norm(pos[first, None, :].astype(np.float64) - pos[None, first, :], axis=-1)
    rows = [np.flatnonzero((d[i] < RC) & (np.arange(len(first)) != i)) for i in range(len(first))]
    width = max(len(r) for r in rows) + 2
    cm = np.full((len(first), width), len(first) + 3, np.int32)
    for i, r in enumerate(rows):
        cm[i, :len(r)] = r
    cluster = dict({k: v[: len(first)].contiguous() for k, v in atoms.items()}, **none, cell=None, batch_idx=None, thole=0.39,
                   mask_value=len(first) + 3)
    cluster["neighbor_matrix"] = _t(cm)
    cluster.update(pair_scales=_pair_scales(_row_of(cluster["neighbor_matrix"]), cluster["neighbor_matrix"], dtype), minimum_image=False)
    return dict(batch=batch, cluster=dict(matrix=cluster))


def cases(name):
    """(label, dict of arguments by name) of every call of one operator."""
    _, _, _, rest, _, _, cell_optional, orders = OPERATORS[name]
    has_list = "neighbor_matrix" in rest
    out = []
    for tag in DTYPES:
        x = inputs(tag)
        for layout in ("matrix", "csr") if has_list else ("matrix",):
            for order in orders or (None,):
                label = f"{tag}" + (f"-{layout}" if has_list else "") + (f"-order{order}" if order else "")
                out.append((label, dict(x["batch"][layout], spline_order=order)))
        if cell_optional:
            out.append((f"{tag}-cluster", x["cluster"]["matrix"]))
    return out


def call_public(name, a, flags):
    from nvalchemiops.interactions import electrostatics as E

    _, _, diff, rest, extra, _, _, orders = OPERATORS[name]
    kw = {k: a[k] for k in diff + rest if k not in ("nx", "ny", "nz")}
    if orders:
        kw["mesh_dimensions"] = (a["nx"], a["ny"], a["nz"])
    return getattr(E, name)(**kw, **flags)


def outputs_of(name):
    extra = OPERATORS[name][4]
    return ("energies", "forces", "charge_gradients", "dipole_gradients") + ((extra,) if extra else ()) + ("virial",)


def flags_of(name, a):
    """Every flag on; no virial for a cluster."""
    return {f"compute_{o}": (o != "virial" or a["cell"] is not None) for o in outputs_of(name)[1:]}


def same(got, ref, what, exact):
    assert got.shape == ref.shape and got.dtype == ref.dtype, what
    if exact:
        assert torch.equal(got, ref), f"{what}: max difference {(got - ref).abs().max().item():.3e}"
    else:
        scale, err = ref.abs().max().item(), (got - ref).abs().max().item()
        assert err <= 1e-12 * scale, f"{what}: max err {err:.3e} > 1e-12 x {scale:.3e}"


def _exact(name, label):
    return not (OPERATORS[name][7] and label.startswith("f64"))  # the float64 spread adds in arrival order


@pytest.mark.parametrize("name", sorted(OPERATORS))
def test_eager_call_matches_op(name):
    from nvalchemiops import _eops  # noqa: F401  (registers the ops)

    _, _, diff, rest, _, _, _, _ = OPERATORS[name]
    op = getattr(torch.ops.alchemiops, f"_{name}")
    for label, a in cases(name):
        flags = flags_of(name, a)
        eager = call_public(name, a, flags)
        direct = op(*[a[k] for k in diff + rest], *flags.values())
        direct = [o for o, w in zip(direct, (True,) + tuple(flags.values())) if w]
        assert len(eager) == len(direct)
        for what, e, d in zip([o for o in outputs_of(name) if o == "energies" or flags[f"compute_{o}"]], eager, direct):
            same(e, d, f"{name} {label} {what}", _exact(name, label))


@pytest.mark.parametrize("name", sorted(OPERATORS))
def test_op_backward_matches_adjoint(name):
    import importlib

    from nvalchemiops import _eops  # noqa: F401

    module, adjoint, diff, rest, _, _, _, _ = OPERATORS[name]
    op = getattr(torch.ops.alchemiops, f"_{name}")
    adjoint = getattr(importlib.import_module(f"nvalchemiops.interactions.electrostatics.{module}"), adjoint)
    for label, a in cases(name):
        leaves = [a[k].clone().requires_grad_(True) for k in diff]
        others = [a[k] for k in rest]
        g = torch.as_tensor(np.random.default_rng(5).normal(size=leaves[0].shape[0]), device=DEV).to(leaves[0].dtype)
        energies = op(*leaves, *others, *[False] * len(flags_of(name, a)))[0]
        grads = torch.autograd.grad(energies, leaves, grad_outputs=g)
        ref = adjoint(*[a[k] for k in diff], *others, g)
        assert len(grads) == len(ref) == len(diff)
        for what, got, r, leaf in zip(diff, grads, ref, leaves):
            assert r.dtype == torch.float64
            same(got, r.to(leaf.dtype), f"{name} {label} d/d{what}", _exact(name, label))


@pytest.mark.parametrize("name", sorted(OPERATORS))
def test_refusals_come_from_the_table(name):
    from nvalchemiops import _eops  # noqa: F401

    _, _, diff, rest, _, no_adjoint, _, _ = OPERATORS[name]
    op = getattr(torch.ops.alchemiops, f"_{name}")
    label, a = cases(name)[0]
    flags = flags_of(name, a)
    for what in no_adjoint:
        args = dict(a, positions=a["positions"].clone().requires_grad_(True))
        args[what] = a[what].clone().requires_grad_(True)
        energies = op(*[args[k] for k in diff + rest], *[False] * len(flags))[0]
        with pytest.raises(NotImplementedError) as err:
            energies.sum().backward()
        assert f"alchemiops::_{name}: gradients w.r.t. {what} are not provided" in str(err.value)
    positions = a["positions"].clone().requires_grad_(True)
    out = op(positions, *[a[k] for k in (diff + rest)[1:]], *flags.values())
    for what, o in zip(outputs_of(name)[1:], out[1:]):
        with pytest.raises(NotImplementedError) as err:
            torch.autograd.grad(o.sum(), positions, retain_graph=True)
        assert f"alchemiops::_{name}: derivatives of the '{what}' output are second derivatives of the pair kernels" in str(err.value)


def test_pair_scales_that_require_a_gradient_are_refused():
    """The one refusal of `pair_scale_correction` that is not a row of the table: it is raised by the public function, before the op."""
    for label, a in cases("pair_scale_correction"):
        args = dict(a, pair_scales=a["pair_scales"].clone().requires_grad_(True))
        with pytest.raises(NotImplementedError, match="pair_scales is not differentiable"):
            call_public("pair_scale_correction", args, {})


# ---- rotate_multipoles: its op is written out beside the table (two differentiable outputs, a frame table) -----------------------------------
@pytest.mark.parametrize("tag", sorted(DTYPES))
def test_rotate_multipoles_eager_matches_op_and_backward_matches_adjoint(tag):
    from nvalchemiops import _eops
    from nvalchemiops.interactions.electrostatics import frames as FR
    from nvalchemiops.interactions.electrostatics import rotate_multipoles
    from tests import test_local_frames_gpu as TLF

    dtype = DTYPES[tag]
    d = TLF._device_inputs(TLF._case("batch"), dtype)
    fr = d["frames"]
    tables = (fr.frame_atoms, fr.frame_kinds, fr.inverse_ptr, fr.inverse_slots)
    op = torch.ops.alchemiops._rotate_multipoles
    eager = FR._forward(d["pos"], d["mu"], d["quad"], d["cell"], d["batch"], fr.frame_atoms, fr.frame_kinds)
    public = rotate_multipoles(d["pos"], d["mu"], d["quad"], fr, d["cell"], batch_idx=d["batch"])
    direct = op(d["pos"], d["mu"], d["quad"], d["cell"], d["batch"], *tables)
    for what, e, p, o in zip(("dipoles", "quadrupoles"), eager, public, direct):
        same(e, o, f"rotate_multipoles {tag} {what}, eager against the op", True)
        same(p, o, f"rotate_multipoles {tag} {what}, public against the op", True)
        assert float(o.abs().max()) > 0
    # an input that is None: an empty [0] tensor in its place, the other output unchanged
    only = op(d["pos"], d["mu"], None, d["cell"], d["batch"], *tables)
    assert tuple(only[1].shape) == (0,) and torch.equal(only[0], direct[0])
    only = op(d["pos"], None, d["quad"], d["cell"], d["batch"], *tables)
    assert tuple(only[0].shape) == (0,) and torch.equal(only[1], direct[1])
    # the op's backward against the adjoint function, both outputs weighted, and each output alone
    for g_mu, g_qd in ((d["w_mu"], d["w_q"]), (d["w_mu"], None), (None, d["w_q"])):
        leaves = [d[k].clone().requires_grad_(True) for k in ("pos", "mu", "quad")]
        out = op(*leaves, d["cell"], d["batch"], *tables)
        used = [(o, g) for o, g in zip(out, (g_mu, g_qd)) if g is not None]
        grads = torch.autograd.grad([o for o, _ in used], leaves, grad_outputs=[g for _, g in used], allow_unused=True)
        ref = FR._adjoint(d["pos"], d["mu"], d["quad"], d["cell"], d["batch"], *tables, g_mu, g_qd)
        for what, got, r, leaf in zip(("positions", "local_dipoles", "local_quadrupoles"), grads, ref, leaves):
            assert r.dtype == torch.float64
            if got is None:  # an output that was not used sends nothing to its own local input
                assert float(r.abs().max()) == 0.0, what
                continue
            same(got, r.to(leaf.dtype), f"rotate_multipoles {tag} d/d{what}", True)
    pos, cell = d["pos"].clone().requires_grad_(True), d["cell"].clone().requires_grad_(True)
    with pytest.raises(NotImplementedError) as err:
        op(pos, d["mu"], d["quad"], cell, d["batch"], *tables)[0].sum().backward()
    assert "alchemiops::_rotate_multipoles: gradients w.r.t. cell are not provided by the local-frame rotation" in str(err.value)
