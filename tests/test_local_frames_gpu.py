"""`mi_frame_rotate`, `mi_frame_adjoint`, `mi_frame_gather` and their public functions `rotate_multipoles` and `multipole_frame_forces` on the
device, against the float64 autograd reference tests/local_frames_reference.py (itself pinned in tests/test_local_frames_reference_cpu.py).

Cases (`_case`): every kind alone on the smallest molecule that holds it (1 atom NONE, 2 atoms Z_ONLY on either side of the 0.866 switch, a
3-atom water, a 4-atom ammonia, a 5-atom z-bisect centre, a chiral centre and its mirror image) and all of them joined; 255 - 513 atoms of
randomly rotated waters with NONE filler (one below, at and one above one and two blocks of 256 threads, the block size of all three kernels);
a hub named as z atom by 200 others beside an atom named by no one and an atom that sits in all three slots of different atoms; the joined
molecules wrapped into a triclinic cell (molecules straddle faces) and a batch of three systems with different cells and sizes.

Bars are those of tests/test_cluster_multipole_gpu.py::_close: 1e-11 of the largest reference component for float64, 1e-6 for float32 against
the reference evaluated at the float32-rounded inputs.  Geometries keep bond lengths in [0.9, 1.6] and angles between frame vectors in
[40, 140] degrees (checked on the CPU, with the reference's own sensitivity to the float32 rounding: at most 1e-7).

Measured on the MI355X.  float64: dipoles <= 5.1e-16, quadrupoles <= 7.3e-16, dL/dr (backward and torque forces) <= 1.4e-15, local gradients
<= 9.4e-16, virial term 7.8e-16 - 1.6e-15, wrapped against unwrapped <= 2.9e-15, end to end 3.7e-16 - 1.8e-15; float32: <= 5.0e-8 for every output
(virial 2.8e-8 - 3.2e-8); determinism, views and torch.compile: bit-identical.  DESIGN 3.31 has the table."""
import functools

import numpy as np
import pytest
import torch

from tests import cluster_multipole_reference as CR
from tests import local_frames_reference as LR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64
MOLECULES = ("none", "z_only", "z_only_y", "water", "ammonia", "z_bisect", "chiral", "mirror")
SIZES = (255, 256, 257, 511, 512, 513)
PLAIN = MOLECULES + ("mixed", "hub") + tuple(f"n{n}" for n in SIZES)
PERIODIC = ("triclinic", "batch")
TRICLINIC = [[9.0, 0.0, 0.0], [1.5, 8.0, 0.0], [-1.0, 2.0, 7.5]]
GRADS = ("positions_grad", "local_dipole_grads", "local_quadrupole_grads")


def _np(x):
    return x.detach().cpu().numpy().astype(np.float64)


def _close(got, ref, what, rel):
    got = _np(got) if isinstance(got, torch.Tensor) else got
    ref = _np(ref) if isinstance(ref, torch.Tensor) else ref
    assert got.shape == ref.shape, f"{what}: shape {got.shape} vs {ref.shape}"
    scale = max(np.abs(ref).max(), 1e-30) if ref.size else 1.0
    err = np.abs(got - ref).max() if ref.size else 0.0
    print(f"{what:64s} rel err {err / scale:.2e} (bar {rel:.0e})")
    assert err <= rel * scale + 1e-14, f"{what}: max err {err:.3e} > {rel * scale:.3e}"


def _bar(dtype):
    return 1e-11 if dtype == torch.float64 else 1e-6


def _api():
    from nvalchemiops.interactions.electrostatics import LocalFrames, multipole_frame_forces, rotate_multipoles

    return LocalFrames, rotate_multipoles, multipole_frame_forces


def _wrap(pos, cell):
    frac = pos @ torch.linalg.inv(cell)
    return (frac - torch.floor(frac)) @ cell, torch.floor(frac)


def _hub():
    """Atom 0 is named as z atom by atoms 1 .. 200 (Z_ONLY, on either side of the switch but 0.06 away from it), atom 201 is named by no one,
    and atom 203 of the chiral centre appended at 202 sits in a z, an x and a y slot of three different atoms."""
    gen = torch.Generator().manual_seed(91)
    dirs = []
    while len(dirs) < 200:
        v = torch.randn(3, dtype=F64, generator=gen)
        v = v / v.norm()
        if abs(abs(float(v[0])) - LR.Z_ONLY_SWITCH) > 0.06:
            dirs.append(v * (0.95 + 0.5 * float(torch.rand(1, generator=gen))))
    pos = torch.cat([torch.zeros((1, 3), dtype=F64), torch.stack(dirs), torch.tensor([[5.0, 5.0, 5.0]], dtype=F64)])
    atoms = torch.full((202, 3), -1, dtype=torch.int32)
    atoms[1:201, 0] = 0
    kinds = torch.zeros(202, dtype=torch.int32)
    kinds[1:201] = LR.Z_ONLY
    return LR.join([(pos, atoms, kinds), LR.molecule("chiral")])[:3]


@functools.lru_cache(maxsize=None)
def _case(name):
    """dict(pos, atoms, kinds, cell | None, batch | None, mu, quad, w_mu, w_q) of float64 / int32 CPU tensors."""
    cell = batch = None
    if name in MOLECULES:
        pos, atoms, kinds = LR.molecule(name)
    elif name == "mixed":
        pos, atoms, kinds, _ = LR.join([LR.molecule(m) for m in MOLECULES])
    elif name == "hub":
        pos, atoms, kinds = _hub()
    elif name.startswith("n"):
        pos, atoms, kinds, _ = LR.waters(int(name[1:]), seed=int(name[1:]))
        assert pos.shape[0] == int(name[1:]) and int((kinds == LR.BISECTOR).sum()) == int(name[1:]) // 3
    elif name in ("triclinic", "unwrapped"):
        pos, atoms, kinds, mol = LR.join([LR.molecule(m) for m in MOLECULES])
        cell = torch.tensor(TRICLINIC, dtype=F64)
        wrapped, images = _wrap(pos, cell)
        assert any(len({tuple(r) for r in images[mol == m].tolist()}) > 1 for m in range(int(mol.max()) + 1)), "no molecule straddles a face"
        if name == "triclinic":
            pos = wrapped
    elif name == "batch":
        cells = [torch.tensor(TRICLINIC, dtype=F64), torch.eye(3, dtype=F64) * 12.5,
                 torch.tensor([[7.0, 0.5, 0.0], [0.0, 8.5, -0.5], [1.0, 0.0, 9.5]], dtype=F64)]
        parts = [LR.join([LR.molecule(m) for m in MOLECULES])[:3], LR.waters(10, seed=3)[:3], LR.molecule("ammonia")]
        parts = [(_wrap(p, c)[0], a, k) for (p, a, k), c in zip(parts, cells)]
        pos, atoms, kinds, batch = LR.join(parts)
        cell, batch = torch.stack(cells), batch.to(torch.int32)
    else:
        raise KeyError(name)
    n = pos.shape[0]
    mu, quad = LR.local_multipoles(n, 100 + n)
    gen = torch.Generator().manual_seed(200 + n)
    return dict(name=name, n=n, pos=pos, atoms=atoms, kinds=kinds, cell=cell, batch=batch, mu=mu, quad=quad,
                w_mu=torch.randn((n, 3), dtype=F64, generator=gen), w_q=torch.randn((n, 3, 3), dtype=F64, generator=gen))


def _rounded(c, dtype):
    return {k: (c[k].to(dtype).to(F64) if c[k] is not None else None) for k in ("pos", "mu", "quad", "w_mu", "w_q", "cell")}


@functools.lru_cache(maxsize=None)
def _reference(name, dtype):
    """The float64 reference at the inputs rounded to `dtype`, computed once on the CPU and shared."""
    c = _case(name)
    r = _rounded(c, dtype)
    return LR.evaluate(r["pos"], r["mu"], r["quad"], c["atoms"], c["kinds"], r["w_mu"], r["w_q"], cell=r["cell"], batch_idx=c["batch"])


def _device_inputs(c, dtype):
    d = {k: (c[k].to(DEV, dtype) if c[k] is not None else None) for k in ("pos", "mu", "quad", "w_mu", "w_q", "cell")}
    d["batch"] = None if c["batch"] is None else c["batch"].to(DEV)
    d["frames"] = _api()[0](c["atoms"].to(DEV), c["kinds"].to(DEV), batch_idx=d["batch"])
    return d


def _check_all(name, dtype):
    """Rotation, `backward()` through it with random output weights, and the explicit path with the same g_mu, g_Q, against the reference."""
    _, rotate, frame_forces = _api()
    c, ref, rel = _case(name), _reference(name, dtype), _bar(dtype)
    d = _device_inputs(c, dtype)
    tag = f"{name} {str(dtype)[6:]}"
    mu, quad = rotate(d["pos"], d["mu"], d["quad"], d["frames"], d["cell"], batch_idx=d["batch"])
    assert mu.dtype == dtype and quad.dtype == dtype and not mu.requires_grad
    _close(mu, ref["dipoles"], f"{tag} dipoles", rel)
    _close(quad, ref["quadrupoles"], f"{tag} quadrupoles", rel)
    assert torch.equal(quad, quad.transpose(-1, -2))
    leaves = [d[k].clone().requires_grad_(True) for k in ("pos", "mu", "quad")]
    mu_g, quad_g = rotate(*leaves, d["frames"], d["cell"], batch_idx=d["batch"])
    assert torch.equal(mu_g.detach(), mu) and torch.equal(quad_g.detach(), quad)
    ((d["w_mu"] * mu_g).sum() + (d["w_q"] * quad_g).sum()).backward()
    for key, leaf in zip(GRADS, leaves):
        assert leaf.grad.dtype == dtype
        _close(leaf.grad, ref[key], f"{tag} backward {key}", rel)
    periodic = d["cell"] is not None
    out = frame_forces(d["pos"], d["mu"], d["quad"], d["frames"], d["w_mu"], d["w_q"], d["cell"], batch_idx=d["batch"],
                       compute_local_gradients=True, compute_virial=periodic)
    assert all(o.dtype == dtype for o in out) and len(out) == (4 if periodic else 3)
    _close(out[0], -ref["positions_grad"], f"{tag} torque forces", rel)
    _close(out[1], ref["local_dipole_grads"], f"{tag} explicit local_dipole_grads", rel)
    _close(out[2], ref["local_quadrupole_grads"], f"{tag} explicit local_quadrupole_grads", rel)
    if periodic:
        _close(out[3], ref["virial"], f"{tag} virial term", rel)
        for o in (frame_forces(d["pos"], d["mu"], d["quad"], d["frames"], d["w_mu"], d["w_q"], d["cell"], batch_idx=d["batch"]),
                  frame_forces(d["pos"], d["mu"], d["quad"], d["frames"], d["w_mu"], d["w_q"], d["cell"], batch_idx=d["batch"], compute_virial=True)[0]):
            assert torch.equal(o, out[0]), "the forces do not depend on what else is asked for"
    # the forces alone, and what a kind without frame atoms must give exactly
    assert torch.equal(frame_forces(d["pos"], d["mu"], d["quad"], d["frames"], d["w_mu"], d["w_q"], d["cell"], batch_idx=d["batch"]), out[0])
    none = (c["kinds"] == LR.NONE).to(DEV)
    if bool(none.any()):
        assert torch.equal(mu[none], d["mu"][none]), "NONE is R = I: the local dipole, bit for bit"
        unnamed = none.clone()
        unnamed[d["frames"].frame_atoms[d["frames"].frame_atoms >= 0].long()] = False
        assert float(out[0][unnamed].abs().max() if bool(unnamed.any()) else 0.0) == 0.0, "a NONE atom named by no one carries no torque force"
    return out


# ---- parity ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", PLAIN)
def test_rotation_adjoint_and_explicit_path_against_the_reference(name, dtype):
    _check_all(name, dtype)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", PERIODIC)
def test_periodic_cells_with_the_virial_term(name, dtype):
    """A triclinic cell with molecules straddling faces, and a batch of three systems with different cells and sizes: minimum-image frame
    vectors, and the virial term against the reference's strain derivative."""
    _check_all(name, dtype)


def test_wrapped_against_unwrapped_coordinates():
    _, rotate, frame_forces = _api()
    a, b = _device_inputs(_case("triclinic"), F64), _device_inputs(_case("unwrapped"), F64)
    assert float((a["pos"] - b["pos"]).abs().max()) > 5.0
    for x, y, what in zip(rotate(a["pos"], a["mu"], a["quad"], a["frames"], a["cell"]), rotate(b["pos"], b["mu"], b["quad"], b["frames"], b["cell"]),
                          ("dipoles", "quadrupoles")):
        _close(x, y, f"wrapped against unwrapped {what}", 1e-11)
    args = lambda d: (d["pos"], d["mu"], d["quad"], d["frames"], d["w_mu"], d["w_q"], d["cell"])  # noqa: E731
    for x, y, what in zip(frame_forces(*args(a), compute_local_gradients=True, compute_virial=True),
                          frame_forces(*args(b), compute_local_gradients=True, compute_virial=True),
                          ("forces", "local_dipole_grads", "local_quadrupole_grads", "virial")):
        _close(x, y, f"wrapped against unwrapped {what}", 1e-11)
    # without a cell the unwrapped molecules give the same rotation, the wrapped ones do not
    free = rotate(b["pos"], b["mu"], b["quad"], b["frames"])
    _close(free[0], rotate(b["pos"], b["mu"], b["quad"], b["frames"], b["cell"])[0], "cell=None on unwrapped molecules", 1e-11)
    assert float((rotate(a["pos"], a["mu"], a["quad"], a["frames"])[0] - free[0]).abs().max()) > 1e-3


def test_inverse_rows_of_the_hub_case():
    fr = _device_inputs(_case("hub"), F64)["frames"]
    ptr, slots = fr.inverse_ptr.tolist(), fr.inverse_slots.tolist()
    assert ptr[1] - ptr[0] == 200 and max(ptr[i + 1] - ptr[i] for i in range(1, fr.num_atoms)) <= 3, "one row far longer than any other"
    assert ptr[202] - ptr[201] == 0, "atom 201 is named by no one"
    assert sorted(code % 4 for code in slots[ptr[203]:ptr[204]]) == [1, 2, 3], "atom 203 sits in a z, an x and a y slot"
    assert len({code // 4 for code in slots[ptr[203]:ptr[204]]}) == 3


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------------
def _abi(c, dtype, dipoles=True, quadrupoles=True, local=True, virial=False, sign=1.0, out_dtype=F64):
    """One `mi_frame_rotate`, `mi_frame_adjoint`, `mi_frame_gather` call each into NaN-filled buffers: dict of every buffer."""
    import ctypes

    from nvalchemiops import _capi as C

    d = _device_inputs(c, dtype)
    fr, L, n = d["frames"], C.lib(), c["n"]
    nsys = 1 if d["batch"] is None else d["cell"].shape[0]
    nan = lambda *shape, dtype=F64: torch.full(shape, float("nan"), dtype=dtype, device=DEV)  # noqa: E731
    out = dict(dipoles=nan(n, 3, dtype=dtype), quadrupoles=nan(n, 3, 3, dtype=dtype), records=nan(n, 4, 3), local_dipole_grads=nan(n, 3),
               local_quadrupole_grads=nan(n, 3, 3), virial_rows=nan(n, 9), out=nan(n, 3, dtype=out_dtype), partial=nan(nsys, L.mi_frame_blocks(), 9))
    mu, quad = (d["mu"] if dipoles else None), (d["quad"] if quadrupoles else None)
    st = C.stream_of(d["pos"])
    head = (C.ptr(d["pos"]), C.ptr(mu), C.ptr(quad), C.ptr(fr.frame_atoms), C.ptr(fr.frame_kinds), C.ptr(d["cell"]), C.ptr(d["batch"]))
    C.check(L.mi_frame_rotate(*head, n, nsys, C.dtype_code(dtype), C.ptr(out["dipoles"]) if dipoles else None,
                              C.ptr(out["quadrupoles"]) if quadrupoles else None, st), "mi_frame_rotate")
    C.check(L.mi_frame_adjoint(*head, C.ptr(d["w_mu"]) if dipoles else None, C.ptr(d["w_q"]) if quadrupoles else None, n, nsys, C.dtype_code(dtype),
                               C.ptr(out["records"]), C.ptr(out["local_dipole_grads"]) if local and dipoles else None,
                               C.ptr(out["local_quadrupole_grads"]) if local and quadrupoles else None,
                               C.ptr(out["virial_rows"]) if virial else None, st), "mi_frame_adjoint")
    C.check(L.mi_frame_gather(C.ptr(out["records"]), C.ptr(fr.inverse_ptr), C.ptr(fr.inverse_slots), ctypes.c_longlong(fr.inverse_slots.shape[0]),
                              C.ptr(out["virial_rows"]) if virial else None, C.ptr(d["batch"]), n, nsys, C.dtype_code(out_dtype), C.cdouble(sign),
                              C.ptr(out["out"]), C.ptr(out["partial"]) if virial else None, st), "mi_frame_gather")
    return out


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_c_abi_writes_what_was_asked_for_and_nothing_else(dtype):
    from nvalchemiops import _capi as C

    assert C.lib().mi_frame_block_threads() == 256 and C.lib().mi_frame_blocks() == 64
    c, ref, rel = _case("batch"), _reference("batch", dtype), _bar(dtype)
    full = _abi(c, dtype, virial=True)
    assert not any(bool(torch.isnan(v).any()) for v in full.values()), "every word of every buffer is written"
    _close(full["dipoles"], ref["dipoles"], "abi dipoles", rel)
    _close(full["quadrupoles"], ref["quadrupoles"], "abi quadrupoles", rel)
    _close(full["out"], ref["positions_grad"], "abi gather, sign +1", 1e-11 if dtype == F64 else rel)
    _close(full["local_dipole_grads"], ref["local_dipole_grads"], "abi local_dipole_grads", rel)
    _close(full["local_quadrupole_grads"], ref["local_quadrupole_grads"], "abi local_quadrupole_grads", rel)
    _close(full["partial"].sum(1).reshape(-1, 3, 3), ref["virial"], "abi virial fold", rel)
    rec = full["records"]
    assert float((rec.sum(1)).abs().max()) <= 1e-12 * float(rec.abs().max()), "the four vectors of a record sum to zero"
    unused = (_device_inputs(c, dtype)["frames"].frame_atoms < 0)
    assert float(rec[:, 1:][unused].abs().max()) == 0.0, "a slot that names no atom holds exact zeros"
    bare = _abi(c, dtype, local=False, virial=False, sign=-1.0, out_dtype=dtype)
    for key in ("local_dipole_grads", "local_quadrupole_grads", "virial_rows", "partial"):
        assert bool(torch.isnan(bare[key]).all()), f"{key} was written without being asked for"
    assert torch.equal(bare["records"], rec)
    _close(bare["out"], -ref["positions_grad"], "abi gather, sign -1, positions dtype", rel)
    only_mu = _abi(c, dtype, quadrupoles=False)
    assert bool(torch.isnan(only_mu["quadrupoles"]).all()) and bool(torch.isnan(only_mu["local_quadrupole_grads"]).all())
    assert torch.equal(only_mu["dipoles"], full["dipoles"]) and torch.equal(only_mu["local_dipole_grads"], full["local_dipole_grads"])
    only_q = _abi(c, dtype, dipoles=False)
    assert bool(torch.isnan(only_q["dipoles"]).all()) and bool(torch.isnan(only_q["local_dipole_grads"]).all())
    assert torch.equal(only_q["quadrupoles"], full["quadrupoles"])
    _close(only_mu["out"] + only_q["out"], ref["positions_grad"], "abi dipole part + quadrupole part", 1e-11 if dtype == F64 else rel)


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------
def test_end_to_end_three_water_cluster_through_the_cluster_corrections():
    """rotate_multipoles -> coulomb_dipole_correction + coulomb_quadrupole_correction -> energies.sum().backward(), against the same pipeline
    in the float64 references; and the explicit path (the operators' forces plus multipole_frame_forces fed their dipole_grads and
    quadrupole_grads) against the same numbers."""
    from nvalchemiops.interactions.electrostatics import coulomb_dipole_correction, coulomb_quadrupole_correction

    LocalFrames, rotate, frame_forces = _api()
    gen = torch.Generator().manual_seed(17)
    parts = []
    for origin in ([0.0, 0.0, 0.0], [3.1, 0.4, -0.3], [0.5, 3.0, 1.2]):
        p, a, k = LR.water(gen)
        parts.append((p + torch.tensor(origin, dtype=F64), a, k))
    pos, atoms, kinds, _ = LR.join(parts)
    n = pos.shape[0]
    q = torch.tensor([-0.8, 0.4, 0.4] * 3, dtype=F64)
    mu_loc, quad_loc = LR.local_multipoles(n, 18)
    mu_loc, quad_loc = 0.3 * mu_loc, 0.2 * quad_loc
    entries = CR.all_pairs((n,))
    # the reference pipeline, float64 autograd on the CPU
    rp, rm, rq = (t.clone().requires_grad_(True) for t in (pos, mu_loc, quad_loc))
    mu_r, quad_r = LR.rotate(rp, rm, rq, atoms, kinds)
    e_ref = CR.dipole_energies(rp, q, mu_r, entries) + CR.quadrupole_energies(rp, q, mu_r, quad_r, entries)
    e_ref.sum().backward()
    # the package, autograd path
    i, j, _ = entries
    nl = torch.stack([i, j]).to(torch.int32).to(DEV)
    ptr = torch.zeros(n + 1, dtype=torch.int32, device=DEV)
    ptr[1:] = torch.cumsum(torch.bincount(i, minlength=n), 0).to(DEV)
    lists = dict(neighbor_list=nl, neighbor_ptr=ptr)
    fr = LocalFrames(atoms.to(DEV), kinds.to(DEV))
    dp, dm, dq = (t.to(DEV).clone().requires_grad_(True) for t in (pos, mu_loc, quad_loc))
    qd = q.to(DEV)
    mu, quad = rotate(dp, dm, dq, fr)
    e = coulomb_dipole_correction(dp, qd, mu, **lists) + coulomb_quadrupole_correction(dp, qd, mu, quad, **lists)
    e.sum().backward()
    _close(e, e_ref, "end to end energies", 1e-11)
    _close(dp.grad, rp.grad, "end to end dE/dpositions", 1e-11)
    _close(dm.grad, rm.grad, "end to end dE/dlocal_dipoles", 1e-11)
    _close(dq.grad, rq.grad, "end to end dE/dlocal_quadrupoles", 1e-11)
    # the explicit path
    with torch.no_grad():
        mu, quad = rotate(dp, dm, dq, fr)
        _, f1, g1 = coulomb_dipole_correction(dp, qd, mu, **lists, compute_forces=True, compute_dipole_gradients=True)
        _, f2, g2, G2 = coulomb_quadrupole_correction(dp, qd, mu, quad, **lists, compute_forces=True, compute_dipole_gradients=True,
                                                      compute_quadrupole_gradients=True)
        ft, lm, lq = frame_forces(dp, dm, dq, fr, g1 + g2, G2, compute_local_gradients=True)
    assert float(ft.abs().max()) > 1e-3 * float((f1 + f2).abs().max()), "the torque forces are not a detail of this cluster"
    _close(f1 + f2 + ft, -rp.grad, "end to end explicit forces", 1e-11)
    _close(lm, rm.grad, "end to end explicit dE/dlocal_dipoles", 1e-11)
    _close(lq, rq.grad, "end to end explicit dE/dlocal_quadrupoles", 1e-11)


# ---- determinism, optional inputs, layouts ----------------------------------------------------------------------------------------------------
def test_two_calls_and_a_side_stream_call_are_bit_identical():
    _, rotate, frame_forces = _api()
    d = _device_inputs(_case("batch"), torch.float32)

    def run():
        mu, quad = rotate(d["pos"], d["mu"], d["quad"], d["frames"], d["cell"], batch_idx=d["batch"])
        f, _, _, vir = frame_forces(d["pos"], d["mu"], d["quad"], d["frames"], d["w_mu"], d["w_q"], d["cell"], batch_idx=d["batch"],
                                    compute_local_gradients=True, compute_virial=True)
        return mu, quad, f, vir

    first, second = run(), run()
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        third = run()
    side.synchronize()
    for a, b, c, what in zip(first, second, third, ("dipoles", "quadrupoles", "forces", "virial")):
        assert torch.equal(a, b) and torch.equal(a, c), what
        assert float(a.abs().max()) > 0


def test_optional_inputs_no_atoms_and_views_give_the_bits_of_the_plain_call():
    LocalFrames, rotate, frame_forces = _api()
    c = _case("mixed")
    d = _device_inputs(c, F64)
    n, fr = c["n"], d["frames"]
    mu, quad = rotate(d["pos"], d["mu"], d["quad"], fr)
    f, lm, lq = frame_forces(d["pos"], d["mu"], d["quad"], fr, d["w_mu"], d["w_q"], compute_local_gradients=True)
    # one multipole order at a time
    m_only, none = rotate(d["pos"], d["mu"], None, fr)
    assert none is None and torch.equal(m_only, mu)
    none, q_only = rotate(d["pos"], None, d["quad"], fr)
    assert none is None and torch.equal(q_only, quad)
    assert rotate(d["pos"], None, None, fr) == (None, None)
    f_m, lm_m, none = frame_forces(d["pos"], d["mu"], None, fr, d["w_mu"], None, compute_local_gradients=True)
    assert none is None and torch.equal(lm_m, lm)
    f_q, none, lq_q = frame_forces(d["pos"], None, d["quad"], fr, None, d["w_q"], compute_local_gradients=True)
    assert none is None and torch.equal(lq_q, lq)
    _close(f_m + f_q, f, "dipole part + quadrupole part of the torque forces", 1e-11)
    assert float(frame_forces(d["pos"], None, None, fr, None, None).abs().max()) == 0.0
    # backward with one of the two outputs unused
    leaves = [d[k].clone().requires_grad_(True) for k in ("pos", "mu", "quad")]
    (d["w_mu"] * rotate(*leaves, fr)[0]).sum().backward()
    _close(leaves[0].grad, -f_m, "backward through the dipoles alone", 1e-11)
    assert leaves[2].grad is None or float(leaves[2].grad.abs().max()) == 0.0
    # no atoms
    empty = LocalFrames(torch.zeros((0, 3), dtype=torch.int32, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV))
    z = lambda *s: torch.zeros(s, dtype=F64, device=DEV)  # noqa: E731
    m0, q0 = rotate(z(0, 3), z(0, 3), z(0, 3, 3), empty)
    assert tuple(m0.shape) == (0, 3) and tuple(q0.shape) == (0, 3, 3)
    p0 = z(0, 3).requires_grad_(True)
    rotate(p0, z(0, 3), z(0, 3, 3), empty)[0].sum().backward()
    f0, vir0 = frame_forces(z(0, 3), z(0, 3), z(0, 3, 3), empty, z(0, 3), z(0, 3, 3), torch.eye(3, dtype=F64, device=DEV) * 9.0, compute_virial=True)
    assert tuple(f0.shape) == (0, 3) and tuple(vir0.shape) == (1, 3, 3) and float(vir0.abs().max()) == 0.0
    # non-contiguous and offset views
    def strided(t):
        wide = torch.full((n + 3,) + tuple(2 * s for s in t.shape[1:]), 7.5, dtype=t.dtype, device=DEV)
        view = wide[2:n + 2, ::2] if t.dim() == 2 else wide[2:n + 2, ::2, ::2]
        view.copy_(t)
        assert not view.is_contiguous() and view.storage_offset() > 0
        return view

    v = {k: strided(d[k]) for k in ("pos", "mu", "quad", "w_mu", "w_q")}
    mu_v, quad_v = rotate(v["pos"], v["mu"], v["quad"], fr)
    assert torch.equal(mu_v, mu) and torch.equal(quad_v, quad)
    for a, b in zip(frame_forces(v["pos"], v["mu"], v["quad"], fr, v["w_mu"], v["w_q"], compute_local_gradients=True), (f, lm, lq)):
        assert torch.equal(a, b)
    leaves = [v[k].clone(memory_format=torch.preserve_format).requires_grad_(True) for k in ("pos", "mu", "quad")]
    (v["w_mu"] * rotate(*leaves, fr)[0]).sum().backward()
    assert torch.equal(leaves[0].grad, -f_m)


def test_refusals_of_the_autograd_path():
    _, rotate, _ = _api()
    d = _device_inputs(_case("triclinic"), F64)
    pos = d["pos"].clone().requires_grad_(True)
    cell = d["cell"].clone().requires_grad_(True)
    mu, _ = rotate(pos, d["mu"], d["quad"], d["frames"], cell)
    with pytest.raises(NotImplementedError, match="gradients w.r.t. cell are not provided by the local-frame rotation"):
        mu.sum().backward()
    pos = d["pos"].clone().requires_grad_(True)
    mu, _ = rotate(pos, d["mu"], d["quad"], d["frames"], d["cell"])
    (g,) = torch.autograd.grad(mu.pow(2).sum(), pos, create_graph=True)
    with pytest.raises(NotImplementedError, match="second derivatives"):
        g.sum().backward()


def test_compile_fullgraph_rotate_into_a_quadrupole_correction_and_backward():
    """Under torch.compile the rotation goes through `alchemiops::_rotate_multipoles`, forward and backward: the bits of eager."""
    from nvalchemiops.interactions.electrostatics import coulomb_quadrupole_correction

    LocalFrames, rotate, _ = _api()
    pos, atoms, kinds, _ = LR.waters(12, seed=5, spacing=3.0)
    n = pos.shape[0]
    i, j, _ = CR.all_pairs((n,))
    nl = torch.stack([i, j]).to(torch.int32).to(DEV)
    ptr = torch.zeros(n + 1, dtype=torch.int32, device=DEV)
    ptr[1:] = torch.cumsum(torch.bincount(i, minlength=n), 0).to(DEV)
    fr = LocalFrames(atoms.to(DEV), kinds.to(DEV))
    q = torch.tensor([-0.8, 0.4, 0.4] * (n // 3), dtype=F64, device=DEV)
    mu_loc, quad_loc = (t.to(DEV) for t in LR.local_multipoles(n, 6))

    def loss(p, m, t):
        mu, quad = rotate(p, m, t, fr)
        return coulomb_quadrupole_correction(p, q, mu, quad, neighbor_list=nl, neighbor_ptr=ptr).sum() * 2.0

    leaves = lambda: [t.clone().requires_grad_(True) for t in (pos.to(DEV), mu_loc, quad_loc)]  # noqa: E731
    x, y = leaves(), leaves()
    torch._dynamo.reset()
    compiled = torch.compile(loss, mode="default", fullgraph=True)(*x)
    compiled.backward()
    eager = loss(*y)
    eager.backward()
    assert torch.equal(compiled.detach(), eager.detach())
    for a, b in zip(x, y):
        assert torch.equal(a.grad, b.grad) and float(b.grad.abs().max()) > 0
