"""Dispersion PME on the device against its float64 restatement (tests/pme_dispersion_reference.py) on the same mesh and order.

fp64: 1e-10 of the largest |value| of each output.  fp32: per output 4 x the error of the restatement's own float32 mode against its float64
mode on the same inputs.  Small systems spread with atomic adds: two device results are compared at 1e-12 relative, never by equality.
Shapes: the 37 atoms, cell and meshes of tests/test_pme_dipole_gpu.py (four atoms outside the cell, stencils across every face, (12, 10, 16)
takes the in-LDS transforms and (14, 12, 16) the plans), atom 11 with c = 0, a batch of 7 + 1 + 12 atoms, atom counts around a gather block."""
import functools

import numpy as np
import pytest
import torch

from nvalchemiops.interactions.vdw import ewald_dispersion_real_space, pme_dispersion_correction, pme_dispersion_reciprocal_space as recip
from tests import dispersion_ewald_reference as X
from tests import pme_dispersion_reference as R
from tests.test_pme_dipole_gpu import ALPHA, CASES, CELL, DEV, MESH, _close, _np, _system, _t

pytestmark = pytest.mark.gpu
NAMES = ("energies", "forces", "coefficient_grads", "virial")
ALL = dict(compute_forces=True, compute_coefficient_gradients=True, compute_virial=True)
GATHER_BLOCK = 256 // 8  # atoms per block of mi_pme_dispersion_gather: 256 threads, 8 lanes per atom
WEIGHTS = np.random.default_rng(9).normal(size=37)
F64, F32 = torch.float64, torch.float32


@functools.lru_cache(maxsize=None)
def _atoms(n=37):
    """(positions, coefficients) of the first n atoms; beyond 37 the fixture shifted along the cell diagonal."""
    pos = np.concatenate([_system()[0] + 0.37 * k * CELL.sum(0) for k in range(-(-n // 37))])[:n]
    c = np.random.default_rng(5).uniform(0.5, 1.5, n)
    c[11:12] = 0.0
    return pos, c


@functools.lru_cache(maxsize=None)
def _reference(order, dims, dtype=F64, n=37, weighted=False):
    pos, c = (torch.tensor(a, dtype=F64) for a in _atoms(n))
    return R.evaluate(pos, c, torch.tensor(CELL), ALPHA, dims, order, dtype=dtype, weights=torch.tensor(WEIGHTS) if weighted else None)


def _inputs(dtype=F64, n=37):
    pos, c = _atoms(n)
    return _t(pos, dtype), _t(c, dtype), _t(CELL, dtype).reshape(1, 3, 3)


def _bar(name, order, dims, dtype, weighted=False):
    if dtype == F64:
        return 1e-10
    ref, ref32 = _reference(order, dims, weighted=weighted), _reference(order, dims, F32, weighted=weighted)
    return 4.0 * np.abs(ref32[name] - ref[name]).max() / np.abs(ref[name]).max()


@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("order,dims", CASES)
def test_parity(order, dims, dtype):
    ref = _reference(order, dims)
    out = recip(*_inputs(dtype), ALPHA, mesh_dimensions=dims, spline_order=order, **ALL)
    assert len(out) == 4 and all(o.dtype == dtype for o in out)
    for name, o in zip(NAMES, out):
        _close(o, ref[name], f"order {order} mesh {dims} {dtype} {name}", _bar(name, order, dims, dtype))
    assert float(out[0][11]) == 0.0 and not out[1][11].any()  # c = 0: exact zeros
    assert np.array_equal(_np(out[3][0]), _np(out[3][0]).T)


def test_batch_with_three_cells_and_alphas():
    pos, c = _atoms(20)
    bi = np.repeat([0, 1, 2], [7, 1, 12])
    cells = np.stack([CELL, 1.1 * CELL[[1, 2, 0]][:, [1, 2, 0]], 0.9 * CELL])
    pos = np.einsum("na,nab->nb", np.linalg.solve(CELL.T, pos.T).T, cells[bi])
    alpha = np.array([0.35, 0.3, 0.42])
    out = recip(_t(pos), _t(c), _t(cells), _t(alpha), mesh_dimensions=MESH, spline_order=5, batch_idx=_t(bi, torch.int32), **ALL)
    for s in range(3):
        own = bi == s
        ref = R.evaluate(torch.tensor(pos[own]), torch.tensor(c[own]), torch.tensor(cells[s]), alpha[s], MESH, 5)
        for name, o in zip(NAMES, out):
            _close(o[s:s + 1] if name == "virial" else o[torch.as_tensor(own, device=DEV)], ref[name], f"system {s} {name}", 1e-10)


@pytest.mark.parametrize("n", [1, GATHER_BLOCK - 1, GATHER_BLOCK, GATHER_BLOCK + 1, 2 * GATHER_BLOCK + 3])
def test_gather_block_ladder(n):
    ref = _reference(5, MESH, n=n)
    for name, o in zip(NAMES, recip(*_inputs(n=n), ALPHA, mesh_dimensions=MESH, spline_order=5, **ALL)):
        _close(o, ref[name], f"{n} atoms {name}", 1e-10)


def test_each_flag_alone_is_its_slot_of_the_full_call():
    args = _inputs()
    full = recip(*args, ALPHA, mesh_dimensions=MESH, **ALL)
    e = recip(*args, ALPHA, mesh_dimensions=MESH)
    assert isinstance(e, torch.Tensor)
    _close(e, full[0], "energies alone", 1e-12)
    for slot, flag in enumerate(ALL, start=1):
        out = recip(*args, ALPHA, mesh_dimensions=MESH, **{flag: True})
        assert len(out) == 2
        _close(out[0], full[0], f"{flag}: energies", 1e-12)
        _close(out[1], full[slot], f"{flag}: {NAMES[slot]}", 1e-12)


@pytest.mark.parametrize("dtype", [F64, F32])
def test_adjoint_against_the_restatements_autograd(dtype):
    pos, c, cell = _inputs(dtype)
    pos.requires_grad_(True), c.requires_grad_(True)
    (recip(pos, c, cell, ALPHA, mesh_dimensions=MESH, spline_order=5) * _t(WEIGHTS, dtype)).sum().backward()
    ref = _reference(5, MESH, weighted=True)
    assert pos.grad.dtype == dtype and c.grad.dtype == dtype
    _close(-pos.grad, ref["forces"], f"{dtype} dL/dr", _bar("forces", 5, MESH, dtype, True))
    _close(c.grad, ref["coefficient_grads"], f"{dtype} dL/dc", _bar("coefficient_grads", 5, MESH, dtype, True))
    e = recip(pos.detach(), c.detach(), cell.clone().requires_grad_(True), ALPHA, mesh_dimensions=MESH)
    with pytest.raises(NotImplementedError, match="cell"):
        e.sum().backward()


def test_correction_is_the_real_half_plus_the_mesh_half():
    pos, c, cell = _inputs()
    i, j, S = X.entries_within(pos.cpu(), cell.cpu(), 6.0)
    order = torch.argsort(i, stable=True)
    ptr = torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(torch.bincount(i, minlength=37), 0)])
    lists = dict(neighbor_list=torch.stack([i, j])[:, order].int().to(DEV), neighbor_ptr=ptr.int().to(DEV), neighbor_shifts=S[order].int().to(DEV),
                 counted_cutoff=5.0, counted_taper=4.5)
    got = pme_dispersion_correction(pos, c, cell, ALPHA, mesh_dimensions=MESH, spline_order=5, **lists, **ALL)
    halves = zip(ewald_dispersion_real_space(pos, c, cell, ALPHA, **lists, **ALL), recip(pos, c, cell, ALPHA, mesh_dimensions=MESH, spline_order=5, **ALL))
    for name, o, (a, b) in zip(NAMES, got, halves):
        _close(o, a + b, f"correction {name}", 1e-12)


def test_compiles_into_one_graph_and_matches_eager():
    pos, c, cell = _inputs()

    def fn(p, q):
        e, f, v = recip(p, q, cell, ALPHA, mesh_dimensions=MESH, spline_order=5, compute_forces=True, compute_virial=True)
        return e * 2.0, f, v

    torch._dynamo.reset()
    torch._dynamo.utils.counters.clear()
    got = torch.compile(fn, fullgraph=True, backend="aot_eager")(pos, c)
    assert torch._dynamo.utils.counters["stats"]["unique_graphs"] == 1
    for name, a, b in zip(("energies", "forces", "virial"), got, fn(pos, c)):
        _close(a, b, f"compiled vs eager {name}", 1e-12)
