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
