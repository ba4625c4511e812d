"""The raw-pointer boundary, CPU half: every shape / dtype / layout mismatch that would let a kernel read or write out of bounds is refused
with a ValueError BEFORE the device check and BEFORE any call into the native library.

Every kernel is reached through `_capi.ptr(t)` = the bare `data_ptr()`; sizes travel as separate integers.  The checks that make the two
agree live in one place each -- `neighborlist/_engine.py::check_outputs` / `check_cache` (caller-owned outputs and cache tensors) and
`_capi.py::check_neighbor_data` (neighbour data, per-atom tensors, cells against N and the number of systems) -- and are host-side shape
reads.  None of these cases is ever run against a GPU: this file is the proof that they cannot launch.  The autouse fixture replaces
`nvalchemiops._capi.lib` by an object whose every attribute access raises `_Launched`; a case that reaches the library therefore fails with
that instead of the ValueError it must raise (CPU tensors would otherwise stop at `require_device`, which raises NativeLibraryError -- a
case seeing THAT has also failed: the shape check must come first)."""
import pytest
import torch

N, M, B = 5, 4, 2
I32, I64 = torch.int32, torch.int64


class _Launched(BaseException):
    """A call into the native library was attempted (BaseException: no `except Exception` of the package can swallow it)."""


class _NoLibrary:
    def __getattr__(self, name):
        raise _Launched(f"the native library was reached: {name}")


@pytest.fixture(autouse=True)
def launch_guard(monkeypatch):
    from nvalchemiops import _capi

    monkeypatch.setattr(_capi, "lib", lambda: _NoLibrary())
    with pytest.raises(_Launched):  # the guard itself is live for every case
        _capi.lib().mi_nl_neighbors
    yield


def _geometry(batch=False):
    pos = torch.rand(N, 3) * 4.0
    cell = (torch.eye(3) * 4.0).repeat(B, 1, 1) if batch else torch.eye(3) * 4.0
    pbc = torch.ones((B, 3) if batch else (3,), dtype=torch.bool)
    bi = torch.tensor([0, 0, 0, 1, 1], dtype=I32)
    return pos, cell, pbc, bi


def _outputs():
    return dict(neighbor_matrix=torch.full((N, M), -7, dtype=I32), neighbor_matrix_shifts=torch.full((N, M, 3), -7, dtype=I32),
                num_neighbors=torch.full((N,), -7, dtype=I32))


# (argument that is wrong, its replacement, the name the message must carry)
BAD_OUTPUTS = [
    ("shifts_other_row_width", dict(neighbor_matrix_shifts=torch.zeros((N, M + 1, 3), dtype=I32)), "neighbor_matrix_shifts"),
    ("shifts_narrower_rows", dict(neighbor_matrix_shifts=torch.zeros((N, M - 1, 3), dtype=I32)), "neighbor_matrix_shifts"),
    ("shifts_last_dim", dict(neighbor_matrix_shifts=torch.zeros((N, M, 2), dtype=I32)), "neighbor_matrix_shifts"),
    ("shifts_rows", dict(neighbor_matrix_shifts=torch.zeros((N - 1, M, 3), dtype=I32)), "neighbor_matrix_shifts"),
    ("counts_short", dict(num_neighbors=torch.zeros((N - 1,), dtype=I32)), "num_neighbors"),
    ("matrix_rows_short", dict(neighbor_matrix=torch.zeros((N - 1, M), dtype=I32)), "neighbor_matrix"),
    ("matrix_rows_long", dict(neighbor_matrix=torch.zeros((N + 1, M), dtype=I32)), "neighbor_matrix"),
    ("matrix_int64", dict(neighbor_matrix=torch.zeros((N, M), dtype=I64)), "neighbor_matrix"),
    ("shifts_int64", dict(neighbor_matrix_shifts=torch.zeros((N, M, 3), dtype=I64)), "neighbor_matrix_shifts"),
    ("counts_int64", dict(num_neighbors=torch.zeros((N,), dtype=I64)), "num_neighbors"),
    ("matrix_column_slice", dict(neighbor_matrix=torch.zeros((N, M + 2), dtype=I32)[:, :M]), "neighbor_matrix"),
    ("shifts_column_slice", dict(neighbor_matrix_shifts=torch.zeros((N, M + 2, 3), dtype=I32)[:, :M]), "neighbor_matrix_shifts"),
    ("counts_strided", dict(num_neighbors=torch.zeros((2 * N,), dtype=I32)[::2]), "num_neighbors"),
]


def _cache(batch=False, ncell=8):
    z = lambda *s: torch.zeros(s, dtype=I32)  # noqa: E731
    lead = (B, 3) if batch else (3,)
    return dict(cells_per_dimension=z(*lead), neighbor_search_radius=z(*lead), atom_periodic_shifts=z(N, 3), atom_to_cell_mapping=z(N, 3),
                atoms_per_cell_count=z(ncell), cell_atom_start_indices=z(ncell), cell_atom_list=z(N))


def _search_entry_points():
    """name -> callable(outputs dict): every entry point that hands caller-owned outputs to the fused search."""
    from nvalchemiops.neighborlist import (batch_cell_list, batch_naive_neighbor_list, batch_query_cell_list, cell_list, naive_neighbor_list,
                                           neighbor_list, query_cell_list)

    pos, cell, pbc, bi = _geometry()
    _, bcell, bpbc, _ = _geometry(batch=True)
    c1, cb = tuple(_cache().values()), tuple(_cache(batch=True).values())
    return {
        "cell_list": lambda o: cell_list(pos, 2.0, cell, pbc, **o),
        "cell_list_coo": lambda o: cell_list(pos, 2.0, cell, pbc, return_neighbor_list=True, **o),
        "batch_cell_list": lambda o: batch_cell_list(pos, 2.0, bcell, bpbc, bi, **o),
        "query_cell_list": lambda o: query_cell_list(pos, 2.0, cell, pbc, *c1, o["neighbor_matrix"], o["neighbor_matrix_shifts"], o["num_neighbors"]),
        "batch_query_cell_list": lambda o: batch_query_cell_list(pos, bcell, bpbc, 2.0, bi, *cb, o["neighbor_matrix"], o["neighbor_matrix_shifts"],
                                                                 o["num_neighbors"]),
        "naive_neighbor_list": lambda o: naive_neighbor_list(pos, 2.0, cell=cell, pbc=pbc, **o),
        "batch_naive_neighbor_list": lambda o: batch_naive_neighbor_list(pos, 2.0, batch_idx=bi, cell=bcell, pbc=bpbc, **o),
        "neighbor_list_cell_list": lambda o: neighbor_list(pos, 2.0, cell=cell, pbc=pbc, method="cell_list", **o),
        "op_neighbor_search": lambda o: torch.ops.nvalchemiops.neighbor_search(pos, cell[None], pbc[None], None, 2.0, 0, N, o["neighbor_matrix"],
                                                                               o["neighbor_matrix_shifts"], o["num_neighbors"], None),
        "op_query_cell_list": lambda o: torch.ops.nvalchemiops.query_cell_list(pos, 2.0, cell, pbc, *c1, o["neighbor_matrix"],
                                                                               o["neighbor_matrix_shifts"], o["num_neighbors"], False),
    }


SEARCHES = ["cell_list", "cell_list_coo", "batch_cell_list", "query_cell_list", "batch_query_cell_list", "naive_neighbor_list",
            "batch_naive_neighbor_list", "neighbor_list_cell_list", "op_neighbor_search", "op_query_cell_list"]


@pytest.mark.parametrize("entry", SEARCHES)
def test_caller_owned_outputs_are_checked_before_any_launch(entry):
    call = _search_entry_points()[entry]
    for what, bad, name in BAD_OUTPUTS:
        out = _outputs()
        out.update(bad)
        with pytest.raises(ValueError, match=name):
            call(out)
        for k, t in out.items():  # nothing was written either: the sentinel / zeros the case put there are still in place
            assert bool((t == (-7 if k not in bad else 0)).all()), (entry, what, k)


@pytest.mark.parametrize("entry", ["naive_neighbor_list_dual_cutoff", "batch_naive_neighbor_list_dual_cutoff"])
def test_dual_cutoff_outputs_follow_the_same_rule(entry):
    """The dual-cutoff entry points had this check first; it is now `_engine.check_outputs`, for both lists."""
    from nvalchemiops import neighborlist as NL

    pos, cell, pbc, bi = _geometry(batch="batch" in entry)
    head = dict(batch_idx=bi) if "batch" in entry else {}
    for which in ("1", "2"):
        for what, bad, name in BAD_OUTPUTS:
            outs = {f"{k}{w}": v for w in ("1", "2") for k, v in _outputs().items()}
            outs.update({f"{k}{which}": v for k, v in bad.items()})
            with pytest.raises(ValueError, match=name + which):
                getattr(NL, entry)(pos, 1.5, 2.0, pbc=pbc, cell=cell, **head, **outs)


def test_outputs_that_do_not_agree_with_each_other_only():
    """Two of the three given, the matrix left to the entry point: the others must fit the width it will allocate (max_neighbors)."""
    from nvalchemiops.neighborlist import cell_list, naive_neighbor_list

    pos, cell, pbc, _ = _geometry()
    for fn, kw in ((cell_list, dict(cell=cell, pbc=pbc)), (naive_neighbor_list, dict(cell=cell, pbc=pbc))):
        with pytest.raises(ValueError, match="neighbor_matrix_shifts"):
            fn(pos, 2.0, max_neighbors=M, neighbor_matrix_shifts=torch.zeros((N, M + 1, 3), dtype=I32), **kw)
        with pytest.raises(ValueError, match="num_neighbors"):
            fn(pos, 2.0, max_neighbors=M, num_neighbors=torch.zeros((N - 1,), dtype=I32), **kw)


BAD_CACHE = [
    ("cells_per_dimension", lambda batch: torch.zeros((2,), dtype=I32)),
    ("cells_per_dimension", lambda batch: torch.zeros((B, 3) if batch else (3,), dtype=I64)),
    ("atom_periodic_shifts", lambda batch: torch.zeros((N - 1, 3), dtype=I32)),
    ("atom_periodic_shifts", lambda batch: torch.zeros((N, 2), dtype=I32)),
    ("atom_to_cell_mapping", lambda batch: torch.zeros((N - 1, 3), dtype=I32)),
    ("atom_to_cell_mapping", lambda batch: torch.zeros((N, 6), dtype=I32)[:, :3]),
    ("atoms_per_cell_count", lambda batch: torch.zeros((0,), dtype=I32)),
    ("atoms_per_cell_count", lambda batch: torch.zeros((16,), dtype=I32)[::2]),
    ("cell_atom_start_indices", lambda batch: torch.zeros((7,), dtype=I32)),  # shorter than the capacity atoms_per_cell_count announces (8)
    ("cell_atom_list", lambda batch: torch.zeros((N - 1,), dtype=I32)),
    ("cell_atom_list", lambda batch: torch.zeros((N,), dtype=I64)),
]


@pytest.mark.parametrize("entry", ["build_cell_list", "batch_build_cell_list", "op_build_cell_list", "cell_list", "batch_cell_list"])
def test_cache_tensors_are_checked_before_any_launch(entry):
    from nvalchemiops.neighborlist import batch_build_cell_list, batch_cell_list, build_cell_list, cell_list

    batch = "batch" in entry
    pos, cell, pbc, bi = _geometry(batch)
    for name, make in BAD_CACHE:
        cache = _cache(batch)
        cache[name] = make(batch)
        with pytest.raises(ValueError, match=name):
            if entry == "build_cell_list":
                build_cell_list(pos, 2.0, cell, pbc, *cache.values())
            elif entry == "op_build_cell_list":
                torch.ops.nvalchemiops.build_cell_list(pos, 2.0, cell, pbc, *cache.values())
            elif entry == "batch_build_cell_list":
                batch_build_cell_list(pos, 2.0, cell, pbc, bi, *cache.values())
            elif entry == "cell_list":
                cell_list(pos, 2.0, cell, pbc, max_neighbors=M, **cache)
            else:
                batch_cell_list(pos, 2.0, cell, pbc, bi, max_neighbors=M, **cache)
    if batch:  # a cache sized for one system handed to a batch of two
        cache = _cache(batch=False)
        with pytest.raises(ValueError, match="cells_per_dimension"):
            batch_build_cell_list(pos, 2.0, cell, pbc, bi, *cache.values())


def test_batch_idx_length_is_checked_by_the_batched_searches():
    from nvalchemiops.neighborlist import batch_build_cell_list, batch_cell_list, batch_naive_neighbor_list, batch_query_cell_list

    pos, cell, pbc, bi = _geometry(batch=True)
    short = bi[:-1]
    out, cache = _outputs(), tuple(_cache(batch=True).values())
    for call in (lambda: batch_cell_list(pos, 2.0, cell, pbc, short), lambda: batch_naive_neighbor_list(pos, 2.0, batch_idx=short, cell=cell, pbc=pbc),
                 lambda: batch_build_cell_list(pos, 2.0, cell, pbc, short, *cache),
                 lambda: batch_query_cell_list(pos, cell, pbc, 2.0, short, *cache, *out.values())):
        with pytest.raises(ValueError, match="batch_idx"):
            call()


# ---- inputs of the interaction kernels ---------------------------------------------------------------------------------------------------

def _tables(nz=6):
    r = torch.rand
    return dict(rcov=r(nz), r4r2=r(nz), c6ab=r(nz, nz, 5, 5), cn_ref=r(nz, nz, 5, 5))


def _neighbour_inputs(p=7):
    nm = torch.full((N, M), N, dtype=I32)
    nsh = torch.zeros((N, M, 3), dtype=I32)
    lst = torch.zeros((2, p), dtype=I32)
    ptr = torch.zeros((N + 1,), dtype=I32)
    lsh = torch.zeros((p, 3), dtype=I32)
    return nm, nsh, lst, ptr, lsh


def _d3_calls():
    from nvalchemiops.interactions.dispersion import dftd3, dftd3_atm, dftd3_zero, dftd3_zero_atm

    r0 = torch.rand(6, 6)
    return {"dftd3": lambda pos, z, **kw: dftd3(pos, z, a1=0.4, a2=4.0, s8=0.8, **kw),
            "dftd3_zero": lambda pos, z, **kw: dftd3_zero(pos, z, rs6=1.2, s8=0.8, **{"cutoff_radii": r0, **kw}),
            "dftd3_atm": lambda pos, z, **kw: dftd3_atm(pos, z, a1=0.4, a2=4.0, three_body_cutoff=6.0, **kw),
            "dftd3_zero_atm": lambda pos, z, **kw: dftd3_zero_atm(pos, z, three_body_cutoff=6.0, **{"cutoff_radii": r0, **kw})}


@pytest.mark.parametrize("entry", ["dftd3", "dftd3_zero", "dftd3_atm", "dftd3_zero_atm"])
def test_dftd3_inputs_are_checked_against_each_other(entry):
    call = _d3_calls()[entry]
    pos, cell, _, bi = _geometry()
    z = torch.ones(N, dtype=I32)
    nm, nsh, lst, ptr, lsh = _neighbour_inputs()
    t = _tables()
    cells = cell[None]
    cases = [
        ("neighbor_matrix", dict(d3_params=t, neighbor_matrix=nm[:-1])),
        ("neighbor_matrix", dict(d3_params=t, neighbor_matrix=torch.full((N + 1, M), N, dtype=I32))),
        ("neighbor_matrix_shifts", dict(d3_params=t, neighbor_matrix=nm, neighbor_matrix_shifts=torch.zeros((N, M + 1, 3), dtype=I32), cell=cells)),
        ("neighbor_matrix_shifts", dict(d3_params=t, neighbor_matrix=nm, neighbor_matrix_shifts=torch.zeros((N, M, 2), dtype=I32), cell=cells)),
        ("neighbor_matrix_shifts", dict(d3_params=t, neighbor_matrix=nm, neighbor_matrix_shifts=torch.zeros((N, M), dtype=I32), cell=cells)),
        ("unit_shifts", dict(d3_params=t, neighbor_list=lst, neighbor_ptr=ptr, unit_shifts=lsh[:-1], cell=cells)),
        ("unit_shifts", dict(d3_params=t, neighbor_list=lst, neighbor_ptr=ptr, unit_shifts=torch.zeros((7, 2), dtype=I32), cell=cells)),
        ("neighbor_ptr", dict(d3_params=t, neighbor_list=lst, neighbor_ptr=ptr[:-1])),
        ("neighbor_ptr", dict(d3_params=t, neighbor_list=lst, neighbor_ptr=torch.zeros((N + 2,), dtype=I32))),
        ("neighbor_list", dict(d3_params=t, neighbor_list=torch.zeros((7, 2), dtype=I32), neighbor_ptr=ptr)),
        ("batch_idx", dict(d3_params=t, neighbor_matrix=nm, batch_idx=bi[:-1])),
        ("cell must have shape", dict(d3_params=t, neighbor_matrix=nm, neighbor_matrix_shifts=nsh, batch_idx=bi, num_systems=3, cell=cells.repeat(2, 1, 1))),
        ("cell must have shape", dict(d3_params=t, neighbor_matrix=nm, neighbor_matrix_shifts=nsh, cell=cells.repeat(2, 1, 1))),
        ("cell must have shape", dict(d3_params=t, neighbor_matrix=nm, neighbor_matrix_shifts=nsh, cell=torch.zeros(3, 2))),
        ("r4r2", dict(d3_params={**t, "r4r2": torch.rand(5)}, neighbor_matrix=nm)),
        ("c6ab", dict(d3_params={**t, "c6ab": torch.rand(5, 6, 5, 5)}, neighbor_matrix=nm)),
        ("cn_ref", dict(d3_params={**t, "cn_ref": torch.rand(6, 5, 5, 5)}, neighbor_matrix=nm)),
        ("r4r2", dict(d3_params=t, r4r2=torch.rand(7), neighbor_matrix=nm)),
    ]
    if "zero" in entry:
        cases.append(("cutoff_radii", dict(d3_params=t, neighbor_matrix=nm, cutoff_radii=torch.rand(6, 5))))
    for match, kw in cases:
        with pytest.raises(ValueError, match=match):
            call(pos, z, **kw)
    with pytest.raises(ValueError, match="numbers"):
        call(pos, z[:-1], d3_params=t, neighbor_matrix=nm)
    with pytest.raises(ValueError, match="numbers"):
        call(pos, z[:-1], d3_params=t, neighbor_list=lst, neighbor_ptr=ptr)


def _ewald_calls():
    from nvalchemiops.interactions.electrostatics import ewald_real_space
    from nvalchemiops.interactions.electrostatics.ewald import ewald_real_space_with_virial

    return {"ewald_real_space": ewald_real_space, "ewald_real_space_forces": lambda *a, **k: ewald_real_space(*a, compute_forces=True, **k),
            "ewald_real_space_with_virial": ewald_real_space_with_virial}


@pytest.mark.parametrize("entry", ["ewald_real_space", "ewald_real_space_forces", "ewald_real_space_with_virial"])
def test_ewald_real_space_inputs_are_checked_against_each_other(entry):
    call = _ewald_calls()[entry]
    pos, cell, _, bi = _geometry()
    q = torch.rand(N)
    nm, nsh, lst, ptr, lsh = _neighbour_inputs()
    a = torch.tensor([0.3])
    cells = cell[None]
    cases = [
        ("neighbor_matrix", dict(neighbor_matrix=nm[:-1], neighbor_matrix_shifts=nsh[:-1])),
        ("neighbor_matrix_shifts", dict(neighbor_matrix=nm, neighbor_matrix_shifts=torch.zeros((N, M + 1, 3), dtype=I32))),
        ("neighbor_matrix_shifts", dict(neighbor_matrix=nm, neighbor_matrix_shifts=torch.zeros((N, M, 2), dtype=I32))),
        ("neighbor_shifts", dict(neighbor_list=lst, neighbor_ptr=ptr, neighbor_shifts=lsh[:-1])),
        ("neighbor_ptr", dict(neighbor_list=lst, neighbor_ptr=ptr[:-1], neighbor_shifts=lsh)),
        ("neighbor_ptr", dict(neighbor_list=lst, neighbor_ptr=torch.zeros((N + 3,), dtype=I32), neighbor_shifts=lsh)),
        ("batch_idx", dict(neighbor_matrix=nm, neighbor_matrix_shifts=nsh, batch_idx=bi[:-1])),
    ]
    for match, kw in cases:
        with pytest.raises(ValueError, match=match):
            call(pos, q, cells, a, **kw)
    with pytest.raises(ValueError, match="charges"):
        call(pos, q[:-1], cells, a, neighbor_matrix=nm, neighbor_matrix_shifts=nsh)
    with pytest.raises(ValueError, match="alpha has 3 values but there are 2 systems"):  # the reference's message (ewald.py:230)
        call(pos, q, cells.repeat(2, 1, 1), torch.tensor([0.3, 0.3, 0.3]), neighbor_matrix=nm, neighbor_matrix_shifts=nsh, batch_idx=bi)


@pytest.mark.parametrize("entry", ["coulomb_energy", "coulomb_forces", "coulomb_energy_forces"])
def test_coulomb_inputs_are_checked_against_each_other(entry):
    from nvalchemiops import _capi as C
    from nvalchemiops.interactions.electrostatics import coulomb as ES

    call = getattr(ES, entry)
    pos, cell, _, bi = _geometry()
    q = torch.rand(N)
    nm, nsh, lst, ptr, lsh = _neighbour_inputs()
    cells = cell[None]
    cases = [
        ("neighbor_matrix", dict(neighbor_matrix=nm[:-1], neighbor_matrix_shifts=nsh[:-1])),
        ("neighbor_matrix_shifts", dict(neighbor_matrix=nm, neighbor_matrix_shifts=torch.zeros((N, M + 1, 3), dtype=I32))),
        ("neighbor_matrix_shifts", dict(neighbor_matrix=nm, neighbor_matrix_shifts=torch.zeros((N, M, 2), dtype=I32))),
        ("neighbor_shifts", dict(neighbor_list=lst, neighbor_ptr=ptr, neighbor_shifts=lsh[:-1])),
        ("neighbor_ptr", dict(neighbor_list=lst, neighbor_ptr=torch.zeros((N + 2,), dtype=I32), neighbor_shifts=lsh)),
        ("batch_idx", dict(neighbor_matrix=nm, neighbor_matrix_shifts=nsh, batch_idx=bi[:-1])),
    ]
    for match, kw in cases:
        with pytest.raises(ValueError, match=match):
            call(pos, q, cells, 3.0, 0.2, **kw)
    with pytest.raises(ValueError, match="charges"):
        call(pos, q[:-1], cells, 3.0, 0.2, neighbor_matrix=nm, neighbor_matrix_shifts=nsh)
    # a neighbor_ptr SHORTER than N + 1 is defined on purpose (the missing rows are empty): it passes the shape checks and stops where any
    # CPU tensor stops, at the device check -- not at a ValueError, and not at the library
    with pytest.raises(C.NativeLibraryError, match="ROCm devices only"):
        call(pos, q, cells, 3.0, 0.2, neighbor_list=lst, neighbor_ptr=ptr[:2], neighbor_shifts=lsh)


def _d4_tables(nz=6):
    r, ones = torch.rand, lambda *s: torch.ones(s, dtype=I32)  # noqa: E731
    return dict(rcov=r(nz), en=r(nz), r4r2=r(nz), zeff=r(nz), gam=r(nz), n_ref=ones(nz), ngw=ones(nz, 7), cn_ref=r(nz, 7), q_ref=r(nz, 7),
                c6_ref=r(nz, nz, 7, 7))


# every D4 table with ONE wrong dimension (the kernels index them with Z < nz = len(rcov) and a reference index < 7)
BAD_D4_TABLES = [
    ("rcov", lambda: torch.rand(6, 1)), ("en", lambda: torch.rand(5)), ("r4r2", lambda: torch.rand(5)), ("zeff", lambda: torch.rand(5)),
    ("gam", lambda: torch.rand(5)), ("n_ref", lambda: torch.ones(5, dtype=I32)), ("ngw", lambda: torch.ones((6, 6), dtype=I32)),
    ("ngw", lambda: torch.ones((5, 7), dtype=I32)), ("cn_ref", lambda: torch.rand(6, 6)), ("cn_ref", lambda: torch.rand(5, 7)),
    ("q_ref", lambda: torch.rand(6, 6)), ("q_ref", lambda: torch.rand(5, 7)), ("c6_ref", lambda: torch.rand(6, 5, 7, 7)),
    ("c6_ref", lambda: torch.rand(5, 6, 7, 7)), ("c6_ref", lambda: torch.rand(6, 6, 6, 7)), ("c6_ref", lambda: torch.rand(6, 6, 7, 6)),
]


def _d4_calls():
    from nvalchemiops.interactions.dispersion import dftd4, dftd4_atm

    return {"dftd4": lambda pos, z, q, **kw: dftd4(pos, z, q, a1=0.4, a2=4.0, s8=0.8, **kw),
            "dftd4_atm": lambda pos, z, q, **kw: dftd4_atm(pos, z, a1=0.4, a2=4.0, three_body_cutoff=6.0, **kw)}


@pytest.mark.parametrize("entry", ["dftd4", "dftd4_atm"])
def test_dftd4_inputs_are_checked_against_each_other(entry):
    from nvalchemiops.interactions.dispersion import D4Parameters

    call = _d4_calls()[entry]
    pos, cell, _, bi = _geometry()
    z, q = torch.ones(N, dtype=I32), torch.rand(N)
    nm, nsh, lst, ptr, lsh = _neighbour_inputs()
    t = _d4_tables()
    cells = cell[None]
    cases = [
        ("neighbor_matrix", dict(neighbor_matrix=nm[:-1])),
        ("neighbor_matrix", dict(neighbor_matrix=torch.full((N + 1, M), N, dtype=I32))),
        ("neighbor_matrix_shifts", dict(neighbor_matrix=nm, neighbor_matrix_shifts=torch.zeros((N, M + 1, 3), dtype=I32), cell=cells)),
        ("neighbor_matrix_shifts", dict(neighbor_matrix=nm, neighbor_matrix_shifts=torch.zeros((N, M - 1, 3), dtype=I32), cell=cells)),
        ("neighbor_matrix_shifts", dict(neighbor_matrix=nm, neighbor_matrix_shifts=torch.zeros((N, M, 2), dtype=I32), cell=cells)),
        ("neighbor_matrix_shifts", dict(neighbor_matrix=nm, neighbor_matrix_shifts=torch.zeros((N - 1, M, 3), dtype=I32), cell=cells)),
        ("neighbor_matrix_shifts", dict(neighbor_matrix=nm, neighbor_matrix_shifts=torch.zeros((N, M), dtype=I32), cell=cells)),
        ("unit_shifts", dict(neighbor_list=lst, neighbor_ptr=ptr, unit_shifts=lsh[:-1], cell=cells)),
        ("unit_shifts", dict(neighbor_list=lst, neighbor_ptr=ptr, unit_shifts=torch.zeros((7, 2), dtype=I32), cell=cells)),
        ("neighbor_ptr", dict(neighbor_list=lst, neighbor_ptr=ptr[:-1])),
        ("neighbor_ptr", dict(neighbor_list=lst, neighbor_ptr=torch.zeros((N + 2,), dtype=I32))),
        ("neighbor_list", dict(neighbor_list=torch.zeros((7, 2), dtype=I32), neighbor_ptr=ptr)),
        ("batch_idx", dict(neighbor_matrix=nm, batch_idx=bi[:-1])),
        ("batch_idx", dict(neighbor_list=lst, neighbor_ptr=ptr, batch_idx=bi[:-1])),
        ("cell must have shape", dict(neighbor_matrix=nm, neighbor_matrix_shifts=nsh, batch_idx=bi, num_systems=3, cell=cells.repeat(2, 1, 1))),
        ("cell must have shape", dict(neighbor_matrix=nm, neighbor_matrix_shifts=nsh, cell=cells.repeat(2, 1, 1))),
        ("cell must have shape", dict(neighbor_list=lst, neighbor_ptr=ptr, unit_shifts=lsh, cell=cells.repeat(2, 1, 1))),
        ("cell must have shape", dict(neighbor_matrix=nm, neighbor_matrix_shifts=nsh, cell=torch.zeros(3, 2))),
    ]
    for match, kw in cases:
        for params in (t, D4Parameters(**t)):
            with pytest.raises(ValueError, match=match):
                call(pos, z, q, d4_params=params, **kw)
    for lists in (dict(neighbor_matrix=nm), dict(neighbor_list=lst, neighbor_ptr=ptr)):
        with pytest.raises(ValueError, match="numbers"):
            call(pos, z[:-1], q, d4_params=t, **lists)
        if entry == "dftd4":
            with pytest.raises(ValueError, match="charges"):
                call(pos, z, q[:-1], d4_params=t, **lists)
    for name, make in BAD_D4_TABLES:
        with pytest.raises(ValueError, match=f"^{name} must"):
            call(pos, z, q, d4_params={**t, name: make()}, neighbor_matrix=nm)
    with pytest.raises(ValueError, match="to match rcov"):  # every table against a shorter rcov
        call(pos, z, q, d4_params={**t, "rcov": torch.rand(5)}, neighbor_matrix=nm)


def _gaussian_calls():
    from nvalchemiops.interactions.electrostatics import gaussian_charge_correction as gcc

    everything = dict(compute_forces=True, compute_charge_gradients=True, compute_sigma_gradients=True)
    return {"energies": gcc, "all_outputs": lambda *a, **k: gcc(*a, **everything, compute_virial=len(a) > 3, **k),  # (the virial needs the cell)
            "autograd": lambda pos, q, *a, **k: gcc(pos.clone().requires_grad_(True), q.clone().requires_grad_(True), *a, **k)}


def _periodic_list_cases(shifts_name):
    """The list disagreements of a periodic call whose CSR shifts are called `shifts_name`: (message, list kwargs)."""
    nm, nsh, lst, ptr, lsh = _neighbour_inputs()
    z = lambda *s: torch.zeros(s, dtype=I32)  # noqa: E731
    return [
        ("neighbor_matrix", dict(neighbor_matrix=nm[:-1], neighbor_matrix_shifts=nsh[:-1])),
        ("neighbor_matrix", dict(neighbor_matrix=torch.full((N + 1, M), N, dtype=I32), neighbor_matrix_shifts=z(N + 1, M, 3))),
        ("neighbor_matrix", dict(neighbor_matrix=torch.full((N * M,), N, dtype=I32), neighbor_matrix_shifts=nsh)),
        ("neighbor_matrix_shifts", dict(neighbor_matrix=nm, neighbor_matrix_shifts=z(N, M + 1, 3))),
        ("neighbor_matrix_shifts", dict(neighbor_matrix=nm, neighbor_matrix_shifts=z(N, M - 1, 3))),
        ("neighbor_matrix_shifts", dict(neighbor_matrix=nm, neighbor_matrix_shifts=z(N, M, 2))),
        ("neighbor_matrix_shifts", dict(neighbor_matrix=nm, neighbor_matrix_shifts=nsh[:-1])),
        (shifts_name, dict(neighbor_list=lst, neighbor_ptr=ptr, **{shifts_name: lsh[:-1]})),
        (shifts_name, dict(neighbor_list=lst, neighbor_ptr=ptr, **{shifts_name: z(7, 2)})),
        ("neighbor_ptr", dict(neighbor_list=lst, neighbor_ptr=ptr[:-1], **{shifts_name: lsh})),
        ("neighbor_ptr", dict(neighbor_list=lst, neighbor_ptr=z(N + 2), **{shifts_name: lsh})),
        ("neighbor_list", dict(neighbor_list=z(7, 2), neighbor_ptr=ptr, **{shifts_name: z(7, 3)})),
    ]


@pytest.mark.parametrize("entry", ["energies", "all_outputs", "autograd"])
def test_gaussian_charge_correction_inputs_are_checked_against_each_other(entry):
    call = _gaussian_calls()[entry]
    pos, cell, _, bi = _geometry()
    q, s = torch.rand(N), torch.rand(N) + 0.3
    nm, nsh, lst, ptr, lsh = _neighbour_inputs()
    cells = cell[None]
    good = dict(neighbor_matrix=nm, neighbor_matrix_shifts=nsh)
    for match, kw in _periodic_list_cases("neighbor_shifts"):
        with pytest.raises(ValueError, match=match):
            call(pos, q, s, cells, **kw)
    for lists in (good, dict(neighbor_list=lst, neighbor_ptr=ptr, neighbor_shifts=lsh)):
        with pytest.raises(ValueError, match="charges"):
            call(pos, q[:-1], s, cells, **lists)
        with pytest.raises(ValueError, match="sigma"):
            call(pos, q, s[:-1], cells, **lists)
        with pytest.raises(ValueError, match="sigma"):
            call(pos, q, s[:, None].expand(N, 2), cells, **lists)
        with pytest.raises(ValueError, match="batch_idx"):
            call(pos, q, s, cells.repeat(B, 1, 1), batch_idx=bi[:-1], **lists)
        with pytest.raises(ValueError, match="cell must have shape"):
            call(pos, q, s, torch.zeros(3, 2), **lists)
    # without a cell: the same list checks, and no shifts
    with pytest.raises(ValueError, match="neighbor_matrix"):
        call(pos, q, s, neighbor_matrix=nm[:-1])
    with pytest.raises(ValueError, match="neighbor_ptr"):
        call(pos, q, s, neighbor_list=lst, neighbor_ptr=ptr[:-1])
    with pytest.raises(ValueError, match="need a cell"):
        call(pos, q, s, **good)


def _qeq_calls():
    from nvalchemiops.interactions.electrostatics import charge_equilibration as qeq

    return {"pme": lambda *a, **k: qeq(*a, reciprocal="pme", **{"alpha": 0.4, "mesh_dimensions": (8, 8, 8), **k}),
            "ewald": lambda *a, **k: qeq(*a, reciprocal="ewald", **{"alpha": 0.4, "k_cutoff": 2.0, **k}),
            "ewald_info_autograd": lambda pos, chi, *a, **k: qeq(pos, chi.clone().requires_grad_(True), *a, reciprocal="ewald", return_info=True,
                                                                 **{"alpha": 0.4, "k_cutoff": 2.0, **k})}


@pytest.mark.parametrize("entry", ["pme", "ewald", "ewald_info_autograd"])
def test_charge_equilibration_inputs_are_checked_against_each_other(entry):
    from nvalchemiops.interactions.electrostatics import charge_equilibration as qeq

    call = _qeq_calls()[entry]
    pos, cell, _, bi = _geometry()
    chi, hard, s, q0 = torch.rand(N), torch.rand(N) + 1.0, torch.rand(N) + 0.3, torch.zeros(N)
    nm, nsh, lst, ptr, lsh = _neighbour_inputs()
    cells, cellb = cell[None], cell[None].repeat(B, 1, 1)
    for match, kw in _periodic_list_cases("neighbor_shifts"):
        with pytest.raises(ValueError, match=match):
            call(pos, chi, hard, s, cells, **kw)
    for lists in (dict(neighbor_matrix=nm, neighbor_matrix_shifts=nsh), dict(neighbor_list=lst, neighbor_ptr=ptr, neighbor_shifts=lsh)):
        for name, args in (("electronegativity", (chi[:-1], hard, s)), ("hardness", (chi, hard[:-1], s)), ("sigma", (chi, hard, s[:-1])),
                           ("electronegativity", (chi[:, None].expand(N, 2), hard, s)), ("hardness", (chi, hard[:, None].expand(N, 2), s))):
            with pytest.raises(ValueError, match=name):
                call(pos, *args, cells, **lists)
        with pytest.raises(ValueError, match="initial_charges"):
            call(pos, chi, hard, s, cells, initial_charges=q0[:-1], **lists)
        with pytest.raises(ValueError, match="batch_idx"):
            call(pos, chi, hard, s, cellb, batch_idx=bi[:-1], **lists)
        with pytest.raises(ValueError, match="batch_idx is required"):
            call(pos, chi, hard, s, cellb, **lists)
        with pytest.raises(ValueError, match="cell must have shape"):
            call(pos, chi, hard, s, cellb, batch_idx=bi, num_systems=3, **lists)
        with pytest.raises(ValueError, match="cell must have shape"):
            call(pos, chi, hard, s, torch.zeros(3, 2), **lists)
        with pytest.raises(ValueError, match="total_charge"):
            call(pos, chi, hard, s, cellb, batch_idx=bi, total_charge=torch.zeros(3), **lists)
        with pytest.raises(ValueError, match="total_charge"):
            call(pos, chi, hard, s, cells, total_charge=torch.zeros(2), **lists)
        with pytest.raises(ValueError, match="alpha has 3 values but there are 2 systems"):
            call(pos, chi, hard, s, cellb, batch_idx=bi, alpha=torch.tensor([0.4, 0.4, 0.4]), **lists)
    # clusters: no cell, the number of systems from num_systems or the length of total_charge
    for match, kw in (("neighbor_matrix", dict(neighbor_matrix=nm[:-1])), ("neighbor_ptr", dict(neighbor_list=lst, neighbor_ptr=ptr[:-1])),
                      ("neighbor_list", dict(neighbor_list=torch.zeros((7, 2), dtype=I32), neighbor_ptr=ptr)),
                      ("need a cell", dict(neighbor_matrix=nm, neighbor_matrix_shifts=nsh)),
                      ("batch_idx", dict(neighbor_matrix=nm, batch_idx=bi[:-1], num_systems=B)),
                      ("batch_idx is required", dict(neighbor_matrix=nm, total_charge=torch.zeros(B))),
                      ("total_charge", dict(neighbor_matrix=nm, batch_idx=bi, num_systems=B, total_charge=torch.zeros(3))),
                      ("initial_charges", dict(neighbor_matrix=nm, initial_charges=q0[:-1]))):
        with pytest.raises(ValueError, match=match):
            qeq(pos, chi, hard, s, **kw)
    with pytest.raises(ValueError, match="hardness"):
        qeq(pos, chi, hard[:-1], s, neighbor_matrix=nm)


def test_well_formed_cpu_arguments_stop_at_the_device_check():
    """The control: the same calls with consistent shapes get past every shape check and are refused for being on the CPU (still without a
    library call) -- so the ValueErrors above are about the mismatch, not about something else in the fixture."""
    from nvalchemiops import _capi as C
    from nvalchemiops.interactions.electrostatics import charge_equilibration, ewald_real_space
    from nvalchemiops.interactions.electrostatics.coulomb import coulomb_energy
    from nvalchemiops.neighborlist import build_cell_list, cell_list

    pos, cell, pbc, bi = _geometry()
    nm, nsh, lst, ptr, lsh = _neighbour_inputs()
    z, q = torch.ones(N, dtype=I32), torch.rand(N)
    calls = [lambda: cell_list(pos, 2.0, cell, pbc, **_outputs()),
             lambda: build_cell_list(pos, 2.0, cell, pbc, *_cache().values()),
             lambda: ewald_real_space(pos, q, cell[None], torch.tensor([0.3]), neighbor_list=lst, neighbor_ptr=ptr, neighbor_shifts=lsh),
             lambda: coulomb_energy(pos, q, cell[None], 3.0, 0.2, neighbor_matrix=nm, neighbor_matrix_shifts=nsh)]
    calls += [lambda c=c: c(pos, z, d3_params=_tables(), neighbor_matrix=nm, neighbor_matrix_shifts=nsh, cell=cell[None]) for c in _d3_calls().values()]
    calls += [lambda c=c: c(pos, z, q, d4_params=_d4_tables(), neighbor_matrix=nm, neighbor_matrix_shifts=nsh, cell=cell[None]) for c in _d4_calls().values()]
    calls += [lambda c=c: c(pos, z, q, d4_params=_d4_tables(), neighbor_list=lst, neighbor_ptr=ptr, unit_shifts=lsh, cell=cell[None])
              for c in _d4_calls().values()]
    s, hard = torch.rand(N) + 0.3, torch.rand(N) + 1.0
    calls += [lambda c=c: c(pos, q, s, cell[None], neighbor_matrix=nm, neighbor_matrix_shifts=nsh) for c in _gaussian_calls().values()]
    calls += [lambda c=c: c(pos, q, s, cell[None].repeat(B, 1, 1), neighbor_list=lst, neighbor_ptr=ptr, neighbor_shifts=lsh, batch_idx=bi)
              for c in _gaussian_calls().values()]
    calls += [lambda c=c: c(pos, q, hard, s, cell[None].repeat(B, 1, 1), neighbor_matrix=nm, neighbor_matrix_shifts=nsh, batch_idx=bi,
                            total_charge=torch.zeros(B), initial_charges=torch.zeros(N), alpha=torch.tensor([0.4, 0.4])) for c in _qeq_calls().values()]
    calls.append(lambda: charge_equilibration(pos, q, hard, s, neighbor_list=lst, neighbor_ptr=ptr, batch_idx=bi, total_charge=torch.zeros(B)))
    for call in calls:
        with pytest.raises(C.NativeLibraryError, match="ROCm devices only"):
            call()
