"""GPU parity tests of the HIP neighbour-list path against the CPU oracle (bit-exact sets / counts).

Everything here goes through the public API -> ctypes -> C ABI -> HIP kernels.  Run with `-m gpu` on an MI355X."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import systems as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _t(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV) if dtype is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def _pairs(nm, num, sh):
    return O.canonical_pairs(nm.cpu().numpy(), num.cpu().numpy(), sh.cpu().numpy())


def _coo_pairs(lst, sh):
    rows = np.column_stack([lst.cpu().numpy().T, sh.cpu().numpy()]).astype(np.int64)
    return rows[np.lexsort(rows.T[::-1])] if len(rows) else rows.reshape(0, 5)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("cutoff", [1.0, 4.0, 6.0])
def test_golden_counts(dtype, cutoff):
    from nvalchemiops.neighborlist import batch_cell_list, cell_list

    pbc = torch.tensor([True] * 3, device=DEV)
    _, num, _ = cell_list(_t(S.HOTLPD_POS.astype(dtype)), cutoff, _t(S.HOTLPD_CELL.astype(dtype)), pbc)
    assert num.cpu().tolist() == S.HOTLPD_COUNTS[cutoff]
    _, num, _ = cell_list(_t(S.SICU_POS.astype(dtype)), cutoff, _t(S.SICU_CELL.astype(dtype)), pbc)
    assert num.cpu().tolist() == S.SICU_COUNTS[cutoff]
    pos = np.concatenate([S.HOTLPD_POS, S.SICU_POS]).astype(dtype)
    cell = np.stack([S.HOTLPD_CELL, S.SICU_CELL]).astype(dtype)
    bi = torch.tensor([0] * 9 + [1] * 2, dtype=torch.int32, device=DEV)
    _, num, _ = batch_cell_list(_t(pos), cutoff, _t(cell), torch.ones((2, 3), dtype=torch.bool, device=DEV), bi)
    assert num.cpu().tolist() == S.HOTLPD_COUNTS[cutoff] + S.SICU_COUNTS[cutoff]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kind", ["cubic", "triclinic", "outside", "mixed_pbc", "no_pbc"])
def test_cell_list_matches_oracle(dtype, kind):
    from nvalchemiops.neighborlist import cell_list

    pos, cell = S.random_box(700, 14.0, seed=42, dtype=dtype, triclinic=(kind == "triclinic"), outside=(kind == "outside"))
    pbc = {"mixed_pbc": [True, False, True], "no_pbc": [False] * 3}.get(kind, [True] * 3)
    for cutoff, m in ((3.2, 64), (6.5, 416)):  # M above the densest row: overflow truncation is order-dependent
        onm, onum, osh = O.cell_list(pos, cutoff, cell, pbc, max_neighbors=m)
        nm, num, sh = cell_list(_t(pos), cutoff, _t(cell), torch.tensor(pbc, device=DEV), max_neighbors=m)
        assert num.cpu().numpy().tolist() == onum.tolist()
        assert np.array_equal(_pairs(nm, num, sh), O.canonical_pairs(onm, onum, osh))
        # padding contract: slots >= num are fill_value (= N) with zero shifts
        nmc, numc, shc = nm.cpu().numpy(), num.cpu().numpy(), sh.cpu().numpy()
        mask = np.arange(m)[None, :] >= numc[:, None]
        assert (nmc[mask] == len(pos)).all() and (shc[mask] == 0).all()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_batch_matches_oracle_and_single(dtype):
    from nvalchemiops.neighborlist import batch_cell_list, cell_list

    parts, cells, pbcs, bis = [], [], [], []
    for s, (n, box, tri, pb) in enumerate([(300, 11.0, False, [True] * 3), (150, 9.0, True, [True, True, False]), (420, 13.0, False, [False] * 3),
                                           (1, 8.0, False, [True] * 3)]):
        p, c = S.random_box(n, box, seed=100 + s, dtype=dtype, triclinic=tri)
        parts.append(p), cells.append(c), pbcs.append(pb), bis.append(np.full(n, s, np.int32))
    pos, cell, pbc, bi = np.concatenate(parts), np.stack(cells), np.array(pbcs), np.concatenate(bis)
    onm, onum, osh = O.cell_list(pos, 4.0, cell, pbc, batch_idx=bi, max_neighbors=128)
    nm, num, sh = batch_cell_list(_t(pos), 4.0, _t(cell), _t(pbc), _t(bi), max_neighbors=128)
    assert np.array_equal(num.cpu().numpy(), onum)
    assert np.array_equal(_pairs(nm, num, sh), O.canonical_pairs(onm, onum, osh))
    off = 0
    for p, c, pb in zip(parts, cells, pbcs):  # batch == per-system
        nm1, num1, sh1 = cell_list(_t(p), 4.0, _t(c), torch.tensor(pb, device=DEV), max_neighbors=128)
        assert np.array_equal(num1.cpu().numpy(), onum[off:off + len(p)])
        off += len(p)


@pytest.mark.parametrize("direct", [True, False])
def test_coo_output(direct):
    from nvalchemiops.neighborlist import cell_list

    pos, cell = S.random_box(500, 12.0, seed=9, dtype=np.float32, outside=True)
    pbc = torch.tensor([True] * 3, device=DEV)
    onm, onum, osh = O.cell_list(pos, 4.5, cell, [True] * 3, max_neighbors=160)
    olst, optr, olsh = O.matrix_to_coo(onm, onum, osh, fill_value=500)
    kw = {} if direct else dict(neighbor_matrix=torch.empty((500, 160), dtype=torch.int32, device=DEV))
    lst, nptr, lsh = cell_list(_t(pos), 4.5, _t(cell), pbc, max_neighbors=160, return_neighbor_list=True, **kw)
    assert lst.dtype == torch.int32 and lst.shape == (2, int(onum.sum())) and lsh.shape == (int(onum.sum()), 3)
    assert np.array_equal(nptr.cpu().numpy(), optr)
    assert np.array_equal(_coo_pairs(lst, lsh), _coo_pairs(torch.as_tensor(olst), torch.as_tensor(olsh)))
    src = lst[0].cpu().numpy()
    assert (np.diff(src) >= 0).all()  # sorted by source atom (docs/userguide/components/neighborlist.md:133-137)


def test_coo_conversion_follows_the_mask_not_the_counts():
    """get_neighbor_list_from_neighbor_matrix: the list is what `neighbor_matrix != fill_value` selects and neighbor_ptr is the cumsum of
    num_neighbors, as in the reference (neighbor_utils.py:428-438) -- also when the two disagree (matrix padded with N, default
    fill_value = -1): then EVERY slot is listed, padding included, and nothing is left uninitialised."""
    from nvalchemiops.neighborlist import cell_list, get_neighbor_list_from_neighbor_matrix

    pos, cell = S.random_box(300, 10.0, seed=9, dtype=np.float32)
    nm, num, sh = cell_list(_t(pos), 3.0, _t(cell), torch.tensor([True] * 3, device=DEV), max_neighbors=48)
    lst, nptr, lsh = get_neighbor_list_from_neighbor_matrix(nm, num, sh)  # default fill_value = -1: nothing equals it
    m = nm.cpu().numpy()
    assert lst.shape[1] == 300 * 48 and np.array_equal(lst[1].cpu().numpy(), m.ravel())
    assert np.array_equal(lst[0].cpu().numpy(), np.repeat(np.arange(300), 48))
    assert np.array_equal(lsh.cpu().numpy(), sh.cpu().numpy().reshape(-1, 3))
    assert np.array_equal(nptr.cpu().numpy(), np.concatenate([[0], np.cumsum(num.cpu().numpy())]))
    lst, nptr, lsh = get_neighbor_list_from_neighbor_matrix(nm, num, sh, fill_value=300)
    mask = m != 300
    assert lst.shape[1] == int(num.sum()) == int(mask.sum()) and np.array_equal(lst[1].cpu().numpy(), m[mask])


def test_half_fill_and_overflow():
    from nvalchemiops.neighborlist import NeighborOverflowError, cell_list

    pos, cell = S.random_box(400, 10.0, seed=3, dtype=np.float64)
    pbc = torch.tensor([True] * 3, device=DEV)
    nm, num, sh = cell_list(_t(pos), 3.5, _t(cell), pbc, max_neighbors=96)
    hm, hnum, hsh = cell_list(_t(pos), 3.5, _t(cell), pbc, max_neighbors=96, half_fill=True)
    full, half = _pairs(nm, num, sh), _pairs(hm, hnum, hsh)
    assert len(half) * 2 == len(full)
    mirrored = np.column_stack([half[:, 1], half[:, 0], -half[:, 2:]])
    both = np.concatenate([half, mirrored])
    assert np.array_equal(both[np.lexsort(both.T[::-1])], full)
    # overflow: counts keep counting past M, the matrix is truncated, COO conversion raises
    sm, snum, ssh = cell_list(_t(pos), 3.5, _t(cell), pbc, max_neighbors=8)
    assert np.array_equal(snum.cpu().numpy(), num.cpu().numpy()) and int(snum.max()) > 8
    with pytest.raises(NeighborOverflowError):
        cell_list(_t(pos), 3.5, _t(cell), pbc, max_neighbors=8, return_neighbor_list=True)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_naive_matches_oracle(dtype):
    from nvalchemiops.neighborlist import naive_neighbor_list, neighbor_list

    # config 1 of BASELINE.json: 1k atoms, non-periodic, naive
    mol, _, side = S.molecule(1000, seed=2000, dtype=dtype)
    onm, onum = O.naive(mol, 5.0, max_neighbors=64)
    nm, num = neighbor_list(_t(mol), 5.0, method="naive", max_neighbors=64)
    assert np.array_equal(num.cpu().numpy(), onum)
    assert np.array_equal(np.sort(nm.cpu().numpy(), 1), np.sort(onm, 1))
    pos, cell = S.random_box(300, 9.0, seed=4, dtype=dtype, triclinic=True)
    onm, onum, osh = O.naive(pos, 3.3, cell, [True, True, False], max_neighbors=160)
    nm, num, sh = naive_neighbor_list(_t(pos), 3.3, cell=_t(cell), pbc=torch.tensor([True, True, False], device=DEV), max_neighbors=160)
    assert int(onum.max()) <= 160  # no overflow: truncated rows are order-dependent
    assert np.array_equal(_pairs(nm, num, sh), O.canonical_pairs(onm, onum, osh))


def test_half_precision_positions_are_accepted():
    """The reference instantiates its neighbour kernels for float16 as well (naive.py:186-188, cell_list.py:761); here fp16 coordinates
    are read exactly and searched in float32 -- the result equals the float32 search of the same (rounded) coordinates."""
    from nvalchemiops.neighborlist import neighbor_list

    mol, _, _ = S.molecule(1000, seed=2001, dtype=np.float32)
    h = _t(mol).half()
    nm, num = neighbor_list(h, 5.0, method="naive", max_neighbors=96)
    nm32, num32 = neighbor_list(h.float(), 5.0, method="naive", max_neighbors=96)
    assert torch.equal(num, num32) and torch.equal(nm, nm32)
    pos, cell = S.random_box(6000, 24.0, seed=5, dtype=np.float32)
    h = _t(pos).half()
    pbc = torch.tensor([True, True, True], device=DEV)
    out = neighbor_list(h, 3.0, cell=_t(cell).half(), pbc=pbc, max_neighbors=96)
    ref = neighbor_list(h.float(), 3.0, cell=_t(cell).half().float(), pbc=pbc, max_neighbors=96)
    assert all(torch.equal(a, b) for a, b in zip(out, ref))


def test_query_api_and_preallocated_buffers():
    from nvalchemiops.neighborlist import (allocate_cell_list, build_cell_list, cell_list, estimate_cell_list_sizes, query_cell_list)

    pos, cell = S.random_box(600, 12.0, seed=11, dtype=np.float32)
    tp, tc, pbc = _t(pos), _t(cell), torch.tensor([True] * 3, device=DEV)
    ncell, radius = estimate_cell_list_sizes(tc, pbc, 3.0)
    _, _, _, ocpd, orad = O.cell_list(pos, 3.0, cell, [True] * 3, max_neighbors=64, return_grid=True)
    assert ncell == int(np.prod(ocpd[0])) and radius.cpu().tolist() == orad[0].tolist()
    cache = allocate_cell_list(600, ncell, radius, tp.device)
    build_cell_list(tp, 3.0, tc, pbc, *cache)
    assert cache[0].cpu().tolist() == ocpd[0].tolist()
    assert int(cache[4].sum()) == 600 and sorted(cache[6].cpu().tolist()) == list(range(600))
    # every cache tensor against the oracle's restatement of build_cell_list (rebuild detection consumes their VALUES)
    want = O.build_cell_cache(pos, 3.0, cell, [True] * 3, ncell)
    names = ("cells_per_dimension", "atom_periodic_shifts", "atom_to_cell_mapping", "atoms_per_cell_count", "cell_atom_start_indices", "cell_atom_list")
    for got, ref, what in zip((cache[0],) + tuple(cache[2:]), want, names):
        assert np.array_equal(got.cpu().numpy().reshape(ref.shape), ref), what
    nm = torch.full((600, 64), 600, dtype=torch.int32, device=DEV)
    sh = torch.zeros((600, 64, 3), dtype=torch.int32, device=DEV)
    num = torch.zeros(600, dtype=torch.int32, device=DEV)
    query_cell_list(tp, 3.0, tc, pbc, *cache, nm, sh, num)
    onm, onum, osh = O.cell_list(pos, 3.0, cell, [True] * 3, max_neighbors=64)
    assert np.array_equal(_pairs(nm, num, sh), O.canonical_pairs(onm, onum, osh))
    a, b, c = cell_list(tp, 3.0, tc, pbc, neighbor_matrix=nm, neighbor_matrix_shifts=sh, num_neighbors=num)
    assert a.data_ptr() == nm.data_ptr() and b.data_ptr() == num.data_ptr()
    assert c.data_ptr() == sh.data_ptr()
    # ... and so do the naive and the batched forms (tests/test_arg_layouts_gpu.py goes through every search entry point)
    from nvalchemiops.neighborlist import batch_cell_list, batch_naive_neighbor_list, naive_neighbor_list

    bi = torch.zeros(600, dtype=torch.int32, device=DEV)
    for out in (naive_neighbor_list(tp, 3.0, cell=tc, pbc=pbc, neighbor_matrix=nm, neighbor_matrix_shifts=sh, num_neighbors=num),
                batch_cell_list(tp, 3.0, tc[None], pbc[None], bi, neighbor_matrix=nm, neighbor_matrix_shifts=sh, num_neighbors=num),
                batch_naive_neighbor_list(tp, 3.0, batch_idx=bi, cell=tc[None], pbc=pbc[None], neighbor_matrix=nm, neighbor_matrix_shifts=sh,
                                          num_neighbors=num)):
        assert [t.data_ptr() for t in out] == [nm.data_ptr(), num.data_ptr(), sh.data_ptr()]
        assert np.array_equal(_pairs(nm, num, sh), O.canonical_pairs(onm, onum, osh))


def test_empty_and_tiny_inputs():
    from nvalchemiops.neighborlist import cell_list

    pbc = torch.tensor([True] * 3, device=DEV)
    cell = torch.eye(3, device=DEV) * 10
    nm, num, sh = cell_list(torch.zeros((0, 3), device=DEV), 2.0, cell, pbc)
    assert nm.shape == (0, 0) and num.shape == (0,) and sh.shape == (0, 0, 3)
    nm, num, sh = cell_list(torch.tensor([[1.0, 1.0, 1.0]], device=DEV), 2.0, cell, pbc, max_neighbors=8)
    assert num.cpu().tolist() == [0] and (nm.cpu() == 1).all()
    two = torch.tensor([[0.5, 5.0, 5.0], [9.5, 5.0, 5.0]], device=DEV)
    nm, num, sh = cell_list(two, 2.0, cell, pbc, max_neighbors=8)
    assert num.cpu().tolist() == [1, 1] and sh[0, 0].cpu().tolist() == [-1, 0, 0] and sh[1, 0].cpu().tolist() == [1, 0, 0]


@pytest.mark.parametrize("n,dtype,cutoff,m", [(50000, np.float32, 5.0, 64), (50000, np.float32, 5.0, None), (100000, np.float64, 9.0, 256)])
def test_baseline_configs_full_size_match_oracle(n, dtype, cutoff, m):
    """BASELINE.json config 2 (50k-atom periodic box, cell_list, padded matrix, fp32; explicit M = 64 AND the default row width
    estimate_max_neighbors(5 A) = 928 the API uses when the caller gives none) and the neighbour list of config 4 (100k atoms,
    fp64, the 9 A real-space cutoff of the headline PME leg) at their FULL sizes: counts and (i, j, S) sets bit-exact vs the oracle
    (1.4 s / 15 s of oracle time); with the default width also the padding itself (fill value N, zero shifts)."""
    from nvalchemiops.neighborlist import cell_list

    pos, cell, _, _ = S.fcc_box(n, dtype=dtype)
    onm, onum, osh = O.cell_list(pos, cutoff, cell, [True] * 3, max_neighbors=m)
    nm, num, sh = cell_list(_t(pos), cutoff, _t(cell), torch.tensor([True] * 3, device=DEV), max_neighbors=m)
    if m is None:
        assert nm.shape[1] == onm.shape[1] == 928
        pad = torch.arange(928, device=DEV)[None, :] >= num[:, None]
        assert bool((nm[pad] == n).all()) and bool((sh[pad] == 0).all())
    assert int(onum.max()) <= nm.shape[1]
    assert np.array_equal(num.cpu().numpy(), onum)
    assert np.array_equal(_pairs(nm, num, sh), O.canonical_pairs(onm, onum, osh))


def test_headline_list_100k_40bohr_full_size_matches_oracle():
    """The list the headline step is timed on -- 100 000 atoms, rc = 40 Bohr, fp32, padded matrix M = 2560, 235 M directed pairs, the
    k = 3 tiled kernel -- against the oracle at FULL size: `num_neighbors` bit-exact, and every row equal as a sorted set of (j, S),
    compared row block by row block on the device (this list used to be checked at <= 16 k atoms only)."""
    from nvalchemiops.neighborlist import cell_list
    from tests import _headline as H

    pos, cell, _ = H.system()
    onm, onum, osh = H.oracle_list()
    nm, num, sh = cell_list(_t(pos), H.CUTOFF, _t(cell), torch.tensor([True] * 3, device=DEV), max_neighbors=H.M)
    assert int(onum.sum()) > 2.3e8 and int(onum.max()) <= H.M
    assert np.array_equal(num.cpu().numpy(), onum), "neighbour counts differ from the oracle"
    # padding as the API promises: fill value N, zero shifts
    pad = torch.arange(H.M, device=DEV)[None, :] >= num[:, None]
    assert bool((nm[pad] == H.N).all()) and bool((sh[pad] == 0).all())
    del pad
    step = 10000
    for lo in range(0, H.N, step):
        hi = lo + step
        got = H.row_keys(nm[lo:hi], sh[lo:hi], num[lo:hi], torch, DEV)
        want = H.row_keys(onm[lo:hi], osh[lo:hi], onum[lo:hi], torch, DEV)
        assert torch.equal(got, want), f"rows {lo}..{hi}: (j, S) sets differ from the oracle"


def test_full_size_properties_100k():
    """BASELINE size (100k-atom periodic box): size-independent properties -- symmetry of the directed pair set under
    (i,j,S)->(j,i,-S), every stored distance < cutoff, the half list is exactly half, large cutoff (k>1 binning) agrees
    with the small-cutoff list restricted by distance."""
    from nvalchemiops.neighborlist import cell_list

    pos, cell, _, _ = S.fcc_box(100000, dtype=np.float32)
    tp, tc, pbc = _t(pos), _t(cell), torch.tensor([True] * 3, device=DEV)
    lst, nptr, sh = cell_list(tp, 9.0, tc, pbc, return_neighbor_list=True)
    n = 100000
    assert int(nptr[-1]) == lst.shape[1]
    key = (lst[0].long() * n + lst[1].long()) * 27 + ((sh[:, 0] + 1) * 9 + (sh[:, 1] + 1) * 3 + (sh[:, 2] + 1)).long()
    mkey = (lst[1].long() * n + lst[0].long()) * 27 + ((-sh[:, 0] + 1) * 9 + (-sh[:, 1] + 1) * 3 + (-sh[:, 2] + 1)).long()
    assert torch.equal(torch.sort(key).values, torch.sort(mkey).values)
    assert torch.unique(key).numel() == key.numel()
    tp64, tc64 = tp.double(), tc.double()
    d = tp64[lst[1].long()] - tp64[lst[0].long()] + sh.double() @ tc64
    d2 = (d * d).sum(1)
    assert float(d2.max()) < 81.0 * (1 + 1e-6)
    hl, hp, hs = cell_list(tp, 9.0, tc, pbc, return_neighbor_list=True, half_fill=True)
    assert hl.shape[1] * 2 == lst.shape[1]
    l5, p5, s5 = cell_list(tp, 5.0, tc, pbc, return_neighbor_list=True)
    # the 5 A list is the 9 A list restricted by distance (up to fp32 rounding of pairs within 1e-5 of the cutoff)
    assert int((d2 < 25.0 - 1e-3).sum()) <= l5.shape[1] <= int((d2 < 25.0 + 1e-3).sum())


def test_rebuild_detection():
    """SURVEY 8f N1 (neighborlist/rebuild_detection.py): skin and cell-crossing checks against numpy restatements."""
    from nvalchemiops.neighborlist import (allocate_cell_list, build_cell_list, cell_list_needs_rebuild, check_neighbor_list_rebuild_needed,
                                           estimate_cell_list_sizes, neighbor_list_needs_rebuild)

    pos, cell = S.random_box(500, 12.0, seed=5, dtype=np.float64, triclinic=True)
    tp, tc, pbc = _t(pos), _t(cell), torch.tensor([True, True, False], device=DEV)
    g = np.random.default_rng(0)
    small = pos + g.uniform(-0.02, 0.02, pos.shape)
    assert not neighbor_list_needs_rebuild(tp, _t(small), 0.5).item()
    moved = small.copy()
    moved[123] += [0.4, 0.4, 0.0]
    assert neighbor_list_needs_rebuild(tp, _t(moved), 0.5).item() and check_neighbor_list_rebuild_needed(tp, _t(moved), 0.5)
    assert neighbor_list_needs_rebuild(tp, _t(moved[:10]), 0.5).item()  # shape mismatch -> rebuild
    ncell, radius = estimate_cell_list_sizes(tc, pbc, 3.0)
    cache = allocate_cell_list(500, ncell, radius, tp.device)
    build_cell_list(tp, 3.0, tc, pbc, *cache)
    assert not cell_list_needs_rebuild(tp, cache[3], cache[0], tc, pbc).item()
    # the cache the checks consume equals the oracle's (mixed pbc, triclinic), and both checks agree with the oracle's restatements of
    # _check_atoms_changed_cells / _check_atoms_moved_beyond_skin (rebuild_detection.py:37-170) on displaced configurations
    want = O.build_cell_cache(pos, 3.0, cell, [True, True, False], ncell)
    assert np.array_equal(cache[3].cpu().numpy(), want[2]) and np.array_equal(cache[0].cpu().numpy().reshape(-1), want[0].reshape(-1))
    for sigma in (0.01, 0.05, 0.35):
        disp = pos + g.normal(0, sigma, pos.shape)
        expect = O.cells_changed(disp, cell, want[2], want[0], [True, True, False])
        assert cell_list_needs_rebuild(_t(disp), cache[3], cache[0], tc, pbc).item() == expect, sigma
        for skin in (0.02, 0.2, 1.5):
            assert neighbor_list_needs_rebuild(tp, _t(disp), skin).item() == O.moved_beyond_skin(pos, disp, skin), (sigma, skin)
    assert O.cells_changed(pos + g.normal(0, 0.35, pos.shape), cell, want[2], want[0], [True, True, False])


@pytest.mark.parametrize("periodic", [False, True])
def test_dual_cutoff_and_batch_naive(periodic):
    """batch_naive / dual-cutoff API (batch_naive.py:480, naive_dual_cutoff.py:544, batch_naive_dual_cutoff.py:592)
    -- tuple layout of the reference and pair sets equal to the oracle's naive search per cutoff."""
    from nvalchemiops.neighborlist import (batch_naive_neighbor_list, batch_naive_neighbor_list_dual_cutoff,
                                           naive_neighbor_list_dual_cutoff, neighbor_list)

    pos, cell = S.random_box(300, 9.0, seed=11, dtype=np.float64)
    pbc_np = np.array([True, True, True])
    kw = dict(cell=_t(cell).unsqueeze(0), pbc=torch.tensor([[True, True, True]], device=DEV)) if periodic else {}
    out = naive_neighbor_list_dual_cutoff(_t(pos), 2.5, 4.5, max_neighbors1=64, max_neighbors2=256, **kw)
    assert len(out) == (6 if periodic else 4)
    half = len(out) // 2
    for rc, res in ((2.5, out[:half]), (4.5, out[half:])):
        nm, num = res[0].cpu().numpy(), res[1].cpu().numpy()
        sh = res[2].cpu().numpy() if periodic else np.zeros(nm.shape + (3,), np.int32)
        ref = O.naive(pos, rc, cell, pbc_np, 400) if periodic else O.naive(pos, rc, max_neighbors=400)
        rsh = ref[2] if periodic else np.zeros(ref[0].shape + (3,), np.int32)
        assert num.max() < nm.shape[1]
        assert np.array_equal(O.canonical_pairs(nm, num, sh), O.canonical_pairs(ref[0], ref[1], rsh))
    # via the dispatcher, COO format
    lst = neighbor_list(_t(pos), 2.5, cutoff2=4.5, return_neighbor_list=True, max_neighbors1=64, max_neighbors2=256, **kw)
    assert len(lst) == (6 if periodic else 4) and lst[0].shape[0] == 2 and lst[0].shape[1] == int(out[1].sum())
    assert lst[half].shape[1] == int(out[half + 1].sum())
    # batched: two copies of the system, second translated
    posb = np.concatenate([pos, pos + 3.0])
    bi = torch.tensor([0] * 300 + [1] * 300, dtype=torch.int32, device=DEV)
    kwb = dict(cell=_t(np.stack([cell, cell])), pbc=torch.tensor([[True] * 3] * 2, device=DEV)) if periodic else {}
    rb = batch_naive_neighbor_list(_t(posb), 4.5, batch_idx=bi, max_neighbors=256, **kwb)
    assert len(rb) == (3 if periodic else 2)
    numb = rb[1].cpu().numpy()
    assert (numb[:300] == out[half + 1].cpu().numpy()).all() and (numb[300:] == numb[:300]).all()
    rd = batch_naive_neighbor_list_dual_cutoff(_t(posb), 2.5, 4.5, batch_idx=bi, max_neighbors1=64, max_neighbors2=256, **kwb)
    assert len(rd) == (6 if periodic else 4)
    assert (rd[1].cpu().numpy()[:300] == out[1].cpu().numpy()).all() and (rd[half + 1].cpu().numpy() == numb).all()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_dual_cutoff_is_one_sweep_with_the_image_table_of_the_long_cutoff(dtype):
    """The reference's dual-cutoff kernels walk ONE shift table, built for cutoff2, and nest the cutoff1 test in the cutoff2 test
    (naive_dual_cutoff.py:215-226, :835).  With atoms far outside the cell (the naive family never wraps) list 1 therefore holds pairs that a
    separate cutoff1 search -- image range of cutoff1 -- cannot see; `mi_nl_neighbors_dual` reproduces the reference, single and batched,
    including the counts of rows that overflow their matrix."""
    from nvalchemiops.neighborlist import batch_naive_neighbor_list_dual_cutoff, naive_neighbor_list_dual_cutoff

    g = np.random.default_rng(77)
    cell = (np.diag([4.0, 4.4, 3.8]) + np.array([[0, 0, 0], [0.6, 0, 0], [-0.4, 0.5, 0]])).astype(dtype)
    pos = (g.uniform(-1.6, 2.6, (150, 3)) @ cell).astype(dtype)
    pbc = np.array([True, True, True])
    rc1, rc2, m = 1.5, 4.6, 2048
    kw = dict(cell=_t(cell).reshape(1, 3, 3), pbc=_t(pbc).reshape(1, 3))
    out = naive_neighbor_list_dual_cutoff(_t(pos), rc1, rc2, max_neighbors1=m, max_neighbors2=m, **kw)
    ref1 = O.naive(pos, rc1, cell, pbc, m, image_range_cutoff=rc2)
    ref2 = O.naive(pos, rc2, cell, pbc, m)
    sep1 = O.naive(pos, rc1, cell, pbc, m)
    assert int(ref1[1].sum()) > int(sep1[1].sum()), "the case must discriminate between the two image tables"
    for res, ref in ((out[:3], ref1), (out[3:], ref2)):
        nm, num, sh = (t.cpu().numpy() for t in res)
        assert np.array_equal(num, ref[1]) and num.max() <= m
        assert np.array_equal(O.canonical_pairs(nm, num, sh), O.canonical_pairs(*ref))
    # rows that overflow: counts keep counting (both lists), stored entries are a subset of the reference's pair set
    small = naive_neighbor_list_dual_cutoff(_t(pos), rc1, rc2, max_neighbors1=8, max_neighbors2=32, **kw)
    assert np.array_equal(small[1].cpu().numpy(), ref1[1]) and np.array_equal(small[4].cpu().numpy(), ref2[1])
    assert int(small[4].max()) > 32 and small[3].shape == (150, 32)
    # batched: the same system twice (second copy translated); list 1 of each copy = the single-system list 1
    posb = np.concatenate([pos, pos + np.asarray([0.3, -0.2, 0.9], dtype)])
    bi = _t(np.repeat(np.arange(2, dtype=np.int32), 150))
    rb = batch_naive_neighbor_list_dual_cutoff(_t(posb), rc1, rc2, batch_idx=bi, cell=_t(np.stack([cell, cell])), pbc=_t(np.stack([pbc, pbc])),
                                               max_neighbors1=m, max_neighbors2=m)
    n1, n2 = rb[1].cpu().numpy(), rb[4].cpu().numpy()
    assert np.array_equal(n1[:150], ref1[1]) and np.array_equal(n2[:150], ref2[1])
    if dtype == np.float64:  # (in fp32 the translated copy rounds differently: pairs on the cutoff edge may flip)
        assert int(n1[150:].sum()) == int(n1[:150].sum()) and int(n2[150:].sum()) == int(n2[:150].sum())
    first = O.canonical_pairs(rb[0].cpu().numpy()[:150], n1[:150], rb[2].cpu().numpy()[:150])
    assert np.array_equal(first, O.canonical_pairs(*ref1))


def test_custom_ops_and_graph_capture():
    """The reference's op seam (`torch.ops.nvalchemiops.*`, cell_list.py:725/892, dftd3.py:1792): same results as the functional
    API, and traceable as opaque mutating ops by torch.compile (fullgraph, aot_eager backend: no code generation involved)."""
    from nvalchemiops.interactions.dispersion import D3Parameters, dftd3
    from nvalchemiops.neighborlist import allocate_cell_list, cell_list, estimate_cell_list_sizes

    pos, cell = S.random_box(400, 14.0, seed=21, dtype=np.float32)
    tp, tc, pbc = _t(pos), _t(cell), torch.tensor([True] * 3, device=DEV)
    ncell, radius = estimate_cell_list_sizes(tc, pbc, 4.0)
    cache = allocate_cell_list(400, ncell, radius, tp.device)
    nm = torch.full((400, 96), 400, dtype=torch.int32, device=DEV)
    sh = torch.zeros((400, 96, 3), dtype=torch.int32, device=DEV)
    num = torch.zeros(400, dtype=torch.int32, device=DEV)

    def step(p):
        torch.ops.nvalchemiops.build_cell_list(p, 4.0, tc, pbc, *cache)
        torch.ops.nvalchemiops.query_cell_list(p, 4.0, tc, pbc, *cache, nm, sh, num, False)
        return num.sum()

    total = torch.compile(step, backend="aot_eager", fullgraph=True)(tp)
    rm, rnum, rsh = cell_list(tp, 4.0, tc, pbc, max_neighbors=96)
    assert int(total) == int(rnum.sum()) and torch.equal(num, rnum)
    assert np.array_equal(O.canonical_pairs(nm.cpu().numpy(), num.cpu().numpy(), sh.cpu().numpy()),
                          O.canonical_pairs(rm.cpu().numpy(), rnum.cpu().numpy(), rsh.cpu().numpy()))
    t = O.d3_test_tables(17)
    prm = D3Parameters(rcov=_t(t["rcov"]), r4r2=_t(t["r4r2"]), c6ab=_t(t["c6ab"]), cn_ref=_t(t["cn_ref"]))
    z = _t(np.random.default_rng(2).choice(np.array([1, 6, 8], np.int32), 400))
    e, f, cn = (torch.zeros(1, device=DEV), torch.zeros((400, 3), device=DEV), torch.zeros(400, device=DEV))
    torch.ops.nvalchemiops.dftd3_nm(tp, z, rm, prm.rcov, prm.r4r2, prm.c6ab, prm.cn_ref, 0.4, 4.0, 0.8, e, f, cn,
                                    torch.zeros((0, 3, 3), device=DEV), fill_value=400, cell=tc[None], neighbor_matrix_shifts=rsh)
    e2, f2, cn2 = dftd3(tp, z, 0.4, 4.0, 0.8, d3_params=prm, neighbor_matrix=rm, neighbor_matrix_shifts=rsh, cell=tc[None], fill_value=400)
    # per-system energy: float atomics over slabs (order-dependent last bit); per-atom outputs are deterministic
    assert torch.allclose(e, e2, rtol=1e-6) and torch.equal(f, f2) and torch.equal(cn, cn2)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_box_exact_multiple_of_cutoff(dtype):
    """Box edge = integer multiple of the cutoff (cell edge == rc is the tightest legal binning): same pair set as the oracle."""
    from nvalchemiops.neighborlist import cell_list

    pos, cell = S.random_box(600, 20.0, seed=13, dtype=dtype)
    nm, num, sh = cell_list(_t(pos), 5.0, _t(cell), torch.tensor([True] * 3, device=DEV), max_neighbors=96)
    onm, onum, osh = O.cell_list(pos, 5.0, cell, [True] * 3, max_neighbors=96)
    assert int(num.max()) < 96 and np.array_equal(num.cpu().numpy(), onum)
    assert np.array_equal(O.canonical_pairs(nm.cpu().numpy(), num.cpu().numpy(), sh.cpu().numpy()), O.canonical_pairs(onm, onum, osh))


def test_step_is_hip_graph_capturable():
    """The matrix-format step (nlist -> D3, nlist -> PME) makes no host sync and no allocation outside torch's allocator, so it
    can be captured into a hipGraph (torch.cuda.graph) and replayed on new positions written into the captured input buffer."""
    from nvalchemiops.interactions.dispersion import D3Parameters, dftd3
    from nvalchemiops.interactions.electrostatics import particle_mesh_ewald
    from nvalchemiops.neighborlist import cell_list

    n = 1500
    pos, cell, q, z = S.fcc_box(n, dtype=np.float64)
    g = np.random.default_rng(0)
    tp, tc, tq, tz = _t(pos), _t(cell), _t(q), _t(z)
    pbc = torch.tensor([True] * 3, device=DEV)
    t = O.d3_test_tables(17)
    prm = D3Parameters(rcov=_t(t["rcov"]), r4r2=_t(t["r4r2"]), c6ab=_t(t["c6ab"]), cn_ref=_t(t["cn_ref"]))
    nm = torch.empty((n, 160), dtype=torch.int32, device=DEV)
    sh = torch.empty((n, 160, 3), dtype=torch.int32, device=DEV)
    num = torch.empty(n, dtype=torch.int32, device=DEV)

    def step():
        cell_list(tp, 7.0, tc, pbc, neighbor_matrix=nm, neighbor_matrix_shifts=sh, num_neighbors=num)
        e, f, cn = dftd3(tp.float() * 1.8897, tz, 0.4289, 4.4407, 0.7875, d3_params=prm, neighbor_matrix=nm, neighbor_matrix_shifts=sh,
                         cell=tc.float()[None] * 1.8897, fill_value=n, num_systems=1)
        ep, fp = particle_mesh_ewald(tp, tq, tc, alpha=0.4, mesh_dimensions=(32, 32, 32), spline_order=4, neighbor_matrix=nm,
                                     neighbor_matrix_shifts=sh, compute_forces=True)
        return e, f, ep, fp

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on a side stream, as torch's graph recipe prescribes
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    moved = pos + g.normal(0, 0.05, pos.shape)
    tp.copy_(_t(moved))
    graph.replay()
    torch.cuda.synchronize()
    got = [o.clone() for o in out]
    ref = step()  # eager, same (moved) positions
    assert int(num.max()) < 160
    for a, b in zip(got, ref):
        torch.testing.assert_close(a, b, rtol=1e-6, atol=1e-9)


@pytest.mark.parametrize("seed", range(12))
def test_randomised_geometry_sweep(seed):
    """Seeded sweep over shapes the fixed cases do not pin down: random triclinic cells, random pbc flags, densities from sparse to
    dense (so that the wave-per-atom, the block-per-cell and the multi-image paths are all selected), batches with tiny / empty
    systems, fp32 and fp64, matrix and direct-CSR output, half lists -- every pair set bit-exact against the oracle (which bins with
    the reference's own rule, not this library's)."""
    from nvalchemiops.neighborlist import batch_cell_list, cell_list

    g = np.random.default_rng(1000 + seed)
    dtype = np.float64 if seed % 2 else np.float32
    nsys = int(g.integers(1, 5))
    parts, cells, pbcs, bis = [], [], [], []
    for s in range(nsys):
        n = int(g.choice([0, 1, 7, 60, 250, 700])) if nsys > 1 else int(g.choice([40, 300, 900]))
        box = float(g.uniform(5.0, 14.0))
        cell = np.diag(g.uniform(0.8, 1.2, 3) * box)
        if g.uniform() < 0.6:
            cell[1, 0], cell[2, 0], cell[2, 1] = g.uniform(-0.3, 0.3, 3) * box
        frac = g.uniform(-0.5, 1.5, (n, 3))  # some atoms outside the cell
        parts.append((frac @ cell).astype(dtype)), cells.append(cell.astype(dtype))
        pbcs.append(g.uniform(size=3) < 0.7), bis.append(np.full(n, s, np.int32))
    pos, cell, pbc, bi = np.concatenate(parts), np.stack(cells), np.array(pbcs), np.concatenate(bis)
    if len(pos) == 0:
        return
    cutoff = float(g.uniform(1.5, 6.5))
    half = bool(seed % 3 == 0)
    m = 1024
    if nsys > 1:
        onm, onum, osh = O.cell_list(pos, cutoff, cell, pbc, batch_idx=bi, max_neighbors=m, half_fill=half)
        nm, num, sh = batch_cell_list(_t(pos), cutoff, _t(cell), _t(pbc), _t(bi), max_neighbors=m, half_fill=half)
        lst, ptr, lsh = batch_cell_list(_t(pos), cutoff, _t(cell), _t(pbc), _t(bi), return_neighbor_list=True, half_fill=half, max_neighbors=m)
    else:
        onm, onum, osh = O.cell_list(pos, cutoff, cell[0], pbc[0], max_neighbors=m, half_fill=half)
        nm, num, sh = cell_list(_t(pos), cutoff, _t(cell[0]), _t(pbc[0]), max_neighbors=m, half_fill=half)
        lst, ptr, lsh = cell_list(_t(pos), cutoff, _t(cell[0]), _t(pbc[0]), return_neighbor_list=True, half_fill=half, max_neighbors=m)
    assert onum.max() <= m, "test sizing"
    if half:  # the half list keeps ONE direction per pair by different rules: compare undirected pairs
        def undirected(rows):
            flip = rows[:, 0] > rows[:, 1]
            r = rows.copy()
            r[flip, 0], r[flip, 1] = rows[flip, 1], rows[flip, 0]
            r[flip, 2:] *= -1
            same = (r[:, 0] == r[:, 1])
            neg = same & ((r[:, 2] < 0) | ((r[:, 2] == 0) & (r[:, 3] < 0)) | ((r[:, 2] == 0) & (r[:, 3] == 0) & (r[:, 4] < 0)))
            r[neg, 2:] *= -1
            return r[np.lexsort(r.T[::-1])]
        assert np.array_equal(undirected(_pairs(nm, num, sh)), undirected(O.canonical_pairs(onm, onum, osh)))
        assert int(num.sum()) == int(onum.sum()) == lst.shape[1]
    else:
        assert np.array_equal(num.cpu().numpy(), onum)
        assert np.array_equal(_pairs(nm, num, sh), O.canonical_pairs(onm, onum, osh))
        # direct CSR: same rows
        coo = np.column_stack([lst[0].cpu().numpy(), lst[1].cpu().numpy(), lsh.cpu().numpy()]).astype(np.int64)
        assert np.array_equal(coo[np.lexsort(coo.T[::-1])], O.canonical_pairs(onm, onum, osh))
        assert np.array_equal(np.diff(ptr.cpu().numpy()), onum)
