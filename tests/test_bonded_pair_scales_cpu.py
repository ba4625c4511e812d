"""`bonded_pair_scales`: the full, symmetric list of scaled pairs of a bonded topology by shortest bond path, against closed cases and against
the plain per-atom breadth-first search of tests/pair_scale_cases.py.  Host only."""
import numpy as np
import pytest
import torch

from tests import pair_scale_cases as PC


def _fn():
    from nvalchemiops.interactions.electrostatics import bonded_pair_scales

    return bonded_pair_scales


def _pairs(res):
    """{(i, j): scale} of a result, its layout checked on the way: int32 matrix padded with N, scale 1 on padding, counts, sorted rows."""
    nm, sc, num = res
    n = nm.shape[0]
    assert nm.dtype == torch.int32 and num.dtype == torch.int32 and nm.shape == sc.shape and num.shape == (n,)
    assert nm.shape[1] == (int(num.max()) if n else 0)
    out = {}
    for i in range(n):
        k = int(num[i])
        row = nm[i, :k].tolist()
        assert row == sorted(set(row)) and all(0 <= j < n and j != i for j in row)
        assert bool((nm[i, k:] == n).all()) and bool((sc[i, k:] == 1).all())
        out.update({(i, j): float(s) for j, s in zip(row, sc[i, :k].tolist())})
    return out


def test_exported_as_documented():
    import inspect

    import nvalchemiops.interactions.electrostatics as E

    assert "bonded_pair_scales" in E.__all__ and "pair_scale_correction" in E.__all__
    p = inspect.signature(E.bonded_pair_scales).parameters
    assert list(p) == ["bonds", "num_atoms", "scales", "dtype", "device"] and p["scales"].default == (0.0, 0.0, 0.4, 0.8)
    assert p["dtype"].default is torch.float64 and p["dtype"].kind is inspect.Parameter.KEYWORD_ONLY and p["device"].default is None
    res = E.bonded_pair_scales([(0, 1)], 2)
    assert res._fields == ("neighbor_matrix", "pair_scales", "num_neighbors") and res.pair_scales.dtype == torch.float64
    assert E.bonded_pair_scales([(0, 1)], 2, dtype=torch.float32).pair_scales.dtype == torch.float32


def test_a_seven_atom_chain_has_the_classes_1_2_to_1_5_and_nothing_beyond():
    got = _pairs(_fn()([(k, k + 1) for k in range(6)], 7))
    want = {(i, j): PC.AMOEBA[abs(i - j) - 1] for i in range(7) for j in range(7) if 1 <= abs(i - j) <= 4}
    assert got == want and (0, 5) not in got and (0, 6) not in got
    assert _fn()([(k, k + 1) for k in range(6)], 7).num_neighbors.tolist() == [4, 5, 6, 6, 6, 5, 4]


def test_a_five_ring_takes_the_shortest_path():
    got = _pairs(_fn()(PC.RING5, 5, scales=(0.1, 0.2, 0.3)))
    assert len(got) == 20
    for i in range(5):
        for j in range(5):
            if i != j:  # two bonds one way and three the other is a 1-3 pair
                assert got[(i, j)] == (0.1 if (i - j) % 5 in (1, 4) else 0.2)


def test_water_has_rows_of_two():
    bonds = [(3 * m, 3 * m + k) for m in range(4) for k in (1, 2)]
    res = _fn()(bonds, 12)
    assert res.neighbor_matrix.shape == (12, 2) and res.num_neighbors.tolist() == [2] * 12 and not bool(res.pair_scales.any())
    assert res.neighbor_matrix[4].tolist() == [3, 5]  # H - H through the oxygen


def test_disjoint_molecules_have_no_cross_entries_and_match_the_plain_search():
    p = PC.molecules()
    res = _fn()(torch.as_tensor(p["bonds"]), p["n"])
    got = _pairs(res)
    assert got == PC.graph_scales(p["bonds"], p["n"], PC.AMOEBA)
    owner = p["batch_idx"]
    assert all(owner[i] == owner[j] for i, j in got)
    assert all(got[(j, i)] == s for (i, j), s in got.items()), "list and scales are symmetric"


def test_a_random_graph_matches_the_plain_search():
    g = np.random.default_rng(2)
    n = 40
    bonds = np.stack([g.integers(0, n, 55), g.integers(0, n, 55)], -1)
    bonds = bonds[bonds[:, 0] != bonds[:, 1]]
    for scales in ((0.0, 0.0, 0.4, 0.8), (0.5,), (0.0, 1.0, 0.25), ()):
        got = _pairs(_fn()(bonds, n, scales=scales))
        assert got == PC.graph_scales(bonds, n, scales), scales
        assert all(got[(j, i)] == s for (i, j), s in got.items())


def test_pairs_of_scale_one_are_dropped():
    chain = [(k, k + 1) for k in range(4)]
    got = _pairs(_fn()(chain, 5, scales=(0.0, 1.0, 0.5)))
    assert set(got.values()) == {0.0, 0.5} and (0, 2) not in got and got[(0, 3)] == 0.5 and got[(0, 1)] == 0.0
    assert _fn()(chain, 5, scales=(1.0, 1.0)).neighbor_matrix.shape == (5, 0)


def test_duplicate_bonds_are_merged():
    a = _fn()([(0, 1), (1, 2)], 3)
    b = _fn()([(0, 1), (1, 0), (0, 1), (2, 1), (1, 2)], 3)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert _fn()(np.zeros((0, 2), dtype=np.int64), 3).neighbor_matrix.shape == (3, 0) and _fn()([], 0).neighbor_matrix.shape == (0, 0)


def test_error_cases():
    fn = _fn()
    with pytest.raises(ValueError, match="joins an atom to itself"):
        fn([(0, 1), (2, 2)], 3)
    for bad in ([(0, 3)], [(-1, 0)]):
        with pytest.raises(ValueError, match=r"atom indices in \[0, 3\)"):
            fn(bad, 3)
    with pytest.raises(ValueError, match=r"shape \[num_bonds, 2\]"):
        fn([(0, 1, 2)], 3)
    with pytest.raises(ValueError, match="integer"):
        fn([(0.0, 1.0)], 3)
    with pytest.raises(ValueError, match="num_atoms"):
        fn([], -1)
    with pytest.raises(ValueError, match="float32 or float64"):
        fn([(0, 1)], 2, dtype=torch.int32)
