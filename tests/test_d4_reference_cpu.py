"""The restatement tests/d4_reference.py checked on its own, without a GPU: its autograd derivatives against central differences, its
one-reference / ga = 0 limit against the DFT-D3 restatement, the max-shifted weights far from every reference, and the condition the
synthetic tables must meet on the systems the GPU module compares (otherwise the weight derivatives would not be exercised)."""
import numpy as np
import pytest
import torch

from tests import atm_reference as A
from tests import d4_cases as K
from tests import d4_reference as R
from tests import systems as S

H = 1e-4
# central differences with step H on an energy E of smooth terms: truncation ~ H^2 |E'''| / 6 ~ 1e-8 x (a few inverse lengths cubed x |E'|)
# and rounding ~ 1e-16 |E| / H ~ 1e-12 |E|; the bar below leaves two orders of magnitude over what the definition measured (1.4e-11)
FD_RTOL, FD_ATOL = 1e-6, 1e-9


def _setup():
    c = K.case("triclinic_f32")
    pos, cell = c["pos"].astype(np.float64), c["cell"].astype(np.float64)
    pairs = A.enumerate_pairs(pos, cell, c["rc"])
    kw = dict(list_cutoff=c["rc"], pairs=pairs, **K.BJ)
    energy = lambda p, q, h: R.reference(p, c["z"], q, c["tables"], cell=h, **kw)["energy"][0]  # noqa: E731
    base = R.reference(pos, c["z"], c["q"], c["tables"], cell=cell, **kw)
    return c, pos, cell, energy, base


def test_forces_charge_gradients_and_virial_equal_central_differences():
    c, pos, cell, energy, base = _setup()
    q = c["q"].astype(np.float64)
    n = len(pos)
    assert n == 18 and abs(base["energy"][0]) > 0
    worst = {}
    fd = np.zeros((n, 3))
    for i in range(n):
        for k in range(3):
            d = np.zeros_like(pos); d[i, k] = H
            fd[i, k] = -(energy(pos + d, q, cell) - energy(pos - d, q, cell)) / (2 * H)
    worst["forces"] = np.abs(fd - base["forces"]).max()
    assert worst["forces"] <= FD_ATOL + FD_RTOL * np.abs(base["forces"]).max()
    fq = np.zeros(n)
    for i in range(n):
        d = np.zeros(n); d[i] = H
        fq[i] = (energy(pos, q + d, cell) - energy(pos, q - d, cell)) / (2 * H)
    worst["charge_grad"] = np.abs(fq - base["charge_grad"]).max()
    assert np.abs(base["charge_grad"]).max() > 0
    assert worst["charge_grad"] <= FD_ATOL + FD_RTOL * np.abs(base["charge_grad"]).max()
    fv = np.zeros((3, 3))
    for a in range(3):
        for b in range(a, 3):
            e = np.zeros((3, 3)); e[a, b] = e[b, a] = 0.5 * H if a != b else H
            up, dn = np.eye(3) + e, np.eye(3) - e
            fv[a, b] = fv[b, a] = -(energy(pos @ up, q, cell @ up) - energy(pos @ dn, q, cell @ dn)) / (2 * H)
    worst["virial"] = np.abs(fv - base["virial"][0]).max()
    assert worst["virial"] <= FD_ATOL + FD_RTOL * np.abs(base["virial"]).max()
    print("central differences vs autograd:", {k: f"{v:.2e}" for k, v in worst.items()})


def test_one_reference_limit_is_dftd3_two_body():
    c = K.case("d3_limit")
    t4 = c["tables"]
    d3 = {k: v.copy() for k, v in S.d3_test_tables(17, seed=1000).items()}
    np.testing.assert_array_equal(d3["rcov"], t4["rcov"])
    d3["c6ab"] = np.broadcast_to(t4["c6_ref"][:, :, 0, 0][:, :, None, None], d3["c6ab"].shape).copy()
    got = R.reference(c["pos"], c["z"], c["q"], t4, list_cutoff=c["rc"], cell=c["cell"], **K.BJ, **c["kw"])
    want = A.reference(c["pos"], c["z"], d3, K.BJ["a1"], K.BJ["a2"], c["rc"], s8=K.BJ["s8"], cell=c["cell"], term="two_body")
    for k in ("energy", "forces", "virial"):
        scale = np.abs(want[k]).max()
        assert scale > 0
        err = np.abs(got[k] - want[k]).max()
        print(f"D3 limit {k}: {err:.2e} on {scale:.2e}")
        assert err <= 1e-12 * scale + 1e-15, k
    assert np.abs(got["charge_grad"]).max() == 0.0  # ga = 0: no charge dependence left


def test_max_shifted_weights_sum_to_one_far_from_every_reference():
    t = R.d4_test_tables(17)
    z = torch.arange(1, 18)
    for wd in (torch.float64, torch.float32):
        W, mask = R.gaussian_weights(torch.full((17,), 50.0, dtype=wd), z, t, wd=wd)
        assert bool(torch.isfinite(W).all()) and bool((W[~mask] == 0).all())
        assert float((W.sum(1) - 1.0).abs().max()) <= 4 * torch.finfo(wd).eps
    # the unshifted form is 0 / 0 there: exp(-6 * 49^2) underflows in either dtype
    assert float(torch.exp(torch.tensor(-6.0 * 49.0 ** 2, dtype=torch.float64))) == 0.0


def test_test_tables_have_the_stated_structure():
    t = R.d4_test_tables(17)
    assert t["n_ref"][R.ONE_REF_Z] == 1 and t["n_ref"][R.SEVEN_REF_Z] == 7 and t["n_ref"][0] == 0
    assert 1 <= t["n_ref"][1:].min() and t["n_ref"].max() == 7 and set(np.unique(t["ngw"])) == {1, 3}
    c6 = t["c6_ref"]
    used = ~np.isnan(c6)
    assert np.isnan(t["cn_ref"][R.ONE_REF_Z, 1:]).all() and np.isnan(c6[R.ONE_REF_Z, :, 1:, :]).all()
    assert np.array_equal(used, used.transpose(1, 0, 3, 2))
    assert np.array_equal(c6[used], c6.transpose(1, 0, 3, 2)[used]) and (c6[used][c6[used] != 0] > 0).all()
    assert (c6[1:, 1:][used[1:, 1:]] > 0).all()


@pytest.mark.parametrize("name", K.NAMES)
def test_tables_exercise_the_weight_derivatives_on_every_gpu_case(name):
    """In every system the GPU module compares, at least half of the atoms whose element has >= 2 references have two references with
    Gaussian weight >= 0.05."""
    c = K.case(name)
    r64, _ = K.references(name)
    ok = R.valid_atoms(c["z"], c["tables"])
    bi = np.zeros(len(c["z"]), np.int64) if c["batch_idx"] is None else c["batch_idx"]
    for s in np.unique(bi):
        multi = ok & (bi == s)
        multi[multi] = c["tables"]["n_ref"][c["z"][multi]] >= 2
        if not multi.any():
            continue
        two = (r64["weights"][multi] >= 0.05).sum(1) >= 2
        print(f"{name} system {s}: {int(two.sum())} of {int(multi.sum())} multi-reference atoms have two weights >= 0.05; "
              f"CN {r64['cn'][bi == s].min():.2f} ... {r64['cn'][bi == s].max():.2f}")
        assert 2 * int(two.sum()) >= int(multi.sum()), name
