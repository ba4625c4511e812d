"""tests/poison.py without a device: the three replaced allocation calls keep everything about the tensor but its contents, hold the stated
poison for every dtype the package allocates, let `meta` and empty tensors through and are undone on exit; every comparison the poisoned
module (tests/test_poisoned_scratch_gpu.py) relies on rejects a result that is NaN throughout; and the package has no other spelling of an
uninitialised allocation than the three that are replaced."""
import ast
import glob
import os
import types

import numpy as np
import pytest
import torch

from tests import poison

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nvalchemi-toolkit-ops_amd", "nvalchemiops")
FLOATS = [torch.float16, torch.bfloat16, torch.float32, torch.float64]
DTYPES = FLOATS + [torch.complex64, torch.complex128, torch.int16, torch.int32, torch.int64, torch.bool, torch.uint8, torch.int8]


def _holds_poison(t):
    if t.dtype.is_complex:
        return bool(torch.isnan(t.real).all() and torch.isnan(t.imag).all())
    if t.dtype.is_floating_point:
        return bool(torch.isnan(t).all())
    if t.dtype == torch.bool:
        return bool(t.all())
    if t.dtype in (torch.uint8, torch.int8):
        return bool((t.view(torch.uint8) == 0xFF).all())
    return bool((t == 1).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_the_three_replacements_keep_the_tensor_and_fill_it(dtype):
    base = torch.zeros((4, 6, 5), dtype=dtype)
    strided = base.transpose(0, 2)  # dense, not contiguous: empty_like preserves these strides
    with poison.poisoned() as state:
        made = [
            (torch.empty((3, 5), dtype=dtype), (3, 5), (5, 1)),
            (torch.empty(7, dtype=dtype, device="cpu"), (7,), (1,)),
            (torch.empty_like(base), (4, 6, 5), (30, 5, 1)),
            (torch.empty_like(strided), (5, 6, 4), strided.stride()),
            (torch.empty_like(strided, memory_format=torch.contiguous_format), (5, 6, 4), (24, 4, 1)),
            (base.new_empty((2, 3)), (2, 3), (3, 1)),
            (base.new_empty((2, 3), dtype=torch.float64 if dtype != torch.float64 else torch.int32), (2, 3), (3, 1)),
            (torch.empty((2, 3, 4, 5), dtype=dtype, memory_format=torch.channels_last), (2, 3, 4, 5), (60, 1, 15, 3)),
        ]
        for i, (t, shape, stride) in enumerate(made):
            want = dtype if i != 6 else (torch.float64 if dtype != torch.float64 else torch.int32)
            assert t.dtype == want and tuple(t.shape) == shape and tuple(t.stride()) == tuple(stride) and t.device.type == "cpu", (i, t.dtype, t.shape, t.stride())
            assert _holds_poison(t), (i, t)
        assert state.counts["cpu"] == len(made) and state.counts["cuda"] == 0
    assert torch.empty_like(strided).stride() == strided.stride()


def test_byte_workspaces_read_minus_one_as_int32_and_nan_as_float():
    with poison.poisoned():
        ws = torch.empty(64, dtype=torch.uint8)
    assert bool((ws.view(torch.int32) == -1).all()) and bool(torch.isnan(ws.view(torch.float32)).all()) and bool(torch.isnan(ws.view(torch.float64)).all())
    # no poison is a large positive integer: an index read from unwritten memory stays at or below 1
    with poison.poisoned():
        assert int(torch.empty(4, dtype=torch.int64).max()) == 1 and int(torch.empty(4, dtype=torch.int8).max()) == -1


def test_meta_and_empty_tensors_pass_through_and_requires_grad_survives():
    with poison.poisoned() as state:
        m = torch.empty((3, 4), device="meta")
        assert m.is_meta and m.shape == (3, 4)
        assert torch.empty_like(m).is_meta and m.new_empty((2,)).is_meta
        z = torch.empty((0, 3), dtype=torch.float64)
        assert z.shape == (0, 3) and torch.zeros(5).new_empty((0,)).numel() == 0
        assert not state.counts
        g = torch.empty(3, dtype=torch.float64, requires_grad=True)
        assert g.requires_grad and g.is_leaf and _holds_poison(g.detach())
        assert state.counts["cpu"] == 1


def test_torch_itself_works_under_the_replacements():
    with poison.poisoned():
        a = torch.arange(12.0, dtype=torch.float64).reshape(3, 4)
        assert torch.allclose(torch.linalg.pinv(a) @ a @ torch.linalg.pinv(a), torch.linalg.pinv(a))
        x = torch.randn(8, 6, dtype=torch.float64)
        assert torch.allclose(torch.fft.irfftn(torch.fft.rfftn(x), s=x.shape), x)
        lin = torch.nn.Linear(4, 3)
        lin(torch.randn(5, 4)).sum().backward()
        assert bool(torch.isfinite(lin.weight.grad).all())


def test_the_originals_are_back_on_exit_also_after_an_exception():
    before = (torch.empty, torch.empty_like, torch.Tensor.new_empty)
    with poison.poisoned():
        assert torch.empty is not before[0] and torch.empty_like is not before[1] and torch.Tensor.new_empty is not before[2]
    assert (torch.empty, torch.empty_like, torch.Tensor.new_empty) == before
    with pytest.raises(KeyError):
        with poison.poisoned():
            raise KeyError("inside")
    assert (torch.empty, torch.empty_like, torch.Tensor.new_empty) == before
    with pytest.raises(BaseException):
        with poison.poisoned_case("a case without allocations", device_type="cpu"):
            pass
    assert (torch.empty, torch.empty_like, torch.Tensor.new_empty) == before
    with poison.poisoned_case("a case with one", device_type="cpu") as state:
        torch.empty(3)
    assert state.counts["cpu"] == 1


def test_an_unknown_dtype_is_refused_not_passed_through_unpoisoned():
    with pytest.raises(TypeError):
        poison.poison_(torch.zeros(4, dtype=torch.uint8).view(torch.uint16))


def test_device_errors_are_told_from_ordinary_ones():
    assert poison.is_device_fault(RuntimeError("HIP error: an illegal memory access was encountered"))
    assert poison.is_device_fault(RuntimeError("Memory access fault by GPU node-2"))
    assert not poison.is_device_fault(RuntimeError("shape mismatch")) and not poison.is_device_fault(ValueError("hip"))


# ---- every comparison of the poisoned module rejects a result that is NaN throughout ------------------------------------------------------------

def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float64)


def _comparisons(monkeypatch):
    """(label, call) for every `_close`, `_check`, `_judge`, `_same`, `_check_solution`, `_bitwise` of the modules the poisoned module draws from
    and the `_close_*` factories of tests/test_arg_layouts_gpu.py: each is handed NaN where the kernel's result goes and a finite reference."""
    from tests import induced_reference as IR
    from tests import test_arg_layouts_gpu as TL
    from tests import test_coulomb_gpu as TC
    from tests import test_d3_atm_gpu as TATM
    from tests import test_d3_gpu as TD3
    from tests import test_d3_zero_atm_gpu as TZA
    from tests import test_d3_zero_gpu as TZ
    from tests import test_d4_atm_gpu as TD4A
    from tests import test_d4_gpu as TD4
    from tests import test_dipole_gpu as TDP
    from tests import test_electrostatic_virial_gpu as TV
    from tests import test_ewald_full_list_gpu as TF
    from tests import test_fold_sizes_gpu as TFS
    from tests import test_gaussian_charges_gpu as TG
    from tests import test_induced_gpu as TI
    from tests import test_pme_dipole_gpu as TPD
    from tests import test_pme_gpu as TP
    from tests import test_qeq_gpu as TQ
    from tests import test_quadrupole_gpu as TQD
    from tests import test_search_cn_gpu as TS
    from tests import test_spline_channels_gpu as TCH
    from tests import test_thole_gpu as TTH

    for m in (TQ, TI, TTH, TF):
        monkeypatch.setattr(m, "DEV", "cpu")
    ref = np.linspace(1.0, 2.0, 12).reshape(4, 3)
    tref = torch.as_tensor(ref)
    got = _nan(4, 3)
    out = [("coulomb._close", lambda: TC._close(got, ref, "x")),
           ("d3._close", lambda: TD3._close(got, ref, 1e-6, 1e-6, "x")),
           ("d3._check", lambda: TD3._check((got, got, got, got), (ref, ref, ref, ref), virial=True)),
           ("search_cn._close", lambda: (_ for _ in ()).throw(AssertionError) if not TS._close(got, ref) else None),
           ("pme._close f64", lambda: TP._close(got, ref, np.float64, "x")),
           ("pme._close f32", lambda: TP._close(got.float(), ref.astype(np.float32), np.float32, "x")),
           ("channels._close", lambda: TCH._close(got, tref, np.float64, "x")),
           ("virial._close", lambda: TV._close(got, tref, 1e-9, "x")),
           ("virial._same", lambda: TV._same(got, tref)),
           ("full_list._same", lambda: TF._same((got, got, got), (tref, tref, tref), np.float64, "x", 1.0)),
           ("gaussian._close", lambda: TG._close(got, ref, "x")),
           ("dipole._close", lambda: TDP._close(got, ref, "x")),
           ("quadrupole._close", lambda: TQD._close(got, ref, "x")),
           ("pme_dipole._close", lambda: TPD._close(got, ref, "x", 1e-9)),
           ("thole._close", lambda: TTH._close(got, ref, "x", 1e-9)),
           ("fold._bitwise", lambda: TFS._bitwise(_nan(8, 3), tref, 2, "x")),
           ("fold._fold_close", lambda: TFS._fold_close(got, tref, tref, "x")),
           ("fold._check_copies", lambda: TFS._check_copies("x", (tref, tref[:1]), (tref.repeat(2, 1), _nan(1, 3)), [], 2, (0,), 1)),
           ("layouts._close_d3", lambda: TL._close_d3((0.0, 5e-6))(got, ref, "x", 1)),
           ("layouts._close_pme", lambda: TL._close_pme(np.float64)(got, ref, "x", 0)),
           ("layouts._close_bars", lambda: TL._close_bars({"forces": (np.full((4, 3), 1e-6),)}, ("forces",))(got, ref, "x", 0)),
           ("layouts._close_gaussian", lambda: TL._close_gaussian(1e-11)(got, ref, "x", 0)),
           ("layouts._close_two_runs", lambda: TL._close_two_runs(1e-9)(got, ref, "x", 0))]
    r3 = {k: ref for k in ("energy", "forces", "virial")}
    l3 = {k: ref + 1e-7 for k in r3}
    for name, mod in (("d3_atm", TATM), ("d3_zero_atm", TZA), ("d4_atm", TD4A)):
        out.append((f"{name}._judge", lambda mod=mod: mod._judge("x", (got, got, got), r3, l3)))
    r5 = {k: ref for k in TD4.KEYS}
    l5 = {k: ref + 1e-7 for k in r5}
    out.append(("d4._judge", lambda: TD4._judge("x", (got,) * 5, r5, l5)))
    r4 = {k: ref for k in ("energy", "forces", "cn", "virial")}
    out.append(("d3_zero._judge", lambda: TZ._judge("x", (got,) * 4, r4, {k: ref + 1e-7 for k in r4})))
    # the solves: a dense positive definite H, a right-hand side, and NaN where the solution goes
    n = 4
    H = torch.eye(3 * n, dtype=torch.float64) * 2.0
    b = torch.linspace(1.0, 2.0, 3 * n, dtype=torch.float64)
    polar = torch.ones(n, dtype=torch.float64)
    bi = torch.zeros(n, dtype=torch.int32)
    sol = types.SimpleNamespace(dipoles=_nan(n, 3), iterations=torch.tensor([3]), residual=torch.tensor([0.0]))
    out.append(("induced._check_solution", lambda: TI._check_solution(sol, H, b, polar, bi, 1, 1e-10, "x")))
    out.append(("thole._check_solution", lambda: TTH._check_solution(sol, H, b, polar, bi, 1, 1e-10, "x")))
    qsol = types.SimpleNamespace(charges=_nan(n), iterations=torch.tensor([3]), residual=torch.tensor([0.0]), chemical_potential=torch.tensor([0.0], dtype=torch.float64))
    hq = torch.eye(n, dtype=torch.float64) * 2.0
    out.append(("qeq._check_solution", lambda: TQ._check_solution(qsol, hq, torch.linspace(0.1, 0.4, n, dtype=torch.float64), 0.0, bi, 1, 1e-10, 50, "x")))
    assert IR is not None
    return out


def test_every_comparison_of_the_selected_tests_rejects_an_all_nan_result(monkeypatch):
    blind = []
    for label, call in _comparisons(monkeypatch):
        try:
            call()
        except AssertionError:
            continue
        blind.append(label)
    assert not blind, f"comparisons that accept NaN for a result: {blind}"


def test_the_comparisons_accept_the_reference_itself(monkeypatch):
    """The other half: the table above fails for NaN, not because its calls are malformed."""
    from tests import test_coulomb_gpu as TC
    from tests import test_d3_gpu as TD3
    from tests import test_fold_sizes_gpu as TFS
    from tests import test_pme_gpu as TP
    from tests import test_search_cn_gpu as TS

    ref = np.linspace(1.0, 2.0, 12).reshape(4, 3)
    t = torch.as_tensor(ref)
    TC._close(t, ref, "x")
    TD3._check((t, t, t, t), (ref, ref, ref, ref), virial=True)
    TP._close(t, ref, np.float64, "x")
    assert TS._close(t, ref)
    TFS._bitwise(t.repeat(2, 1), t, 2, "x")


# ---- the package allocates uninitialised memory through the three replaced calls only ------------------------------------------------------------

def _package_sources():
    files = sorted(glob.glob(os.path.join(PKG, "**", "*.py"), recursive=True))
    assert len(files) > 30
    return [(f, ast.parse(open(f).read(), filename=f)) for f in files]


def test_no_other_spelling_of_an_uninitialised_allocation_in_the_package():
    """Every call whose name contains `empty` or `resize` is `torch.empty`, `torch.empty_like`, `<tensor>.new_empty`, `torch.cuda.empty_cache`
    or a helper the package defines itself (whose body this walk covers too).  A new spelling -- `torch.empty_strided`, `resize_`,
    `from torch import empty` -- would allocate past the fixture of the poisoned module unnoticed: it fails here first."""
    sources = _package_sources()
    own = set()
    for _, tree in sources:
        for node in ast.walk(tree):
            if isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef)):
                own.add(node.name)
            elif isinstance(node, ast.Assign) and isinstance(node.value, ast.Lambda):
                own.update(t.id for t in node.targets if isinstance(t, ast.Name))
    assert not {"empty", "empty_like", "new_empty", "empty_strided", "new_empty_strided"} & (own - {"empty"}), own
    counts = {"empty": 0, "empty_like": 0, "new_empty": 0}
    bad = []
    for f, tree in sources:
        where = os.path.relpath(f, PKG)
        for node in ast.walk(tree):
            if isinstance(node, ast.ImportFrom) and (node.module or "").split(".")[0] == "torch":
                bad += [f"{where}:{node.lineno} from {node.module} import {a.name}" for a in node.names if "empty" in a.name or "resize" in a.name]
            if (isinstance(node, ast.Assign) and isinstance(node.value, ast.Attribute) and ("empty" in node.value.attr or "resize" in node.value.attr)
                    and not (node.value.attr == "new_empty" and node not in tree.body)):
                # `e = torch.empty` is looked up once, not per call (a local `new = positions.new_empty` is looked up on every call of its function)
                bad.append(f"{where}:{node.lineno} binds {ast.unparse(node.value)} to a name")
            if not isinstance(node, ast.Call):
                continue
            fn = node.func
            name = fn.attr if isinstance(fn, ast.Attribute) else fn.id if isinstance(fn, ast.Name) else ""
            if "empty" not in name and "resize" not in name:
                continue
            text = ast.unparse(fn)
            if text in ("torch.empty", "torch.empty_like"):
                counts[name] += 1
            elif isinstance(fn, ast.Attribute) and name == "new_empty":
                counts[name] += 1
            elif text == "torch.cuda.empty_cache" or (name in own and name not in counts) or (isinstance(fn, ast.Name) and name == "empty" and "empty" in own):
                continue  # the package's own helpers: `empty_result`, `_empty_result`, the local `empty = lambda: x.new_empty((0,))`
            else:
                bad.append(f"{where}:{node.lineno} {text}(...)")
    assert not bad, "allocation spellings tests/poison.py does not replace:\n" + "\n".join(bad)
    assert counts["empty"] > 100 and counts["new_empty"] > 50 and counts["empty_like"] > 10, counts


def test_the_local_empty_helpers_are_new_empty_lambdas():
    """The one bare-name `empty()` the walk above lets through: it must stay a lambda over `new_empty`."""
    for f, tree in _package_sources():
        for node in ast.walk(tree):
            if isinstance(node, ast.Assign) and any(isinstance(t, ast.Name) and t.id == "empty" for t in node.targets):
                text = ast.unparse(node.value)
                assert (isinstance(node.value, ast.Lambda) and ".new_empty(" in text) or text.startswith("torch.zeros("), (f, node.lineno, text)


def test_the_poisoned_module_takes_every_fold_size_test_and_has_no_name_twice():
    from tests import test_fold_sizes_gpu as TFS
    from tests import test_poisoned_scratch_gpu as TPS

    taken = {getattr(TPS, n) for n in dir(TPS) if n.startswith("test_fold__")}
    missing = [n for n in dir(TFS) if n.startswith("test_") and getattr(TFS, n) not in taken]
    # (the one fold test that hands the C entry points the test's own zeroed buffers: no allocation of the package's, nothing to poison)
    assert missing == ["test_induced_dot_and_apply_partials_beyond_one_trip"], missing
    names = [n for n in dir(TPS) if n.startswith("test_")]
    assert len(names) > 150 and all("__" in n for n in names)
    assert TPS._poisoned_scratch is not None and TPS.pytestmark.name == "gpu"
