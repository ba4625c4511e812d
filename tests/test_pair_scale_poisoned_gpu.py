"""The parity tests of `pair_scale_correction` (tests/test_pair_scale_gpu.py), run again on POISONED scratch: no kernel may read memory that
nothing has written.

The mechanism is that of tests/test_poisoned_scratch_gpu.py: every `torch.empty`, `torch.empty_like` and `Tensor.new_empty` block is filled
first (tests/poison.py: NaN in floating tensors, 1 in integer tensors, 0xFF in every byte of a byte workspace -- here the record scratch and
the per-row virials of the pair kernel, its outputs and the virial block partials), and the home module's own comparisons run unchanged:
every test below IS a test function of the home module under a new name, with its reference and its bar.  Every case asserts at teardown
that at least one poisoned allocation was made on the device while it ran.  A device error ends the session (tests/poison.py
`device_guard`)."""
import pytest

from tests import poison
from tests import test_pair_scale_gpu as TPS

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _poisoned_scratch(request):
    with poison.poisoned_case(request.node.nodeid) as state:
        yield state


@pytest.fixture(scope="module", autouse=True)
def _references():
    """The float64 references of the home module, evaluated BEFORE the poison starts (a module-scoped fixture is set up before the
    function-scoped one); they are the home module's own, computed once for both (`functools.lru_cache`)."""
    f32, f64 = TPS.torch.float32, TPS.torch.float64
    for kind in TPS.LADDERS:
        TPS._reference(kind)
        TPS._reference(kind, f32)
    for kind in ("ladder70", "molecules"):
        TPS._reference(kind, f32)
    for kind in ("periodic", "molecules"):
        TPS._reference(kind)
    TPS._reference("molecules", weighted=True)
    TPS._reference("molecules", f32, minimum_image=True)
    for mu, Q in ((False, True), (True, False), (False, False)):
        TPS._reference("ladder33", mu=mu, Q=Q)


for _name in """c_abi_every_flag_word_against_the_yardstick c_abi_null_dipoles_and_quadrupoles c_abi_weights_give_the_adjoint_and_energies_may_be_null
        group_ladder_and_partial_blocks_through_the_public_function missing_multipoles fused_equals_the_composed_existing_operators
        periodic_triclinic_cell_with_the_nine_word_virial minimum_image_equals_explicit_shifts_wrapped_or_not""".split():
    globals()[f"test_pair_scale__{_name}"] = getattr(TPS, "test_" + _name)
del _name
