"""The parity tests of the local-frame kernels (tests/test_local_frames_gpu.py), run again on POISONED scratch: no kernel may read memory that
nothing has written.

The mechanism is that of tests/test_poisoned_scratch_gpu.py: every `torch.empty`, `torch.empty_like` and `Tensor.new_empty` block is filled
first (tests/poison.py: NaN in floating tensors, 1 in integer tensors -- here the outputs of the rotation, the records of four 3-vectors per
atom, the local gradients, the per-atom virial rows and their block partials), and the home module's own comparisons run unchanged: every test
below IS a test function of the home module under a new name, with its reference and its bar.  Every case asserts at teardown that at least
one poisoned allocation was made on the device while it ran.  A device error ends the session (tests/poison.py `device_guard`)."""
import pytest

from tests import poison
from tests import test_local_frames_gpu as TLF

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _poisoned_scratch(request):
    with poison.poisoned_case(request.node.nodeid) as state:
        yield state


@pytest.fixture(scope="module", autouse=True)
def _references():
    """The float64 references of the home module, evaluated BEFORE the poison starts (a module-scoped fixture is set up before the
    function-scoped one); they are the home module's own, computed once for both (`functools.lru_cache`)."""
    for name in TLF.PLAIN + TLF.PERIODIC + ("unwrapped",):
        for dtype in (TLF.torch.float64, TLF.torch.float32):
            TLF._reference(name, dtype)


for _name in """rotation_adjoint_and_explicit_path_against_the_reference periodic_cells_with_the_virial_term
        wrapped_against_unwrapped_coordinates end_to_end_three_water_cluster_through_the_cluster_corrections""".split():
    globals()[f"test_frames__{_name}"] = getattr(TLF, "test_" + _name)
del _name
