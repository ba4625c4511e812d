"""The parity tests of the cluster multipole operators (tests/test_cluster_multipole_gpu.py), run again on POISONED scratch: no kernel may read
memory that nothing has written.

The mechanism is that of tests/test_poisoned_scratch_gpu.py: every `torch.empty`, `torch.empty_like` and `Tensor.new_empty` block is filled
first (tests/poison.py: NaN in floating tensors, 1 in integer tensors, 0xFF in every byte of a byte workspace -- the record scratch and the
per-row virials of the pair kernels, the stored tensors, the solver's vectors, states and block partials), and the home module's own
comparisons run unchanged: every test below IS a test function of the home module under a new name, with its reference and its bar.  Every
case asserts at teardown that at least one poisoned allocation was made on the device while it ran.  A device error ends the session
(tests/poison.py `device_guard`)."""
import pytest

from tests import poison
from tests import test_cluster_multipole_gpu as TCM

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _poisoned_scratch(request):
    with poison.poisoned_case(request.node.nodeid) as state:
        yield state


@pytest.fixture(scope="module", autouse=True)
def _references():
    """The float64 references of the home module, evaluated BEFORE the poison starts (a module-scoped fixture is set up before the
    function-scoped one); they are the home module's own, computed once for both (`functools.lru_cache`)."""
    for which in ("dipole", "quadrupole"):
        for kind in ("c150", "batch"):
            for dtype in (TCM.torch.float64, TCM.torch.float32):
                TCM._reference(which, kind, dtype)
            TCM._reference(which, kind, TCM.torch.float64, True)
        for weighted in (False, True):
            TCM._reference(which, "periodic", TCM.torch.float64, weighted)
    for kind in ("c150", "batch"):
        for damped in (False, True):
            TCM._solver_case(kind, damped)


for _name in """c_abi_every_flag_combination_against_the_reference c_abi_weights_give_the_adjoint_and_energies_may_be_null
        public_function_outputs_and_adjoint periodic_cut_off_sum_with_the_nine_word_virial
        stored_tensors_against_the_reference_and_the_pair_kernels solve_against_the_dense_reference""".split():
    globals()[f"test_cluster__{_name}"] = getattr(TCM, "test_" + _name)
del _name
