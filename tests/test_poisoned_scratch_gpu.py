"""The parity tests of every operator family, run again on POISONED scratch: no kernel may read memory that nothing has written.

The package allocates every output, partial-sum table and byte workspace with `torch.empty`, `torch.empty_like` or `Tensor.new_empty` and
hands the kernels raw pointers.  In a pytest process those blocks come fresh from the driver, which hands out zeros -- the one value that
hides a forgotten clear of an accumulator, a fold that reads one partial slot more than the grid wrote, or padding that is "already" zero.
Here every such allocation is filled first (tests/poison.py: NaN in floating and complex tensors, 1 in integer tensors, True in bool, 0xFF
in every byte of a byte workspace), and the operators' own comparisons run unchanged: every test below IS a test function of its home module
(the same object under a new name, or a plain call of it with the smallest of its parameters), with the home module's oracle or float64
restatement and the home module's bar.  Nothing is compared here that is not compared there, and no bar is new.  DESIGN.md section 3.26 has
the inventory of the integer and byte allocations (who writes them, who reads them first), the selection and what the run found.

Names: `test_<family>__<name in the home module>`.  Fixtures the home modules apply to all their tests (`spread_path`, the fixed companion
policy of the chain-record tests) are applied by name to the tests that come from there: `_under(fn, fixture)` is a copy of the function
object -- same code, same globals, same parametrize marks -- that also uses the fixture.

Every case asserts at teardown that at least one poisoned allocation was made on the device while it ran; a case that makes none does not
belong in this list.  Three tests left it for that reason after the first run on the device: they hand the C entry points buffers that the
TEST allocates with `torch.zeros` (`test_qeq_gpu.py::test_coefficients_and_product_against_the_dense_reference`,
`test_induced_gpu.py::test_non_polarisable_atoms_have_identity_rows_and_empty_columns`,
`test_fold_sizes_gpu.py::test_induced_dot_and_apply_partials_beyond_one_trip`); the same kernels run on the package's own `torch.empty`
blocks in the solve tests below.  `test_dense_row_needs_more_than_one_lds_tile` of the two D3 three-body modules is left out for its time
(9 - 11 s, nearly all of it the reference on the CPU); `test_row_of_three_lds_tiles_runs_every_tile_pair_once` takes the same multi-tile path
in 3 s.  Of tests/test_sweep_pme_quadrupole_gpu.py the sweep, the knot cases, the batch test and the ladder rungs 1, apb + 1 and 33 of each
order are here (the four-mesh memset of the adjoint and its `accumulate` launch run in each): every one makes poisoned allocations and
none left the list; the restatements of the sweep seeds are evaluated by a module-scoped fixture before the poison starts.  A device error ends the session (tests/poison.py `device_guard`)."""
import types

import pytest

from tests import poison
from tests import test_autograd_gpu as TA
from tests import test_coulomb_gpu as TC
from tests import test_d3_atm_gpu as TATM
from tests import test_d3_chain_records_gpu as TCR
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
from tests import test_math_gpu as TM
from tests import test_nlist_gpu as TN
from tests import test_packed_companion_gpu as TPK
from tests import test_pme_dipole_gpu as TPD
from tests import test_pme_gpu as TP
from tests import test_qeq_gpu as TQ
from tests import test_quadrupole_gpu as TQD
from tests import test_search_cn_gpu as TS
from tests import test_spline_channels_gpu as TCH
from tests import test_sweep_multipoles_gpu as TSM
from tests import test_sweep_pme_quadrupole_gpu as TSQ
from tests import test_thole_gpu as TTH
from tests.test_search_cn_gpu import engine  # noqa: F401  (requested by name; tests/test_packed_companion_gpu.py has the same fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _poisoned_scratch(request, monkeypatch):
    """Poison, and what the neighbour engine has LEARNED forgotten: under its "auto" policy a search into a matrix shape that `dftd3` has seen
    before writes the packed companion and sums the coordination numbers itself (another summation order).  Every test here has run once
    already in its home module when the whole suite runs, so without this a test that compares bits between two list paths
    (`test_packed_list_equals_plain_walk`) meets the second-run state its home module never sees."""
    from nvalchemiops.neighborlist import _engine as E

    monkeypatch.setattr(E, "_PACKED_WANTED", set())
    monkeypatch.setattr(E, "_D3CTX_BY_SHAPE", {})
    with poison.poisoned_case(request.node.nodeid) as state:
        yield state


@pytest.fixture(params=["tile", "auto"])
def pme_spread_path(request, monkeypatch):
    """`spread_path` of tests/test_pme_gpu.py and tests/test_autograd_gpu.py: the tile pipeline forced, and the library's own policy."""
    from nvalchemiops import spline

    monkeypatch.setattr(spline, "_SPREAD_PATH", request.param)
    return request.param


@pytest.fixture(params=["tile", "atomic", "auto"])
def channels_spread_path(request, monkeypatch):
    """`spread_path` of tests/test_spline_channels_gpu.py."""
    from nvalchemiops import spline

    monkeypatch.setattr(spline, "_SPREAD_PATH", request.param)
    return request.param


@pytest.fixture
def no_companion(monkeypatch):
    """`_fixed_companion_policy` of tests/test_d3_chain_records_gpu.py."""
    from nvalchemiops.neighborlist import _engine as E

    monkeypatch.setattr(E, "_PACKED_POLICY", "0")


def _under(fn, *fixtures):
    """A copy of the test function `fn` (its code, globals, defaults and marks) that also uses the named fixtures of this module."""
    g = types.FunctionType(fn.__code__, fn.__globals__, fn.__name__, fn.__defaults__, fn.__closure__)
    g.__dict__.update(fn.__dict__)
    g.__doc__ = fn.__doc__
    g.pytestmark = list(getattr(fn, "pytestmark", [])) + [pytest.mark.usefixtures(*fixtures).mark]
    return g


def _take(family, module, names, *fixtures):
    for name in names.split():
        fn = getattr(module, "test_" + name)
        alias = f"test_{family}__{name}"
        assert alias not in globals(), alias
        globals()[alias] = _under(fn, *fixtures) if fixtures else fn


# ---- neighbour lists ------------------------------------------------------------------------------------------------------------------------------

_take("nlist", TN, """cell_list_matches_oracle batch_matches_oracle_and_single coo_output coo_conversion_follows_the_mask_not_the_counts
      half_fill_and_overflow naive_matches_oracle query_api_and_preallocated_buffers empty_and_tiny_inputs rebuild_detection
      dual_cutoff_and_batch_naive dual_cutoff_is_one_sweep_with_the_image_table_of_the_long_cutoff box_exact_multiple_of_cutoff""")


@pytest.mark.parametrize("seed", range(6))  # wave-per-atom, block-per-cell and multi-image kernels
def test_nlist__randomised_geometry_sweep(seed):
    TN.test_randomised_geometry_sweep(seed)


_take("search_cn", TS, "search_cn_equals_the_oracle_pass search_cn_triclinic_batch")
_take("packed", TPK, "companion_words_describe_the_matrix d3_with_and_without_the_companion_is_bit_identical batch_companion")

# ---- dispersion -----------------------------------------------------------------------------------------------------------------------------------

_take("d3", TD3, """golden_ne2_hcl small_molecules_and_edge_cases small_cases_against_the_reference_order_oracle_at_the_reference_tolerance
      periodic_with_virial batch_equals_individual_and_oracle c6_table_structures more_than_16_species_uses_global_table
      out_of_range_indices_are_padding packed_list_equals_plain_walk""")
_take("d3_atm", TATM, """molecules_matrix_and_csr general_tables_and_more_than_16_species periodic_boxes_energy_forces_virial
      small_cell_own_images_and_repeated_neighbours batch_of_three_systems row_of_three_lds_tiles_runs_every_tile_pair_once""")
_take("d3_zero", TZ, """molecules_matrix_and_csr tables_that_do_not_factorise_and_more_than_16_species periodic_boxes_energy_forces_virial
      periodic_matrix_with_the_other_table_paths small_cell_own_images batch_of_three_systems
      packed_companion_and_search_side_coordination_numbers""")
_take("d3_zero_atm", TZA, """molecules_matrix_and_csr general_tables_more_than_16_species_and_missing_radii periodic_boxes_energy_forces_virial
      batch_of_three_systems row_of_three_lds_tiles_runs_every_tile_pair_once""")
_take("d4", TD4, """molecules_matrix_and_csr padding_atoms_fill_values_and_wide_matrix species_count_at_and_beyond_the_lds_slots
      triclinic_box_with_virial cell_shorter_than_the_cutoff_self_images batch_of_three_systems_one_of_them_a_single_atom
      zero_float64_and_strongly_negative_charges backward_gives_minus_forces_and_charge_gradients
      charge_equilibration_into_dftd4_total_gradient""")
_take("d4_atm", TD4A, """every_case_matrix_and_csr_against_the_restatement int64_lists_and_a_wider_matrix_with_another_fill_value
      row_of_three_lds_tiles_runs_every_tile_pair_once backward_gives_minus_forces_and_differentiating_twice_raises""")
_take("d3_chain", TCR, """up_to_seven_species_bit_identical eight_to_fifteen_species_within_the_reference_bar
      sixteen_or_more_species_take_the_two_gather_walk huge_dE_dCN_raises_the_flag spatial_order_and_batches
      packed_list_fallback_keeps_the_two_gather_walk molecules_without_a_cell""", "no_companion")

# ---- charges --------------------------------------------------------------------------------------------------------------------------------------

_take("coulomb", TC, "list_and_matrix_match_oracle batched_match_oracle_and_single energy_autograd forces_can_be_differentiated")
_take("pme", TP, """spline_ops_match_oracle spline_high_order_properties green_structure_factor_and_corrections real_space_matches_oracle
      real_space_on_lists_that_are_not_symmetric pme_reciprocal_matches_oracle orders_5_6_vs_extended_oracle pme_batch_matches_oracle_and_single
      pme_madelung_and_explicit_ewald ewald_reciprocal_space_vs_oracle ewald_reciprocal_space_batch_and_summation
      ewald_reciprocal_space_autograd ewald_reciprocal_space_cell_alpha_kvector_gradients""", "pme_spread_path")


@pytest.mark.parametrize("dims", [(12, 10, 14), (31, 9, 6)])
@pytest.mark.parametrize("order", [1, 3, 4, 6])
def test_pme__tile_owned_spread(dims, order, pme_spread_path):
    TP.test_tile_owned_spread(dims, order)


@pytest.mark.parametrize("dims", [(12, 10, 14), (31, 9, 6)])
@pytest.mark.parametrize("order", [3, 4])
def test_pme__tile_staged_gather_epilogue(dims, order, pme_spread_path):
    TP.test_tile_staged_gather_epilogue(dims, order)


@pytest.mark.parametrize("dims", [(8, 8, 8), (16, 8, 32)])  # the cases of the round-4 hand probe of the solve, now here
@pytest.mark.parametrize("order", [4, 5])
def test_pme__fused_mesh_solve(dims, order, pme_spread_path, monkeypatch):
    TP.test_fused_mesh_solve(dims, order, monkeypatch)


@pytest.mark.parametrize("dims,batch", [((3, 2, 1), 2), ((1, 5, 4), 2)])
def test_pme__dense_dft_matches_numpy(dims, batch):
    TP.test_dense_dft_matches_numpy(dims, batch)


def test_pme__pme_through_the_dense_dft(pme_spread_path, monkeypatch):
    TP.test_pme_through_the_dense_dft((16, 8, 32), monkeypatch)


_take("autograd", TA, """pme_autograd_equals_explicit_forces_and_fd reciprocal_forces_can_be_differentiated
      real_space_forces_can_be_differentiated total_pme_forces_can_be_differentiated
      explicit_k_forces_and_charge_gradients_can_be_differentiated charge_gradient_outputs_can_be_differentiated""", "pme_spread_path")


def test_autograd__fused_forward_under_autograd_equals_the_composition(pme_spread_path, monkeypatch):
    TA.test_fused_forward_under_autograd_equals_the_composition(False, 4, monkeypatch)


def test_autograd__fused_particle_mesh_ewald_node_equals_the_composition(pme_spread_path, monkeypatch):
    TA.test_fused_particle_mesh_ewald_node_equals_the_composition("matrix", monkeypatch)


def test_autograd__fused_nodes_with_charge_gradient_outputs_equal_the_composition(pme_spread_path, monkeypatch):
    TA.test_fused_nodes_with_charge_gradient_outputs_equal_the_composition("reciprocal", True, monkeypatch)


def test_autograd__fused_nodes_with_explicit_forces_equal_the_composition(pme_spread_path, monkeypatch):
    TA.test_fused_nodes_with_explicit_forces_equal_the_composition("pme_reciprocal_space", True, monkeypatch)


def test_autograd__fused_node_through_the_mesh_solve(pme_spread_path, monkeypatch):
    TA.test_fused_node_through_the_mesh_solve(True, monkeypatch)


_take("virial", TV, "real_space_matches_strain_derivative pme_reciprocal_matches_strain_derivative ewald_reciprocal_matches_strain_derivative")
_take("full_list", TF, "full_list_takes_the_trusted_form_and_gives_the_same_numbers overflowed_rows_raise_the_mark")

# ---- multi-channel splines, at their smallest mesh ------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("order", [1, 2, 3, 4, 5, 6])
def test_channels__spread_channels_match_oracle_and_scalar(order, channels_spread_path):
    TCH.test_spread_channels_match_oracle_and_scalar((8, 8, 8), order)


@pytest.mark.parametrize("order", [1, 2, 3, 4, 5, 6])
def test_channels__gather_channels_match_oracle_and_scalar_bitwise(order, channels_spread_path):
    TCH.test_gather_channels_match_oracle_and_scalar_bitwise((8, 8, 8), order)


_take("channels", TCH, "adjointness_across_channels", "channels_spread_path")

# ---- the newer electrostatics ---------------------------------------------------------------------------------------------------------------------

_take("gaussian", TG, """parity_fp64_matrix_and_csr padding_rules_empty_rows_and_point_charges batch_parity_slices_and_per_system_background
      non_periodic fp32_inputs autograd_matches_reference_and_explicit_outputs""")
_take("qeq", TQ, """product_is_the_sum_of_the_public_charge_gradients solve_cluster_single_and_batched solve_periodic_ewald_batch solve_pme_against_ewald zero_right_hand_side_and_symmetric_lattice
      warm_start_and_non_convergence gradients_against_the_reference_autograd""")
_take("dipole", TDP, """parity_fp64_matrix_and_csr parity_fp32_inputs self_images_padding_kinds_empty_row_and_wide_matrix
      batch_equals_single_calls_and_reference one_k_vector_and_empty_k_set autograd_matches_reference_and_explicit_outputs
      autograd_fp32_only_dipoles_and_batch virial_is_the_strain_derivative_and_not_symmetric""")
_take("pme_dipole", TPD, """parity_fp64 parity_fp32 batch_against_single_calls_and_the_restatement weighted_loss_against_the_restatement
      backward_equals_the_explicit_outputs_of_the_same_call correction_agrees_with_the_explicit_ewald_routine""")
_take("induced", TI, """product_against_the_dense_reference solve_explicit_ewald_batch solve_pme_against_ewald zero_right_hand_side external_field_only_warm_start_and_non_convergence
      float32_positions gradients_against_the_reference_autograd""")
_take("induced", TSM, "induced_dipoles_with_a_system_without_atoms_and_one_without_a_polarisable_atom")
_take("thole", TTH, """c_abi_every_flag_combination_against_the_reference c_abi_weights_give_the_adjoint_and_energies_may_be_null
      entries_beyond_the_exit_contribute_exact_zeros public_function_outputs_and_adjoint
      stored_operator_is_the_dipole_gradient_of_the_two_pair_kernels damped_solve_explicit_ewald_batch
      damped_solve_single_system_and_thole_none_is_the_undamped_path damped_solve_pme_single_and_batched
      damped_gradients_against_the_reference_autograd""")
_take("quadrupole", TQD, """parity_fp64_matrix_and_csr parity_fp32_inputs self_images_padding_kinds_empty_row_wide_matrix_and_no_dipoles
      row_length_ladder k_count_ladder empty_k_set_is_the_self_term_alone batch_equals_single_calls_and_reference
      autograd_matches_reference_and_explicit_outputs autograd_fp32_only_quadrupoles_and_batch
      virial_is_the_strain_derivative_and_not_symmetric""")

# the quadrupole mesh term: the four-mesh memset of the adjoint (`weights ? 4 : 2`) and its `accumulate` launch run in every one of these
@pytest.fixture(scope="module")
def pme_quadrupole_references():
    """The restatements of the sweep seeds, evaluated BEFORE the poison starts (a module-scoped fixture is set up before the autouse one): on
    poisoned CPU allocations an evaluation takes twice as long -- the float32 seeds 3, 7, 9 and 11 took 5.1 - 7.5 s that way --, and the
    references are the home module's, computed once for both (`functools.lru_cache`)."""
    W = TSQ.W
    for seed in W.SEEDS:
        both = W.pmeq_case("sweep", seed)["dtype"] == "float32" or seed == W.pmeq_batch_seed()
        for mode in ("float64", "float32") if both else ("float64",):
            for weighted in (False, True):
                W.pme_quadrupole_reference("sweep", seed, mode, weighted)


_take("pme_quadrupole", TSQ, "atoms_on_spline_knots")
_take("pme_quadrupole", TSQ, "sweep batch_systems_equal_single_calls_forward_and_backward", "pme_quadrupole_references")


@pytest.mark.parametrize("dt", [TSQ.F64, TSQ.F32], ids=["float64", "float32"])
@pytest.mark.parametrize("order,n", [(o, n) for o in TSQ.W.PMEQ_ORDERS for n in (1, TSQ.W.spread_atoms_per_block(o) + 1, TSQ.W.PG_ATOMS + 1)])
def test_pme_quadrupole__spread_gather_ladder(order, n, dt):
    TSQ.test_spread_gather_ladder(order, n, dt)


# ---- nvalchemiops.math: the closed forms ----------------------------------------------------------------------------------------------------------

_take("math", TM, """spherical_harmonics_against_closed_forms harmonic_gradients gto_density_against_closed_forms_and_integrals
      gto_fourier_against_closed_forms gto_fourier_l0_is_the_transform_of_the_l0_density""")

# ---- the fold-size tests, all of them: the second trip of a fold kernel is where an unwritten partial slot would be read --------------------------

_take("fold", TFS, """d4_copies_as_one_system_and_as_a_batch gaussian_copies_as_one_system_and_as_a_batch
      dipole_real_space_copies_as_one_system_and_as_a_batch ewald_real_space_virial_copies_as_one_system_and_as_a_batch
      charge_equilibration_copies_as_one_system_and_as_a_batch quadrupole_real_space_copies_as_one_system_and_as_a_batch
      thole_dipole_correction_copies_as_one_system_and_as_a_batch induced_dipoles_copies_as_one_system_and_as_a_batch
      pair_scale_copies_as_one_system_and_as_a_batch pair_scale_minimum_image_copies_as_one_system_and_as_a_batch
      local_frames_copies_as_one_system_and_as_a_batch cluster_corrections_periodic_copies_as_one_system_and_as_a_batch
      cluster_induced_dipoles_copies_as_one_system_and_as_a_batch""")
