"""Electrostatics on the MI355X hot path: PME = real-space erfc sum + B-spline/FFT reciprocal sum
(reference exports: interactions/electrostatics/__init__.py:33-80; plus the explicit-k Ewald sum; plain Coulomb is outside this path)."""
from nvalchemiops.interactions.electrostatics.ewald import (ewald_real_space, ewald_real_space_with_virial, ewald_reciprocal_space,
                                                            ewald_reciprocal_space_with_virial, ewald_summation, ewald_summation_with_virial)
from nvalchemiops.interactions.electrostatics.dipole import ewald_dipole_correction, ewald_dipole_real_space, ewald_dipole_reciprocal_space
from nvalchemiops.interactions.electrostatics.pme_dipole import pme_dipole_correction, pme_dipole_reciprocal_space
from nvalchemiops.interactions.electrostatics.quadrupole import (ewald_quadrupole_correction, ewald_quadrupole_real_space,
                                                                 ewald_quadrupole_reciprocal_space)
from nvalchemiops.interactions.electrostatics.pme_quadrupole import pme_quadrupole_correction, pme_quadrupole_reciprocal_space
from nvalchemiops.interactions.electrostatics.gaussian import gaussian_charge_correction
from nvalchemiops.interactions.electrostatics.induced import (InducedDipoleError, InducedDipoleResult, induced_dipoles,
                                                              thole_induced_dipoles)
from nvalchemiops.interactions.electrostatics.thole import thole_dipole_correction
from nvalchemiops.interactions.electrostatics.cluster import (cluster_induced_dipoles, coulomb_dipole_correction,
                                                              coulomb_quadrupole_correction)
from nvalchemiops.interactions.electrostatics.pair_scale import BondedPairScales, bonded_pair_scales, pair_scale_correction
from nvalchemiops.interactions.electrostatics.frames import (FRAME_BISECTOR, FRAME_NONE, FRAME_THREE_FOLD, FRAME_Z_BISECT, FRAME_Z_ONLY,
                                                             FRAME_Z_THEN_X, LocalFrames, multipole_frame_forces, rotate_multipoles)
from nvalchemiops.interactions.electrostatics.k_vectors import generate_k_vectors_ewald_summation, generate_k_vectors_pme
from nvalchemiops.interactions.electrostatics.parameters import (EwaldParameters, PMEParameters, estimate_ewald_parameters,
                                                                 estimate_pme_mesh_dimensions, estimate_pme_parameters,
                                                                 mesh_spacing_to_dimensions)
from nvalchemiops.interactions.electrostatics.qeq import ChargeEquilibrationError, ChargeEquilibrationResult, charge_equilibration
from nvalchemiops.interactions.electrostatics.pme import (particle_mesh_ewald, pme_energy_corrections,
                                                          particle_mesh_ewald_with_virial, pme_energy_corrections_with_charge_grad,
                                                          pme_green_structure_factor, pme_reciprocal_space, pme_reciprocal_space_with_virial)

__all__ = [
    "particle_mesh_ewald", "pme_reciprocal_space", "ewald_real_space", "pme_green_structure_factor", "pme_energy_corrections",
    "pme_energy_corrections_with_charge_grad", "generate_k_vectors_pme", "estimate_pme_parameters", "estimate_ewald_parameters",
    "estimate_pme_mesh_dimensions", "mesh_spacing_to_dimensions", "PMEParameters", "EwaldParameters", "ewald_reciprocal_space", "ewald_summation", "generate_k_vectors_ewald_summation",
    "ewald_real_space_with_virial", "pme_reciprocal_space_with_virial", "particle_mesh_ewald_with_virial", "ewald_reciprocal_space_with_virial",
    "ewald_summation_with_virial", "gaussian_charge_correction", "charge_equilibration", "ChargeEquilibrationError", "ChargeEquilibrationResult",
    "ewald_dipole_correction", "ewald_dipole_real_space", "ewald_dipole_reciprocal_space", "pme_dipole_correction", "pme_dipole_reciprocal_space",
    "induced_dipoles", "InducedDipoleError", "InducedDipoleResult", "thole_dipole_correction", "thole_induced_dipoles",
    "ewald_quadrupole_correction", "ewald_quadrupole_real_space", "ewald_quadrupole_reciprocal_space",
    "pme_quadrupole_correction", "pme_quadrupole_reciprocal_space",
    "coulomb_dipole_correction", "coulomb_quadrupole_correction", "cluster_induced_dipoles",
    "LocalFrames", "rotate_multipoles", "multipole_frame_forces", "FRAME_NONE", "FRAME_Z_ONLY", "FRAME_Z_THEN_X", "FRAME_BISECTOR",
    "FRAME_Z_BISECT", "FRAME_THREE_FOLD",
    "pair_scale_correction", "bonded_pair_scales", "BondedPairScales",
]
