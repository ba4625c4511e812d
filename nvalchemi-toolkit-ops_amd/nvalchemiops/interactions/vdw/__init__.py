"""Van der Waals terms of the force-field stack: buffered 14-7 and Lennard-Jones between reduced sites (HIP: csrc/vdw.hip) and the lattice
sum of their r^-6 tail, by explicit Ewald summation (HIP: csrc/dispersion_ewald.hip) or on a mesh (HIP: csrc/dispersion_pme.hip)."""
from nvalchemiops.interactions.vdw.ewald import (ewald_dispersion_correction, ewald_dispersion_real_space, ewald_dispersion_reciprocal_space,
                                                 lennard_jones_dispersion_coefficients)
from nvalchemiops.interactions.vdw.pair import buffered_14_7, lennard_jones
from nvalchemiops.interactions.vdw.pme import pme_dispersion_correction, pme_dispersion_reciprocal_space
from nvalchemiops.interactions.vdw.sites import ReducedSites

__all__ = ["buffered_14_7", "lennard_jones", "ReducedSites", "ewald_dispersion_correction", "ewald_dispersion_real_space",
           "ewald_dispersion_reciprocal_space", "pme_dispersion_correction", "pme_dispersion_reciprocal_space",
           "lennard_jones_dispersion_coefficients"]
