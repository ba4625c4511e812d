"""Van der Waals pair potentials of the force-field stack: buffered 14-7 and Lennard-Jones between reduced sites (HIP: csrc/vdw.hip)."""
from nvalchemiops.interactions.vdw.pair import buffered_14_7, lennard_jones
from nvalchemiops.interactions.vdw.sites import ReducedSites

__all__ = ["buffered_14_7", "lennard_jones", "ReducedSites"]
