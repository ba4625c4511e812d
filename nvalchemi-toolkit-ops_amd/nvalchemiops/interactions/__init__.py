"""Neighbour-driven interactions of the MI355X hot path: dispersion (DFT-D3), electrostatics (PME) and van der Waals pair potentials."""
__all__ = ["buffered_14_7", "lennard_jones", "ReducedSites", "ewald_dispersion_correction", "ewald_dispersion_real_space",
           "ewald_dispersion_reciprocal_space", "pme_dispersion_correction", "pme_dispersion_reciprocal_space",
           "lennard_jones_dispersion_coefficients"]


def __getattr__(name):
    """The vdW exports, imported on first use: importing a subpackage does not pull in the others."""
    if name in __all__:
        from nvalchemiops.interactions import vdw

        return getattr(vdw, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
