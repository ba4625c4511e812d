"""Dispersion corrections (reference: nvalchemiops/interactions/dispersion/__init__.py): DFT-D3 with BJ damping, zero damping and the
three-body terms, and DFT-D4: the two-body term with charge-dependent C6 and its three-body term."""
from nvalchemiops.interactions.dispersion.dftd3 import D3Parameters, dftd3, dftd3_atm, dftd3_zero, dftd3_zero_atm
from nvalchemiops.interactions.dispersion.dftd4 import D4Parameters, dftd4, dftd4_atm

__all__ = ["D3Parameters", "D4Parameters", "dftd3", "dftd3_atm", "dftd3_zero", "dftd3_zero_atm", "dftd4", "dftd4_atm"]
